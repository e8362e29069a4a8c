"""Data-parallel learner updates that equal one process over the shards: who holds which shard (ShardGroup over torch.distributed,
LocalShards in one process), the step alignment and its weights, and the advantages' moments over all shards.

The contract is sharding.py's, moved to the learner: a W-rank update gives the SAME BYTES as one process that holds the W shards and runs
their forward and backward one after another.  Everything that crosses shards is therefore combined in shard (= rank) order from values
every rank holds alike: the gradients by grad_pack -> all-gather -> grad_combine (ops.py), the statistics and the moments here, on the
host, in float64.  LocalShards is that one process; ShardGroup is one of the W ranks.  Importing this module touches neither the GPU nor
torch.distributed."""
import math

import numpy as np
import torch

from .batch import standardize


# ------------------------------------------------------------------------------------------------------------------ sums in shard order
def ordered_sum(values):
    """values[0] + values[1] + ... in float64, in that order (numpy's pairwise sum would depend on the count)"""
    it = iter(values)
    acc = np.float64(next(it))
    for v in it:
        acc = acc + np.float64(v)
    return float(acc)


def step_weights(rows_of_shard):
    """The alignment of W shards' schedules.  rows_of_shard: per shard the unpadded rows of its minibatch steps in its own order
    (update_schedule's column 2; an empty list for a shard without rows).  Global step i is shard r's i-th row, or empty for r once its rows
    are used up; the update takes max_r len steps.
    -> (n int64 [steps, W]: the rows shard r brings to step i (0: empty), n_glob int64 [steps], weight f64 [steps, W] = n / n_glob)"""
    cols = [np.asarray(c, dtype=np.int64).reshape(-1) for c in rows_of_shard]
    if any((c < 1).any() for c in cols):
        raise ValueError("step_weights: a minibatch step holds at least one unpadded row")
    steps = max((len(c) for c in cols), default=0)
    n = np.zeros((steps, len(cols)), dtype=np.int64)
    for r, c in enumerate(cols):
        n[:len(c), r] = c
    n_glob = n.sum(axis=1)
    weight = n.astype(np.float64) / n_glob.astype(np.float64)[:, None] if steps else np.zeros((0, len(cols)), dtype=np.float64)
    return n, n_glob, weight


def combine_stats(stats, weight, n_glob):
    """The steps' statistics over all shards: stats f64 [W, steps, 6] (a shard's empty steps hold zeros), weight and n_glob step_weights'
    -> f64 [steps, 6]: sum_r weight[i, r] * stats[r, i] in shard order, starting from shard 0's product (so one shard with weight 1.0 keeps
    its bytes), slot 5 (the unpadded rows) = n_glob"""
    stats = np.asarray(stats, dtype=np.float64)
    acc = stats[0] * weight[:, 0:1]
    for r in range(1, stats.shape[0]):
        acc = acc + stats[r] * weight[:, r:r + 1]
    acc[:, 5] = n_glob
    return acc


def combined_mean(sums, counts):
    """the mean over all shards from per-shard (float64 sum, count), in shard order -> (mean, n); n == 0: (nan, 0)"""
    n = int(sum(int(c) for c in counts))
    return (ordered_sum(sums) / n if n else float("nan")), n


def combined_std(sq_sums, n):
    """the population standard deviation over all shards from per-shard float64 sums of (x - mean)^2, in shard order"""
    return math.sqrt(ordered_sum(sq_sums) / n)


def standardize_shards(xs, group):
    """`standardize` over the rows of ALL shards.  xs: this process's shards' advantage vectors (float32 [R_r], R_r >= 0), one per entry
    of group.local.  One shard: batch.standardize as it stands.  More: per shard the float64 sum and count are gathered, the mean is
    sum_r sum(x) / sum_r n, then per shard the float64 sum of (x - mean)^2 is gathered and std = sqrt(sum_r ssq / n) — both in shard order —
    and every shard computes (x - float32(mean)) / max(1e-4, float32(std)) in float32.  Two small gathers; collective.
    -> (the standardised vectors, the rows of all shards)"""
    if group.W == 1:
        return [standardize(x) if x.numel() else x for x in xs], int(xs[0].numel())
    first = group.gather_host(np.array([[float(x.double().sum()) if x.numel() else 0.0, float(x.numel())] for x in xs], dtype=np.float64))
    mean, n = combined_mean(first[:, 0], first[:, 1])
    if n == 0:
        return list(xs), 0
    second = group.gather_host(np.array([[float((x.double() - mean).square().sum()) if x.numel() else 0.0] for x in xs], dtype=np.float64))
    std = combined_std(second[:, 0], n)
    m32, s32 = float(np.float32(mean)), float(max(np.float32(1e-4), np.float32(std)))
    return [(x - m32) / s32 for x in xs], n


# ------------------------------------------------------------------------------------------------------------------ the groups
class LocalShards:
    """K shards in ONE process: the in-process twin of K ranks.  A learner built with it is handed K batches (or rollouts) per update and
    runs the K shards' forward and backward one after another; nothing is communicated, every gather is the identity."""

    def __init__(self, K):
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 64:
            raise ValueError(f"LocalShards: K is an integer in 1 .. 64 (hh_grad_combine's weights travel by value), got {K!r}")
        self.W, self.rank, self.local = K, 0, tuple(range(K))
        self.in_process = True      # a learner's update takes K batches

    def gather_host(self, rows):
        """rows: float64 or int64 numpy [len(local), m], this process's shards -> [W, m], all shards in shard order"""
        rows = np.ascontiguousarray(rows)
        if rows.ndim != 2 or rows.shape[0] != len(self.local):
            raise ValueError(f"gather_host: one row per local shard ({len(self.local)}), got {rows.shape}")
        return rows

    def gather_ragged(self, cols):
        """cols: per local shard a 1-D int64 array of any length -> per shard of the group its array, in shard order"""
        return [np.asarray(c, dtype=np.int64).reshape(-1) for c in cols]

    def pack_target(self, buckets, r):
        """where shard r's grad_pack writes: its row of buckets f32 [W, E]"""
        return buckets[r]

    def gather_buckets(self, buckets):
        """every shard's row of buckets filled in (here they already are)"""
        return buckets


class ShardGroup:
    """One rank of W: rank and W from torch.distributed (the default process group, or `process_group`); this process holds shard `rank`.
    Host rows travel through all_gather_into_tensor on CPU tensors ("gloo") or device tensors ("nccl"); the gradient buckets are gathered
    on the device for "nccl" and through a pinned host copy for "gloo".  The constructor is collective: every rank sends its rank and the
    blocks must arrive in rank order (sharding.gather_evidence's check).  world_size: the shards the caller cut its data for; another
    group size is refused."""

    def __init__(self, process_group=None, world_size=None, device=None):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("ShardGroup: torch.distributed is not initialised (init_process_group first; LocalShards(K) needs no group)")
        self.pg = process_group
        self.W, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        self.backend = dist.get_backend(process_group)
        if world_size is not None and int(world_size) != self.W:
            raise RuntimeError(f"ShardGroup: the process group has {self.W} ranks but the data was sharded over {int(world_size)}")
        if not 1 <= self.W <= 64:
            raise RuntimeError(f"ShardGroup: 1 .. 64 ranks (hh_grad_combine's weights travel by value), the group has {self.W}")
        self.local = (self.rank,)
        self.in_process = False     # a learner's update takes this rank's batch
        self.device = torch.device(device) if device is not None else (torch.device("cuda", torch.cuda.current_device()) if self.backend == "nccl" else None)
        self._mine = self._host = None
        seen = self.gather_host(np.array([[self.rank]], dtype=np.int64))[:, 0].tolist()
        if seen != list(range(self.W)):
            raise RuntimeError(f"ShardGroup: the blocks of {self.W} ranks arrived as ranks {seen}")

    def _all_gather(self, out, mine):
        import torch.distributed as dist
        dist.all_gather_into_tensor(out, mine, group=self.pg)
        if out.numel() != self.W * mine.numel():
            raise RuntimeError(f"ShardGroup: {out.numel()} elements gathered, {self.W} blocks of {mine.numel()} expected")
        return out

    def gather_host(self, rows):
        """rows: float64 or int64 numpy [1, m], this rank's -> [W, m], all ranks in rank order.  Collective."""
        rows = np.ascontiguousarray(rows)
        if rows.ndim != 2 or rows.shape[0] != 1 or rows.dtype not in (np.float64, np.int64):
            raise ValueError(f"gather_host: this rank's one row, float64 or int64 [1, m], got {rows.dtype} {rows.shape}")
        mine = torch.from_numpy(rows)
        if self.backend == "nccl":
            mine = mine.to(self.device)
        out = self._all_gather(torch.empty((self.W * rows.shape[1],), dtype=mine.dtype, device=mine.device), mine.reshape(-1))
        return out.cpu().numpy().reshape(self.W, rows.shape[1])

    def gather_ragged(self, cols):
        """cols: [this rank's 1-D int64 array] -> per rank its array, in rank order: the lengths first, then the arrays padded to the longest"""
        mine = np.asarray(cols[0], dtype=np.int64).reshape(-1)
        lens = self.gather_host(np.array([[len(mine)]], dtype=np.int64))[:, 0]
        most = int(lens.max())
        if most == 0:
            return [np.zeros((0,), dtype=np.int64) for _ in range(self.W)]
        padded = np.zeros((1, most), dtype=np.int64)
        padded[0, :len(mine)] = mine
        got = self.gather_host(padded)
        return [got[r, :int(lens[r])].copy() for r in range(self.W)]

    def pack_target(self, buckets, r):
        """where this rank's grad_pack writes: a block of its own beside buckets f32 [W, E] (an all-gather's input may not alias its output)"""
        if self._mine is None or self._mine.numel() != buckets.shape[1] or self._mine.device != buckets.device:
            self._mine = torch.zeros((buckets.shape[1],), dtype=torch.float32, device=buckets.device)
        return self._mine

    def gather_buckets(self, buckets):
        """this rank's packed block to every rank: buckets f32 [W, E] in rank order.  Collective; "gloo" synchronises with the device."""
        if self.backend == "nccl":
            self._all_gather(buckets.view(-1), self._mine)
            return buckets
        if self._host is None or self._host[0].shape != buckets.shape:
            self._host = (torch.empty(buckets.shape, dtype=torch.float32).pin_memory(), torch.empty((buckets.shape[1],), dtype=torch.float32).pin_memory())
        all_h, mine_h = self._host
        mine_h.copy_(self._mine)                 # device -> pinned host; copy_ to a CPU tensor waits for the stream
        self._all_gather(all_h.view(-1), mine_h)
        buckets.copy_(all_h, non_blocking=True)
        return buckets
