"""Batch geometry: chunks and their masks, the minibatch partition, orders and schedules, the KL rule, standardisation, and the
window cut and gather"""
import numpy as np
import torch

from .. import _lib as L
from ._ffi import _need_gpu, _p, _stream

# ------------------------------------------------------------------------------------------------------------------ batch geometry
def cut_chunks(ep_start, ep_len, max_seq_len):
    """chop_into_sequences (rllib/policy/rnn_sequencing.py) on an episode table: every episode's rows cut into chunks of max_seq_len
    (L, ..., L, remainder).  ep_start / ep_len integer tensors [E] (any device) -> (seq_start, seq_len) int64 [S], episodes in order"""
    Lm = int(max_seq_len)
    ep_start, ep_len = ep_start.long(), ep_len.long()
    n_ch = (ep_len + (Lm - 1)) // Lm
    seq_ep = torch.repeat_interleave(torch.arange(ep_len.numel(), device=ep_len.device), n_ch)
    first = torch.cumsum(n_ch, dim=0) - n_ch
    j = torch.arange(seq_ep.numel(), device=ep_len.device) - first[seq_ep]
    return ep_start[seq_ep] + j * Lm, torch.clamp(ep_len[seq_ep] - j * Lm, max=Lm)


def pad_chunks(col, seq_start, seq_len, max_seq_len):
    """pad_batch_to_sequences_of_same_size on one column [R, ...]: -> [S, L, ...], zero beyond each chunk's seq_len"""
    Lm = int(max_seq_len)
    t = torch.arange(Lm, device=col.device)
    mask = t[None, :] < seq_len[:, None]
    idx = torch.where(mask, seq_start[:, None] + t[None, :], torch.zeros_like(seq_start[:, None]))
    out = col[idx.reshape(-1)].reshape((idx.shape[0], Lm) + tuple(col.shape[1:]))
    return out * mask.reshape(mask.shape + (1,) * (col.dim() - 1)).to(col.dtype)


def chunk_mask(seq_len, max_seq_len):
    """sequence_mask: bool [S, L], the unpadded rows"""
    return torch.arange(int(max_seq_len), device=seq_len.device)[None, :] < seq_len[:, None]


def minibatch_partition(seq_len, sgd_minibatch_size):
    """the chunks (escape: rows, seq_len all 1) in order, split into consecutive minibatches of at least sgd_minibatch_size unpadded rows
    (the last one holds what is left).  seq_len: host integers [S] -> list of (first chunk, last chunk + 1)"""
    csum = np.cumsum(np.asarray(seq_len, dtype=np.int64))
    out, s0, base = [], 0, 0
    S = len(csum)
    while s0 < S:
        s1 = int(np.searchsorted(csum, base + int(sgd_minibatch_size), side="left")) + 1
        s1 = min(s1, S)
        out.append((s0, s1))
        base, s0 = int(csum[s1 - 1]), s1
    return out


def minibatch_order(n, seed, update, policy, sgd_pass):
    """the order in which one pass visits its n minibatches: keyed by (seed, update count, policy, pass), so two learners with the same
    seed visit the same order.  (RLlib shuffles with the unseeded global numpy generator: its order is not reproducible at all.)"""
    return np.random.default_rng([int(seed), int(update), int(policy), int(sgd_pass)]).permutation(int(n))


def sequence_order(n, seed, update, policy, sgd_pass):
    """shuffle_sequences: the order of one pass's n chunks (escape: rows), a permutation keyed by (seed, update count, policy, pass) and a
    fifth entry 1 that keeps it a different stream from minibatch_order's -> int64 [n]"""
    return np.random.default_rng([int(seed), int(update), int(policy), int(sgd_pass), 1]).permutation(int(n))


def shuffled_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy):
    """shuffle_sequences: the minibatch steps of one update over S chunks of these lengths (host integers [S]) as hh_minibatch_stage_gather's
    two tables -> (order int32 [num_sgd_iter * S], sched int32 [n_steps, 4]).  Pass p owns order[p S:(p + 1) S] = sequence_order(S, seed,
    update, policy, p); its minibatches are minibatch_partition's of the lengths in that order — consecutive runs of at least
    sgd_minibatch_size unpadded rows, the last one what is left — visited in position order.  A schedule row is (o0, o1, unpadded rows, 0)
    with o0, o1 absolute positions in order; the passes may differ in their number of steps."""
    seq_len = np.asarray(seq_len, dtype=np.int64).reshape(-1)
    S, passes = len(seq_len), int(num_sgd_iter)
    if passes * S > np.iinfo(np.int32).max:
        raise ValueError(f"shuffled_schedule: the order table of {passes} passes over {S} chunks does not fit int32 positions")
    order = np.empty((max(passes, 0) * S,), dtype=np.int32)
    rows = []
    for p in range(passes):
        perm = sequence_order(S, seed, update, policy, p)
        order[p * S:(p + 1) * S] = perm
        lens = seq_len[perm]
        csum = np.concatenate([[0], np.cumsum(lens)])
        rows += [(p * S + s0, p * S + s1, int(csum[s1] - csum[s0]), 0) for s0, s1 in minibatch_partition(lens, sgd_minibatch_size)]
    return order, np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def update_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy, shuffle):
    """The minibatch steps of one policy's update as the ONE table that every step mode walks row by row, the eager loop on the host and
    the graph's cursor on the device -> (order, sched int32 [n_steps, 4], need).  shuffle False: order is None and sched is
    sequence_schedule's — rows (first chunk, last chunk + 1, unpadded rows, 0), per pass in minibatch_order's order.  True:
    shuffled_schedule's (order, sched), the rows naming positions of order.  need: the chunks of the largest minibatch, the smallest
    staging capacity (1 where there is no minibatch)."""
    if shuffle:
        order, sched = shuffled_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy)
        return order, sched, int((sched[:, 1] - sched[:, 0]).max()) if len(sched) else 1
    parts, sched = sequence_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy)
    return None, sched, max((s1 - s0 for s0, s1 in parts), default=1)


def minibatch_schedule(parts, n_valid, num_sgd_iter, seed, update, policy):
    """the minibatch steps of one policy's update as hh_minibatch_stage's table: per pass the parts of minibatch_partition in
    minibatch_order's order -> int32 [num_sgd_iter * len(parts), 4] = (first chunk, last chunk + 1, unpadded rows, 0)"""
    rows = [(parts[i][0], parts[i][1], int(n_valid[i]), 0) for sgd_pass in range(int(num_sgd_iter))
            for i in minibatch_order(len(parts), seed, update, policy, sgd_pass)]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def sequence_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy):
    """the minibatch steps of one update over sequences of these lengths (host integers [S]): minibatch_partition's parts and their
    minibatch_schedule — per pass minibatch_order's order, what the eager path visits -> (parts, int32 [num_sgd_iter * len(parts), 4])"""
    seq_len = np.asarray(seq_len, dtype=np.int64)
    parts = minibatch_partition(seq_len, sgd_minibatch_size)
    csum = np.concatenate([[0], np.cumsum(seq_len)])
    return parts, minibatch_schedule(parts, [csum[s1] - csum[s0] for s0, s1 in parts], num_sgd_iter, seed, update, policy)


def kl_coeff_update(kl_coeff, sampled_kl, kl_target):
    """KLCoeffMixin.update_kl (ray/rllib/policy/torch_mixins.py): above 2 x target the coefficient grows by 1.5, below 0.5 x target it halves"""
    if sampled_kl > 2.0 * kl_target:
        return kl_coeff * 1.5
    if sampled_kl < 0.5 * kl_target:
        return kl_coeff * 0.5
    return kl_coeff


def standardize(adv):
    """standardized (ray/rllib/utils/sgd.py) over a policy's whole batch: (x - mean) / max(1e-4, std), population std"""
    return (adv - adv.mean()) / torch.clamp(adv.std(unbiased=False), min=1e-4)


def standardize_masked(adv, mask):
    """`standardize` over the rows that `mask` keeps (RLlib standardises the train batch before it is padded); 0 elsewhere"""
    w = mask.to(adv.dtype)
    n = w.sum()
    mean = (adv * w).sum() / n
    std = torch.sqrt((((adv - mean) * w) ** 2).sum() / n)
    return (adv - mean) / torch.clamp(std, min=1e-4) * w


# ------------------------------------------------------------------------------------------------------------------ the window batch
def _cut_args(who, done, max_seq_len):
    """the checks that window_cut and window_cut_torch share -> (T, N, max_seq_len)"""
    if isinstance(max_seq_len, bool) or int(max_seq_len) != max_seq_len or not 1 <= int(max_seq_len) <= L.WINDOW_MAX_LEN:
        raise ValueError(f"{who}: max_seq_len is an integer in 1 .. {L.WINDOW_MAX_LEN}, got {max_seq_len!r}")
    if not isinstance(done, torch.Tensor) or done.dtype != torch.uint8 or done.dim() != 2 or done.shape[0] < 1 or done.shape[1] < 1:
        raise ValueError(f"{who}: done is a uint8 tensor [T, N] with T, N >= 1 (the rollouts' done buffer)")
    if done.shape[0] * done.shape[1] >= 2 ** 31:
        raise ValueError(f"{who}: T N = {done.shape[0] * done.shape[1]} rows do not fit int32 sequence tables")
    return done.shape[0], done.shape[1], int(max_seq_len)


def window_cut(done, max_seq_len, out=None):
    """The sequences of a rollout's [T, N] window (hh_window_cut, include/hh_learner.h): per arena, walking t, a sequence ends at a done
    row (any non-zero byte of done u8 [T, N]), at its max_seq_len-th row, or at t = T-1 — chop_into_sequences on the window's
    fragments.  -> (seq_t0, seq_arena, seq_len): int32 [S] device views, arena-major, then time; S <= T N.  Three launches, then ONE
    synchronising read of the count, as EpisodeBatch.rows() makes one.  out: the three tables to write into (contiguous int32 CUDA
    tensors of at least T N elements each; entries at and beyond S are left as they were); default: new ones."""
    T, N, Lm = _cut_args("window_cut", done, max_seq_len)
    _need_gpu("window_cut")
    if not (done.is_cuda and done.is_contiguous()):
        raise ValueError("window_cut: done is a contiguous CUDA tensor (the torch-op form is window_cut_torch)")
    dev = done.device
    if out is None:
        out = tuple(torch.empty((T * N,), dtype=torch.int32, device=dev) for _ in range(3))
    if len(out) != 3 or any(not (o.is_cuda and o.device == dev and o.dtype == torch.int32 and o.is_contiguous() and o.dim() == 1 and o.numel() >= T * N) for o in out):
        raise ValueError(f"window_cut: out is three contiguous int32 CUDA tensors of at least T N = {T * N} elements on done's device")
    small = torch.empty((N + 1,), dtype=torch.int32, device=dev)        # the scratch [N], then n_seq
    L.check(L.lib().hh_window_cut(T, N, _p(done), Lm, _p(out[0]), _p(out[1]), _p(out[2]), _p(small[N:]), _p(small), _stream(dev)))
    S = int(small[N])
    return out[0][:S], out[1][:S], out[2][:S]


def window_cut_torch(done, max_seq_len):
    """window_cut with torch ops, any device -> (seq_t0, seq_arena, seq_len) int32 [S], the same entries in the same order"""
    T, N, Lm = _cut_args("window_cut_torch", done, max_seq_len)
    dev = done.device
    end = (done != 0).t().contiguous()                                    # [N, T]: arena-major
    end[:, T - 1] = True
    t = torch.arange(T, device=dev)[None, :].expand(N, T)
    first = torch.ones((N, T), dtype=torch.bool, device=dev)
    first[:, 1:] = end[:, :-1]                                            # a fragment starts at t = 0 and behind every done row
    frag_t0 = torch.cummax(torch.where(first, t, torch.zeros_like(t)), dim=1).values
    r0 = torch.nonzero((first | ((t - frag_t0) % Lm == 0)).reshape(-1)).reshape(-1)   # every sequence's first row, r = n T + t
    nxt = torch.cat([r0[1:], torch.full((1,), N * T, dtype=r0.dtype, device=dev)])    # t = 0 starts one in every arena: none crosses arenas
    return (r0 % T).to(torch.int32), (r0 // T).to(torch.int32), (nxt - r0).to(torch.int32)


def _gather_args(who, cols, tables, max_seq_len):
    """the checks that window_gather and window_gather_torch share.  cols: per column (src, tail, offset, per_seq) — src a contiguous
    tensor [T_src, N, ...] (a step-row is src[t, n]), tail the trailing shape of one gathered row in src's dtype, offset the BYTES from the
    step-row's start to it, per_seq False | True -> (S, max_seq_len, T_src, N, [(src, tail, offset, width, step_bytes, per_seq)])"""
    if isinstance(max_seq_len, bool) or int(max_seq_len) != max_seq_len or not 1 <= int(max_seq_len) <= L.WINDOW_MAX_LEN:
        raise ValueError(f"{who}: max_seq_len is an integer in 1 .. {L.WINDOW_MAX_LEN}, got {max_seq_len!r}")
    if not 1 <= len(cols) <= L.STAGE_MAX_COLS:
        raise ValueError(f"{who}: 1 .. {L.STAGE_MAX_COLS} columns per call, got {len(cols)}")
    if len(tables) != 3 or any(not isinstance(x, torch.Tensor) or x.dtype != torch.int32 or x.dim() != 1 or x.numel() != tables[0].numel() for x in tables):
        raise ValueError(f"{who}: tables is (seq_t0, seq_arena, seq_len), int32 [S] each (window_cut's)")
    out, T_src, N = [], None, None
    for col in cols:
        src, tail, offset, per_seq = col
        tail = tuple(int(x) for x in tail)
        if not isinstance(src, torch.Tensor) or src.dim() < 2 or not src.is_contiguous() or src.shape[0] < 1 or src.shape[1] < 1:
            raise ValueError(f"{who}: a column's source is a contiguous tensor [T_src, N, ...]")
        if N is not None and src.shape[1] != N:
            raise ValueError(f"{who}: the columns of one call hold the same N arenas")
        N = src.shape[1]
        T_src = src.shape[0] if T_src is None else min(T_src, src.shape[0])     # the rows EVERY column of the call holds
        step_bytes = (src.numel() // (src.shape[0] * N)) * src.element_size()
        width = int(np.prod(tail, dtype=np.int64)) * src.element_size()
        if width < 1 or int(offset) < 0 or int(offset) % src.element_size() or int(offset) + width > step_bytes:
            raise ValueError(f"{who}: a slice of {width} bytes at offset {offset} does not lie, element-aligned, inside its {step_bytes}-byte step-row")
        out.append((src, tail, int(offset), width, step_bytes, bool(per_seq)))
    return tables[0].numel(), int(max_seq_len), T_src, N, out


def window_gather(cols, tables, max_seq_len, out=None):
    """The window's columns as padded sequences in ONE launch (hh_window_gather, include/hh_learner.h).  cols: up to 8 tuples
    (src, tail, offset, per_seq) — src a contiguous CUDA tensor [T_src, N, ...] (the rollout's buffer as it lies), tail the trailing shape
    of one gathered row in src's dtype, offset the bytes from the step-row src[t, n] to that slice (one agent's part), per_seq True for
    the first row of every sequence only; tables: window_cut's (seq_t0, seq_arena, seq_len).  -> per column a new tensor
    [S, max_seq_len, *tail], zero beyond every sequence's length, or [S, *tail] with per_seq.  The kernel may read the rows that every
    column of the call holds (T_src = the smallest of the sources' first dimensions).  A table entry that names no rows of the window
    stages zeros.  out: the destinations to write into instead (contiguous, the same shapes and dtypes; every byte of them is written).
    No host synchronisation, HIP-graph capturable."""
    S, Lm, T_src, N, cs = _gather_args("window_gather", cols, tables, max_seq_len)
    _need_gpu("window_gather")
    dev = tables[0].device
    if any(not (x.is_cuda and x.is_contiguous() and x.device == dev) for x in tables) or any(not (c[0].is_cuda and c[0].device == dev) for c in cs):
        raise ValueError("window_gather: the tables and the sources are contiguous CUDA tensors on one device (the torch-op form is window_gather_torch)")
    shapes = [((S,) if per_seq else (S, Lm)) + tail for _, tail, _, _, _, per_seq in cs]
    if out is None:
        out = [torch.empty(sh, dtype=c[0].dtype, device=dev) for sh, c in zip(shapes, cs)]
    if len(out) != len(cs) or any(not (o.is_cuda and o.device == dev and o.is_contiguous() and o.dtype == c[0].dtype and tuple(o.shape) == sh)
                                  for o, sh, c in zip(out, shapes, cs)):
        raise ValueError("window_gather: out holds per column a contiguous CUDA tensor [S, max_seq_len, *tail] ([S, *tail] with per_seq) of the source's dtype")
    if S == 0:
        return list(out)
    desc = (L.HHWindowCol * len(cs))()
    for d, o, (src, _, offset, width, step_bytes, per_seq) in zip(desc, out, cs):
        d.src, d.dst, d.step_bytes, d.offset, d.width, d.per_seq = src.data_ptr(), o.data_ptr(), step_bytes, offset, width, int(per_seq)
    L.check(L.lib().hh_window_gather(len(cs), desc, S, Lm, T_src, N, _p(tables[0]), _p(tables[1]), _p(tables[2]), _stream(dev)))
    return list(out)


def window_gather_torch(cols, tables, max_seq_len):
    """window_gather with torch ops, any device: the same arguments -> per column a new tensor with the same bytes (index_select through the
    tables; an entry that names no rows of the window gives zeros)"""
    S, Lm, T_src, N, cs = _gather_args("window_gather_torch", cols, tables, max_seq_len)
    t0, n, ln = (x.long() for x in tables)
    ok = (t0 >= 0) & (ln >= 0) & (ln <= Lm) & (n >= 0) & (n < N) & (t0 + ln <= T_src)
    t0, n, ln = (torch.where(ok, x, torch.zeros_like(x)) for x in (t0, n, ln))
    out = []
    for src, tail, offset, width, step_bytes, per_seq in cs:
        rows = 1 if per_seq else Lm
        j = torch.arange(rows, device=src.device)[None, :]
        keep = j < ln[:, None]                                                     # [S, rows]
        r = torch.where(keep, (t0[:, None] + j) * N + n[:, None], torch.zeros_like(keep, dtype=torch.int64))
        flat = src.reshape(src.shape[0] * N, -1).view(torch.uint8)[:, offset:offset + width]
        got = flat.index_select(0, r.reshape(-1)).reshape(S, rows, width) * keep[:, :, None].to(torch.uint8)
        got = got.contiguous().view(src.dtype).reshape((S, rows) + tail)
        out.append(got[:, 0] if per_seq else got)
    return out
