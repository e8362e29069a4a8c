"""learner/shards.py without a GPU: the step alignment and its weights for ragged schedules, the statistics and the advantages' moments
combined in shard order against numpy float64, and ShardGroup over two gloo ranks with CPU tensors — rank order, ragged gathers, and
the refusal of a group of another size than the data was cut for."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_alignment_and_weights_for_ragged_schedules():
    from hhmarl_2d_amd.learner import step_weights
    cols = [[64, 64, 37, 64, 64, 37], [21, 22], [], [3]]                 # four shards: lengths 6, 2, 0, 1
    n, n_glob, weight = step_weights(cols)
    assert n.shape == (6, 4) and n.dtype == np.int64 and weight.dtype == np.float64
    assert n.tolist() == [[64, 21, 0, 3], [64, 22, 0, 0], [37, 0, 0, 0], [64, 0, 0, 0], [64, 0, 0, 0], [37, 0, 0, 0]]
    assert n_glob.tolist() == [88, 86, 37, 64, 64, 37]
    for i in range(6):
        for r in range(4):
            assert weight[i, r] == np.float64(n[i, r]) / np.float64(n_glob[i])      # one correctly rounded division, in host float64
    assert weight[2:].tolist() == [[1.0, 0.0, 0.0, 0.0]] * 4, "a shard alone in a step has weight exactly 1.0"
    assert (weight[:, 2] == 0.0).all(), "the shard of length 0 is empty in every step"
    # one shard: every weight is exactly 1.0
    n1, g1, w1 = step_weights([[5, 7, 1]])
    assert w1.tolist() == [[1.0], [1.0], [1.0]] and g1.tolist() == [5, 7, 1]
    # no shard has a step
    n0, g0, w0 = step_weights([[], []])
    assert n0.shape == (0, 2) and g0.shape == (0,) and w0.shape == (0, 2)
    with pytest.raises(ValueError, match="at least one unpadded row"):
        step_weights([[4, 0]])


def test_statistics_are_combined_in_shard_order():
    from hhmarl_2d_amd.learner import combine_stats, step_weights
    rng = np.random.default_rng(3)
    n, n_glob, weight = step_weights([[64, 64, 30], [64, 11], [7]])
    stats = rng.standard_normal((3, 3, 6)) * np.array([1.0, 1e-3, 10.0, 1e-6, 3.0, 1.0])
    stats[1, 2] = 0.0
    stats[2, 1:] = 0.0                                                                # empty steps hold zeros
    got = combine_stats(stats, weight, n_glob)
    want = np.zeros((3, 6))
    for i in range(3):
        for k in range(6):
            acc = np.float64(stats[0, i, k]) * np.float64(weight[i, 0])
            for r in (1, 2):
                acc = acc + np.float64(stats[r, i, k]) * np.float64(weight[i, r])
            want[i, k] = acc
    want[:, 5] = n_glob
    assert np.array_equal(got, want)
    # one shard, weight 1.0: the rows come back bit for bit (-0.0 included), slot 5 the step's rows
    one = rng.standard_normal((1, 4, 6))
    one[0, 1, 2] = -0.0
    _, g1, w1 = step_weights([[9, 9, 9, 2]])
    back = combine_stats(one, w1, g1)
    assert np.array_equal(back[:, :5].view(np.int64), one[0][:, :5].view(np.int64)) and back[:, 5].tolist() == [9.0, 9.0, 9.0, 2.0]


class _Gather:
    """a group of W shards held in one process, with the gathers counted"""

    def __init__(self, W):
        self.W, self.local, self.calls = W, tuple(range(W)), 0

    def gather_host(self, rows):
        self.calls += 1
        assert rows.shape[0] == self.W and rows.dtype == np.float64
        return rows


def test_moments_over_all_shards_against_numpy_float64():
    from hhmarl_2d_amd.learner import combined_mean, combined_std, ordered_sum, standardize, standardize_shards
    rng = np.random.default_rng(11)
    xs = [torch.from_numpy((rng.standard_normal(n) * s + m).astype(np.float32)) for n, s, m in ((1536, 2.0, 0.5), (384, 0.1, -3.0), (0, 1.0, 0.0), (5, 30.0, 1.0))]
    # the reference: float64 sums per shard (numpy over the float64 copies, as torch's .double().sum() is checked against below), added in shard order
    sums = [float(x.double().sum()) for x in xs]
    n = sum(x.numel() for x in xs)
    acc = np.float64(sums[0])
    for s in sums[1:]:
        acc = acc + np.float64(s)
    mean = float(acc / n)
    assert combined_mean(sums, [x.numel() for x in xs]) == (mean, n)
    ssq = [float((x.double() - mean).square().sum()) for x in xs]
    acc = np.float64(ssq[0])
    for s in ssq[1:]:
        acc = acc + np.float64(s)
    std = float(np.sqrt(acc / n))
    assert combined_std(ssq, n) == std
    # against the moments of the concatenation in numpy float64: the same to float64 rounding of sums over 1925 values
    allx = np.concatenate([x.numpy().astype(np.float64) for x in xs])
    assert abs(mean - allx.mean()) <= 1925 * 2.0 ** -52 * np.abs(allx).mean() and abs(std - allx.std()) <= 1e-12 * allx.std()
    group = _Gather(4)
    got, rows = standardize_shards(xs, group)
    assert rows == n and group.calls == 2, "two small gathers"
    m32, s32 = np.float32(mean), max(np.float32(1e-4), np.float32(std))
    for g, x in zip(got, xs):
        assert g.dtype == torch.float32 and np.array_equal(g.numpy(), (x.numpy() - m32) / s32)
    assert got[2].numel() == 0
    # a spread below the floor: the divisor is float32(1e-4)
    flat = [torch.full((8,), 2.5), torch.full((3,), 2.5)]
    got, _ = standardize_shards(flat, _Gather(2))
    assert all(torch.equal(g, torch.zeros_like(g)) for g in got)
    # no rows anywhere
    assert standardize_shards([torch.zeros(0), torch.zeros(0)], _Gather(2))[1] == 0
    # one shard: batch.standardize as it stands, no gather
    one = _Gather(1)
    got, rows = standardize_shards(xs[:1], one)
    assert one.calls == 0 and rows == 1536 and torch.equal(got[0], standardize(xs[0]))
    assert ordered_sum([0.1, 0.2, 0.3]) == (0.1 + 0.2) + 0.3


def test_local_shards_is_the_identity():
    from hhmarl_2d_amd.learner import LocalShards
    g = LocalShards(3)
    assert (g.W, g.rank, g.local) == (3, 0, (0, 1, 2))
    rows = np.arange(6, dtype=np.float64).reshape(3, 2)
    assert np.array_equal(g.gather_host(rows), rows)
    assert [c.tolist() for c in g.gather_ragged([[1, 2], [], [3]])] == [[1, 2], [], [3]]
    b = torch.zeros((3, 8))
    assert g.pack_target(b, 1).data_ptr() == b[1].data_ptr() and g.gather_buckets(b) is b
    with pytest.raises(ValueError, match="one row per local shard"):
        g.gather_host(rows[:2])
    for bad in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="1 .. 64"):
            LocalShards(bad)


def _rank(rank, world_size, rendezvous, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["GLOO_SOCKET_IFNAME"] = "lo"
    import datetime
    dist.init_process_group("gloo", init_method=f"file://{rendezvous}", rank=rank, world_size=world_size, timeout=datetime.timedelta(seconds=60))
    from hhmarl_2d_amd.learner import ShardGroup, standardize_shards
    g = ShardGroup(world_size=world_size)
    assert (g.W, g.rank, g.local, g.backend) == (world_size, rank, (rank,), "gloo")
    rows = g.gather_host(np.array([[10.0 * rank + 1.0, 0.5]], dtype=np.float64))
    assert rows.tolist() == [[10.0 * r + 1.0, 0.5] for r in range(world_size)], "blocks in rank order"
    ragged = g.gather_ragged([np.arange(3 * rank, dtype=np.int64) + 100 * rank])            # rank 0 sends nothing
    assert [c.tolist() for c in ragged] == [[100 * r + k for k in range(3 * r)] for r in range(world_size)]
    assert [c.tolist() for c in g.gather_ragged([[]])] == [[] for _ in range(world_size)]
    # the moments over both ranks' rows: every rank computes the same bytes
    x = torch.from_numpy(np.random.default_rng(rank).standard_normal(100 + 50 * rank).astype(np.float32))
    got, n = standardize_shards([x], g)
    np.save(os.path.join(out_dir, f"std{rank}.npy"), got[0].numpy())
    assert n == sum(100 + 50 * r for r in range(world_size))
    with pytest.raises(RuntimeError, match="sharded over 3"):
        ShardGroup(world_size=world_size + 1)
    with pytest.raises(ValueError, match="this rank's one row"):
        g.gather_host(np.zeros((2, 2)))
    dist.barrier()
    dist.destroy_process_group()


def test_shard_group_over_two_gloo_ranks(tmp_path):
    from hhmarl_2d_amd.learner import LocalShards, standardize_shards
    mp.spawn(_rank, args=(2, str(tmp_path / "rendezvous"), str(tmp_path)), nprocs=2, join=True)
    xs = [torch.from_numpy(np.random.default_rng(r).standard_normal(100 + 50 * r).astype(np.float32)) for r in range(2)]
    want, _ = standardize_shards(xs, LocalShards(2))
    for r in range(2):
        assert np.array_equal(np.load(tmp_path / f"std{r}.npy"), want[r].numpy()), "a rank standardises as one process over both shards does"


def test_shard_group_needs_an_initialised_process_group():
    from hhmarl_2d_amd.learner import ShardGroup
    assert not dist.is_initialized()
    with pytest.raises(RuntimeError, match="not initialised"):
        ShardGroup()
