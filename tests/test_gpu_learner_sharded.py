"""PPOLearner(group=LocalShards(K)) on the MI355X: the in-process twin of K data-parallel ranks (learner/shards.py).

  (a) LocalShards(1) IS group=None: after two update_windows, and after an update on whole episodes, every result dict, every parameter,
      Adam's m / v / t and kl_coeff are the same bytes — the pack, the combine with weight 1.0 and the statistics' path change nothing;
  (b) two shards (worlds at arena offsets 0 and 64): finite statistics, rows = the sum of the shards' rows, steps = the longer shard's count;
  (c) shards of 64 and 16 arenas: the short shard is empty at the tail, and the combined gradient of such a step is the long shard's own;
  (d) the refusals.
The rollouts are tests/test_gpu_learner_window.py's (level 3, horizon 10, T = 24, num_sgd_iter 2, sgd_minibatch_size 64, logits recorded);
fight and escape kinds, both optimizers, without and with grad_clip and shuffle_sequences.  All comparisons are exact."""
import numpy as np
import pytest
import torch

import learner_rank_child as RC

pytestmark = pytest.mark.gpu
T = RC.T
BASE = dict(num_sgd_iter=2, sgd_minibatch_size=64)
OPTIONS = {"plain": {}, "clip and shuffle": dict(grad_clip=0.5, shuffle_sequences=True)}
_CACHE = {}


def _shard(mode, n_arenas, offset, batch_mode="truncate_episodes"):
    """one collected shard per key for the tests, which only read it"""
    key = (mode, n_arenas, offset, batch_mode)
    if key not in _CACHE:
        ro, bank = RC.build_shard(n_arenas, offset, mode, batch_mode)
        for _ in range(2):
            ro.collect()
        torch.cuda.synchronize()
        _CACHE[key] = (ro, bank)
    return _CACHE[key]


def _same(a, b, path=""):
    """two state dicts (or parts of them), bit for bit"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a, key=str) == sorted(b, key=str), path
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}/{i}")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8)), path
    else:
        assert a == b and type(a) is type(b), f"{path}: {a!r} != {b!r}"


def _same_learners(one, ref):
    sa, sb = one.state_dict(), ref.state_dict()
    assert sa["options"].pop("shards") == 1 and "shards" not in sb["options"]
    _same(sa, sb)
    assert one.kl_coeff == ref.kl_coeff and one.updates == ref.updates


def _same_results(got, want, rows_local):
    for g, w in zip(got, want):
        assert g.pop("rows_local") == rows_local
        assert list(g) == list(w)
        for k in w:
            assert g[k] == w[k] and type(g[k]) is type(w[k]), f"{k}: {g[k]!r} != {w[k]!r}"


@pytest.mark.parametrize("options", list(OPTIONS))
@pytest.mark.parametrize("optimizer", ["torch", "fused"])
@pytest.mark.parametrize("mode", ["fight", "escape"])
def test_one_local_shard_is_no_group(mode, optimizer, options):
    from hhmarl_2d_amd.learner import LocalShards
    kw = dict(BASE, optimizer=optimizer, **OPTIONS[options])
    ro, bank = _shard(mode, 64, 0)
    eps, ebank = _shard(mode, 64, 0, "complete_episodes")
    ref, one = RC.make_learner(mode, **kw), RC.make_learner(mode, group=LocalShards(1), **kw)
    for _ in range(2):
        want, got = ref.update_window(ro, bank), one.update_window([ro], bank)
        print(f"{mode} {optimizer} {options}: {want}")
        assert all(w["steps"] >= 4 and w["rows"] == T * 64 and np.isfinite(w["total_loss"]) for w in want)
        _same_results(got, want, T * 64)
    _same_learners(one, ref)
    rows = int(eps.episodes.rows()["obs"].shape[0])
    assert rows > 0
    want, got = ref.update(eps.episodes, ebank), one.update([eps.episodes], [ebank])
    _same_results(got, want, rows)
    _same_learners(one, ref)
    assert one.updates == 3 and ("grad_gnorm" in want[0]) == bool(OPTIONS[options])


def _expected(learner, shards, W):
    """per policy (rows over all shards, the longest shard's schedule length) from the shards' own cuts at sgd_minibatch_size // W"""
    from hhmarl_2d_amd import learner as LR
    out = []
    for a in range(2):
        lens = []
        for ro, bank in shards:
            with torch.no_grad():
                _, seq_len = learner._columns(learner.window_batch(ro, bank, a))
            _, sched, _ = LR.update_schedule(seq_len, max(1, learner.sgd_minibatch_size // W), learner.num_sgd_iter, learner.seed, learner.updates, a,
                                             learner.shuffle_sequences)
            lens.append(len(sched))
        out.append((sum(T * ro.w.N for ro, _ in shards), lens))
    return out


@pytest.mark.parametrize("optimizer", ["torch", "fused"])
@pytest.mark.parametrize("mode", ["fight", "escape"])
def test_two_shards_at_arena_offsets_0_and_64(mode, optimizer):
    from hhmarl_2d_amd.learner import LocalShards
    shards = [_shard(mode, 64, 0), _shard(mode, 64, 64)]
    assert not torch.equal(shards[0][0].obs, shards[1][0].obs), "the two worlds fly different arenas"
    learner = RC.make_learner(mode, group=LocalShards(2), **dict(BASE, optimizer=optimizer, **OPTIONS["clip and shuffle"]))
    before = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in learner.modules]
    want = _expected(learner, shards, 2)
    stats = learner.update_window([s[0] for s in shards], [s[1] for s in shards])
    for a, (st, (rows, lens)) in enumerate(zip(stats, want)):
        print(f"{mode} {optimizer} policy {a}: {st}; the shards' schedules hold {lens} steps")
        assert all(np.isfinite(st[k]) for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "kl_coeff", "grad_gnorm")), st
        assert st["rows"] == rows == 2 * T * 64 == st["rows_local"] and st["steps"] == max(lens) >= 2
        changed = [k for k, v in learner.modules[a].state_dict().items() if not torch.equal(v, before[a][k])]
        assert len(changed) == len(before[a]), "every tensor of the policy is trained"
    assert learner.state_dict()["options"]["shards"] == 2 and learner.updates == 1


@pytest.mark.parametrize("mode", ["fight", "escape"])
def test_the_short_shard_is_empty_at_the_tail(mode, monkeypatch):
    from hhmarl_2d_amd.learner import LocalShards, ops
    shards = [_shard(mode, 64, 0), _shard(mode, 16, 64)]
    learner = RC.make_learner(mode, group=LocalShards(2), **dict(BASE, optimizer="fused"))
    want = _expected(learner, shards, 2)
    seen = []
    combine = ops.grad_combine

    def watched(grads, buckets, weight, layout=None):
        combine(grads, buckets, weight, layout)
        w = [float(x) for x in weight]
        if w[1] == 0.0:         # the short shard has run out: the sum must be the long shard's own gradient, and its bucket zeros
            ns, offs, _ = layout
            assert w[0] == 1.0 and not buckets[1].view(torch.int32).any().item()
            assert all(torch.equal(g.reshape(-1), buckets[0, off:off + n]) for g, n, off in zip(grads, ns, offs))
        seen.append(w)
    monkeypatch.setattr(ops, "grad_combine", watched)
    stats = learner.update_window([s[0] for s in shards], [s[1] for s in shards])
    at = 0
    for a, (st, (rows, lens)) in enumerate(zip(stats, want)):
        print(f"{mode} policy {a}: {st}; the shards' schedules hold {lens} steps")
        assert lens[0] > lens[1] >= 2 and st["steps"] == lens[0] and st["rows"] == rows == T * 80 == st["rows_local"]
        ws = seen[at:at + lens[0]]
        at += lens[0]
        assert all(0.0 < w[0] < 1.0 and 0.0 < w[1] < 1.0 for w in ws[:lens[1]]) and all(w == [1.0, 0.0] for w in ws[lens[1]:])
        assert np.isfinite(st["total_loss"]) and np.isfinite(st["kl"])
    assert at == len(seen)


def test_refusals():
    from hhmarl_2d_amd.learner import CommanderLearner, LocalShards
    ro, bank = _shard("fight", 64, 0)
    with pytest.raises(ValueError, match='group needs step="eager"'):
        RC.make_learner("fight", optimizer="fused", step="graph", group=LocalShards(2))
    with pytest.raises(ValueError, match="a LocalShards or a ShardGroup"):
        RC.make_learner("fight", group=2)
    with pytest.raises(ValueError, match="group=None for now"):
        CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, group=LocalShards(1))
    two = RC.make_learner("fight", group=LocalShards(2), **BASE)
    with pytest.raises(ValueError, match="a sequence of 2 rollouts"):
        two.update_window(ro, bank)
    with pytest.raises(ValueError, match="a sequence of 2 EpisodeBatches"):
        two.update([None], bank)
    with pytest.raises(ValueError, match="one bank or one per shard"):
        two.update_window([ro, ro], [bank])
    assert two.updates == 0
