"""PPOLearner.window_batch / update_window on the MI355X: a PPORollout in its default batch_mode ("truncate_episodes"), fight and escape,
whose second window opens mid-episode.  The contract: the window batch equals policy_batch fed the same rows as episodes
(tests/window_batch_ref.py: the window's fragments, arena-major), and update_window equals the driver run on that reference batch.

Equality of a column is byte for byte on every unpadded row and in the escape kinds everywhere; a padded row of the window batch is
all-zero BYTES, where pad_chunks (row 0 times 0.0) leaves -0.0 behind a negative value — equal in value, so torch.equal holds on the
whole tensor as well."""
import numpy as np
import pytest
import torch

import window_batch_ref as WR

pytestmark = pytest.mark.gpu
N, T, HORIZON = 64, 24, 10


def _rollout(mode, record_logits, collects=2):
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    dev = torch.device("cuda", 0)
    w = World(make_config(n_arenas=N, level=3, seed=23, auto_reset=True, horizon=HORIZON, agent_mode=1 if mode == "escape" else 0), device=0)
    bank = PolicyBank.trainable_init(dev, mode=mode, seed=5, max_rows=2 * N)
    ro = PPORollout(w, bank, T, record_logits=record_logits)
    assert ro.batch_mode == "truncate_episodes" and ro.episodes is None
    for _ in range(collects):
        ro.collect()
    torch.cuda.synchronize()
    return ro, bank


_CACHE = {}


def _shared_rollout(mode, record_logits):
    """one rollout per (mode, record_logits) for the tests that only read it"""
    key = (mode, record_logits)
    if key not in _CACHE:
        _CACHE[key] = _rollout(mode, record_logits)
    return _CACHE[key]


def _learner(mode, **kw):
    from hhmarl_2d_amd.learner import PPOLearner
    return PPOLearner.trainable_init(torch.device("cuda", 0), mode=mode, seed=5, **kw)


def _preconditions(ro):
    done = ro.done.cpu().numpy() != 0
    assert (done.sum(axis=0) >= 2).any(), "some arena ends two episodes inside the window"
    assert (~done[T - 1]).any(), "some arena's last fragment is truncated: no done at t = T-1"
    assert done[:HORIZON - 1].any(), "an episode ends before a whole horizon has passed in the window"


def _reference_batches(learner, ro, bank):
    """policy_batch on the window presented as episodes -> (rows, [batch of policy 0, batch of policy 1])"""
    rows = WR.window_rows(ro)
    if ro.record_logits:
        old = rows["logits"]
    else:
        D = ro.obs.shape[3]
        old = learner.old_logits(ro.obs[:T].reshape(T * N, 2, D), bank, N).reshape(T, N, 2, 32).transpose(0, 1).reshape(N * T, 2, 32).contiguous()
    with torch.no_grad():
        return rows, [learner.policy_batch(rows, old, a) for a in range(2)]


def _same(got, want, mask, what):
    """byte equality where the reference holds no padding artefact (module docstring)"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    g, w = got.contiguous(), want.contiguous()
    if mask is None or g.dim() < 2 or what in ("seq_len", "mask"):
        assert torch.equal(g.view(torch.uint8), w.view(torch.uint8)), what
        return
    assert torch.equal(g, w), what
    m = mask.bool()
    assert torch.equal(g[m].view(torch.uint8), w[m].view(torch.uint8)), what
    assert not g[~m].view(torch.uint8).any().item(), f"{what}: the padding is zero bytes"


@pytest.mark.parametrize("record_logits", [False, True], ids=["bank logits", "recorded logits"])
@pytest.mark.parametrize("L", [20, 4])
@pytest.mark.parametrize("mode", ["fight", "escape"])
def test_window_batch_is_policy_batch_on_the_window_as_episodes(mode, L, record_logits):
    ro, bank = _shared_rollout(mode, record_logits)
    _preconditions(ro)
    learner = _learner(mode, max_seq_len=L)
    rows, want = _reference_batches(learner, ro, bank)
    for a in range(2):
        with torch.no_grad():
            got = learner.window_batch(ro, bank, a)
        assert list(got) == list(want[a])
        mask = want[a].get("mask")
        for k in want[a]:
            _same(got[k], want[a][k], mask, f"{mode} L {L} policy {a}: {k}")
        if mode == "fight":
            assert got["obs"].shape[1] == L and int(got["seq_len"].sum()) == T * N and got["seq_len"].max().item() <= L
            print(f"{mode} L {L} policy {a}: {got['obs'].shape[0]} sequences over {T * N} rows")
        else:
            assert got["obs"].shape[0] == T * N and "mask" not in got


@pytest.mark.parametrize("record_logits", [False, True], ids=["bank logits", "recorded logits"])
@pytest.mark.parametrize("mode", ["fight", "escape"])
def test_update_window_is_the_driver_on_the_reference_batch(mode, record_logits):
    ro, bank = _rollout(mode, record_logits)
    _preconditions(ro)
    kw = dict(num_sgd_iter=2, sgd_minibatch_size=256)
    l1, l2 = _learner(mode, **kw), _learner(mode, **kw)
    names = ("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target") + (("logits",) if record_logits else ())
    before = {k: getattr(ro, k).clone() for k in names}
    params = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in l1.modules]
    stats = l1.update_window(ro, bank)
    _, want = _reference_batches(l2, ro, bank)
    ref = [d.run(*l2._columns(b)) for d, b in zip(l2._sgd, want)]
    assert l1.updates == 1 and len(stats) == 2
    for a, (st, rf) in enumerate(zip(stats, ref)):
        print(f"{mode} policy {a}: update_window {st}\n{mode} policy {a}: driver on the reference batch {rf}")
        assert st["rows"] == T * N == rf["rows"]
        assert all(np.isfinite(st[k]) for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "kl_coeff")), st
        assert st["steps"] == rf["steps"] and st["steps"] >= 2
        assert abs(st["total_loss"] - rf["total_loss"]) <= 1e-4 * max(1.0, abs(rf["total_loss"]))
        changed = [k for k, v in l1.modules[a].state_dict().items() if not torch.equal(v, params[a][k])]
        assert len(changed) == len(params[a]), "every tensor of the policy is trained"
    assert all(torch.equal(before[k].view(torch.uint8), getattr(ro, k).view(torch.uint8)) for k in names), "the window is only read"
    # publish, then the next collect with no start(): every row of the next window is sampled by the published weights
    l1.publish(bank)
    ro.collect()
    torch.cuda.synchronize()
    assert ro.collects == 3 and not torch.equal(before["obs"], ro.obs)
    again = l1.update_window(ro, bank)
    assert l1.updates == 2 and all(s["rows"] == T * N and np.isfinite(s["total_loss"]) for s in again)


def test_update_window_replays_the_captured_step():
    """optimizer="fused", step="graph" next to fused eager on the same window, compared the way tests/test_gpu_learner_driver.py compares
    the step modes: the same steps and rows, and each step's unpadded rows are update_schedule's column 2, row for row"""
    from hhmarl_2d_amd import learner as LR
    ro, bank = _shared_rollout("fight", True)
    kw = dict(num_sgd_iter=2, sgd_minibatch_size=256, kl_coeff=0.0, optimizer="fused")
    eager, graph = _learner("fight", step="eager", **kw), _learner("fight", step="graph", **kw)
    with torch.no_grad():
        seq_lens = [eager._columns(eager.window_batch(ro, bank, a))[1] for a in range(2)]
    st_e, st_g = eager.update_window(ro, bank), graph.update_window(ro, bank)
    torch.cuda.synchronize()
    for a in range(2):
        _, sched, _ = LR.update_schedule(seq_lens[a], 256, 2, eager.seed, 0, a, False)
        steps = len(sched)
        print(f"policy {a}: eager {st_e[a]}\npolicy {a}: graph {st_g[a]}")
        assert st_e[a]["steps"] == st_g[a]["steps"] == steps >= 6 and st_e[a]["rows"] == st_g[a]["rows"] == T * N
        for what, ln in (("eager", eager), ("graph", graph)):
            d = ln._sgd[a]
            assert d.book.table[:steps, 5].tolist() == sched[:, 2].tolist(), f"{what} visited update_schedule's rows in its order"
            assert int(d.book.cursor.item()) == steps and int(d.optimizer.t.item()) == steps
        assert graph._sgd[a].book.captures == 1 and np.isfinite(st_g[a]["total_loss"])


def test_refusals():
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    ro, bank = _shared_rollout("fight", False)
    with pytest.raises(ValueError, match="flies fight mode"):
        _learner("escape").update_window(ro, bank)
    with pytest.raises(ValueError, match="a bank is needed"):
        _learner("fight").update_window(ro)
    w = World(make_config(n_arenas=8, level=3, seed=1, auto_reset=True, horizon=HORIZON), device=0)
    b2 = PolicyBank.trainable_init(torch.device("cuda", 0), mode="fight", seed=5, max_rows=16)
    with pytest.raises(RuntimeError, match="has not collected yet"):
        _learner("fight").update_window(PPORollout(w, b2, 4), b2)
    with pytest.raises(ValueError, match="unmasked view"):
        _learner("fight").update_window(PPORollout(w, b2, 4, semantics="masked").collect(), b2)
