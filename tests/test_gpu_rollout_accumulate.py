"""PPORollout / CommanderRollout with train_batch_size on the MI355X, on small worlds (N = 64, T = 8, horizon 20): the accumulating
rollout's batch after every collect is, byte for byte, the shifted concatenation (tests/episodes_accumulate_ref.py) of the per-collect
batches of a rollout WITHOUT train_batch_size on a world of the same seed (collects are deterministic through the keyed RNG); graph and
eager collects give the same bytes; collect_batch() stops at the first collect with rows >= B; and one learner update on a ready batch
reports the accumulated rows."""
import numpy as np
import pytest
import torch

from episodes_accumulate_ref import accumulate

pytestmark = pytest.mark.gpu
N, T_STEPS, HORIZON, K, B = 64, 8, 20, 12, 2000   # B: more than any one collect emits (at most 64 x 20 rows), so batches span collects


def _ppo(train_batch_size, use_graph=True):
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, level=3, seed=23, auto_reset=True, horizon=HORIZON), device=0)
    bank = PolicyBank.trainable_init(torch.device("cuda", 0), mode="fight", seed=5, max_rows=2 * N)
    return PPORollout(w, bank, T_STEPS, use_graph=use_graph, batch_mode="complete_episodes", train_batch_size=train_batch_size), bank


def _commander(train_batch_size, use_graph=True):
    """the fixture of tests/test_gpu_commander_learner.py: random CommanderGru weights (seed 6), VariantNetPilot (seed 8)"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True,
                          horizon=HORIZON), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    ro = CommanderRollout(w, net, VariantNetPilot(w, seed=8), T_STEPS, use_graph=use_graph, batch_mode="complete_episodes", max_seq_len=20,
                          train_batch_size=train_batch_size)
    return ro, net


MAKE = {"ppo": _ppo, "commander": _commander}


def _numpy(rows):
    return {k: v.cpu().numpy() for k, v in rows.items()}


@pytest.fixture(scope="module")
def reference():
    """per rollout kind: the K per-collect batches of the rollout without train_batch_size and their accumulation to B (computed once,
    never modified)"""
    out = {}
    for kind, make in MAKE.items():
        ro, _ = make(None)
        assert ro.episodes.train_batch_size is None and ro.episodes._acc is None
        per = []
        for _ in range(K):
            ro.collect()
            per.append(_numpy(ro.episodes.rows()))
        ref = accumulate(per, B)
        rows = [len(p["t"]) for p in per]
        print(f"{kind}: rows per collect {rows}, acc after each {[r[1].tolist() for r in ref]}")
        assert ref[-1][1][6] >= 1 and any(r[1][5] >= 2 and r[1][4] for r in ref), f"{kind}: B = {B} must complete a batch of several collects: {rows}"
        out[kind] = (per, ref)
    return out


def _check(ro, entry, what):
    batch, acc, counts = entry
    got = _numpy(ro.episodes.rows())
    assert set(got) == set(batch), what
    for k in batch:
        assert got[k].dtype == batch[k].dtype and got[k].shape == batch[k].shape, f"{what}: {k} {got[k].shape} vs {batch[k].shape}"
        assert got[k].tobytes() == batch[k].tobytes(), f"{what}: {k} differs from the shifted concatenation"
    assert ro.episodes._acc.cpu().tolist() == acc.tolist(), what
    info = ro.episodes.batch_info()
    assert (info["rows"], info["episodes"], info["collects"], info["batches"]) == (acc[0], acc[1], acc[5], acc[6]) and ro.episodes.ready() == bool(acc[4])
    if "seq_start" in batch:
        seqs = ro.episodes.sequences()
        assert seqs["obs"].shape[0] == acc[3] == info["sequences"] and int(seqs["mask"].sum()) == acc[0]
    return got


@pytest.mark.parametrize("kind", list(MAKE))
def test_accumulated_batch_is_the_shifted_concatenation_graph_and_eager(reference, kind):
    per, ref = reference[kind]
    graph, eager = MAKE[kind](B)[0], MAKE[kind](B, use_graph=False)[0]
    for k in range(K):
        graph.collect()
        eager.collect()
        g = _check(graph, ref[k], f"{kind} collect {k} (graph)")
        e = _check(eager, ref[k], f"{kind} collect {k} (eager)")
        assert all(g[name].tobytes() == e[name].tobytes() for name in g)
    assert graph._graph is not None and eager._graph is None


@pytest.mark.parametrize("kind", list(MAKE))
def test_collect_batch_stops_at_the_first_collect_that_reaches_b(reference, kind):
    per, ref = reference[kind]
    done = [k for k in range(K) if ref[k][1][4]]
    first = done[0]
    ro = MAKE[kind](B)[0]
    assert ro.collect_batch(max_collects=1) is ro and not ro.episodes.ready() and first > 0, "one collect does not reach B"
    assert ro.episodes.batch_info()["collects"] == 1
    ro.collect_batch()                           # goes on with the partial batch
    _check(ro, ref[first], f"{kind} collect_batch()")
    info = ro.episodes.batch_info()
    assert info["collects"] == first + 1 and info["rows"] >= B > ref[first - 1][1][0] and info["batches"] == 0
    if len(done) > 1:                            # the next call starts the next batch by itself
        ro.collect_batch()
        _check(ro, ref[done[1]], f"{kind} second collect_batch()")
        assert ro.episodes.batch_info()["batches"] == 1
    with pytest.raises(RuntimeError, match="train_batch_size"):
        MAKE[kind](None)[0].collect_batch()


def test_ppo_learner_updates_on_a_ready_batch():
    from hhmarl_2d_amd.learner import PPOLearner
    ro, bank = _ppo(B)
    learner = PPOLearner.trainable_init(torch.device("cuda", 0), mode="fight", seed=5, num_sgd_iter=1, sgd_minibatch_size=256)
    ro.collect_batch()
    info = ro.episodes.batch_info()
    assert ro.episodes.ready() and info["rows"] >= B and info["collects"] >= 2
    stats = learner.update(ro.episodes, bank)
    assert len(stats) == 2
    for st in stats:
        assert st["rows"] == info["rows"] and st["steps"] >= 1
        assert all(np.isfinite(st[k]) for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "kl_coeff")), st
    assert ro.episodes.batch_info() == info, "the update reads the batch, it does not consume it"


def test_commander_learner_updates_on_a_ready_batch():
    from hhmarl_2d_amd.learner import CommanderLearner
    ro, net = _commander(B)
    learner = CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, num_sgd_iter=1)
    ro.collect_batch()
    info = ro.episodes.batch_info()
    assert ro.episodes.ready() and info["rows"] >= B and info["collects"] >= 2
    st = learner.update(ro.episodes, net)
    assert st["rows"] == 3 * info["rows"] and st["steps"] >= 1, "rows: unpadded, all three agents"
    assert all(np.isfinite(st[k]) for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "kl_coeff")), st
