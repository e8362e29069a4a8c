"""batch_mode = "complete_episodes" on the MI355X (train_hetero.py:212): PPORollout's EpisodeBatch after every collect against the
host restatement of tests/episodes_ref.py (the collects' own [T, N] buffers concatenated per arena, cut at the done
rows, oracle/gae_ref.compute_advantages with last_r = 0 per agent and whole episode) — bit for bit, every column, in emission
order — and its bookkeeping: every episode whole, from a reset row to its only done row, emitted exactly once."""
import numpy as np
import pytest
import torch

from episodes_ref import restate
from test_complete_episodes import IN_COLS, OUT_COLS

pytestmark = pytest.mark.gpu
TABLE = ("ep_start", "ep_len", "ep_arena")


def _rollout(N, T, horizon=30, level=3, mode="fight", seed=23, use_graph=True, batch_mode="complete_episodes"):
    from hhmarl_2d_amd import pilots
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    kw = dict(n_arenas=N, level=level, seed=seed, auto_reset=True, horizon=horizon, agent_mode=1 if mode == "escape" else 0)
    if level >= 4:
        kw["ext_opp_actions"] = True
    w = World(make_config(**kw), device=0)
    bank = PolicyBank.trainable_init(torch.device("cuda", 0), mode=mode, seed=5, max_rows=2 * N, tie_shared=False)
    opp = pilots.OpponentNets(w, seed=4, skip_first=False) if level >= 4 else None
    return PPORollout(w, bank, T, opponents=opp, use_graph=use_graph, batch_mode=batch_mode)


def _collect(ro, K):
    """K collects -> (the [T, N] buffers of each, the emitted batch of each (numpy), carried [N] after each)"""
    T = ro.T
    collects, emitted, carried = [], [], []
    for _ in range(K):
        ro.collect()
        torch.cuda.synchronize()
        collects.append({k: getattr(ro, k)[:T].cpu().numpy() for k in IN_COLS})
        if ro.episodes is not None:
            emitted.append({k: v.cpu().numpy() for k, v in ro.episodes.rows().items()})
            carried.append(ro.episodes.carried.cpu().numpy())
    return collects, emitted, carried


def _assert_equal_batches(got, want, what):
    for k in OUT_COLS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, f"{what}: {k} {got[k].shape} {got[k].dtype} vs {want[k].shape} {want[k].dtype}"
        assert np.array_equal(got[k], want[k]), f"{what}: column {k} differs from the restatement"


def _check_table(b):
    """the episode table describes the rows: one entry per episode, in row order"""
    starts = np.nonzero(b["t"] == 0)[0]
    ends = np.nonzero(b["done"])[0]
    assert len(b["ep_start"]) == len(starts) == len(ends)
    assert np.array_equal(b["ep_start"], starts) and np.array_equal(b["ep_len"], ends - starts + 1)
    assert np.array_equal(b["ep_arena"], b["arena"][starts])


def _check_against_restatement(ro, K):
    collects, emitted, carried = _collect(ro, K)
    want, want_carried = restate(collects, gamma=ro.gamma, lam=ro.lam)
    for i, (g, w) in enumerate(zip(emitted, want)):
        _assert_equal_batches(g, w, f"collect {i}")
        _check_table(g)
    cat = lambda bs: {k: np.concatenate([b[k] for b in bs], axis=0) for k in OUT_COLS}
    _assert_equal_batches(cat(emitted), cat(want), "all collects")
    assert np.array_equal(carried[-1], want_carried)
    return collects, emitted, carried


def _check_bookkeeping(collects, emitted, carried, T):
    K, N = len(collects), collects[0]["done"].shape[1]
    allb = {k: np.concatenate([b[k] for b in emitted], axis=0) for k in OUT_COLS}
    done = np.concatenate([c["done"] for c in collects], axis=0)          # [K T, N]
    # every emitted episode: t = 0, 1, ... from its first row, done = 1 on its last row only
    starts = np.nonzero(allb["t"] == 0)[0]
    bounds = np.append(starts, len(allb["t"]))
    for s, e in zip(bounds[:-1], bounds[1:]):
        assert np.array_equal(allb["t"][s:e], np.arange(e - s)) and allb["done"][e - 1] == 1 and not allb["done"][s:e - 1].any()
        assert (allb["arena"][s:e] == allb["arena"][s]).all() and (allb["episode"][s:e] == allb["episode"][s]).all()
    # no (arena, episode) twice; every episode that ended is emitted, numbered 0, 1, ... per arena from start()
    keys = allb["arena"][starts].astype(np.int64) * 1_000_000 + allb["episode"][starts]
    assert len(np.unique(keys)) == len(keys)
    ended = done.sum(axis=0)
    for n in range(N):
        eps = allb["episode"][starts][allb["arena"][starts] == n]
        assert np.array_equal(np.sort(eps), np.arange(ended[n])), n
    # an episode starts at a reset row: the first row after start() or the row after a done (its first obs is that row's)
    for n in np.unique(allb["arena"])[:64]:
        ends = np.nonzero(done[:, n])[0]
        first = np.concatenate([[0], ends[:-1] + 1])
        obs_stream = np.concatenate([c["obs"][:, n] for c in collects], axis=0)
        got = allb["obs"][starts][allb["arena"][starts] == n]
        assert np.array_equal(got, obs_stream[first]), n
    # rows emitted + rows carried = every row collected, per arena
    per_arena = np.bincount(allb["arena"], minlength=N)
    assert np.array_equal(per_arena + carried[-1], np.full(N, K * T))


def test_exact_against_the_host_restatement_and_bookkeeping():
    """N = 1536, level 3 fight, horizon 30, T = 24, K = 6: most episodes span two or three collects"""
    ro = _rollout(1536, 24)
    collects, emitted, carried = _check_against_restatement(ro, 6)
    _check_bookkeeping(collects, emitted, carried, 24)
    spans = [b["t"][b["done"] == 1] + 1 for b in emitted]
    assert max(int(s.max()) for s in spans if len(s)) > 24, "some episodes span collects"
    assert sum(len(b["t"]) for b in emitted) > 0.5 * 1536 * 24 * 6
    # the central critic's rows of the emitted batch
    rows = ro.episodes.critic_rows(1)
    last = ro.episodes.rows()
    assert rows.shape == (len(last["t"]), 57) and torch.equal(rows[:, 0], last["actions"][:, 0, 0].double().div(12.0).float())


@pytest.mark.parametrize("N,T,horizon,K", [(1536, 8, 30, 12), (1536, 70, 30, 3), (512, 1, 30, 80), (1000, 24, 30, 5), (777, 5, 8, 10)],
                         ids=["T8-spans-four", "T70-several-per-collect", "T1", "N1000", "runs-to-horizon"])
def test_edge_shapes(N, T, horizon, K):
    ro = _rollout(N, T, horizon=horizon, seed=31)
    collects, emitted, carried = _check_against_restatement(ro, K)
    _check_bookkeeping(collects, emitted, carried, T)
    lens = np.concatenate([b["t"][b["done"] == 1] + 1 for b in emitted])
    assert lens.max() <= horizon
    if T == 8:
        assert lens.max() > 3 * T, "an episode spans four collects"
    if T == 70:
        per = [np.bincount(b["arena"][b["done"] == 1], minlength=N).max() for b in emitted]
        assert max(per) >= 2, "several episodes of one arena in one collect"
    if horizon == 8:
        assert (lens == horizon).any() and max(int(c.max()) for c in carried) == horizon - 1, "episodes of exactly H rows, a carry of H - 1 rows"


def test_start_again_discards_the_carry():
    N, T = 1024, 16
    ro = _rollout(N, T, seed=41)
    _collect(ro, 3)
    assert int(ro.episodes.carried.max()) > 0
    ro.start()
    assert int(ro.episodes.carried.abs().sum()) == 0
    _check_against_restatement(ro, 4)     # after start(): no row of before, episodes numbered from 0 again


def test_buffers_unchanged_and_graph_equals_eager():
    N, T, K = 1024, 20, 4
    a, b = _rollout(N, T, seed=7), _rollout(N, T, seed=7, batch_mode="truncate_episodes")
    assert b.episodes is None
    ca, ea, _ = _collect(a, K)
    cb, _, _ = _collect(b, K)
    for i in range(K):
        for k in IN_COLS:
            assert np.array_equal(ca[i][k], cb[i][k]), (i, k)
    full = ("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target")
    for k in full:                        # the whole [T(+1), N] buffers, not only what the restatement reads
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    e = _rollout(N, T, seed=7, use_graph=False)
    _, ee, _ = _collect(e, K)
    for i in range(K):
        for k in OUT_COLS + TABLE:
            assert np.array_equal(ea[i][k], ee[i][k]), (i, k)


@pytest.mark.parametrize("level,mode", [(4, "fight"), (3, "escape")], ids=["L4-self-play", "L3-escape"])
def test_other_configs(level, mode):
    ro = _rollout(1536, 24, level=level, mode=mode, seed=29)
    collects, emitted, carried = _check_against_restatement(ro, 6)
    _check_bookkeeping(collects, emitted, carried, 24)
    assert emitted[-1]["obs"].shape[1:] == (2, 30 if mode == "escape" else 26)
