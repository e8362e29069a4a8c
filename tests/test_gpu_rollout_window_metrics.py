"""window_metrics=True on the MI355X: PPORollout (fight and escape: N = 64, T = 4, horizon 10, level 3, as tests/test_gpu_learner_window.py
sets its world up) and CommanderRollout (the world of tests/test_gpu_commander_learner_window.py with T below its horizon) in
batch_mode = "truncate_episodes", five collects each.

Preconditions on the five windows' done flags (`preconditions`; the seeds are chosen so that they hold): some episode spans at least
three windows, some window ends with every arena mid-episode, some arena ends two episodes in one window.  The commander's setup (T = 8,
seed 21) holds all three.  The 2-vs-2 setups hold the first two; the third CANNOT hold there: at level 3 with horizon 10 every episode
runs to the horizon (measured over eight world seeds, fight and escape: 128 episodes of exactly 10 rows each), and a window of 4 rows
cannot end two of them.  So that PPORollout meets the pattern too, one more setup, "fight-short", is the fight setup with horizon 3: its
episodes of 3 rows end twice in every third window (and it is held to that precondition alone).

(a) a twin rollout on an identically seeded world and sampler with batch_mode = "complete_episodes", metrics = True, whose window buffers
    are the same bytes (asserted first): in every collect episodes_this_iter, episode_len_min / max / mean, episodes_total and the
    multiset of (arena, length) are identical, timesteps_total = collects x T N, and the episode returns and reward means agree within
    the sum of both sides' reordering bounds of tests/episode_metrics_ref.py (the window's returns are the restatement's own sequential
    sums: their bound is 0).  vf_explained_var is deliberately NOT compared: the window's is over the window's rows (targets that
    bootstrap at the cut), the twin's over the emitted rows.
(b) metrics() and episodes() equal the stateful restatement (tests/window_metrics_ref.py) fed the window buffers read back after each
    collect: tables, counts, carry, totals, integer slots and min / max exactly, the means and vf_explained_var within its bounds.
(c) use_graph = True and use_graph = False give the same bytes.   (d) start() in mid-run clears the carry and the totals.
(e) with the option off `window_metrics` is None and the captured collect writes the bytes of a rollout built without the keyword (and
    the option does not change the window either).
(f) checkpoint.save after three collects, two more collects; loaded into fresh objects, two collects: metrics(), the tables and the
    carry are the same bytes."""
import math

import numpy as np
import pytest
import torch

from episode_metrics_ref import bounds, restate_metrics
from window_metrics_ref import WindowMetricsRef, window_bounds

pytestmark = pytest.mark.gpu
N, T, HORIZON, COLLECTS = 64, 4, 10, 5
N_HL, T_HL, HORIZON_HL = 64, 8, 150
SEEDS = {"fight": 23, "escape": 23, "fight-short": 23, "commander": 21}
KINDS = ("fight", "escape", "fight-short", "commander")
NEEDS = {"fight": ("spans", "mid"), "escape": ("spans", "mid"), "fight-short": ("two",), "commander": ("spans", "mid", "two")}
WINDOW = ("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target")


def build(kind, seed=None, **kw):
    """fresh objects of one setup -> dict: rollout, and world / sampler(s) under the names a checkpoint holds them by"""
    from hhmarl_2d_amd import _lib as L
    seed = SEEDS[kind] if seed is None else seed
    dev = torch.device("cuda", 0)
    if kind == "commander":
        from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
        from hhmarl_2d_amd.pilots import VariantNetPilot
        from hhmarl_2d_amd.world import World, make_config
        w = World(make_config(n_arenas=N_HL, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=seed, arena_offset=500, auto_reset=True,
                              horizon=HORIZON_HL), device=0)
        net = CommanderNet(0, 3 * N_HL).set_weights(random_weights(6))
        pilot = VariantNetPilot(w, seed=8)
        ro = CommanderRollout(w, net, pilot, T_HL, max_seq_len=7, **kw)
        return dict(world=w, commander=net, pilots=pilot.bank, rollout=ro, _keep=pilot)
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    mode = "escape" if kind == "escape" else "fight"
    w = World(make_config(n_arenas=N, level=3, seed=seed, auto_reset=True, horizon=3 if kind == "fight-short" else HORIZON,
                          agent_mode=1 if mode == "escape" else 0), device=0)
    bank = PolicyBank.trainable_init(dev, mode=mode, seed=5, max_rows=2 * N)
    return dict(world=w, bank=bank, rollout=PPORollout(w, bank, T, **kw))


def saved(objs):
    return {k: v for k, v in objs.items() if not k.startswith("_")}


def _np(t):
    return t.detach().cpu().numpy().copy()


def window_of(ro):
    torch.cuda.synchronize()
    return {k: _np(getattr(ro, k)) for k in WINDOW + (("state_in",) if hasattr(ro, "state_in") else ())}


def wm_record(ro):
    """everything the option holds after a collect, as host copies"""
    wm = ro.window_metrics
    rec = {"metrics": wm.metrics(), "episodes": {k: _np(v) for k, v in wm.episodes().items()}}
    rec.update({k: _np(getattr(wm, k)) for k in ("run_return", "run_len", "counts", "_summary", "_totals")})
    return rec


def same_record(a, b, what):
    for k in ("run_return", "run_len", "counts", "_summary", "_totals"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{what}: {k}"
    for k in a["episodes"]:
        assert a["episodes"][k].tobytes() == b["episodes"][k].tobytes(), f"{what}: {k}"
    assert same_metrics(a["metrics"], b["metrics"]), f"{what}: metrics() {a['metrics']} / {b['metrics']}"


def same_metrics(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_metrics(a[k], b[k]) for k in a)
    if isinstance(a, float):
        return isinstance(b, float) and ((math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes())
    return type(a) is type(b) and a == b


def preconditions(done, needs=("spans", "mid", "two")):
    """done: bool [collects, T, N] of successive windows -> the preconditions of the module docstring that the setup is held to"""
    C_, T_, N_ = done.shape
    flat = done.reshape(C_ * T_, N_)
    spans = False
    for n in range(N_):
        ends = np.flatnonzero(flat[:, n])
        starts = np.concatenate([[0], ends[:-1] + 1])
        spans = spans or any(e // T_ - s // T_ >= 2 for s, e in zip(starts, ends))
    assert spans or "spans" not in needs, "some episode spans at least three windows"
    assert any(not done[c, T_ - 1].any() for c in range(C_)) or "mid" not in needs, "some window ends with every arena mid-episode"
    assert (done.sum(axis=1) >= 2).any() or "two" not in needs, "some arena ends two episodes in one window"


_MAIN = {}


def main_run(kind):
    """the option's rollout (captured graph) next to its complete-episodes twin, five collects, recorded once per kind"""
    if kind not in _MAIN:
        on, twin = build(kind, window_metrics=True), build(kind, batch_mode="complete_episodes", metrics=True)
        ro, tw = on["rollout"], twin["rollout"]
        assert ro.window_metrics is not None and ro.episodes is None and ro.batch_mode == "truncate_episodes" and tw.window_metrics is None
        recs = []
        for _ in range(COLLECTS):
            ro.collect()
            tw.collect()
            rows = {k: _np(v) for k, v in tw.episodes.rows().items() if k in ("reward", "vf", "target", "ep_start", "ep_len", "ep_arena", "ep_return")}
            recs.append({"window": window_of(ro), "twin_window": window_of(tw), "wm": wm_record(ro), "twin_metrics": tw.episodes.metrics(), "twin_rows": rows})
        preconditions(np.stack([r["window"]["done"] for r in recs]) != 0, NEEDS[kind])
        _MAIN[kind] = (on, recs)
    return _MAIN[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_a_the_complete_episodes_twin_agrees(kind):
    _, recs = main_run(kind)
    TN = recs[0]["window"]["done"].size
    for c, r in enumerate(recs):
        for k in r["window"]:
            assert r["window"][k].tobytes() == r["twin_window"][k].tobytes(), f"precondition: collect {c}: the twin's {k} is another window"
        m, tm, ep, rows = r["wm"]["metrics"], r["twin_metrics"], r["wm"]["episodes"], r["twin_rows"]
        assert list(m) == list(tm) and all(type(m[k]) is type(tm[k]) for k in m), "the keys and types of EpisodeBatch.metrics()"
        assert all(list(m[k]) == list(tm[k]) for k in m if isinstance(m[k], dict)), "the same AGENT_KEYS"
        for k in ("episodes_this_iter", "episode_len_min", "episode_len_max", "episode_len_mean", "episodes_total"):
            assert same_metrics(m[k], tm[k]), f"collect {c}: {k} {m[k]} / {tm[k]}"
        assert m["timesteps_total"] == (c + 1) * TN and m["timesteps_this_iter"] == TN
        E = m["episodes_this_iter"]
        assert sorted(zip(ep["ep_arena"].tolist(), ep["ep_len"].tolist())) == sorted(zip(rows["ep_arena"].tolist(), rows["ep_len"].tolist()))
        assert ep["ep_arena"].tolist() == rows["ep_arena"].tolist() and ep["ep_len"].tolist() == rows["ep_len"].tolist(), "arena-major, then time: the same order"
        if E == 0:
            assert math.isnan(m["episode_reward_mean"]) and math.isnan(tm["episode_reward_mean"])
            continue
        ref = restate_metrics(rows["reward"], rows["vf"], rows["target"], rows["ep_start"], rows["ep_len"])
        b = bounds(rows["reward"], rows["ep_start"], rows["ep_len"], ref)          # the twin's side: its sums run in another order
        own = window_bounds({"ep_return": ep["ep_return"], "episode_reward": ref["episode_reward"], "rows": TN, "ep_len": ep["ep_len"]},
                            r["window"]["vf"], r["window"]["target"])                 # the window's side: only its means' own summation
        err = np.abs(ep["ep_return"] - rows["ep_return"])
        print(f"{kind} collect {c}: {E} episodes, ep_return max err {err.max():.3e} (bound there {b['ep_return'].flat[err.argmax()]:.3e})")
        assert (err <= b["ep_return"]).all()
        assert abs(m["episode_reward_mean"] - tm["episode_reward_mean"]) <= b["episode_reward_mean"] + own["episode_reward_mean"]
        for k in ("episode_reward_min", "episode_reward_max"):
            assert abs(m[k] - tm[k]) <= b["episode_reward"].max()
        for a, key in enumerate(m["policy_reward_mean"]):
            assert abs(m["policy_reward_mean"][key] - tm["policy_reward_mean"][key]) <= b["agent_return_mean"][a] + own["agent_return_mean"][a]
            for k in ("policy_reward_min", "policy_reward_max"):
                assert abs(m[k][key] - tm[k][key]) <= b["ep_return"][:, a].max()


@pytest.mark.parametrize("kind", KINDS)
def test_b_metrics_and_episodes_are_the_restatement_on_the_windows(kind):
    on, recs = main_run(kind)
    keys = list(on["rollout"].window_metrics.AGENT_KEYS)
    nA = len(keys)
    ref = WindowMetricsRef(recs[0]["window"]["done"].shape[1], nA)
    for c, r in enumerate(recs):
        w, rec = r["window"], r["wm"]
        want = ref.window(w["reward"], w["vf"], w["target"], w["done"])
        E, m, tag = int(want["episodes"]), rec["metrics"], f"{kind} collect {c}"
        for k in ("ep_return", "ep_len", "ep_arena", "ep_end"):
            assert rec["episodes"][k].dtype == want[k].dtype and rec["episodes"][k].tobytes() == want[k].tobytes(), f"{tag}: {k}"
        assert rec["counts"].tolist() == want["counts"].tolist() and rec["_totals"].tolist() == want["totals"].tolist(), tag
        assert rec["run_return"].tobytes() == want["run_return"].tobytes() and rec["run_len"].tobytes() == want["run_len"].tobytes(), tag
        assert m["episodes_this_iter"] == E and m["timesteps_this_iter"] == want["rows"] and m["episodes_total"] == want["totals"][0]
        assert m["timesteps_total"] == want["totals"][1] and isinstance(m["episodes_this_iter"], int) and isinstance(m["timesteps_total"], int)
        b = window_bounds(want, w["vf"], w["target"])
        for k in ("episode_reward_min", "episode_reward_max", "episode_len_min", "episode_len_max"):
            assert same_metrics(m[k], float(want[k])), f"{tag}: {k}"
        for a, key in enumerate(keys):
            assert same_metrics(m["policy_reward_min"][key], float(want["agent_return_min"][a])), tag
            assert same_metrics(m["policy_reward_max"][key], float(want["agent_return_max"][a])), tag
        if E:
            assert abs(m["episode_reward_mean"] - want["episode_reward_mean"]) <= b["episode_reward_mean"], tag
            assert abs(m["episode_len_mean"] - want["episode_len_mean"]) <= b["episode_len_mean"], tag
            for a, key in enumerate(keys):
                assert abs(m["policy_reward_mean"][key] - want["agent_return_mean"][a]) <= b["agent_return_mean"][a], tag
        else:
            assert math.isnan(m["episode_reward_mean"]) and math.isnan(m["episode_len_mean"]) and all(math.isnan(v) for v in m["policy_reward_mean"].values())
        ev = np.array([m["vf_explained_var"][key] for key in keys])
        err = np.abs(ev - want["vf_explained_var"])
        print(f"{tag}: {E} episodes, vf_explained_var {ev}, error {err}, bound {b['vf_explained_var']}")
        assert np.isfinite(ev).all() and (err <= b["vf_explained_var"]).all(), tag


@pytest.mark.parametrize("kind", KINDS)
def test_c_d_eager_gives_the_graphs_bytes_and_start_clears_the_state(kind):
    _, recs = main_run(kind)
    eager = build(kind, window_metrics=True, use_graph=False)
    ro = eager["rollout"]
    for c in range(2):                                              # 8 / 16 steps: no setup's episodes all end there
        ro.collect()
        assert ro._graph is None
        w = window_of(ro)
        assert all(w[k].tobytes() == recs[c]["window"][k].tobytes() for k in w), f"collect {c}: the eager window"
        same_record(wm_record(ro), recs[c]["wm"], f"{kind} collect {c}, eager against graph")
    wm = ro.window_metrics
    # something to clear: every setup is mid-episode after two windows (the returns so far may still be 0.0: sparse rewards)
    assert int(wm.run_len.max()) > 0 and recs[1]["wm"]["metrics"]["timesteps_total"] > 0 and wm._totals.tolist()[1] > 0
    print(f"{kind}: before start() the carry holds up to {int(wm.run_len.max())} rows, |run_return| sums to {wm.run_return.abs().sum().item():.6g}")
    ro.start()                                                      # (d) in mid-run
    torch.cuda.synchronize()
    assert not wm.run_len.any().item() and not wm.run_return.any().item() and wm._totals.tolist() == [0, 0] and wm.counts.tolist() == [0, 0]
    m = wm.metrics()
    assert m["episodes_this_iter"] == 0 and m["timesteps_this_iter"] == 0 and m["episodes_total"] == 0 and m["timesteps_total"] == 0
    assert math.isnan(m["episode_reward_mean"]) and all(math.isnan(v) for v in m["vf_explained_var"].values())
    assert all(v.shape[0] == 0 for v in wm.episodes().values())
    ro.collect()
    w = window_of(ro)
    want = WindowMetricsRef(w["done"].shape[1], wm.n_agents).window(w["reward"], w["vf"], w["target"], w["done"])
    got = wm_record(ro)
    assert got["run_return"].tobytes() == want["run_return"].tobytes() and got["run_len"].tobytes() == want["run_len"].tobytes()
    assert got["_totals"].tolist() == [int(want["episodes"]), w["done"].size] and got["episodes"]["ep_return"].tobytes() == want["ep_return"].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_e_default_off_is_the_rollout_without_the_keyword(kind):
    _, recs = main_run(kind)
    plain, off = build(kind), build(kind, window_metrics=False)
    for objs in (plain, off):
        assert objs["rollout"].window_metrics is None and "window_metrics" not in objs["rollout"].state_dict()
    for c in range(2):
        plain["rollout"].collect()
        off["rollout"].collect()
        a, b = window_of(plain["rollout"]), window_of(off["rollout"])
        assert plain["rollout"]._graph is not None and off["rollout"]._graph is not None
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), f"collect {c}: {k}"
            assert a[k].tobytes() == recs[c]["window"][k].tobytes(), f"collect {c}: {k} with the option on"
    assert list(plain["rollout"].state_dict()) == ["options", "window", "collects", "started", "episodes"]
    assert plain["rollout"]._options() == build(kind, window_metrics=True)["rollout"]._options()


@pytest.mark.parametrize("kind", KINDS)
def test_f_a_resumed_run_reports_the_same_metrics(kind, tmp_path):
    from hhmarl_2d_amd import checkpoint
    _, recs = main_run(kind)
    first = build(kind, window_metrics=True)
    for c in range(3):
        first["rollout"].collect()
    same_record(wm_record(first["rollout"]), recs[2]["wm"], f"{kind}: the run to be saved")
    path = tmp_path / "run.ckpt"
    checkpoint.save(path, **saved(first))
    sd = first["rollout"].state_dict()
    assert list(sd)[-1] == "window_metrics" and list(sd["window_metrics"]) == ["options", "state", "table"]
    resumed = build(kind, window_metrics=True)
    checkpoint.load(path, **saved(resumed))
    same_record(wm_record(resumed["rollout"]), recs[2]["wm"], f"{kind}: right after the load")
    for c in (3, 4):
        resumed["rollout"].collect()
        w = window_of(resumed["rollout"])
        assert all(w[k].tobytes() == recs[c]["window"][k].tobytes() for k in w), f"collect {c}: the resumed window"
        same_record(wm_record(resumed["rollout"]), recs[c]["wm"], f"{kind} collect {c}, resumed against uninterrupted")
    # the option in the other position: refused by name, nothing changed
    other = build(kind)
    with pytest.raises(ValueError, match="window_metrics"):
        checkpoint.load(path, **saved(other))
    assert other["rollout"].collects == 0 and not other["rollout"]._started
    plain_sd = other["rollout"].state_dict()
    before = wm_record(resumed["rollout"])
    with pytest.raises(ValueError, match="window_metrics"):
        resumed["rollout"].load_state_dict(plain_sd)
    same_record(wm_record(resumed["rollout"]), before, "a refused load changes nothing")
