"""Win / lose / draw of training episodes on the MI355X: hh_outcome_tap against the CPU oracle, hh_episode_outcomes on synthetic tables
against tests/outcome_ref.py, and outcomes=True on both rollouts — against a twin world stepped eagerly from the recorded actions with
episode_stats() read after every tick, against the restatement applied to the rollout's own done / outcome / tables, graph against
eager, default off, and save / resume.  Everything is compared byte for byte (the float64 means too: the restatement adds in the
kernel's order)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import outcome_ref as R
from outcome_fixtures import TICKS, fixture, world_kwargs

pytestmark = pytest.mark.gpu
N_PPO, T_PPO = 67, 16
N_HL, HORIZON_HL = 9, 20
TODAY_METRICS = {"episode_reward_mean", "episode_reward_min", "episode_reward_max", "episode_len_mean", "episode_len_min", "episode_len_max",
                 "episodes_this_iter", "timesteps_this_iter", "policy_reward_mean", "policy_reward_min", "policy_reward_max", "vf_explained_var",
                 "episodes_total", "timesteps_total"}
NEW_METRICS = {"agents_win", "opps_win", "draw", "outcome_pct", "episode_reward_mean_by_outcome", "episode_len_mean_by_outcome"}


def _np(t):
    return t.detach().cpu().numpy().copy()


def same_value(a, b):
    """dicts key by key, floats by their bits (nan == nan), everything else by type and value"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, float):
        return isinstance(b, float) and ((math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes())
    return type(a) is type(b) and a == b


def same_f64(a, b):
    """two float64 arrays: nan where nan, the same bytes elsewhere"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


# ------------------------------------------------------------------------------------------------------------------ 1. the tap
@pytest.mark.parametrize("n_arenas", [67, 1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_1_outcome_tap_after_every_step_is_the_oracles_poll(name, n_arenas):
    from hhmarl_2d_amd.world import World, make_config
    f = fixture(name, n_arenas)
    w = World(make_config(**world_kwargs(name, n_arenas)), device=0)
    w.reset()
    acts = torch.from_numpy(f["actions"].copy()).cuda()
    obs, rew, val, _ = w.alloc_outputs()
    done = torch.zeros((TICKS, n_arenas), dtype=torch.uint8, device="cuda")
    out = torch.full((TICKS, n_arenas), 7, dtype=torch.int8, device="cuda")
    for t in range(TICKS):
        w.step(acts[t], out=(obs, rew, val, done[t]))
        assert w.outcome_tap(done[t], out[t]) is not None
    torch.cuda.synchronize()
    assert _np(done).tobytes() == f["done"].tobytes(), "precondition: the HIP world follows the oracle"
    want = np.stack([R.tap(f["done"][t], f["polled"][t]) for t in range(TICKS)])
    assert _np(out).tobytes() == want.tobytes()
    assert _np(w.episode_stats()[2]).tobytes() == f["polled"][-1].tobytes(), "the tap only reads the world"
    if (name, n_arenas) == ("A", 67):
        got = _np(out)
        assert [(got == c).sum() for c in (1, -1, 0)] == [4, 7, 56] and (got == 2).sum() == TICKS * 67 - 67
    for bad_done, bad_out in ((done[0].to(torch.int8), out[0]), (done[0], out[0].to(torch.uint8)), (done[:2].reshape(-1), out[0]), (done[0], out[0].cpu())):
        with pytest.raises(ValueError, match="outcome_tap"):
            w.outcome_tap(bad_done, bad_out)


# ------------------------------------------------------------------------------------------------------------------ 2. the table
class Table:
    """a synthetic episode table on the device and hh_episode_outcomes over it"""

    def __init__(self, T, N, done, outcome, prefix, n_agents=2, seed=0):
        from hhmarl_2d_amd import _lib as L
        rng = np.random.default_rng(seed)
        self.T, self.N, self.nA, self.prefix = T, N, n_agents, prefix
        n_idx, _ = np.nonzero(done.T != 0)
        self.m = len(n_idx)
        self.e1 = prefix + self.m
        self.cap = prefix + T * N + 5
        self.done, self.outcome = done, outcome
        self.ep_arena = rng.integers(0, N, self.cap).astype(np.int32)
        self.ep_arena[prefix:self.e1] = n_idx
        self.ep_len = rng.integers(1, 301, self.cap).astype(np.int32)
        self.ep_return = rng.normal(0.0, 3.0, (self.cap, n_agents))
        self.ep_outcome = np.full(self.cap, 9, dtype=np.int8)
        self.ep_outcome[:prefix] = rng.choice(np.array([-1, 0, 1], dtype=np.int8), prefix)
        self.L = L

    def run(self, e1=None, ep_arena=None, times=1):
        """-> list of (ep_outcome, summary, flags) host copies, one per call (every call starts from the same table)"""
        L = self.L
        dev = torch.device("cuda", 0)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in (
            ("done", self.done), ("outcome", self.outcome), ("ep_arena", self.ep_arena if ep_arena is None else ep_arena), ("ep_len", self.ep_len),
            ("ep_return", self.ep_return), ("n", np.array([self.e1 if e1 is None else e1], dtype=np.int32)))}
        nbytes = C.c_int64(0)
        L.check(L.lib().hh_episode_outcomes_scratch_bytes(self.T, self.N, self.cap, C.byref(nbytes)))
        scratch = torch.zeros((nbytes.value // 8,), dtype=torch.float64, device=dev)
        outs = []
        for _ in range(times):
            eo = torch.from_numpy(self.ep_outcome.copy()).to(dev)
            summary = torch.full((12,), -7.0, dtype=torch.float64, device=dev)
            flags = torch.full((2,), -7, dtype=torch.int32, device=dev)
            b = L.HHEpisodeOutcomeBufs(T=self.T, N=self.N, n_agents=self.nA, reserved0=0, ep_cap=self.cap, done=d["done"].data_ptr(),
                                       outcome=d["outcome"].data_ptr(), n_episodes=d["n"].data_ptr(), ep_arena=d["ep_arena"].data_ptr(),
                                       ep_len=d["ep_len"].data_ptr(), ep_return=d["ep_return"].data_ptr(), ep_outcome=eo.data_ptr(),
                                       summary=summary.data_ptr(), flags=flags.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=nbytes.value)
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            L.check(L.lib().hh_episode_outcomes(C.byref(b), st))
            torch.cuda.synchronize()
            outs.append((_np(eo), _np(summary), _np(flags)))
        return outs

    def want(self, e1=None, ep_arena=None):
        e1 = self.e1 if e1 is None else e1
        eo, flags = R.fill(self.done, self.outcome, e1, self.ep_arena if ep_arena is None else ep_arena, self.ep_outcome)
        return eo, R.summary(e1, eo, self.ep_len, self.ep_return), flags


def _pattern(kind, T, N, rng):
    if kind == "none":
        return np.zeros((T, N), dtype=np.uint8)
    if kind == "all":
        return np.ones((T, N), dtype=np.uint8)
    return (rng.random((T, N)) < 0.3).astype(np.uint8)


@pytest.mark.parametrize("prefix", [0, 37])
@pytest.mark.parametrize("kind", ["none", "all", "random"])
@pytest.mark.parametrize("T,N", [(1, 1), (5, 67), (16, 130), (3, 1025)])
def test_2_episode_outcomes_on_synthetic_tables(T, N, kind, prefix):
    rng = np.random.default_rng(1000 * T + N)
    done = _pattern(kind, T, N, rng)
    outcome = rng.choice(np.array([-1, 0, 1], dtype=np.int8), (T, N))
    tab = Table(T, N, done, outcome, prefix, n_agents=3 if N == 130 else 2, seed=T + N)
    (eo, s, flags), (eo2, s2, flags2) = tab.run(times=2)
    w_eo, w_s, w_flags = tab.want()
    assert flags.tolist() == w_flags.tolist() == [0, tab.m]
    assert eo.tobytes() == w_eo.tobytes(), "ep_outcome: the window's segment, nothing before and nothing behind it"
    assert eo[:prefix].tobytes() == tab.ep_outcome[:prefix].tobytes() and (eo[tab.e1:] == 9).all()
    assert s[:4].tolist() == w_s[:4].tolist() and s[10] == 0 and s[11] == 0 and s[0] == tab.e1
    assert same_f64(s, w_s), f"summary {s} / {w_s}"
    for k in range(3):
        assert math.isnan(s[4 + k]) == (s[1 + k] == 0) == math.isnan(s[7 + k]), "a class without an episode gives nan"
    assert eo2.tobytes() == eo.tobytes() and s2.tobytes() == s.tobytes() and flags2.tobytes() == flags.tobytes(), "two runs: the same bytes"
    assert tab.m > 0 or kind == "none" or (T, N) == (1, 1)
    if tab.m == 0:
        assert s[0] == prefix
        return
    # one entry of another arena: flagged, nothing written (the summary is then over the table's bytes as they stand)
    bad = tab.ep_arena.copy()
    at = prefix + tab.m // 2
    bad[at] = (bad[at] + 1) % max(N, 2) if N > 1 else 1
    eo_b, s_b, flags_b = tab.run(ep_arena=bad)[0]
    assert flags_b.tolist() == [1, tab.m] and eo_b.tobytes() == tab.ep_outcome.tobytes()
    w_eo, w_s, w_flags = tab.want(ep_arena=bad)
    assert w_flags.tolist() == [1, tab.m] and same_f64(s_b, w_s) and s_b[10] == tab.m
    # e1 < m
    eo_c, _, flags_c = tab.run(e1=tab.m - 1)[0]
    assert flags_c.tolist() == [1, tab.m] and eo_c.tobytes() == tab.ep_outcome.tobytes()
    # a done row whose code is 2 is counted in slot 10
    n_idx, t_idx = np.nonzero(done.T != 0)
    oc2 = outcome.copy()
    oc2[t_idx[-1], n_idx[-1]] = 2
    tab2 = Table(T, N, done, oc2, prefix, n_agents=tab.nA, seed=T + N)
    eo_d, s_d, flags_d = tab2.run()[0]
    w_eo, w_s, _ = tab2.want()
    assert flags_d.tolist() == [0, tab.m] and eo_d.tobytes() == w_eo.tobytes() and eo_d[tab.e1 - 1] == 2
    assert s_d[10] == 1 and same_f64(s_d, w_s) and s_d[1:4].sum() == tab.e1 - 1


# ------------------------------------------------------------------------------------------------------------------ the rollouts
def build_ppo(horizon, level=3, **kw):
    from hhmarl_2d_amd import pilots
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    cfg = dict(n_arenas=N_PPO, level=level, seed=5, auto_reset=True, horizon=horizon, ext_opp_actions=level >= 4)
    w = World(make_config(**cfg), device=0)
    bank = pilots.PolicyBank.trainable_init(torch.device("cuda", 0), mode="fight", seed=5, max_rows=2 * N_PPO)
    objs = dict(world=w, bank=bank, _cfg=cfg)
    if level >= 4:
        opp = pilots.OpponentNets(w, seed=4, skip_first=False)
        objs.update(opponents=opp.bank, _keep=opp)
        kw["opponents"] = opp
    objs["rollout"] = PPORollout(w, bank, T_PPO, **kw)
    return objs


def build_commander(T, **kw):
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N_HL, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True,
                          horizon=HORIZON_HL), device=0)
    net = CommanderNet(0, 3 * N_HL).set_weights(random_weights(6))
    pilot = VariantNetPilot(w, seed=8)
    return dict(world=w, commander=net, pilots=pilot.bank, rollout=CommanderRollout(w, net, pilot, T, max_seq_len=7, **kw), _keep=pilot)


MODES = {"episodes": dict(batch_mode="complete_episodes", metrics=True), "window": dict(window_metrics=True)}


def saved(objs):
    return {k: v for k, v in objs.items() if not k.startswith("_")}


def consumer(ro):
    return ro.episodes if ro.episodes is not None else ro.window_metrics


def record(ro):
    """what outcomes=True holds after a collect, as host copies"""
    c = consumer(ro)
    m = c.metrics()
    table = c.rows() if ro.episodes is not None else c.episodes()
    md = c.metrics_device()
    rec = {k: _np(table[k]) for k in ("ep_arena", "ep_len", "ep_return", "ep_outcome")}
    rec.update(done=_np(ro.done), outcome=_np(ro.outcome), actions=_np(ro.actions), full=_np(md["ep_outcome"]), summary=_np(md["outcome_summary"]),
               flags=_np(md["outcome_flags"]), metrics=m)
    return rec


def same_record(a, b, what):
    for k in a:
        if k == "metrics":
            assert same_value(a[k], b[k]), f"{what}: metrics() {a[k]} / {b[k]}"
        elif k == "summary":
            assert same_f64(a[k], b[k]), f"{what}: summary"
        else:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{what}: {k}"


def check_against_ref(rec, before, what):
    """ep_outcome, the summary and the new metrics() keys are the restatement applied to the rollout's own done, outcome and tables"""
    e1 = len(rec["ep_arena"])
    assert rec["ep_outcome"].shape == (e1,) and rec["ep_outcome"].dtype == np.int8
    want_full, want_flags = R.fill(rec["done"], rec["outcome"], e1, rec["ep_arena"], before)
    assert rec["flags"].tolist() == want_flags.tolist() == [0, int((rec["done"] != 0).sum())], what
    assert rec["full"].tobytes() == want_full.tobytes(), f"{what}: ep_outcome"
    assert rec["ep_outcome"].tobytes() == want_full[:e1].tobytes()
    want_s = R.summary(e1, want_full, rec["ep_len"], rec["ep_return"])
    assert same_f64(rec["summary"], want_s), f"{what}: summary {rec['summary']} / {want_s}"
    want_m = R.metrics(want_s)
    assert set(rec["metrics"]) == TODAY_METRICS | NEW_METRICS
    for k in NEW_METRICS:
        assert same_value(rec["metrics"][k], want_m[k]), f"{what}: {k} {rec['metrics'][k]} / {want_m[k]}"
    assert rec["metrics"]["agents_win"] + rec["metrics"]["opps_win"] + rec["metrics"]["draw"] == e1 == rec["metrics"]["episodes_this_iter"]


def check_rows(rec, what):
    d = rec["done"] != 0
    assert np.isin(rec["outcome"][d], (-1, 0, 1)).all() and (rec["outcome"][~d] == 2).all(), f"{what}: done rows hold -1 / 0 / 1, the others 2"


class Twin:
    """a second World of the same configuration, stepped eagerly from the recorded actions, episode_stats() read after every tick"""

    def __init__(self, cfg, opp_seed=None):
        from hhmarl_2d_amd import pilots
        from hhmarl_2d_amd.world import World, make_config
        self.w = World(make_config(**cfg), device=0)
        self.nets = pilots.OpponentNets(self.w, seed=opp_seed, skip_first=False) if opp_seed is not None else None
        self.w.reset()

    def follow(self, rec, what):
        acts = torch.from_numpy(rec["actions"]).cuda()
        for t in range(acts.shape[0]):
            if self.nets is None:
                done = self.w.step(acts[t])[3]
            else:
                done = self.w.step_finish(self.nets(self.w.step_begin(acts[t], 0), None).contiguous())[3]
            done, polled = _np(done), _np(self.w.episode_stats()[2])
            assert done.tobytes() == rec["done"][t].tobytes(), f"{what}, tick {t}: the twin's done"
            assert R.tap(done, polled).tobytes() == rec["outcome"][t].tobytes(), f"{what}, tick {t}: outcome"


PPO_CASES = [(h, m) for h in (6, 60) for m in ("episodes", "accumulate", "window")]


def ppo_kwargs(horizon, mode):
    if mode == "accumulate":     # the first batch is still incomplete after two collects that emitted rows
        return dict(MODES["episodes"], train_batch_size={6: 2 * N_PPO * T_PPO + 1, 60: N_PPO * 60 + 1}[horizon])
    return dict(MODES[mode])


@pytest.mark.parametrize("horizon,mode", PPO_CASES)
def test_3_ppo_rollout_outcomes_twin_restatement_and_eager(horizon, mode):
    collects = {6: 5, 60: 8}[horizon]
    on = build_ppo(horizon, outcomes=True, **ppo_kwargs(horizon, mode))
    eager = build_ppo(horizon, outcomes=True, use_graph=False, **ppo_kwargs(horizon, mode))
    ro, re_ = on["rollout"], eager["rollout"]
    assert ro.outcome.dtype == torch.int8 and tuple(ro.outcome.shape) == (T_PPO, N_PPO)
    twin = Twin(on["_cfg"])
    seen, spanned = np.zeros(3, dtype=np.int64), 0
    for c in range(collects):
        before = _np(consumer(ro).ep_outcome)
        ro.collect()
        re_.collect()
        assert ro._graph is not None and re_._graph is None
        rec, what = record(ro), f"horizon {horizon}, {mode}, collect {c}"
        twin.follow(rec, what)
        check_rows(rec, what)
        check_against_ref(rec, before, what)
        same_record(record(re_), rec, what + ", eager against graph")
        seen += [(rec["outcome"] == code).sum() for code in (1, -1, 0)]
        if mode == "accumulate":
            spanned = max(spanned, ro.episodes.batch_info()["collects"])
    print(f"horizon {horizon}, {mode}: wins / losses / draws over {collects} collects: {seen.tolist()}")
    assert seen.sum() >= N_PPO, "precondition: every arena finished an episode"
    if mode == "accumulate":
        assert spanned >= 3, "precondition: a batch spanned three collects"


def test_3_level_4_goes_through_the_split_step():
    on = build_ppo(6, level=4, outcomes=True, window_metrics=True)
    ro = on["rollout"]
    assert ro.split
    before = _np(ro.window_metrics.ep_outcome)
    ro.collect()
    rec = record(ro)
    assert (rec["done"] != 0).sum() >= N_PPO, "precondition: every arena finished an episode"
    Twin(on["_cfg"], opp_seed=4).follow(rec, "level 4")
    check_rows(rec, "level 4")
    check_against_ref(rec, before, "level 4")


@pytest.mark.parametrize("mode", ["episodes", "window"])
def test_4_commander_rollout_one_step_collects_are_episode_stats(mode):
    runs = {g: build_commander(1, outcomes=True, use_graph=g, **MODES[mode]) for g in (True, False)}
    n_done = 0
    for c in range(8):
        recs = {}
        for g, objs in runs.items():
            ro = objs["rollout"]
            ro.collect()
            assert (ro._graph is not None) == g
            recs[g] = record(ro)
            polled = _np(objs["world"].episode_stats()[2])
            assert R.tap(recs[g]["done"][0], polled).tobytes() == recs[g]["outcome"][0].tobytes(), f"collect {c}, graph {g}"
        same_record(recs[False], recs[True], f"{mode} collect {c}, eager against graph")
        n_done += int((recs[True]["done"] != 0).sum())
    assert 0 < n_done < 8 * N_HL, "precondition: some steps end an episode, some do not"


@pytest.mark.parametrize("mode", ["episodes", "window"])
def test_4_commander_rollout_tables_and_metrics(mode):
    runs = {g: build_commander(4, outcomes=True, use_graph=g, **MODES[mode]) for g in (True, False)}
    ro = runs[True]["rollout"]
    n_done = 0
    for c in range(4):
        before = _np(consumer(ro).ep_outcome)
        for objs in runs.values():
            objs["rollout"].collect()
        rec, what = record(ro), f"commander {mode}, collect {c}"
        same_record(record(runs[False]["rollout"]), rec, what + ", eager against graph")
        check_rows(rec, what)
        check_against_ref(rec, before, what)
        assert list(rec["metrics"]["policy_reward_mean"]) == [1, 2, 3]
        n_done += int((rec["done"] != 0).sum())
    assert n_done >= N_HL, "precondition: every arena finished an episode"


# ------------------------------------------------------------------------------------------------------------------ 5. default off
def _key_sets(ro):
    sd = ro.state_dict()
    out = {"top": list(sd), "options": sorted(sd["options"]), "window": list(sd["window"])}
    for part in ("episodes", "window_metrics"):
        if sd.get(part) is not None:
            out[part] = {k: (sorted(v) if isinstance(v, dict) else None) for k, v in sd[part].items()}
    return out


@pytest.mark.parametrize("kind,mode", [(k, m) for k in ("ppo", "commander") for m in ("episodes", "window")])
def test_5_default_off_changes_nothing(kind, mode):
    make = (lambda **kw: build_ppo(6, **kw)) if kind == "ppo" else (lambda **kw: build_commander(4, **kw))
    plain, off, on = make(**MODES[mode]), make(outcomes=False, **MODES[mode]), make(outcomes=True, **MODES[mode])
    window = ("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target")
    for objs in (plain, off, on):
        for _ in range(2):
            objs["rollout"].collect()
    torch.cuda.synchronize()
    for objs in (plain, off):
        ro = objs["rollout"]
        assert getattr(ro, "outcome", None) is None
        c = consumer(ro)
        assert set(c.metrics()) == TODAY_METRICS and not hasattr(c, "ep_outcome") and c._outcomes is None
        assert "ep_outcome" not in c.metrics_device() and "ep_outcome" not in (c.rows() if ro.episodes is not None else c.episodes())
    assert _key_sets(plain["rollout"]) == _key_sets(off["rollout"])
    ks, ks_on = _key_sets(plain["rollout"]), _key_sets(on["rollout"])
    assert "outcomes" not in ks["options"] and "outcome" not in ks["window"]
    assert ks_on["options"] == sorted(ks["options"] + ["outcomes"]) and ks_on["window"] == ks["window"] + ["outcome"] and ks_on["top"] == ks["top"]
    part = "episodes" if mode == "episodes" else "window_metrics"
    assert ks_on[part]["options"] == sorted(ks[part]["options"] + ["outcomes"])
    assert ks_on[part]["state"] == sorted(ks[part]["state"] + ["outcome_flags", "outcome_summary"])
    table = "batch" if mode == "episodes" else "table"
    assert ks_on[part][table] == sorted(ks[part][table] + ["ep_outcome"])
    for k in window:       # the option does not change the window
        a, b, c_ = (_np(getattr(o["rollout"], k)) for o in (plain, off, on))
        assert a.tobytes() == b.tobytes() == c_.tobytes(), k
    m_on, m_off = consumer(on["rollout"]).metrics(), consumer(plain["rollout"]).metrics()
    assert all(same_value(m_on[k], m_off[k]) for k in m_off), "today's keys keep their values"
    for bad in (1, None):
        with pytest.raises(ValueError, match="outcomes: False or True"):
            make(outcomes=bad, **MODES[mode])
    with pytest.raises(ValueError, match="needs a consumer"):
        make(outcomes=True)


# ------------------------------------------------------------------------------------------------------------------ 6. resume
@pytest.mark.parametrize("kind", ["ppo", "commander"])
def test_6_a_resumed_run_equals_the_uninterrupted_one(kind, tmp_path):
    from hhmarl_2d_amd import checkpoint
    if kind == "ppo":
        kw = dict(MODES["episodes"], train_batch_size=2 * N_PPO * T_PPO + 1)
        make = lambda **more: build_ppo(6, **dict(kw, **more))
    else:
        make = lambda **more: build_commander(4, **dict(MODES["window"], **more))
    whole = make(outcomes=True)
    recs = []
    for _ in range(4):
        whole["rollout"].collect()
        recs.append(record(whole["rollout"]))
    assert sum(int((r["done"] != 0).sum()) for r in recs[2:]) > 0, "precondition: episodes end after the save point"
    first = make(outcomes=True)
    for c in range(2):
        first["rollout"].collect()
    same_record(record(first["rollout"]), recs[1], f"{kind}: the run to be saved")
    path = tmp_path / "run.ckpt"
    checkpoint.save(path, **saved(first))
    resumed = make(outcomes=True)
    checkpoint.load(path, **saved(resumed))
    same_record(record(resumed["rollout"]), recs[1], f"{kind}: right after the load")
    for c in (2, 3):
        before = _np(consumer(resumed["rollout"]).ep_outcome)
        resumed["rollout"].collect()
        rec = record(resumed["rollout"])
        same_record(rec, recs[c], f"{kind} collect {c}, resumed against uninterrupted")
        check_against_ref(rec, before, f"{kind} collect {c}, resumed")
    # a file saved with the other setting is refused by name, nothing changed
    other = make()
    with pytest.raises(ValueError, match="outcome"):
        checkpoint.load(path, **saved(other))
    assert other["rollout"].collects == 0 and not other["rollout"]._started
    state = record(resumed["rollout"])
    with pytest.raises(ValueError, match="outcome"):
        resumed["rollout"].load_state_dict(other["rollout"].state_dict())
    same_record(record(resumed["rollout"]), state, "a refused load changes nothing")
