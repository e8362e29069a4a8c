"""hh_world_snapshot / hh_world_restore on the MI355X (World.snapshot / restore): a world restored from a snapshot — the same world, or a
freshly created one that was never reset — runs on exactly as the original did: observations, rewards, valid, done, the statistics of
finished episodes, eval_info, the sticky action-fault flags, the level-5 policy draw and the macro-step tick counter, tick by tick.

Every world steps K ticks (HighLevelEnv: commander steps, the save point INSIDE one, six sub-steps in), is saved, and steps M more with
recorded actions.  Actions before the save point steer at the nearest opponent and shoot (helpers.pursuit_actions, from a seeded
generator) so that aircraft die and rockets fly; short horizons make every arena reset at least once before the save.  The save point's
preconditions are asserted (and were checked with the CPU oracle when the seeds and tick counts were picked)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import pursuit_actions

pytestmark = pytest.mark.gpu

HORIZON_LL, K_LL, M_LL = 40, 64, 24          # LowLevelEnv: every arena has finished an episode by tick 40; the M ticks cross tick 80
HORIZON_HL, K_HL, SUB_HL, M_HL = 64, 8, 6, 6  # HighLevelEnv: 8 commander steps and 6 sub-steps of the ninth, then 6 more commander steps
FAULT_TICK, FAULT_ARENA = 3, 5               # one out-of-range action word before the save point: the arena's sticky flag
FAULT_STEP_HL = 0                            # HighLevelEnv: in the first sub-step of the first commander step (every aircraft alive: the word is consumed)

CASES = {
    "level3_fight": dict(n_arenas=48, level=3, horizon=HORIZON_LL, auto_reset=True, seed=11),
    "level5_ext_opp": dict(n_arenas=48, level=5, horizon=HORIZON_LL, auto_reset=True, seed=12, ext_opp_actions=True),
    "escape": dict(n_arenas=48, level=3, agent_mode=1, horizon=HORIZON_LL, auto_reset=True, seed=13),
    "hl_3v3": dict(n_arenas=40, env_kind=1, n_agents=3, n_opps=3, horizon=HORIZON_HL, auto_reset=True, seed=14),
    "hl_5v5_ten_slot": dict(n_arenas=24, env_kind=1, n_agents=5, n_opps=5, horizon=HORIZON_HL, auto_reset=True, seed=15),
}


def _world(name, **over):
    from hhmarl_2d_amd.world import World, make_config
    return World(make_config(**dict(CASES[name], **over)), device=0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _read(w):
    """everything a caller can read of a world without stepping it"""
    out = [x.cpu().numpy() for x in w.episode_stats()] + [x.cpu().numpy() for x in w.eval_info()]
    out += [w.action_faults().cpu().numpy(), w.opp_policy().cpu().numpy(), w.arena_status().cpu().numpy()]
    if w.cfg.env_kind == 1:
        out += [np.asarray(w.hl_tick_count()), w.hl_commands()]
    return out


class LowLevel:
    """ticks of hh_step; actions[t] int8 [N, n_ctrl, 4]"""

    @staticmethod
    def before(w, rng):
        acts = []
        for t in range(K_LL):
            a = pursuit_actions(rng, w.get_state(), 2, w.n_ctrl)
            if t == FAULT_TICK:
                a[FAULT_ARENA, 0, 0] = 20          # heading component outside [0, 12]: sanitised, the arena's flag set
            w.step(_dev(a))
            acts.append(a)
        return acts

    @staticmethod
    def after(w, rng=None, actions=None):
        rec, acts = [], []
        for t in range(M_LL):
            a = actions[t] if actions is not None else pursuit_actions(rng, w.get_state(), 2, w.n_ctrl)
            out = w.step(_dev(a))
            rec.append([x.cpu().numpy() for x in out] + _read(w))
            acts.append(a)
        return rec, acts


class HighLevel:
    """commander steps in their phases (hh_hl_begin, 16 x (hh_hl_agents_act, hh_hl_tick), hh_hl_end); actions[t] = (cmd, [16 x int8 [N, A, 4]])"""

    @staticmethod
    def _step(w, rng, given, first_sub=0, last_sub=16, end=True):
        cmd, subs = given if given is not None else (rng.integers(0, 3, size=(w.N, w.n_agents)).astype(np.int8), [None] * 16)
        subs = list(subs)
        if first_sub == 0:
            w.hl_begin(_dev(cmd))
        for k in range(first_sub, last_sub):
            if subs[k] is None:
                subs[k] = pursuit_actions(rng, w.get_state(), w.n_agents, w.A)
            a = _dev(subs[k])
            w.hl_agents_act(a)
            w.hl_tick(a)
        return (cmd, subs), (w.hl_end() if end else None)

    @classmethod
    def before(cls, w, rng):
        for t in range(K_HL):
            if t == FAULT_STEP_HL:
                cmd = rng.integers(0, 3, size=(w.N, w.n_agents)).astype(np.int8)
                subs = [pursuit_actions(rng, w.get_state(), w.n_agents, w.A)] * 16
                subs[0] = subs[0].copy()
                subs[0][FAULT_ARENA, 0, 1] = 11     # speed component outside [0, 8]
                cls._step(w, rng, (cmd, subs))
            else:
                cls._step(w, rng, None)
        open_step, _ = cls._step(w, rng, None, 0, SUB_HL, end=False)      # the save point: inside the ninth commander step
        return open_step

    @classmethod
    def after(cls, w, rng=None, actions=None, open_step=None):
        rec, acts = [], []
        given = actions[0] if actions is not None else open_step
        for t in range(M_HL + 1):
            g, out = cls._step(w, rng, given, SUB_HL if t == 0 else 0)
            rec.append([x.cpu().numpy() for x in out] + _read(w))
            acts.append(g)
            given = actions[t + 1] if actions is not None and t + 1 < len(actions) else None
        return rec, acts


_RUNS = {}


def _run(name):
    """one uninterrupted run per case, shared: the world at its save point is not kept — (blob, host state at the save point, the actions
    of the M ticks, what they recorded)"""
    if name not in _RUNS:
        w = _world(name)
        drv = HighLevel if w.cfg.env_kind == 1 else LowLevel
        rng = np.random.default_rng(7)
        w.reset()
        open_step = drv.before(w, rng)
        st = w.get_state()
        at_save = _read(w)
        blob = w.snapshot()
        assert blob.dtype == torch.uint8 and blob.device.type == "cpu" and bytes(blob[:4].tolist()) == b"HHSW"
        # the save point is not a trivial one
        steps, alive = st["ar_i"][:, 0], st["ac_i"][:, :, 0]
        n_units = w.cfg.n_agents + w.cfg.n_opps
        running = (steps > 0) & (st["ar_i"][:, 1] > 0) & (st["ar_i"][:, 2] > 0)
        assert running.any(), "an arena is mid-episode"
        assert (st["rk_i"][:, :, 0] > 0).any(), "a rocket is in flight"
        assert ((alive[:, :n_units] == 0).any(axis=1) & running).any(), "a running arena has a dead aircraft"
        finished = at_save[2] != 2
        assert finished.all() if w.cfg.env_kind == 0 else finished.any(), "arenas have finished an episode (episode_stats hold one)"
        assert at_save[5][FAULT_ARENA] == 1 and at_save[5].sum() == 1, "exactly the arena that was fed a bad action word is flagged"
        if w.cfg.env_kind == 1:
            assert at_save[4].any() and at_save[8] > 0, "eval_info totals and the tick counter have counted"
            assert int((w.hl_commands() != 0).sum()) > 0, "commands of the step in flight are set"
        if name == "level5_ext_opp":
            assert len(np.unique(at_save[6])) > 1, "the level-5 draw differs between arenas"
        if drv is HighLevel:
            rec, acts = drv.after(w, rng, open_step=open_step)
        else:
            rec, acts = drv.after(w, rng)
        assert sum(int(r[3].sum()) for r in rec) > 0, "episodes end after the save point as well"
        _RUNS[name] = (blob, st, acts, rec, w)
    return _RUNS[name]


def _same(got, want, what):
    assert len(got) == len(want)
    for t, (g, x) in enumerate(zip(got, want)):
        assert len(g) == len(x)
        for i, (a, b) in enumerate(zip(g, x)):
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), f"{what}: tick {t}, record {i} differs"


def _replay(w, acts):
    drv = HighLevel if w.cfg.env_kind == 1 else LowLevel
    return drv.after(w, actions=acts)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_restore_into_the_same_world_replays_the_run(name):
    blob, _, acts, rec, w = _run(name)
    w.restore(blob)
    _same(_replay(w, acts), rec, name)
    assert torch.equal(w.snapshot()[:208], blob[:208]), "the header does not depend on the state"


@pytest.mark.parametrize("name", list(CASES))
def test_restore_into_a_fresh_world_replays_the_run(name):
    blob, _, acts, rec, _ = _run(name)
    fresh = _world(name)                     # never reset
    fresh.restore(blob)
    assert torch.equal(fresh.snapshot(), blob), "a restored world's snapshot is the blob, byte for byte"
    _same(_replay(fresh, acts), rec, name)


def test_state_dict_round_trip():
    blob, _, acts, rec, _ = _run("level3_fight")
    fresh = _world("level3_fight")
    fresh.load_state_dict({"blob": blob})
    assert torch.equal(fresh.state_dict()["blob"], blob)
    with pytest.raises(ValueError, match="unexpected `extra`"):
        fresh.load_state_dict({"blob": blob, "extra": 1})
    with pytest.raises(ValueError, match="truncated"):
        fresh.load_state_dict({"blob": blob[:1000].clone()})
    _same(_replay(fresh, acts), rec, "state_dict")


def test_get_state_set_state_alone_does_not_resume():
    """why the snapshot ABI exists: hh_state_view carries the simulation state, not what the world keeps besides it"""
    name = "level3_fight"
    _, st, acts, rec, _ = _run(name)
    other = _world(name)
    other.reset()
    other.set_state(st)
    got = _replay(other, acts)
    stats = all(np.array_equal(a, b) for g, x in zip(got, rec) for a, b in zip(g[4:7], x[4:7]))
    faults = all(np.array_equal(g[9], x[9]) for g, x in zip(got, rec))
    assert not stats, "episode_stats differ: the running return and the last finished episode are not in a state view"
    assert not faults, "action_faults differ: the sticky flags are not in a state view"


REFUSED = {"another seed": dict(seed=99), "another n_arenas": dict(n_arenas=32), "another level": dict(level=2),
           "another arena_offset": dict(arena_offset=48), "another mode": dict(agent_mode=1), "another horizon": dict(horizon=HORIZON_LL + 1)}


@pytest.mark.parametrize("what", list(REFUSED) + ["truncated", "another env kind", "another format version", "not a snapshot"])
def test_refused_blobs_leave_the_world_untouched(what):
    from hhmarl_2d_amd import _lib as L
    blob, _, acts, rec, w = _run("level3_fight")
    w.restore(blob)
    if what in REFUSED:
        donor = _world("level3_fight", **REFUSED[what])
        donor.reset()
        bad = donor.snapshot()
    elif what == "another env kind":
        bad = _run("hl_3v3")[0]
    elif what == "truncated":
        bad = blob[:blob.numel() - 4096].clone()
    else:
        bad = blob.clone()
        if what == "another format version":
            bad[4] = 2
        else:
            bad[:4] = 0
    rc = L.lib().hh_world_restore(w.h, C.c_void_p(bad.data_ptr()), bad.numel(), None)
    assert rc == -1, "HH_E_ARG"
    msg = L.lib().hh_last_error().decode()
    assert msg.startswith("hh_world_restore: ") and len(msg) > 30
    if what in ("another seed", "another level", "another arena_offset"):
        assert what.split()[1] in msg, msg
    with pytest.raises(ValueError, match="hh_world_restore"):
        w.restore(bad)
    assert torch.equal(w.snapshot(), blob), "nothing was written"
    _same(_replay(w, acts), rec, what)
