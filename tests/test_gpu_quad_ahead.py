"""The 2-vs-2 two-wave kernel's AHEAD mailbox (hh_kernels_quad.h: QAheadMail): in the 8-arenas-per-wave form the output wave draws, in its idle
window before barrier X, the key-only draws of the tick after next (rocket guidance noise, missile wait) and the simulation wave takes them in
place of its own draw when the two ticks in between ran in the same launch without a reset.  Nothing of it may change a bit: every case runs the
level-3 fight preset on the keyed action tape (fire and launch bits set half the time) and compares, field by field with array_equal, against
the CPU oracle — state, observations, reward, valid, done, episode statistics, action faults — and against the same world run single-wave
(HH_NO_TWO=1).  The cases are the validity rules of the mailbox: a full workgroup and a one-arena tail, resets inside a launch, launch
boundaries (nothing carried across a launch), state set mid-episode, arenas that stay done, out-of-range action words.

Every fixture starts from a state the oracle reached after 100 ticks on the tape (rockets in flight, missile waits running) with the step
counters rewritten so that the horizon ends episodes inside the launch.  The simulation wave takes a draw from the mailbox only on a tick whose
two predecessors ran in the same launch and reset no arena of its wave (QPre.a_ok), so the short-horizon fixtures put their arenas in two groups
whose episodes end on the same tick: the resets cluster and leave runs of valid ticks between them.  What each fixture exercises, counted on the
CPU with the oracle (test_fixtures_exercise_rockets_and_resets asserts lower bounds on all of it).  Over all arenas and ticks:

    fixture         rocket launches   steered rocket ticks   missile-wait draws   arena resets / done ticks
    full-8                10                 106                    25                    9
    tail-9                11                 117                    27                   10
    resets-8              11                  90                    29                   24
    boundaries-8           7                  52                    18                   16
    set-state-8            1                   9                     5                    4   (starts 70 ticks in, not 100; half its arenas run past the reset)
    no-auto-reset-8        1                  23                     1                   92 (done ticks: the arenas stay done)
    dirty-8               11                  87                    27                   24

and the wave-ticks on which the mailbox is valid (a_ok), by launch pattern, derived from the oracle's done flags:

    fixture, launches      a_ok wave-ticks   with a steered rocket   with a wait draw   valid again after a reset in the launch
    full-8, 1 x 64               44                  38                    13                 44
    tail-9, 1 x 64              104 (two waves)      49                    15                 76
    resets-8, 1 x 40             26                  26                     8                 23
    boundaries-8, 1 x 24         14                  14                     5                 11
    boundaries-8, 24 x 1          0                   0                     0                  0   (the fallback draw only)
    boundaries-8, 12 x 2          0                   0                     0                  0   (the fallback draw only)
    boundaries-8, 3 x 8          11                  11                     4                  8
    set-state-8, 1 x 8            5                   3                     2                  0   (its one reset is two ticks from the end)
    no-auto-reset-8, 1 x 20      18                   9                     1                  -   (the wait draw is made beside an arena that stays done)
    dirty-8, 1 x 36              22                  22                     4                 19
"""
import functools

import numpy as np
import pytest

WARM = 100   # ticks the oracle runs from reset before a fixture starts
SEED = 77

# horizon: the configuration's; steps0: step counter of arena n at the start = steps0[n % len]; launches: T of each hh_rollout call in a row
FIXTURES = {
    "full-8": dict(N=8, horizon=60, auto_reset=True, steps0=(10, 25, 33, 41, 48, 52, 55, 58), launches=(64,)),
    "tail-9": dict(N=9, horizon=60, auto_reset=True, steps0=(10, 25, 33, 41, 48, 52, 55, 58, 30), launches=(64,)),
    "resets-8": dict(N=8, horizon=12, auto_reset=True, steps0=(2, 2, 2, 2, 7, 7, 7, 7), launches=(40,)),
    "boundaries-8": dict(N=8, horizon=12, auto_reset=True, steps0=(2, 2, 2, 2, 7, 7, 7, 7), launches=(24,)),
    "set-state-8": dict(N=8, horizon=12, auto_reset=True, steps0=(5, 5, 5, 5, 0, 0, 0, 0), launches=(8,), wait_cap=3, warm=70),
    "no-auto-reset-8": dict(N=8, horizon=12, auto_reset=False, steps0=(0, 0, 1, 1, 2, 3, 5, 8), launches=(20,), wait_cap=4),
    "dirty-8": dict(N=8, horizon=12, auto_reset=True, steps0=(2, 2, 2, 2, 7, 7, 7, 7), launches=(36,), dirty=True),
}
APW = 8   # arenas per simulation wave of the form under test: QPre.a_ok is uniform over them
# lower bounds asked of every fixture: (rocket launches, steered rocket ticks, resets or done ticks)
MIN_COUNTS = (1, 1, 1)


def _cfg(fx):
    return dict(n_arenas=fx["N"], level=3, seed=SEED, auto_reset=fx["auto_reset"], horizon=fx["horizon"])


@functools.lru_cache(maxsize=None)
def _start(name):
    """(state the fixture starts from, tape int8 [T, N, 2, 4]) — computed once, read-only afterwards"""
    import oracle_lib as O
    fx = FIXTURES[name]
    N, T = fx["N"], sum(fx["launches"])
    o = O.OracleWorld(O.make_config(n_arenas=N, level=3, seed=SEED, auto_reset=True))
    o.reset()
    o.rollout(O.action_tape_uniform(SEED, 0, 0, fx.get("warm", WARM), N))
    st = o.get_state()
    st["ar_i"][:, 0] = [fx["steps0"][n % len(fx["steps0"])] for n in range(N)]
    if "wait_cap" in fx:   # missile waits about to run out: the arenas that keep running make wait draws beside the ones that are done
        st["ac_i"][:, :, 7] = np.minimum(st["ac_i"][:, :, 7], fx["wait_cap"])
    assert (st["rk_i"][:, :, 0] != 0).any() and (st["ac_i"][:, :, 7] > 0).any(), "a rocket in flight and a missile wait running at the start"
    tape = O.action_tape_uniform(SEED, 0, fx.get("warm", WARM), T, N).copy()
    if fx.get("dirty"):
        # out-of-range words (heading component 100, speed component -5, launch component 77) at t = 0 (arenas 0-2), at t = 1 (arenas 3, 4) and at
        # the tick after a reset (arenas 5, 6: the horizon ends their episode at tick horizon - steps0 - 1, and every `horizon` ticks after); arena 7 stays clean
        junk = np.array([100, -5, 1, 77], dtype=np.int8)
        tape[0, 0:3, :] = junk
        tape[1, 3:5, :] = junk
        for n in (5, 6):
            for t in range(fx["horizon"] - fx["steps0"][n], T, fx["horizon"]):
                tape[t, n, :] = junk
    for a in st.values():
        a.setflags(write=False)
    tape.setflags(write=False)
    return st, tape


def _copy_state(st):
    return {k: np.array(v) for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    """the oracle's outputs of the fixture in ONE launch, its final state, statistics and fault flags, and the event counts of the docstring"""
    import oracle_lib as O
    fx = FIXTURES[name]
    st, tape = _start(name)
    o = O.OracleWorld(O.make_config(**_cfg(fx)))
    o.reset()
    o.set_state(_copy_state(st))
    outs = [np.array(x) for x in o.rollout(np.array(tape))]
    res = dict(outs=outs, state=_copy_state(o.get_state()), stats=[np.array(x) for x in o.episode_stats()], faults=np.array(o.action_faults()))
    # the counts: a second world stepped tick by tick
    c = O.OracleWorld(O.make_config(**_cfg(fx)))
    c.reset()
    c.set_state(_copy_state(st))
    launches = steered = waits = dones = 0
    T_, N_ = tape.shape[0], fx["N"]
    steer_tn, wait_tn, idle_tn = np.zeros((T_, N_), bool), np.zeros((T_, N_), bool), np.zeros((T_, N_), bool)
    for t in range(tape.shape[0]):
        s0 = c.get_state()
        got = c.step(np.array(tape[t]))
        s1 = c.get_state()
        ran = np.ones(fx["N"], bool) if fx["auto_reset"] or t == 0 else ~prev_done
        steered += int(((s0["rk_i"][:, :, 0] != 0) & (s0["ac_i"][:, :, 8] != 0) & (s0["ac_i"][:, :, 0] != 0) & ran[:, None]).sum())
        fresh = ~got[3].astype(bool)   # an arena that reset in this tick shows its NEW episode's state
        launches += int(((s0["rk_i"][:, :, 0] == 0) & (s1["rk_i"][:, :, 0] != 0) & fresh[:, None]).sum())
        waits += int(((s0["ac_i"][:, :2, 7] == 0) & (s1["ac_i"][:, :2, 7] > 0) & fresh[:, None]).sum())
        dones += int(got[3].sum())
        steer_tn[t] = ((s0["rk_i"][:, :, 0] != 0) & (s0["ac_i"][:, :, 8] != 0) & (s0["ac_i"][:, :, 0] != 0) & ran[:, None]).any(1)
        wait_tn[t] = ((s0["ac_i"][:, :2, 7] == 0) & (s1["ac_i"][:, :2, 7] > 0) & fresh[:, None]).any(1)
        idle_tn[t] = ~ran
        prev_done = got[3].astype(bool)
        for x, y in zip(got, outs):
            assert np.array_equal(x, y[t]), "oracle: step by step = rollout"
    res["counts"] = (launches, steered, waits, dones)
    res["per_tick"] = (steer_tn, wait_tn, idle_tn)
    return res


def _ahead_counts(name, launches):
    """Wave-ticks on which the simulation wave TAKES a draw from the mailbox under this launch pattern, counted from the oracle's run: QPre.a_ok
    holds on tick t of a launch when t >= 2 and no arena of the wave was reset on ticks t - 1 and t - 2 (a reset tick = an arena of the wave
    done, with auto-reset) -> (a_ok wave-ticks, of them with a steered rocket, with a missile-wait draw, with a wait draw beside an arena
    of the wave that stays done, a_ok wave-ticks that follow a reset in the same launch)"""
    fx, res = FIXTURES[name], _oracle_run(name)
    done = res["outs"][3].astype(bool)
    steer_tn, wait_tn, idle_tn = res["per_tick"]
    n_ok = n_steer = n_wait = n_wait_idle = n_after = 0
    for w0 in range(0, fx["N"], APW):
        sl = slice(w0, min(w0 + APW, fx["N"]))
        reset_t = done[:, sl].any(1) & fx["auto_reset"]
        t0 = 0
        for T in launches:
            for k in range(2, T):
                t = t0 + k
                if reset_t[t - 1] or reset_t[t - 2]:
                    continue
                n_ok += 1
                n_steer += int(steer_tn[t, sl].any())
                n_wait += int(wait_tn[t, sl].any())
                n_wait_idle += int(wait_tn[t, sl].any() and idle_tn[t, sl].any())
                n_after += int(reset_t[t0:t - 2].any())
            t0 += T
    return n_ok, n_steer, n_wait, n_wait_idle, n_after


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixtures_exercise_rockets_and_resets(oracle, name):
    """CPU: a fixture in which no rocket is launched, none is steered or no episode ends would test nothing"""
    launches, steered, waits, dones = _oracle_run(name)["counts"]
    print(name, "launches", launches, "steered rocket ticks", steered, "missile-wait draws", waits, "resets / done ticks", dones)
    assert launches >= MIN_COUNTS[0] and steered >= MIN_COUNTS[1] and dones >= MIN_COUNTS[2]
    assert waits >= 1
    # ... and one in which the simulation wave never takes a draw from the mailbox tests the fallback only
    for pat in _patterns(name):
        n_ok, n_steer, n_wait, n_wait_idle, n_after = _ahead_counts(name, pat)
        print(name, pat[:3], len(pat), "launches: a_ok wave-ticks", n_ok, "with a steered rocket", n_steer, "with a wait draw", n_wait,
              "with a wait draw beside a done arena", n_wait_idle, "after a reset in the launch", n_after)
        if max(pat) >= 8:
            assert n_ok >= 3 and n_steer >= 1 and n_wait >= 1
            if FIXTURES[name]["auto_reset"] and sum(pat) >= 24:   # (the 8-tick launch of set-state-8 ends two ticks after its reset)
                assert n_after >= 1, "the mailbox becomes valid again after a reset inside the launch"
        else:
            assert n_ok == 0, "launches of one or two ticks never take a draw from the mailbox"
    if not FIXTURES[name]["auto_reset"]:
        assert _ahead_counts(name, FIXTURES[name]["launches"])[3] >= 1, "a wait draw from the mailbox beside an arena that stays done"
    if FIXTURES[name].get("dirty"):
        f = _oracle_run(name)["faults"]
        assert f[:7].all() and not f[7], "every dirtied word was consumed by a live, running agent; the clean arena stays clean"


def _gpu_run(name, launches):
    import torch
    from hhmarl_2d_amd.world import World, make_config
    fx = FIXTURES[name]
    st, tape = _start(name)
    g = World(make_config(**_cfg(fx)))
    g.reset()
    g.set_state(_copy_state(st))
    dev = torch.from_numpy(np.array(tape)).cuda()
    parts, t0 = [], 0
    for T in launches:
        parts.append([x.cpu().numpy() for x in g.rollout(dev[t0:t0 + T].contiguous())])
        t0 += T
    assert t0 == tape.shape[0]
    outs = [np.concatenate([p[k] for p in parts]) for k in range(4)]
    res = dict(outs=outs, state=g.get_state(), stats=[x.cpu().numpy() for x in g.episode_stats()], faults=g.action_faults().cpu().numpy(),
               kernel=g.kernel_instance())
    g.close()
    return res


def _assert_same(a, b, what):
    for x, y, field in zip(a["outs"], b["outs"], ("obs", "reward", "valid", "done")):
        assert np.array_equal(x, y), f"{what}: {field}"
    for k in a["state"]:
        assert np.array_equal(a["state"][k], b["state"][k]), f"{what}: state {k}"
    for i, (x, y) in enumerate(zip(a["stats"], b["stats"])):
        assert np.array_equal(x, y), f"{what}: episode statistics [{i}]"
    assert np.array_equal(a["faults"], b["faults"]), f"{what}: action faults"


def _patterns(name):
    T = sum(FIXTURES[name]["launches"])
    if name == "boundaries-8":   # one launch, T launches of one tick, T / 2 launches of two ticks, three launches of eight
        return [(T,), (1,) * T, (2,) * (T // 2), (8,) * (T // 8)]
    return [FIXTURES[name]["launches"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FIXTURES))
def test_ahead_mailbox_changes_no_bit(oracle, monkeypatch, name):
    want = _oracle_run(name)
    monkeypatch.setenv("HH_FORCE_W", "0")
    runs = []
    for launches in _patterns(name):
        monkeypatch.setenv("HH_NO_TWO", "0")
        two = _gpu_run(name, launches)
        assert two["kernel"] == "hh_k_world_quad<1, 1, true, 8, true, true>", "the instance with the ahead mailbox"
        monkeypatch.setenv("HH_NO_TWO", "1")
        one = _gpu_run(name, launches)
        assert one["kernel"] != two["kernel"], "single-wave form"
        _assert_same(two, want, f"{name} {launches[:3]}: two-wave form vs oracle")
        _assert_same(one, want, f"{name} {launches[:3]}: single-wave form vs oracle")
        _assert_same(two, one, f"{name} {launches[:3]}: two-wave vs single-wave form")
        runs.append(two)
    for r in runs[1:]:
        _assert_same(runs[0], r, f"{name}: one launch vs many")
    if FIXTURES[name].get("dirty"):
        assert want["faults"].any() and not want["faults"].all()
    if not FIXTURES[name]["auto_reset"]:
        assert want["outs"][3][-1].all(), "every arena ended its episode and stayed done"
