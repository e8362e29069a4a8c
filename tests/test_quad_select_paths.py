"""Fixtures for the select-form sites of the 2-vs-2 tick in front of barrier X (hh_kernels_quad.h: tick_quad from its first line to the
move, and the mailbox reads behind barrier Y), and the CPU half of their test: the oracle runs every fixture and counts how often each
rewritten site is reached.  A fixture that never reaches a site would let the GPU test (test_gpu_quad_select_paths.py) pass on nothing, so
a zero count fails HERE, on the CPU.

Every fixture: 8 arenas (one full workgroup of the 8-arena form), 9 (a one-arena tail) or 17 (one full wave of the 16-arena forms and a one-arena
tail), two launches of LAUNCH ticks, the keyed action tape.
The start is the state the oracle reached after WARM ticks of the same configuration, with these injections (set_state):

    arena 0   agent 0 has no cannon ammunition and no burst running, and the tape orders it to fire on ticks 0..3   (fire with no ammunition)
    arena 1   agent 0: burst 1 of 50 rounds, agent 1: burst 2 with ONE round left; no fire order on ticks 0..3        (a burst that ends)
    arena 2   agent 0 carries a rocket in flight towards unit 3 (slot 2), two ticks old                               (steered on ticks 0 and 1 of a launch)
    arena 3   agent 1 is dead, arena 4: opponent 1 (slot 3) is dead                                                   (a dead aircraft)
    arena 5   levels 1 and 2 only: opponent 0 (slot 2) stands still with a commanded speed of 0 — level 3 and the external policy always
              command >= 100 kn, so there the site `spd == 0` cannot be reached by a live aircraft                   (a stationary aircraft)
    arena 6   its step counter is 3 ticks short of the horizon: it resets on tick 2, beside the rocket of arena 2     (the tick after a reset)
    arena 5   one out-of-range action word on tick 3                                                                  (action faults)
    every arena: step counters spread so that the horizon ends episodes inside both launches

The fixture "l3-stay-done" runs without auto-reset: its arenas end one after the other and stay done beside the ones still running.
The fixture "l3-escape-shaping" is "l3-escape" with the escape distance shaping (env_hetero.py:198-214), the one way into the general instances
that keep the pair table on the simulation wave with the shaping term live: the site `shaping_live` counts the ticks whose rewards differ from
those of "l3-escape", so the fixture cannot pass with the term dead.
"""
import functools

import numpy as np
import pytest

WARM = 60      # ticks the oracle runs from reset before a fixture starts
LAUNCH = 200   # ticks per launch, two launches per fixture
SEED = 91
MODE_FIGHT, MODE_ESCAPE = 0, 1

# what make_config takes beyond n_arenas / seed; the kernel instance family each one selects is named in the comment
CONFIGS = {
    "l3": dict(level=3, auto_reset=True, horizon=70),                                                   # preset 1 (the headline)
    "l1": dict(level=1, auto_reset=True, horizon=70),                                                   # preset 2
    "l2": dict(level=2, auto_reset=True, horizon=70),                                                   # preset 3
    "l3-escape": dict(level=3, agent_mode=MODE_ESCAPE, auto_reset=True, horizon=70),                    # preset 4
    "l3-general": dict(level=3, auto_reset=True, horizon=70, rew_scale=2.0, friendly_punish=True),      # no preset: PRE = 0
    "l3-stay-done": dict(level=3, auto_reset=False, horizon=70),                                        # arenas that are done and stay done
    "l3-escape-shaping": dict(level=3, agent_mode=MODE_ESCAPE, esc_dist_rew=True, auto_reset=True, horizon=70),   # no preset, the shaping term live
}
SIZES = (8, 9, 17)
CASES = [(c, n) for c in CONFIGS for n in SIZES]
STEPS0 = (5, 12, 20, 31, 44, 57, 67, 63, 50)   # arena 6: horizon - 3

# the sites, and the configurations in which each must be reached (None: all of them)
SITES = {
    "fire_no_ammo": None, "burst_ends": None, "burst_without_rounds": None, "steer_first_two_ticks": None, "steer_after_reset": ("auto",),
    "launch_tick": None, "dead_aircraft": None, "stationary": ("l1", "l2"), "done_stays": ("l3-stay-done",), "reset": ("auto",),
    "shaping_live": ("l3-escape-shaping",),
}


def _needs(site, cfg):
    w = SITES[site]
    if w is None:
        return True
    if w == ("auto",):
        return CONFIGS[cfg]["auto_reset"]
    return cfg in w


def make_cfg(mod, cfg, N):
    return mod.make_config(n_arenas=N, seed=SEED, **CONFIGS[cfg])


@functools.lru_cache(maxsize=None)
def start(cfg, N):
    """(state the fixture starts from, tape int8 [2 * LAUNCH, N, 2, 4]) — computed once, read-only afterwards"""
    import oracle_lib as O
    kw = dict(CONFIGS[cfg], auto_reset=True)
    o = O.OracleWorld(O.make_config(n_arenas=N, seed=SEED, **kw))
    o.reset()
    o.rollout(O.action_tape_uniform(SEED, 0, 0, WARM, N))
    st = o.get_state()
    ac_f, ac_i, rk_f, rk_i, ar_i = st["ac_f"], st["ac_i"], st["rk_f"], st["rk_i"], st["ar_i"]
    # every aircraft alive at the start except the two taken out below (the warm-up may have removed some: put them back where they stood)
    ac_i[:, :, 0] = 1
    ar_i[:, 1] = 2; ar_i[:, 2] = 2
    ar_i[:, 0] = [STEPS0[n % len(STEPS0)] for n in range(N)]
    # arena 0: no ammunition
    ac_i[0, 0, 2] = 0; ac_i[0, 0, 3] = 0
    # arena 1: bursts about to end
    ac_i[1, 0, 2] = 50; ac_i[1, 0, 3] = 1
    ac_i[1, 1, 2] = 1; ac_i[1, 1, 3] = 2
    # arena 2: agent 0 (an AC1) with a rocket in flight, launched two ticks ago from where it stands
    assert ac_i[2, 0, 1] == 1, "slot 0 is the missile carrier"
    ac_i[2, 0, 8] = 1; ac_i[2, 0, 5] = max(int(ac_i[2, 0, 5]) - 1, 1)
    rk_f[2, 0, 0] = ac_f[2, 0, 0]; rk_f[2, 0, 1] = ac_f[2, 0, 1]; rk_f[2, 0, 2] = ac_f[2, 0, 2]; rk_f[2, 0, 3] = ac_f[2, 0, 2]
    rk_i[2, 0, 3] = int(rk_i[2, :, 3].max()) + 1   # launch order: the youngest rocket of the arena
    rk_i[2, 0, 0] = 1; rk_i[2, 0, 1] = 3; rk_i[2, 0, 2] = 2
    # arenas 3 and 4: a dead agent, a dead opponent
    ac_i[3, 1, 0] = 0; ar_i[3, 1] = 1
    ac_i[4, 3, 0] = 0; ar_i[4, 2] = 1
    for n, s in ((3, 1), (4, 3)):   # a dead aircraft carries nothing in flight
        ac_i[n, s, 8] = 0; ac_i[n, s, 3] = 0; rk_i[n, s, 0] = 0
    # arena 5: a stationary opponent (it keeps the commanded speed of its state at levels 1 and 2)
    if CONFIGS[cfg]["level"] <= 2:
        ac_f[5, 2, 3] = 0.0; ac_f[5, 2, 5] = 0.0
    tape = O.action_tape_uniform(SEED, 0, WARM, 2 * LAUNCH, N).copy()
    tape[0:4, 0, 0, 2] = 1
    tape[0:4, 1, :, 2] = 0
    tape[3, 5, :, :] = np.array([100, -5, 1, 77], dtype=np.int8)
    for a in st.values():
        a.setflags(write=False)
    tape.setflags(write=False)
    return st, tape


def copy_state(st):
    return {k: np.array(v) for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def oracle_run(cfg, N):
    """the oracle's run of the fixture in two launches: per launch the four outputs and the event masks behind it, then the final state and
    the action faults; and, from a second world stepped tick by tick, how often each site is reached"""
    import oracle_lib as O
    st, tape = start(cfg, N)
    o = O.OracleWorld(make_cfg(O, cfg, N))
    o.reset()
    o.set_state(copy_state(st))
    launches = []
    for k in range(2):
        outs = [np.array(x) for x in o.rollout(np.array(tape[k * LAUNCH:(k + 1) * LAUNCH]))]
        launches.append(dict(outs=outs, events=np.array(o.event_masks())))
    res = dict(launches=launches, state=copy_state(o.get_state()), faults=np.array(o.action_faults()))

    auto = CONFIGS[cfg]["auto_reset"]
    c = O.OracleWorld(make_cfg(O, cfg, N))
    c.reset()
    c.set_state(copy_state(st))
    n = dict.fromkeys(SITES, 0)
    prev_done = np.zeros(N, bool)
    for t in range(2 * LAUNCH):
        s0 = c.get_state()
        got = c.step(np.array(tape[t]))
        s1 = c.get_state()
        for x, y in zip(got, launches[t // LAUNCH]["outs"]):
            assert np.array_equal(x, y[t % LAUNCH]), "oracle: step by step = rollout"
        ran = np.ones(N, bool) if auto else ~prev_done            # the arena ran this tick
        done = got[3].astype(bool)
        fresh = ~(done & auto)                                     # its state behind the tick is the tick's own, not a new episode's
        live = (s0["ac_i"][:, :, 0] != 0) & ran[:, None]
        agents = live[:, :2]
        n["fire_no_ammo"] += int((agents & (tape[t][:, :, 2] != 0) & (s0["ac_i"][:, :2, 2] <= 0)).sum())
        ends = live & (s0["ac_i"][:, :, 3] > 0) & (s1["ac_i"][:, :, 3] == 0) & fresh[:, None]
        n["burst_ends"] += int(ends.sum())
        n["burst_without_rounds"] += int((live & (s0["ac_i"][:, :, 3] > 0) & (s0["ac_i"][:, :, 2] <= 0)).sum())   # the countdown's clamp at 0
        steer = live & (s0["ac_i"][:, :, 8] != 0) & (s0["rk_i"][:, :, 0] != 0)
        if t % LAUNCH < 2:
            n["steer_first_two_ticks"] += int(steer.sum())
        if t % LAUNCH >= 1 and (prev_done[:8] & auto).any():       # an arena of the first wave was reset a tick ago (both two-wave forms)
            n["steer_after_reset"] += int(steer[:8].sum())
        n["launch_tick"] += int(((s0["rk_i"][:, :, 0] == 0) & (s1["rk_i"][:, :, 0] != 0) & fresh[:, None] & ran[:, None]).sum())
        n["dead_aircraft"] += int(((s0["ac_i"][:, :, 0] == 0) & ran[:, None]).sum())
        n["stationary"] += int((live & (s1["ac_i"][:, :, 0] != 0) & (s1["ac_f"][:, :, 3] == 0.0) & fresh[:, None]).sum())
        n["done_stays"] += int((~ran).sum())
        n["reset"] += int((done & auto).sum())
        prev_done = done
    if cfg == "l3-escape-shaping":   # the same run without the shaping term: same start, same tape, other rewards
        plain = oracle_run("l3-escape", N)
        for k in range(2):
            assert np.array_equal(launches[k]["outs"][3], plain["launches"][k]["outs"][3]), "the shaping term changes rewards only"
            n["shaping_live"] += int((launches[k]["outs"][1] != plain["launches"][k]["outs"][1]).any(axis=(1, 2)).sum())
    res["counts"] = n
    return res


@pytest.mark.parametrize("cfg,N", CASES)
def test_fixture_reaches_every_site(oracle, cfg, N):
    res = oracle_run(cfg, N)
    n = res["counts"]
    print(cfg, N, n)
    for site in SITES:
        if _needs(site, cfg):
            assert n[site] >= 1, f"{cfg}, {N} arenas: the fixture never reaches `{site}`"
    f = res["faults"]
    assert f[5] and not f[:5].any(), "the one dirtied word was consumed; the arenas in front of it stay clean"
    if not CONFIGS[cfg]["auto_reset"]:
        assert res["launches"][1]["outs"][3][-1].all(), "every arena ended its episode and stayed done"
        running_beside_done = n["done_stays"] < (2 * LAUNCH) * N
        assert running_beside_done
    if N in (9, 17):
        assert res["launches"][0]["outs"][2][:, N - 1].any(), "the tail arena runs"
