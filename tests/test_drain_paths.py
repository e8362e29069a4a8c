"""Fixtures for the draw-first drain of the envelope queue (hh_kernels.h: drain_envelope_queue_t) and the CPU half of their test.

The drain takes a cannon entry's keyed Bernoulli draw in front of the geometry and leaves the pass on a miss; a fuse entry gets the range of the
mid-latitude estimate without its bearing; the cannon prefilter of the register-exchange kernels drops the two separation clauses its range
prefilter implies.  Nothing of that may change a bit, so test_gpu_drain_paths.py runs the fixtures below on every kernel form that compiles the
drain and compares with array_equal against the oracle.  That proves something only if the fixtures reach every class of queue entry the new order
treats differently; this module classifies every queue candidate of every tick from the oracle's states and FAILS HERE, on the CPU, when a class
is missing:

    1  cannon entry, target truly in the cone, the draw misses            (skipped now; before: decided, then drawn)
    2  cannon entry, target in the cone, the draw hits                    (the kill)
    3  cannon entry that passes the planar stage, truly outside, the draw WOULD hit   (the verdict decides: skipping the geometry here is a kill too many)
    4  as 3, the draw misses
    5  fuse entry inside the 0.01 deg box, under 1 km                     (range only)
    6  fuse entry inside the box, over 1 km
    7  a wave-tick (8 consecutive arenas) with a missing cannon entry AND an entry that needs geometry: masked lanes beside working ones

Fixtures: 64 arenas of 2-vs-2 level 3 with friendly fire in the headline preset ("l3") and in a general configuration ("l3-general", PRE = 0),
and a 3-vs-3 HighLevelEnv world of 16 arenas ("hier"); two launches each from a fixed seed — 150 ticks a launch for the 2-vs-2 worlds, ten
commander steps (at most 160 ticks) a launch for the HighLevelEnv world, whose launches are whole commander steps.

Class 3 needs a firing aircraft with a target just outside its cone's edge, inside the 0.3 deg the planar stage leaves undecided, on a tick whose
draw is below the hit probability: plain rollouts of this size meet it or not depending on the seed, so arenas 60 .. 63 of the 2-vs-2 fixtures are
laid out for it through set_state (as tests/hier_crowded.py lays out its columns): an agent with a running burst, and an opponent on its nose + (half
width + 0.15 deg) at 1.5 km, both at 300 kn on the same heading, so that the pair stays in the undecided band for the first ticks.

Same file: the sibling prefilter hh_cannon_cone_planar_outside_near against the original ANDed with the range box on a grid, and
hh_geo_inverse_estimate_range against hh_geo_inverse_estimate's s12, both through a small C hook compiled for the test (tests/drain_hooks.c)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import hier_crowded as H

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 1234
N2, TICKS = 64, 150          # 2-vs-2: arenas, ticks per launch
NH, HL_STEPS = 16, 10        # HighLevelEnv: arenas, commander steps per launch (H.SUB ticks each)
QUAD_CONFIGS = {
    "l3": dict(level=3, friendly_kill=True, auto_reset=True),                                                  # preset 1, the headline instance
    "l3-general": dict(level=3, friendly_kill=True, auto_reset=True, rew_scale=2.0, friendly_punish=True),   # no preset: PRE = 0
}
HIER_CFG = dict(n_arenas=NH, env_kind=1, friendly_kill=True, auto_reset=True, seed=SEED)
CLASSES = ("cannon_in_cone_miss", "cannon_in_cone_hit", "cannon_outside_would_hit", "cannon_outside_miss", "fuse_box_under_1km", "fuse_box_over_1km",
           "wave_tick_miss_beside_geometry")
LAID_OUT = (60, 61, 62, 63)
SITE_CANNON = 21             # hh_spec.h: HH_SITE_CANNON


def quad_cfg(mod, cfg):
    return mod.make_config(n_arenas=N2, seed=SEED, **QUAD_CONFIGS[cfg])


def hier_cfg(mod):
    return mod.make_config(**HIER_CFG)


def copy_state(st):
    return {k: np.array(v) for k, v in st.items()}


def hit_prob(t):
    return (0.75 / (5.0 / 1.0)) if t == 1 else (0.9 / (3.0 / 1.0))   # hh_spec.h: HH_AC_HIT_PROB


# ------------------------------------------------------------------ the classes of one tick
def classify(O, seed, s0, s1, fresh, n_agents, tick_off, friendly_kill=True):
    """the queue candidates of the tick s0 -> s1 by class, from the oracle's states alone.  `fresh`: arenas whose s1 is the tick's own state (not a
    new episode's); `tick_off`: the tick number in the draw's key is the step counter of s0 + tick_off (LowLevelEnv counts the step before the tick: 1;
    HighLevelEnv behind it: 0).  Returns (counts per class, per arena: a missing cannon entry, an entry that needs geometry; cannon candidates, fuse candidates,
    per arena the bit mask of target slots that an in-cone candidate's draw hits = the tick's cannon kills)."""
    f0, i0, f1, i1 = s0["ac_f"], s0["ac_i"], s1["ac_f"], s1["ac_i"]
    Nn, nU = i0.shape[:2]
    cnt = dict.fromkeys(CLASSES, 0)
    miss_in = np.zeros(Nn, bool)
    geo_in = np.zeros(Nn, bool)
    kill_mask = np.zeros(Nn, dtype=np.int64)
    alive = (i0[:, :, 0] != 0) & fresh[:, None]
    # an aircraft fired on this tick exactly when a round left its magazine (ac1.py:101-103)
    fired = alive & (i1[:, :, 2] < i0[:, :, 2])
    n_, i_, j_ = [x.ravel() for x in np.meshgrid(np.arange(Nn), np.arange(nU), np.arange(nU), indexing="ij")]
    moved = j_ < i_                                  # a target with a lower id has moved already (cmano_simulator.py:142)
    tl = np.where(moved, f1[n_, j_, 0], f0[n_, j_, 0]); to = np.where(moved, f1[n_, j_, 1], f0[n_, j_, 1])
    sl, so, sh = f0[n_, i_, 0], f0[n_, i_, 1], f1[n_, i_, 2]   # the shooter where it stood, its heading after the turn
    typ = i0[n_, i_, 1]
    o1, e1 = O.cannon_cone_planar(1, sl, so, sh, tl, to)
    o2, e2 = O.cannon_cone_planar(2, sl, so, sh, tl, to)
    outside, exact = np.where(typ == 1, o1, o2), np.where(typ == 1, e1, e2)
    lim = np.where(typ == 1, 2.0, 4.5) / 100.0       # hh_device.h: d_maybe_within_km
    box = (np.abs(tl - sl) <= lim) & (np.abs(to - so) <= lim)
    enemy = (i_ < n_agents) != (j_ < n_agents)
    cand = fired[n_, i_] & alive[n_, j_] & (i_ != j_) & (enemy | friendly_kill) & box & (outside == 0)
    n_cannon = 0
    for k in np.flatnonzero(cand):
        n, i, j = int(n_[k]), int(i_[k]), int(j_[k])
        u = O.lib().hho_rng_u01(seed, n, int(s0["ar_i"][n, 5]), int(s0["ar_i"][n, 0]) + tick_off, i + 1, SITE_CANNON, j + 1)
        hit = u < hit_prob(int(typ[k]))
        name = ("cannon_in_cone_hit" if hit else "cannon_in_cone_miss") if exact[k] else ("cannon_outside_would_hit" if hit else "cannon_outside_miss")
        cnt[name] += 1
        n_cannon += 1
        if hit:
            geo_in[n] = True
            if exact[k]:
                kill_mask[n] |= 1 << j
        else:
            miss_in[n] = True
    # fuses: the rockets in flight where they stand before their move, against the MOVED target and "friend" (rocket_unit.py:37-58)
    rk = (s0["rk_i"][:, :, 0] != 0) & fresh[:, None]
    rn, rs = np.nonzero(rk)
    n_fuse = 0
    if len(rn):
        rl, ro = s0["rk_f"][rn, rs, 0], s0["rk_f"][rn, rs, 1]
        pairs = [s0["rk_i"][rn, rs, 1] - 1]
        if friendly_kill:
            pairs.append(np.where(rs == 1, 0, 1))
        for j in pairs:
            inbox = (np.abs(f1[rn, j, 0] - rl) <= 0.01) & (np.abs(f1[rn, j, 1] - ro) <= 0.01)
            km = O.geo_inverse(rl, ro, f1[rn, j, 0], f1[rn, j, 1])[0] / 1000.0
            cnt["fuse_box_under_1km"] += int((inbox & (km < 1.0)).sum())
            cnt["fuse_box_over_1km"] += int((inbox & (km >= 1.0)).sum())
            geo_in[rn[inbox]] = True
            n_fuse += int(inbox.sum())
    return cnt, miss_in, geo_in, n_cannon, n_fuse, kill_mask


def _add(total, cnt, miss_in, geo_in, wave):
    for k, v in cnt.items():
        total[k] += v
    for w in range(0, len(miss_in), wave):
        total["wave_tick_miss_beside_geometry"] += int(miss_in[w:w + wave].any() and geo_in[w:w + wave].any())


# ------------------------------------------------------------------ 2-vs-2
def _lay_out_edge(O, st):
    """arenas LAID_OUT: agent 0 fires a running burst at opponent 0 (slot 2) standing just outside its cone's edge, inside the planar stage's undecided band"""
    for n in LAID_OUT:
        t = int(st["ac_i"][n, 0, 1])
        half = 5.0 if t == 1 else 3.5
        side = 1.0 if n % 2 else -1.0
        lat, lon = 5.12, 7.15 + 0.01 * (n - LAID_OUT[0])
        H._clean(st, n)
        st["ac_i"][n, :, 0] = 1
        st["ar_i"][n, 1] = 2; st["ar_i"][n, 2] = 2
        H._put(st, n, 0, lat, lon, 0.0, 300.0)
        H._put(st, n, 2, *H._at(O, lat, lon, side * (half + 0.15), 1.5), 0.0, 300.0)
        H._put(st, n, 1, *H._at(O, lat, lon, 180.0, 6.0), 180.0, 300.0)
        H._put(st, n, 3, *H._at(O, lat, lon, 180.0, 12.0), 180.0, 300.0)
        st["ac_i"][n, 0, 3] = 5 if t == 1 else 3       # a burst that runs from the first tick
        st["ac_i"][n, 0, 2] = max(int(st["ac_i"][n, 0, 2]), 50)


@functools.lru_cache(maxsize=None)
def quad_start(cfg):
    """(state the fixture starts from, tape int8 [2 * TICKS, N2, 2, 4]) — computed once, read-only afterwards"""
    import oracle_lib as O
    o = O.OracleWorld(quad_cfg(O, cfg))
    o.reset()
    st = o.get_state()
    _lay_out_edge(O, st)
    tape = O.action_tape_uniform(SEED, 0, 0, 2 * TICKS, N2).copy()
    tape[:6, LAID_OUT[0]:, :, 0] = 6      # the laid-out arenas keep their heading for the first ticks
    tape[:6, LAID_OUT[0]:, :, 1] = 2
    for a in list(st.values()) + [tape]:
        a.setflags(write=False)
    return st, tape


@functools.lru_cache(maxsize=None)
def quad_oracle_run(cfg):
    """the oracle's run of a 2-vs-2 fixture in two launches (outputs and event masks per launch, final state, action faults) and, from a second world
    stepped tick by tick, the class counts"""
    import oracle_lib as O
    st, tape = quad_start(cfg)
    o = O.OracleWorld(quad_cfg(O, cfg))
    o.reset()
    o.set_state(copy_state(st))
    launches = []
    for k in range(2):
        outs = [np.array(x) for x in o.rollout(np.array(tape[k * TICKS:(k + 1) * TICKS]))]
        launches.append(dict(outs=outs, events=np.array(o.event_masks())))
    res = dict(launches=launches, state=copy_state(o.get_state()), faults=np.array(o.action_faults()))
    c = O.OracleWorld(quad_cfg(O, cfg))
    c.reset()
    c.set_state(copy_state(st))
    total = dict.fromkeys(CLASSES, 0)
    n_cannon = n_fuse = kills = 0
    for t in range(2 * TICKS):
        s0 = c.get_state()
        got = c.step(np.array(tape[t]))
        s1, ev = c.get_state(), np.array(c.event_masks())
        for x, y in zip(got, launches[t // TICKS]["outs"]):
            assert np.array_equal(x, y[t % TICKS]), "oracle: step by step = rollout"
        fresh = ~got[3].astype(bool)
        cnt, miss_in, geo_in, nc, nf, kill_mask = classify(O, SEED, s0, s1, fresh, 2, 1)
        _add(total, cnt, miss_in, geo_in, 8)
        n_cannon += nc; n_fuse += nf
        # the classification reads the same draws as the tick: in every arena that did not end its episode, the aircraft the tick's event mask reports
        # as killed by cannon (hh_spec.h: HH_EV_BIT class 0 = the low bits, one per slot) are exactly the targets some in-cone candidate's draw hits
        assert np.array_equal((ev.astype(np.int64) & 0xf)[fresh], kill_mask[fresh]), f"tick {t}: cannon kills differ from the classified hits"
        kills += int(sum(bin(int(m)).count("1") for m in kill_mask[fresh]))
    res["counts"], res["n_cannon"], res["n_fuse"], res["cannon_kills"] = total, n_cannon, n_fuse, kills
    return res


# ------------------------------------------------------------------ HighLevelEnv
@functools.lru_cache(maxsize=None)
def hier_start():
    """(commands int8 [2 * HL_STEPS, NH, 3], tape int8 [2 * HL_STEPS, SUB, NH, 6, 4]): every pilot keeps the trigger pulled on two sub-ticks in three"""
    from helpers import random_actions
    rng = np.random.default_rng(SEED)
    cmds = rng.integers(0, 3, (2 * HL_STEPS, NH, 3)).astype(np.int8)
    tape = random_actions(rng, (2 * HL_STEPS, H.SUB, NH), 6)
    tape[:, np.arange(H.SUB) % 3 != 2, :, :, 2] = 1
    cmds.setflags(write=False); tape.setflags(write=False)
    return cmds, tape


@functools.lru_cache(maxsize=None)
def hier_oracle_run():
    """per commander step the sub-ticks' records, outputs, state, event masks (hier_crowded._macro_step); after each launch the state; class counts"""
    import oracle_lib as O
    cmds, tape = hier_start()
    o = O.OracleWorld(hier_cfg(O))
    o.reset()
    total = dict.fromkeys(CLASSES, 0)
    seen = dict(n_cannon=0, n_fuse=0)

    def probe(k, s0, s1, act, cmd_act, events):
        ran = s1["ar_i"][:, 0] != s0["ar_i"][:, 0]
        cnt, miss_in, geo_in, nc, nf, kill_mask = classify(O, SEED, s0, s1, ran, 3, 0)
        assert np.array_equal((np.asarray(events).astype(np.int64) & 0x3f)[ran], kill_mask[ran]), "cannon kills differ from the classified hits"
        _add(total, cnt, miss_in, geo_in, 8)
        seen["n_cannon"] += nc; seen["n_fuse"] += nf

    steps = []
    for step in range(2 * HL_STEPS):
        rec = []
        r = H._macro_step(o, np.array(cmds[step]), tape[step], 6, record=rec, probe=probe)
        r["ticks"] = rec
        steps.append(r)
    return dict(steps=steps, stats=[np.array(x) for x in o.episode_stats()], faults=np.array(o.action_faults()), counts=total, **seen)


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("cfg", list(QUAD_CONFIGS))
def test_quad_fixture_reaches_every_class(oracle, cfg):
    res = quad_oracle_run(cfg)
    print(cfg, res["counts"], "cannon candidates", res["n_cannon"], "fuse candidates", res["n_fuse"], "cannon kills", res["cannon_kills"])
    for k in CLASSES:
        assert res["counts"][k] >= 1, f"{cfg}: the fixture never reaches `{k}`"
    assert res["cannon_kills"] >= 1, "a cannon kill (checked tick by tick against the event masks in quad_oracle_run)"
    assert not res["faults"].any()


def test_hier_fixture_queues_entries(oracle):
    res = hier_oracle_run()
    print("hier", res["counts"], "cannon candidates", res["n_cannon"], "fuse candidates", res["n_fuse"])
    assert res["n_cannon"] >= 1 and res["counts"]["cannon_in_cone_miss"] + res["counts"]["cannon_outside_miss"] >= 1, "a cannon entry whose draw misses"
    assert res["n_fuse"] >= 1, "a fuse entry"
    assert not res["faults"].any()


@functools.lru_cache(maxsize=None)
def hooks():
    """tests/drain_hooks.c compiled with the oracle's flags into a library of this test's own (a temporary directory: nothing is added to the tree)"""
    import tempfile
    d = tempfile.mkdtemp(prefix="hh_drain_hooks_")
    so = os.path.join(d, "libdrain_hooks.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-fvisibility=hidden", "-shared",
                           "-I" + os.path.join(ROOT, "include"), "-o", so, os.path.join(HERE, "drain_hooks.c"), "-lm"])
    return C.CDLL(so)


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def test_near_prefilter_equals_original_and_box():
    """hh_cannon_cone_planar_outside_near ANDed with the range box = hh_cannon_cone_planar_outside ANDed with it, bit for bit, on a grid over the
    box edges of both cannon ranges, the dropped clause's 0.06 deg, latitudes on either side of 10 and 25 deg and separations under 1e-5 deg"""
    L = hooks()
    eps = 2.0 ** -40
    seps = sorted({s * sg for sg in (1.0, -1.0) for b in (0.02, 0.045, 0.06) for s in (b - 1e-3, b - eps, b, b + eps, b + 1e-3)} |
                  {0.0, 1e-6, -1e-6, 3e-6, 7e-6, -7e-6, 9.9e-6, 1e-5, 1.1e-5, 0.001, -0.001, 0.01, -0.013, 0.03, -0.03, 0.05, 0.07, -0.2})
    lats = [0.0, 5.12, 9.97, 9.99, 10.0 - eps, 10.0, 10.0 + eps, 10.03, 10.05, -9.99, -10.0, -10.02, 24.95, 24.99, 25.0 - eps, 25.0, 25.0 + eps, 25.03, -25.0, 40.0]
    hdgs = [0.0, 3.4, 5.2, 45.0, 90.0, 181.0, 268.5, 359.0]
    la, dy, dx, hd = [x.ravel() for x in np.meshgrid(lats, seps, seps, hdgs, indexing="ij")]
    lat1, lon1 = la, np.full_like(la, 7.15)
    lat2, lon2 = lat1 + dy, lon1 + dx
    he, hn = np.sin(np.radians(hd)), np.cos(np.radians(hd))
    n = len(la)
    checked = decided = 0
    for t, km in ((1, 2.0), (2, 4.5)):
        full, near = np.empty(n, np.int32), np.empty(n, np.int32)
        L.dh_cannon_cone(n, t, _p(lat1), _p(lon1), _p(lat2), _p(lon2), _p(he), _p(hn), _p(full, C.c_int32), _p(near, C.c_int32))
        lim = km / 100.0                                     # hh_device.h: d_maybe_within_km, the same expressions
        box = (np.abs(lat2 - lat1) <= lim) & (np.abs(lon2 - lon1) <= lim)
        maybe = box | ~((np.abs(lat1) < 25.0) & (np.abs(lat2) < 25.0))
        assert np.array_equal(maybe & (full == 0), maybe & (near == 0)), f"type {t}: the push bit differs at {np.flatnonzero((maybe & (full == 0)) != (maybe & (near == 0)))[:5]}"
        # the grid is not vacuous: the forms DO differ outside the box, both answers occur inside it, and the guard d2 < 1e-10 is met
        assert (full != near).any() and not (full != near)[maybe].any()
        assert (full[maybe] == 1).any() and (full[maybe] == 0).any()
        checked += n; decided += int((full[maybe] == 1).sum())
    d2 = dx * dx + dy * dy
    assert ((d2 < 1e-10) & (d2 > 0.0)).any() and (d2 == 0.0).any()
    print("points", checked, "decided outside inside the box", decided)


def test_estimate_range_equals_estimate(oracle):
    """hh_geo_inverse_estimate_range = the s12 of hh_geo_inverse_estimate, bit for bit, over the drain's domain (and the oracle's own export of the latter)"""
    L = hooks()
    rng = np.random.default_rng(SEED)
    n = 200000
    lat1 = rng.uniform(-10.0, 10.0, n); lon1 = rng.uniform(-169.0, 169.0, n)
    sep = np.where(np.arange(n) % 2 == 0, 0.06, 0.85)
    lat2 = lat1 + rng.uniform(-1.0, 1.0, n) * sep; lon2 = lon1 + rng.uniform(-1.0, 1.0, n) * sep
    lat2[:100] = lat1[:100]; lon2[100:200] = lon1[100:200]; lat2[200:210] = lat1[200:210]; lon2[200:210] = lon1[200:210]   # meridians, parallels, a point
    s_full, s_range = np.empty(n), np.empty(n)
    L.dh_estimate_range(n, _p(lat1), _p(lon1), _p(lat2), _p(lon2), _p(s_full), _p(s_range))
    assert np.array_equal(s_full, s_range)
    assert np.array_equal(s_full, oracle.geo_inverse_estimate(lat1, lon1, lat2, lon2)[0])
    assert (s_full[210:] > 0.0).all() and (s_full[200:210] == 0.0).all()
