"""Fixtures that crowd the envelope queue of a HighLevelEnv tick, and the oracle's run of them (no test in this module: test_hier_crowded.py
proves on the CPU that every site below is reached, test_gpu_hier_crowded.py runs every HighLevelEnv kernel instance on them bit for bit).

Every geodesic envelope test of a tick (missile launch, cannon hit, the two rocket fuses) goes through a per-workgroup queue: hh_kernels.h `tick`
(code registers c0..c11, QCAP 8 / 12, one atomicAdd reservation), hh_kernels_oct.h HH_O_PUSH (wave ballot + mbcnt).  From a spawn the aircraft
stand tens of kilometres apart and a lane queues one or two entries; here the arenas are laid out through set_state so that one lane queues up
to 1 launch + 9 cannon candidates + 2 fuses and a whole wave queues at once.

A fixture: N = 21 arenas (two full waves and a tail at 8, at 10 and at 6 arenas per wave), env_kind 1, friendly fire, auto-reset, 3 commander
steps of 16 ticks.  Steps 0 and 1 start from an injected state (step 1: what survived step 0, laid out again), step 2 runs a random tape on what
survived.  The tape of steps 0 and 1: heading action 6 (keep), speed level 0 (100 kn, the speed everybody holds), the trigger pulled from
sub-tick K_FIRE[step] on: 0 in step 0, 7 in step 1 — hh_hl_rollout meets the crowded tick first and mid-launch.  Every agent is commanded to
fight its nearest opponent (command 1) in steps 0 and 1.

Layouts by arena % 7 (v = arena // 7; nU = aircraft of the arena, unit slots 0 .. nU - 1; columns stand on the meridian 7.25 E, heading north):

    0  rear shooter   column, the HIGHEST slot (named an AC2: 4.5 km, +-3.5 deg) at the rear, the others 450 m apart in front of it in descending
                      slot order: every target has a lower id and is tested where it stands AFTER its move.  v = 1: the step counter one short of
                      the horizon (the episode ends on the crowded tick); v = 2: only the rear shooter's trigger is pulled (several kills by one shooter,
                      the first of them of its own side)
    1  front shooter  column, slot 0 (an AC1: 2 km, +-5 deg) at the rear, the others 200 m apart in ascending slot order: targets are tested where
                      they stand BEFORE their move, slots 8 and 9 stand in front of eight shooters
    2  clusters       agents line abreast (8 m apart) heading north, 1.6 km north of them the opponents line abreast heading south: the whole opposing
                      cluster lies in every shooter's cone, nobody of the own.  Mutual kills; a shooter killed by a lower id still shoots.
                      v = 1: the horizon ends on step 1's crowded tick
    3  column + rocket  layout 0 at 200 m with the rear shooter named an AC1 that carries a rocket in flight (two ticks old), 0.4 km behind its target,
                      the firer's "friend" (rocket_unit.py:46: slot 0 if the firer is slot 1, else slot 1) 0.3 km beyond the target: (nU - 1) cannon
                      candidates + 2 fuses on one lane.  The target stands near the rear (v = 0: it mostly survives the cannons and the rocket fuses
                      on it), in front (v = 1: it mostly dies by cannon on that tick and the fuse passes to the friend) or in the middle (v = 2)
    4  first-tick fuse  slot 0 (AC1) launches at tick 0 of the step on its nearest opponent 1.2 km away 30 deg right of the nose — a DECIDED planar
                      launch (pre == 1) — which closes at 600 kn: the rocket fuses on its first tick.  The others stay where they spawned
    5  undecided launch  slot 0 (AC1) at the rear of a column orders trigger and missile on the same tick, its nearest opponent on the h - 1 deg edge
                      of the missile cone, the bearing found by scanning oracle_lib.missile_cone_planar for pre == -1.  v = 0: the target 0.6 km
                      away, agents and the other opponents on the meridian within 2 km: 1 launch + (nU - 1) cannon + 2 fuses on one lane (the full
                      12 with ten aircraft), the launch passes; v = 1: the opponents 8 km away, the launch passes; v = 2: the same, it is refused
    6  untouched      the spawn state, beside the crowded ones: a stale code drained from a neighbour's queue region would change something
"""
import functools

import numpy as np

N = 21
STEPS, SUB = 3, 16
K_FIRE = (0, 7)
HORIZON = 60
# sides -> (n_agents, n_opps); "default" = the compiled-in default configuration (KI.HL_CONFIGS["default"]: horizon 500), 3-vs-3 only
SIDES = ((3, 3), (5, 5), (5, 4), (4, 4))
KEYS = [((3, 3), False), ((3, 3), True), ((5, 5), False), ((5, 4), False), ((4, 4), False)]
# seed, arena_offset per fixture: hits are Bernoulli draws keyed by them, tuned on the CPU until the oracle alone reaches every site
SEEDS = {k: (4, 0) for k in KEYS}
LAT0, LON0 = 5.23, 7.25          # rear end of every column
STEPS_LEFT = {7: 1, 9: 9}        # arena -> ticks its step counter is short of the horizon at the start
OUTS = ("obs", "reward", "valid", "done")
SITES = ("cannon_target_8_or_9", "kill_hangs_on_ninth_entry_or_later", "multi_kill_one_shooter", "mutual_kill", "friendly_cannon_kill", "fuse_on_target", "fuse_on_friend",
         "fuse_on_launch_tick", "launch_through_queue_passes", "launch_through_queue_refused", "rocket_target_dies_by_cannon_same_tick",
         "episode_ends_on_crowded_tick", "reset", "arena_survives_crowded_tick")


def key_id(key):
    (a, b), default = key
    return f"{a}v{b}" + ("-default" if default else "")


def cfg_kwargs(key, seed=None):
    (nA, nO), default = key
    sd, off = SEEDS[key] if seed is None else seed
    return dict(n_arenas=N, env_kind=1, n_agents=nA, n_opps=nO, friendly_kill=True, auto_reset=True, horizon=500 if default else HORIZON,
                seed=sd, arena_offset=off)


def slots_of(key):
    (nA, nO), _ = key
    return 10 if max(nA, nO) > 3 else 6


def ev_bit(slots, cls, slot):
    """hh_spec.h: HH_EV_BIT for the classes 0 killed by cannon, 1 killed by rocket, 2 out of bounds"""
    return 1 << ((8 if slots <= 8 else 10) * cls + slot)


def copy_state(st):
    return {k: np.array(v) for k, v in st.items()}


def pad_state(st, A):
    """the oracle's state ([N, nU, ...]: exactly the units that exist) in the unit slots of a device world ([N, A, ...])"""
    out = {}
    for k, v in st.items():
        if k == "ar_i" or v.shape[1] == A:
            out[k] = np.array(v)
        else:
            p = np.zeros((v.shape[0], A) + v.shape[2:], dtype=v.dtype)
            p[:, :v.shape[1]] = v
            out[k] = p
    return out


# ------------------------------------------------------------------ layouts
def _at(O, lat, lon, brg, km):
    a, b = O.geo_direct([lat], [lon], [brg % 360.0], [km * 1000.0])
    return float(a[0]), float(b[0])


def _put(st, n, s, lat, lon, hdg, spd=100.0):
    st["ac_f"][n, s] = (lat, lon, hdg, spd, hdg, spd)


def _name_type(st, n, s, t):
    q = st["ac_i"][n, s]
    q[1] = t
    q[5] = q[6] = 8 if t == 1 else 0   # env_base.py: a HighLevelEnv AC1 carries 8 missiles, an AC2 none


def _clean(st, n):
    """nobody of the arena fires, waits or carries anything in flight"""
    st["ac_i"][n, :, 3] = 0; st["ac_i"][n, :, 7] = 0; st["ac_i"][n, :, 8] = 0
    st["rk_f"][n] = 0.0; st["rk_i"][n] = 0


def _column(O, st, n, order, gaps, base=(LAT0, LON0)):
    """order[0] at the rear end, order[k] gaps[k - 1] km in front of order[k - 1], all heading north"""
    d = 0.0
    for k, s in enumerate(order):
        if k:
            d += gaps[k - 1]
        lat, lon = _at(O, base[0], base[1], 0.0, d) if d else base
        _put(st, n, s, lat, lon, 0.0)
    return d


@functools.lru_cache(maxsize=None)
def edge_bearing(km, want_exact):
    """a bearing relative to a northward nose at (LAT0, LON0) on the h - 1 deg edge of the missile cone at which the planar stage of the launch
    predicate is undecided (pre == -1) and the exact predicate says want_exact"""
    import oracle_lib as O
    beta = np.linspace(-1.45, -0.55, 3601)
    la, lo = O.geo_direct(np.full_like(beta, LAT0), np.full_like(beta, LON0), beta % 360.0, np.full_like(beta, km * 1000.0))
    pre, exact, _, _ = O.missile_cone_planar(np.full_like(beta, LAT0), np.full_like(beta, LON0), np.zeros_like(beta), la, lo)
    ok = np.flatnonzero((pre == -1) & (exact == int(want_exact)))
    assert len(ok), f"no undecided bearing with exact == {want_exact} at {km} km"
    # the one farthest from the exact edge: the verdict must not hang on the aircraft's last bits
    return float(beta[ok[np.argmax(np.abs(beta[ok] + 1.0))]])


def rocket_order(nU, v):
    """layout 3: the column in front of the rear shooter nU - 1, the rocket's target t directly followed by the firer's friend, slot 1"""
    t = (0, 0, 2)[v]
    rest = [s for s in range(nU - 2, -1, -1) if s not in (t, 1)]
    at = (min(2, len(rest)), len(rest), len(rest) // 2)[v]
    return rest[:at] + [t, 1] + rest[at:], t


def lay_out(O, st, key, step):
    """write the layouts into st (the oracle's state shape), in place: the aircraft that are alive in st keep living, the dead stay dead"""
    (nA, nO), default = key
    nU = nA + nO
    horizon = 500 if default else HORIZON
    for n in range(N):
        lay, v = n % 7, n // 7
        if lay == 6:
            continue
        _clean(st, n)
        if step == 0:
            st["ar_i"][n, 0] = horizon - STEPS_LEFT[n] if n in STEPS_LEFT else 3 + n
        rear = nU - 1
        if lay == 0:
            _name_type(st, n, rear, 2)
            _column(O, st, n, list(range(nU - 1, -1, -1)), [0.45] * (nU - 1))
        elif lay == 1:
            _column(O, st, n, list(range(nU)), [0.2] * (nU - 1))
        elif lay == 2:
            for s in range(nU):
                ag = s < nA
                i, cnt = (s, nA) if ag else (s - nA, nO)
                lat, lon = _at(O, LAT0, LON0, 0.0, 1.6) if not ag else (LAT0, LON0)
                off = (i - (cnt - 1) / 2.0) * 0.008
                if off:
                    lat, lon = _at(O, lat, lon, 90.0 if off > 0 else 270.0, abs(off))
                _put(st, n, s, lat, lon, 0.0 if ag else 180.0)
        elif lay == 3:
            _name_type(st, n, rear, 1)
            order, t = rocket_order(nU, v)
            gaps = [0.3 if s == 1 else 0.2 for s in order]
            _column(O, st, n, [rear] + order, gaps)
            if st["ac_i"][n, rear, 0]:   # a dead aircraft carries nothing in flight
                tl, to = st["ac_f"][n, t, 0], st["ac_f"][n, t, 1]
                rl, ro = _at(O, tl, to, 180.0, 0.4)
                st["ac_i"][n, rear, 8] = 1; st["ac_i"][n, rear, 5] = 7
                st["rk_f"][n, rear] = (rl, ro, 0.0, 0.0)
                st["rk_i"][n, rear] = (1, t + 1, 2, 1)
        elif lay == 4:
            _put(st, n, 0, LAT0, LON0, 0.0)
            lat, lon = _at(O, LAT0, LON0, 30.0, 1.2)
            _put(st, n, nA, lat, lon, 210.0, 600.0)
        elif lay == 5:
            if v == 0:
                b = edge_bearing(0.6, True)
                meridian = [s for s in range(1, nU) if s != nA]      # agents first: the nearest opponent is the one on the edge
                dist = [d for d in (0.2, 0.4, 0.8, 1.0, 1.2, 1.4, 1.6, 1.8)][:len(meridian)]
                _put(st, n, 0, LAT0, LON0, 0.0)
                for s, d in zip(meridian, dist):
                    _put(st, n, s, *_at(O, LAT0, LON0, 0.0, d), 0.0)
                _put(st, n, nA, *_at(O, LAT0, LON0, b, 0.6), 0.0)
            else:
                b = edge_bearing(8.0, v == 1)
                _column(O, st, n, list(range(nA)), [0.2] * (nA - 1))
                for i in range(nO):
                    _put(st, n, nA + i, *_at(O, LAT0, LON0, b, 8.0 + 0.3 * i), 0.0)


def armed(key, n):
    """the unit slots whose trigger the tape of steps 0 and 1 pulls in arena n"""
    (nA, nO), _ = key
    return [nA + nO - 1] if n == 14 else list(range(nA + nO))


@functools.lru_cache(maxsize=None)
def start(sides, default=False, seed=None):
    """(state step 0 starts from, commands int8 [STEPS, N, n_agents], tape int8 [STEPS, SUB, N, A, 4]) — computed once, read-only afterwards"""
    import oracle_lib as O
    from helpers import random_actions
    key = (sides, default)
    nA, nO = sides
    A = slots_of(key)
    o = O.OracleWorld(O.make_config(**cfg_kwargs(key, seed)))
    o.reset()
    st = o.get_state()
    lay_out(O, st, key, 0)
    rng = np.random.default_rng(N)
    cmds = np.ones((STEPS, N, nA), dtype=np.int8)
    cmds[2] = rng.integers(0, 3, (N, nA))
    tape = np.zeros((STEPS, SUB, N, A, 4), dtype=np.int8)
    tape[..., 0] = 6
    for step, k_fire in enumerate(K_FIRE):
        for n in range(N):
            tape[step, k_fire:, n, armed(key, n), 2] = 1
            if n % 7 == 4:
                tape[step, :, n, 0, 3] = 1
            if n % 7 == 5:
                tape[step, k_fire:, n, 0, 3] = 1
    tape[2] = random_actions(rng, (SUB, N), A)
    tape[:, :, :, nA + nO:] = 0
    for a in list(st.values()) + [cmds, tape]:
        a.setflags(write=False)
    return st, cmds, tape


# ------------------------------------------------------------------ the lower bound on what a lane queues in a tick
def lane_bounds(O, s0, s1, act, cmd_act, ran):
    """[N, nU] entries lane (arena, slot) queues at least in the tick s0 -> s1, from exact geometry: the kernels' prefilters
    (d_maybe_within_km, hh_cannon_cone_planar_outside) are conservative, so whatever is truly inside an envelope is queued.
    Also returns the launches tried (arena, slot, target slot, pre, exact), the fuse tests of the tick's rockets and the cannon candidates
    [N, shooter, target]."""
    f0, i0, f1 = s0["ac_f"], s0["ac_i"], s1["ac_f"]
    Nn, nU = i0.shape[:2]
    alive = (i0[:, :, 0] != 0) & ran[:, None]
    fired = alive & ((i0[:, :, 3] > 0) | ((act[:, :nU, 2] != 0) & (i0[:, :, 2] > 0)))
    n_, i_, j_ = np.meshgrid(np.arange(Nn), np.arange(nU), np.arange(nU), indexing="ij")
    n_, i_, j_ = n_.ravel(), i_.ravel(), j_.ravel()
    moved = j_ < i_                                   # a target with a lower id has moved already (cmano_simulator.py:142)
    tl = np.where(moved, f1[n_, j_, 0], f0[n_, j_, 0]); to = np.where(moved, f1[n_, j_, 1], f0[n_, j_, 1])
    sl, so, sh = f0[n_, i_, 0], f0[n_, i_, 1], f1[n_, i_, 2]   # the shooter where it stood, its heading after the turn
    inside = np.where(i0[n_, i_, 1] == 1, O.cannon_cone_planar(1, sl, so, sh, tl, to)[1], O.cannon_cone_planar(2, sl, so, sh, tl, to)[1])
    cand = (inside != 0) & (i_ != j_) & fired[n_, i_] & alive[n_, j_]
    bound = cand.reshape(Nn, nU, nU).sum(-1).astype(np.int64)
    # launches: env_base.py:227-236 with the stored target the command selects (env_hier.py: commander_actions[i] - 1, -1 = the last)
    tgt_n = (s0["tgt_id"] != 0).sum(-1)
    k = np.where(cmd_act > 0, cmd_act - 1, tgt_n - 1)
    tgt = np.where(k >= 0, np.take_along_axis(s0["tgt_id"], np.maximum(k, 0)[..., None], -1)[..., 0], 0)
    tried = alive & (i0[:, :, 1] == 1) & (act[:, :nU, 3] != 0) & (tgt > 0) & (i0[:, :, 5] > 0) & (i0[:, :, 8] == 0) & (i0[:, :, 7] == 0)
    nn, ss = np.nonzero(tried)
    tj = tgt[nn, ss] - 1
    pre, exact, _, _ = O.missile_cone_planar(f0[nn, ss, 0], f0[nn, ss, 1], f0[nn, ss, 2], f0[nn, tj, 0], f0[nn, tj, 1])
    np.add.at(bound, (nn[pre == -1], ss[pre == -1]), 1)
    # fuses: the rockets of the tick (in flight, or launched on it) where they stand before their move against the MOVED target and friend
    rk = (s0["rk_i"][:, :, 0] != 0) & ran[:, None]
    rl, ro, rt = np.array(s0["rk_f"][:, :, 0]), np.array(s0["rk_f"][:, :, 1]), s0["rk_i"][:, :, 1] - 1
    ln, ls = nn[exact != 0], ss[exact != 0]
    rk[ln, ls] = True; rl[ln, ls] = f0[ln, ls, 0]; ro[ln, ls] = f0[ln, ls, 1]; rt[ln, ls] = tj[exact != 0]
    rn, rs = np.nonzero(rk)
    fuse = {}
    for name, j in (("target", rt[rn, rs]), ("friend", np.where(rs == 1, 0, 1))):
        km = O.geo_inverse(rl[rn, rs], ro[rn, rs], f1[rn, j, 0], f1[rn, j, 1])[0] / 1000.0
        np.add.at(bound, (rn[km < 1.0], rs[km < 1.0]), 1)
        fuse[name] = (rn, rs, j, km < 1.0)
    return bound, dict(n=nn, s=ss, tgt=tj, pre=pre, exact=exact), fuse, cand.reshape(Nn, nU, nU)


# ------------------------------------------------------------------ the oracle's run
def _macro_step(o, cmd, tape_step, nU, record=None, probe=None):
    """one commander step on an oracle world; record: list that receives a dict per sub-tick; probe(k, s0, s1, act, ran_before)"""
    o.hl_begin(cmd)
    for k in range(SUB):
        act = np.ascontiguousarray(tape_step[k][:, :nU])
        s0 = o.get_state() if probe else None
        cmd_act = o.hl_cmd()[0] if probe else None
        po_a, pm_a = o.hl_pilot_obs(0)
        o.hl_agents_act(act)
        po_o, pm_o = o.hl_pilot_obs(1)
        running = o.hl_tick(act)
        events = o.event_masks()
        if record is not None:
            record.append(dict(po_a=po_a, pm_a=pm_a, po_o=po_o, pm_o=pm_o, running=running, events=events))
        if probe:
            probe(k, s0, o.get_state(), act, cmd_act, events)
    outs = [np.array(x) for x in o.hl_end()]
    return dict(outs=outs, state=copy_state(o.get_state()), events=np.array(o.event_masks()), eval=[np.array(x) for x in o.eval_info()])


def _run(key, seed=None, untouched=False):
    import oracle_lib as O
    (nA, nO), default = key
    nU, slots = nA + nO, slots_of(key)
    sd, off = SEEDS[key] if seed is None else seed
    st0, cmds, tape = start(key[0], default, seed)
    cfg = lambda: O.make_config(**cfg_kwargs(key, seed))
    o = O.OracleWorld(cfg())
    o.reset()
    steps, injected, ticks = [], [], 0
    for step in range(STEPS):
        if step < 2:
            st = copy_state(st0) if step == 0 and not untouched else copy_state(o.get_state())
            if step == 1 and not untouched:
                lay_out(O, st, key, 1)
            o.set_state(copy_state(st))
            injected.append(st)
        rec = []
        res = _macro_step(o, np.array(cmds[step]), tape[step], nU, record=rec)
        res["ticks"] = rec
        running_before = N   # auto-reset worlds: every arena enters the macro step
        for r in rec:
            ticks += running_before
            running_before = r["running"]
        res["tick_count"] = ticks
        steps.append(res)
    out = dict(steps=steps, injected=injected, stats=[np.array(x) for x in o.episode_stats()], faults=np.array(o.action_faults()))
    if untouched:
        return out

    # a second world stepped with get_state() around every tick: the sites, and the lower bound per lane
    c = O.OracleWorld(cfg())
    c.reset()
    cnt = dict.fromkeys(SITES, 0)
    lane_max = np.zeros(N, dtype=np.int64)
    waves = {G: dict(ticks=0, best=0) for G in ((6,) if slots == 10 else (8, 10))}
    crowded_last = np.zeros(N, bool)      # the arena's last tick of this step was a crowded one
    survived = np.zeros(N, bool)
    agents, opps = np.arange(nU) < nA, np.arange(nU) >= nA
    unit_bits = np.array([[ev_bit(slots, cls, s) for s in range(nU)] for cls in range(3)], dtype=np.int64)
    cls_bits = lambda m, cls: (m.astype(np.int64)[:, None] & unit_bits[cls][None, :]) != 0

    def probe(k, s0, s1, act, cmd_act, events):
        ran = s1["ar_i"][:, 0] != s0["ar_i"][:, 0]
        bound, launch, fuse, cand = lane_bounds(O, s0, s1, act, cmd_act, ran)
        np.maximum(lane_max, bound.max(-1), out=lane_max)
        per_arena = bound.sum(-1)
        for G, w in waves.items():
            crowded = [n for n in range(G) if n % 7 != 6]
            if all(per_arena[n] > 0 for n in crowded):
                w["ticks"] += 1
                w["best"] = max(w["best"], int(per_arena[:G].sum()))
        is_crowded = ran & (bound.max(-1) >= 4)
        crowded_last[ran] = is_crowded[ran]
        a0, a1 = (s0["ac_i"][:, :, 0] != 0) & ran[:, None], s1["ac_i"][:, :, 0] != 0
        gone = a0 & ~a1
        by_cannon, by_rocket = cls_bits(events, 0) & gone, cls_bits(events, 1) & gone
        assert not (gone & ~by_cannon & ~by_rocket & ~cls_bits(events, 2)).any(), "every removal has its event bit"
        cnt["cannon_target_8_or_9"] += int(by_cannon[:, 8:].sum())
        # the Bernoulli draws of the tick's cannon candidates (ac1.py:112-113, keyed by shooter and target id): which kill hangs on which queue entry
        hit = np.zeros_like(cand)
        for n, i, j in zip(*np.nonzero(cand)):
            u = O.lib().hho_rng_u01(sd, off + int(n), int(s0["ar_i"][n, 5]), int(s0["ar_i"][n, 0]), int(i) + 1, 21, int(j) + 1)
            hit[n, i, j] = u < ((0.75 / (5.0 / 1.0)) if s0["ac_i"][n, i, 1] == 1 else (0.9 / (3.0 / 1.0)))
        assert np.array_equal(hit.any(1), by_cannon), "the cannon kills of the tick are the targets some candidate's draw hits"
        for n, i, j in zip(*np.nonzero(hit)):
            # entry number of (i -> j) in lane i's queue, at least: the candidates with a lower target slot stand in front of it
            if cand[n, i, :j].sum() >= 8 and hit[n, :, j].sum() == 1:
                cnt["kill_hangs_on_ninth_entry_or_later"] += 1
        fired = a0 & ((s0["ac_i"][:, :, 3] > 0) | ((act[:, :, 2] != 0) & (s0["ac_i"][:, :, 2] > 0)))
        one = fired.sum(-1) == 1
        cnt["multi_kill_one_shooter"] += int((one & (by_cannon.sum(-1) >= 2)).sum())
        cnt["mutual_kill"] += int(((by_cannon & agents).any(-1) & (by_cannon & opps).any(-1) & (np.arange(N) % 7 == 2)).sum())
        # a cannon kill whose every possible shooter is of the victim's side
        shooters_ag, shooters_op = (fired & agents).any(-1), (fired & opps).any(-1)
        cnt["friendly_cannon_kill"] += int(((by_cannon & agents).any(-1) & ~shooters_op).sum() + ((by_cannon & opps).any(-1) & ~shooters_ag).sum())
        rn, rs, tj, t_in = fuse["target"]
        _, _, fj, f_in = fuse["friend"]
        launched_now = np.zeros((N, nU), bool)
        launched_now[launch["n"][launch["exact"] != 0], launch["s"][launch["exact"] != 0]] = True
        for n, s, t, tin, f, fin in zip(rn, rs, tj, t_in, fj, f_in):
            rocket_gone = s1["rk_i"][n, s, 0] == 0
            on_target = tin and by_rocket[n, t] and rocket_gone
            cnt["fuse_on_target"] += int(on_target)
            cnt["fuse_on_launch_tick"] += int(on_target and launched_now[n, s])
            if tin and by_cannon[n, t]:
                cnt["rocket_target_dies_by_cannon_same_tick"] += 1
            on_friend = not on_target and fin and by_rocket[n, f] and rocket_gone
            cnt["fuse_on_friend"] += int(on_friend)
            # the fuse entries stand behind the lane's cannon candidates
            if (on_target and cand[n, s].sum() >= 8) or (on_friend and cand[n, s].sum() + int(tin) >= 8):
                cnt["kill_hangs_on_ninth_entry_or_later"] += 1
        for n, s, pre, exact in zip(launch["n"], launch["s"], launch["pre"], launch["exact"]):
            if pre == -1:
                # the rocket exists behind the tick, or fused on it, exactly when the exact predicate says so
                has = bool(s1["ac_i"][n, s, 8]) or bool(s1["rk_i"][n, s, 0]) or launched_now[n, s] and by_rocket[n].any()
                assert has == bool(exact), "an undecided launch follows the exact predicate"
                cnt["launch_through_queue_passes" if exact else "launch_through_queue_refused"] += 1

    for step in range(STEPS):
        if step < 2:
            c.set_state(copy_state(injected[step]))
        crowded_last[:] = False
        got = _macro_step(c, np.array(cmds[step]), tape[step], nU, probe=probe)
        want = steps[step]
        for x, y in zip(got["outs"], want["outs"]):
            assert np.array_equal(x, y), "oracle: stepped with get_state around every tick = its own run over whole steps"
        for k2 in want["state"]:
            assert np.array_equal(got["state"][k2], want["state"][k2]), k2
        done = got["outs"][3].astype(bool)
        cnt["episode_ends_on_crowded_tick"] += int((done & crowded_last).sum())
        cnt["reset"] += int(done.sum())
        if step == 0:
            survived |= crowded_last & ~done
    ac1 = steps[0]["state"]["ac_i"]   # step 1 starts from it: both sides alive behind a crowded tick
    cnt["arena_survives_crowded_tick"] = int((survived & (ac1[:, :nA, 0] != 0).any(-1) & (ac1[:, nA:, 0] != 0).any(-1)).sum())
    out["counts"] = cnt
    out["lane_max"] = lane_max
    out["waves"] = waves
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(sides, default=False):
    """the oracle's record of the fixture: per step the sub-ticks (pilot rows and selector bytes of both sides, `running`, event masks), the four
    hl_end outputs, state, event masks, eval counters and arena-ticks behind it; the two injected states; episode statistics; action faults; and
    from a second world stepped with get_state() around every tick `counts` (how often each site is reached), `lane_max` (per arena the largest
    lower bound of a lane) and `waves`"""
    return _run((sides, default))


@functools.lru_cache(maxsize=None)
def untouched_run(sides, default=False):
    """the same world, commands and tape with NO arena laid out: what the untouched arenas (arena % 7 == 6) of the fixture must equal"""
    return _run((sides, default), untouched=True)


# ------------------------------------------------------------------ 2-vs-2: the generic kernel hh_k_world<4, 64, W, false> (HH_NO_QUAD=1) shares `tick`, QCAP = 8
# 17 arenas (one full wave of 16 and a tail), level 3 with friendly fire, one rollout of QUAD_T ticks; both agents keep heading and 100 kn, pull the
# trigger and order a missile on every tick.  Layouts by arena % 4, columns on the meridian 7.15 E heading north:
#     0  slot 0 (AC1) at the rear, slot 1 200 m, the opponents 400 and 600 m in front of it: its launch on the nearest opponent is undecided by the
#        planar stage (closer than HH_PLANAR_MIN_DEG) and stands beside 3 cannon candidates and the 2 fuses of the rocket it would launch: 6 entries
#     1  slot 0 at the rear with a rocket in flight 0.4 km behind its target (slot 2), slot 1 0.3 km beyond the target: 3 cannon candidates + 2 fuses
#     2  the agents line abreast heading north, the opponents 1.2 km north of them heading south
#     3  untouched
QUAD_N, QUAD_T = 17, 40
QUAD_CFG = dict(level=3, auto_reset=True, horizon=70, friendly_kill=True, seed=4)
QUAD_BASE = (5.12, 7.15)
QUAD_SITES = ("cannon_kill", "rocket_kill", "launch_through_queue", "reset")
QUAD_LANE = {0: 6, 1: 5, 2: 2, 3: 0}   # layout -> entries one of its lanes queues at least


def quad_cfg(mod):
    return mod.make_config(n_arenas=QUAD_N, **QUAD_CFG)


@functools.lru_cache(maxsize=None)
def quad_start():
    """(state the 2-vs-2 fixture starts from, tape int8 [QUAD_T, QUAD_N, 2, 4]) — computed once, read-only afterwards"""
    import oracle_lib as O
    o = O.OracleWorld(quad_cfg(O))
    o.reset()
    st = o.get_state()
    for n in range(QUAD_N):
        lay = n % 4
        if lay == 3:
            continue
        _clean(st, n)
        st["ar_i"][n, 0] = 2 * n
        if lay == 0:
            _column(O, st, n, [0, 1, 2, 3], [0.2, 0.2, 0.2], QUAD_BASE)
        elif lay == 1:
            _column(O, st, n, [0, 3, 2, 1], [0.2, 0.3, 0.3], QUAD_BASE)
            st["ac_i"][n, 0, 8] = 1; st["ac_i"][n, 0, 5] -= 1
            st["rk_f"][n, 0] = _at(O, QUAD_BASE[0], QUAD_BASE[1], 0.0, 0.1) + (0.0, 0.0)
            st["rk_i"][n, 0] = (1, 3, 2, 1)
        else:
            for s in range(4):
                lat, lon = QUAD_BASE if s < 2 else _at(O, QUAD_BASE[0], QUAD_BASE[1], 0.0, 1.2)
                lat, lon = _at(O, lat, lon, 90.0 if s % 2 else 270.0, 0.004)
                _put(st, n, s, lat, lon, 0.0 if s < 2 else 180.0)
    tape = np.zeros((QUAD_T, QUAD_N, 2, 4), dtype=np.int8)
    tape[..., 0] = 6; tape[..., 2] = 1; tape[..., 3] = 1
    for a in list(st.values()) + [tape]:
        a.setflags(write=False)
    return st, tape


@functools.lru_cache(maxsize=None)
def quad_oracle_run():
    """the oracle's rollout of the 2-vs-2 fixture (outputs, event masks, final state, action faults) and, from a second world stepped tick by tick,
    `counts` and `lane_max` as in oracle_run"""
    import oracle_lib as O
    st, tape = quad_start()
    o = O.OracleWorld(quad_cfg(O))
    o.reset()
    o.set_state(copy_state(st))
    outs = [np.array(x) for x in o.rollout(np.array(tape))]
    res = dict(outs=outs, events=np.array(o.event_masks()), state=copy_state(o.get_state()), faults=np.array(o.action_faults()))
    c = O.OracleWorld(quad_cfg(O))
    c.reset()
    c.set_state(copy_state(st))
    cnt = dict.fromkeys(QUAD_SITES, 0)
    lane_max = np.zeros(QUAD_N, dtype=np.int64)
    for t in range(QUAD_T):
        s0 = c.get_state()
        got = c.step(np.array(tape[t]))
        s1, m = c.get_state(), c.event_masks()
        for x, y in zip(got, outs):
            assert np.array_equal(x, y[t]), "oracle: step by step = rollout"
        done = got[3].astype(bool)
        act = np.zeros((QUAD_N, 4, 4), dtype=np.int8)
        act[:, :2] = tape[t]
        bound, launch, _, _ = lane_bounds(O, s0, s1, act, np.ones((QUAD_N, 4), dtype=np.int32), ~done)   # a finished arena shows its next episode in s1
        np.maximum(lane_max, bound.max(-1), out=lane_max)
        cnt["cannon_kill"] += int(np.count_nonzero(m & 0xff))
        cnt["rocket_kill"] += int(np.count_nonzero(m & 0xff00))
        cnt["launch_through_queue"] += int((launch["pre"] == -1).sum())
        cnt["reset"] += int(done.sum())
    # the first tick once more on a world that does not restart: an arena that ends its episode on the crowded tick itself shows the tick's own state
    z = O.OracleWorld(O.make_config(n_arenas=QUAD_N, **dict(QUAD_CFG, auto_reset=False)))
    z.reset()
    z.set_state(copy_state(st))
    z.step(np.array(tape[0]))
    act = np.zeros((QUAD_N, 4, 4), dtype=np.int8)
    act[:, :2] = tape[0]
    first = lane_bounds(O, st, z.get_state(), act, np.ones((QUAD_N, 4), dtype=np.int32), np.ones(QUAD_N, bool))[0]
    res["counts"], res["lane_max"] = cnt, np.maximum(lane_max, first.max(-1))
    return res
