"""Every row of the table of world-kernel instances (kernel_instances.py) runs on the GPU against the CPU oracle, bit for bit (array_equal
throughout).  The HH_* switches force each form at small arena counts; every row whose instance hh_kernel_instance can name asserts that the
world reports exactly that instance before anything runs, and that World.kernel_name() names the same kernel family.

2-vs-2 rows run the fixtures of test_quad_select_paths.py (which proves on the CPU that each fixture reaches the rare sites of the tick): two
launches of 200 ticks from the injected states, every tick's obs / reward / valid / done, the event masks behind each launch, the final
state and the action faults.  HighLevelEnv rows run 12 commander steps on 170 arenas, the phase path, hh_hl_rollout and the variant-row
launches of one setting from the same tape: every pilot row of the phase path, outputs, state, event masks, eval counters and tick counts.
The last tests create worlds on both sides of every arena count at which the launcher changes form (nothing is launched)."""
import numpy as np
import pytest

import kernel_instances as KI
from helpers import pursuit_actions, random_actions
from test_quad_select_paths import LAUNCH, SEED, copy_state, make_cfg, oracle_run, start

pytestmark = pytest.mark.gpu

OUTS = ("obs", "reward", "valid", "done")


def _set_switches(monkeypatch, env):
    for k in KI.SWITCHES:   # read in hh_world_create: set before the world exists
        monkeypatch.setenv(k, env.get(k, "0"))


def _family(name):
    return name.split("<")[0]


def _check_names(w, row, what):
    if row["printed"] is not None:
        assert w.kernel_instance(row["which"]) == row["printed"], f"{what}: the world reports another instance than the row names"
    assert _family(w.kernel_name()) == _family(w.kernel_instance(0)), f"{what}: kernel_name() and kernel_instance() name different kernel families"


# ------------------------------------------------------------------ 2-vs-2: hh_k_world_quad, hh_k_world
ROLLOUT_CASES = [(r, n) for r in KI.QUAD_ROWS if r["path"] == "rollout" for n in r["sizes"]]
SPLIT_CASES = [(r, n) for r in KI.QUAD_ROWS if r["path"] == "split-step" for n in r["sizes"]]


@pytest.mark.parametrize("row,N", ROLLOUT_CASES, ids=[f"{KI.row_id(r)}-{n}" for r, n in ROLLOUT_CASES])
def test_rollout_row_equals_oracle(oracle, monkeypatch, row, N):
    import torch
    import hhmarl_2d_amd.world as W
    cfg = row["config"]
    want = oracle_run(cfg, N)
    st, tape = start(cfg, N)
    _set_switches(monkeypatch, row["env"])
    g = W.World(make_cfg(W, cfg, N))
    what = f"{KI.row_id(row)}, {N} arenas ({row['printed']})"
    _check_names(g, row, what)
    g.reset()
    g.set_state(copy_state(st))
    dev = torch.from_numpy(np.array(tape)).cuda()
    for k in range(2):
        outs = [x.cpu().numpy() for x in g.rollout(dev[k * LAUNCH:(k + 1) * LAUNCH].contiguous())]
        for x, y, field in zip(outs, want["launches"][k]["outs"], OUTS):
            assert np.array_equal(x, y), f"{what}: launch {k}: {field}"
        assert np.array_equal(g.event_masks(), want["launches"][k]["events"]), f"{what}: launch {k}: event masks"
    got = g.get_state()
    for k in want["state"]:
        assert np.array_equal(got[k], want["state"][k]), f"{what}: state {k}"
    assert np.array_equal(g.action_faults().cpu().numpy(), want["faults"]), f"{what}: action faults"
    g.close()


@pytest.mark.parametrize("row,N", SPLIT_CASES, ids=[f"{KI.row_id(r)}-{n}" for r, n in SPLIT_CASES])
def test_split_step_row_equals_oracle(oracle, monkeypatch, row, N):
    """level 4 with external opponent actions through hh_step_begin / hh_step_finish: hh_k_world<4, 64, 1, true>, which hh_kernel_instance cannot
    name (it names the world's rollout kernel).  150 ticks at horizon 70: every tick's opponent observations, outputs and event masks, one dirtied
    action word on either side, the final state and the action faults."""
    import torch
    from hhmarl_2d_amd.world import World, make_config
    assert row["config"] == "l4-split" and row["printed"] is None
    _set_switches(monkeypatch, row["env"])
    kw = dict(n_arenas=N, seed=SEED, **KI.L4_SPLIT)
    g, o = World(make_config(**kw)), oracle.OracleWorld(oracle.make_config(**kw))
    _check_names(g, row, "split step")
    assert np.array_equal(g.reset().cpu().numpy(), o.reset())
    rng = np.random.default_rng(N)
    dones = 0
    for t in range(150):
        act = pursuit_actions(rng, o.get_state(), 2, 4) if t % 2 else random_actions(rng, (N,), 4)
        if t == 3:
            act[5, 0] = [100, -5, 1, 77]
        if t == 4:
            act[N - 1, 3] = [-1, 9, 2, 0]
        a_ag, a_op = np.ascontiguousarray(act[:, :2]), np.ascontiguousarray(act[:, 2:])
        oo = g.step_begin(torch.from_numpy(a_ag).cuda(), 0).cpu().numpy()
        assert np.array_equal(oo, o.step_begin(a_ag, 0)), f"t={t}: opponents' observations"
        outs = [x.cpu().numpy() for x in g.step_finish(torch.from_numpy(a_op).cuda())]
        for x, y, field in zip(outs, o.step_finish(a_op), OUTS):
            assert np.array_equal(x, y), f"t={t}: {field}"
        assert np.array_equal(g.event_masks(), o.event_masks()), f"t={t}: event masks"
        dones += int(outs[3].sum())
    sg, so = g.get_state(), o.get_state()
    for k in so:
        assert np.array_equal(sg[k], so[k]), f"state {k}"
    faults = o.action_faults()
    assert faults[5] and faults[N - 1] and faults.sum() == 2, "both dirtied words were consumed"
    assert np.array_equal(g.action_faults().cpu().numpy(), faults), "action faults"
    assert dones > N, "episodes end and restart inside the run"
    g.close()


# ------------------------------------------------------------------ HighLevelEnv: hh_k_hier, hh_k_hier_oct, hh_k_hier_oct_v, hh_k_hier_macro, hh_k_hier_macro_oct
HL_SETTINGS = KI.hl_settings()


def _hl_id(env, config):
    return config + "-" + (",".join(f"{k[3:]}={v}" for k, v in sorted(env.items())) or "default")


def _same_units(a, b, nU, what):
    """a: [N, A, ...] of a world (six or ten unit slots), b: [N, nU, ...] of the oracle (exactly the units that exist)"""
    assert np.array_equal(a[:, :nU], b), what
    assert not a[:, nU:].any(), f"{what}: an unused unit slot carries something"


def _hl_compare_after_step(w, o_outs, o_state, o_events, o_eval, ticks, nU, what):
    outs = w["outs"]
    for x, y, field in zip(outs, o_outs, OUTS):
        assert np.array_equal(x.cpu().numpy(), y), f"{what}: {field}"
    g = w["world"]
    assert np.array_equal(g.event_masks(), o_events), f"{what}: event masks"
    sg = g.get_state()
    for k in o_state:
        if k == "ar_i":
            assert np.array_equal(sg[k], o_state[k]), f"{what}: state {k}"
        else:
            assert np.array_equal(sg[k][:, :nU], o_state[k]), f"{what}: state {k}"
    assert not sg["ac_i"][:, nU:, 0].any(), f"{what}: an unused unit slot is alive"
    for x, y, field in zip(g.eval_info(), o_eval, ("last", "total")):
        assert np.array_equal(x.cpu().numpy(), y), f"{what}: eval counters ({field})"
    assert g.hl_tick_count() == ticks, f"{what}: arena-ticks {g.hl_tick_count()}, the oracle ran {ticks}"


@pytest.mark.parametrize("env,config,paths", HL_SETTINGS, ids=[_hl_id(e, c) for e, c, _ in HL_SETTINGS])
def test_highlevel_rows_equal_oracle(oracle, monkeypatch, env, config, paths):
    import torch
    from hhmarl_2d_amd.world import World, make_config
    N = KI.HL_N
    _set_switches(monkeypatch, env)
    kw = dict(n_arenas=N, env_kind=1, seed=8, arena_offset=11, auto_reset=True, **KI.HL_CONFIGS[config])
    o = oracle.OracleWorld(oracle.make_config(**kw))
    nA, nU = o.n_agents, o.A
    worlds = {p: dict(world=World(make_config(**kw))) for p in paths}
    A = next(iter(worlds.values()))["world"].A
    for p, w in worlds.items():
        _check_names(w["world"], paths[p], f"{_hl_id(env, config)} / {p}")
    obs0 = o.reset()
    for p, w in worlds.items():
        assert np.array_equal(w["world"].reset().cpu().numpy(), obs0), f"{p}: reset"
    rng = np.random.default_rng(N)
    dones, ticks, first_done = 0, 0, None
    for step in range(KI.HL_STEPS):
        cmd_h = rng.integers(0, 3, (N, nA)).astype(np.int8)
        tape_h = random_actions(rng, (16, N), A)
        tape_h[..., 2] |= (step % 2)            # every other step everybody keeps the trigger pulled
        cmd, tape = torch.from_numpy(cmd_h).cuda(), torch.from_numpy(tape_h).cuda()
        o.hl_begin(cmd_h)
        if "phases" in worlds:
            po, pm = worlds["phases"]["world"].hl_begin(cmd)
        if "variant-rows" in worlds:
            vo, vm = worlds["variant-rows"]["world"].hl_begin_variants(cmd)
        running_before = N                       # auto-reset worlds: every arena enters the macro step
        for k in range(16):
            what = f"step {step} sub-step {k}"
            ticks += running_before
            act_o = np.ascontiguousarray(tape_h[k][:, :nU])
            po_a, pm_a = o.hl_pilot_obs(0)
            o.hl_agents_act(act_o)
            po_o, pm_o = o.hl_pilot_obs(1)
            running_before = o.hl_tick(act_o)
            events = o.event_masks()
            if "phases" in worlds:
                g = worlds["phases"]["world"]
                _same_units(pm.cpu().numpy(), pm_a, nU, f"{what}: agents' selector bytes")
                _same_units(po.cpu().numpy(), po_a, nU, f"{what}: agents' pilot rows")
                po, pm = g.hl_agents_act(tape[k])
                _same_units(pm.cpu().numpy(), pm_o, nU, f"{what}: opponents' selector bytes")
                _same_units(po.cpu().numpy(), po_o, nU, f"{what}: opponents' pilot rows")
                po, pm, running = g.hl_tick(tape[k])
                assert running == running_before, f"{what}: running {running}, oracle {running_before}"
                assert np.array_equal(g.event_masks(), events), f"{what}: event masks"
            if "variant-rows" in worlds:         # 3-vs-3 only: rows 0..2 the agents, opponent j's variant v at 3 + 4 j + v
                g = worlds["variant-rows"]["world"]
                vm_h, vo_h = vm.cpu().numpy(), vo.cpu().numpy()
                live = pm_a[:, :nA] != 0
                assert np.array_equal(vm_h[:, :nA], pm_a[:, :nA]) and np.array_equal(vo_h[:, :nA][live], po_a[:, :nA][live]), f"{what}: variant rows of the agents"
                ovo, ovm = vo_h[:, 3:].reshape(N, 3, 4, 30), vm_h[:, 3:].reshape(N, 3, 4)
                for j in range(nU - nA):         # the row the opponent's pilot sees once the agents acted is one of its variants
                    on = pm_o[:, nA + j] != 0
                    match = (ovo[:, j] == po_o[:, nA + j][:, None, :]).all(-1) & (ovm[:, j] == pm_o[:, nA + j][:, None])
                    assert match[on].any(-1).all(), f"{what}: opponent {j}: its row is not among the variants"
                vact = np.zeros((N, 15, 4), dtype=np.int8)
                vact[:, :3] = tape_h[k][:, :3]
                for j in range(3):
                    vact[:, 3 + 4 * j:7 + 4 * j] = tape_h[k][:, 3 + j][:, None, :]   # the same action whichever variant matches
                vo, vm, running = g.hl_act_tick(torch.from_numpy(vact).cuda())
                assert running == running_before, f"{what}: variant rows: running {running}, oracle {running_before}"
                assert np.array_equal(g.event_masks(), events), f"{what}: variant rows: event masks"
        o_outs, o_state, o_events, o_eval = o.hl_end(), o.get_state(), o.event_masks(), o.eval_info()
        for p, w in worlds.items():
            g = w["world"]
            w["outs"] = g.hl_rollout(cmd, tape) if p == "hl_rollout" else g.hl_end()
            _hl_compare_after_step(w, o_outs, o_state, o_events, o_eval, ticks, nU, f"{_hl_id(env, config)} / {p}: step {step}")
        dones += int(o_outs[3].sum())
        if first_done is None and o_outs[3].any():
            first_done = step
    print(_hl_id(env, config), "first done in step", first_done, "dones", dones, "arena-ticks", ticks)
    assert dones > 0, "no episode ended inside the compared steps"
    assert ticks < KI.HL_STEPS * 16 * N, "arenas do leave their macro step early"
    o_stats = o.episode_stats()
    for p, w in worlds.items():
        for x, y in zip(w["world"].episode_stats(), o_stats):
            assert np.array_equal(x.cpu().numpy(), y), f"{p}: episode statistics"
        assert not w["world"].action_faults().any()
        w["world"].close()


# ------------------------------------------------------------------ the arena counts at which the launcher changes form (creation only)
def _n_simd():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 4


def _created(monkeypatch, env, **kw):
    from hhmarl_2d_amd.world import World, make_config
    _set_switches(monkeypatch, env)
    w = World(make_config(**kw))
    got = (w.kernel_instance(0), w.kernel_instance(1) if kw.get("env_kind") == 1 else None, w.kernel_name())
    w.close()
    assert _family(got[0]) == _family(got[2]), got
    return got


def test_dispatch_boundaries_2v2(monkeypatch):
    """level 3 (the headline preset), no switch set: 8 -> 16 arenas per wave where the 8-arena two-wave form stops fitting one wave per SIMD
    (2 * ceil(N / 8) <= n_simd), two-wave -> single-wave where the workgroups stop having a SIMD pair each (ceil(N / 16) <= n_simd / 2),
    W = 1 -> 2 where there are more waves than SIMDs (ceil(N / 16) > n_simd)"""
    S = _n_simd()
    assert S >= 8 and S % 2 == 0
    inst = lambda N: _created(monkeypatch, {}, n_arenas=N, level=3)[0]
    n = 8 * (S // 2)
    assert inst(n) == "hh_k_world_quad<1, 1, true, 8, true, true>" and inst(n + 1) == "hh_k_world_quad<1, 1, true, 16, false, true>"
    n = 16 * (S // 2)
    assert inst(n) == "hh_k_world_quad<1, 1, true, 16, false, true>" and inst(n + 1) == "hh_k_world_quad<1, 1, false, 16, false, true>"
    n = 16 * S
    assert inst(n) == "hh_k_world_quad<1, 1, false, 16, false, true>" and inst(n + 1) == "hh_k_world_quad<2, 1, false, 16, false, true>"
    # the presets of levels 1 / 2 and of escape mode above it: what a user gets by default at large N
    assert _created(monkeypatch, {}, n_arenas=n + 1, level=1)[0] == "hh_k_world_quad<2, 2, false, 16, false, true>"
    assert _created(monkeypatch, {}, n_arenas=n + 1, level=2)[0] == "hh_k_world_quad<2, 3, false, 16, false, true>"
    assert _created(monkeypatch, {}, n_arenas=n + 1, level=3, agent_mode=1)[0] == "hh_k_world_quad<2, 4, false, 16, false, true>"
    # the generic kernel changes W at the same count
    assert _created(monkeypatch, dict(HH_NO_QUAD="1"), n_arenas=n, level=3)[0] == "hh_k_world<4, 64, 1, false>"
    assert _created(monkeypatch, dict(HH_NO_QUAD="1"), n_arenas=n + 1, level=3)[0] == "hh_k_world<4, 64, 2, false>"


def test_dispatch_boundaries_highlevel(monkeypatch):
    """the register-exchange forms go to two waves per SIMD by the 8-arena grid (ceil(N / 8) > n_simd); under HH_NO_OCT=1 the LDS macro step leaves
    its 8-arena form at the same count, and the LDS forms go to two waves per SIMD by the 10-arena grid (ceil(N / 10) > n_simd)"""
    S = _n_simd()
    hl = lambda env, N: _created(monkeypatch, env, n_arenas=N, env_kind=1)[:2]
    n = 8 * S
    assert hl({}, n) == ("hh_k_hier_oct<1, phase>", "hh_k_hier_macro_oct<1, true>")
    assert hl({}, n + 1) == ("hh_k_hier_oct<2, phase>", "hh_k_hier_macro_oct<2, true>")
    assert hl({}, 10 * S + 1) == ("hh_k_hier_oct<2, phase>", "hh_k_hier_macro_oct<2, true>")
    lds = dict(HH_NO_OCT="1")
    assert hl(lds, n) == ("hh_k_hier<6, 64, 1>", "hh_k_hier_macro<6, 64, 1, true, 8>")
    assert hl(lds, n + 1) == ("hh_k_hier<6, 64, 1>", "hh_k_hier_macro<6, 64, 1, true, 10>")
    n = 10 * S
    assert hl(lds, n) == ("hh_k_hier<6, 64, 1>", "hh_k_hier_macro<6, 64, 1, true, 10>")
    assert hl(lds, n + 1) == ("hh_k_hier<6, 64, 2>", "hh_k_hier_macro<6, 64, 2, true, 10>")
    # n-vs-m arenas keep the W = 1 phase kernel of the LDS form (its W = 2 instance stages the pilot rows per side of three)
    assert _created(monkeypatch, lds, n_arenas=n + 1, env_kind=1, n_agents=2, n_opps=3)[0] == "hh_k_hier<6, 64, 1>"
