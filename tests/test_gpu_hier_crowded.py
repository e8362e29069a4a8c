"""Every HighLevelEnv kernel instance on crowded arenas, bit for bit against the CPU oracle (array_equal throughout): the fixtures of
hier_crowded.py — columns, opposed clusters, rockets about to fuse and launches on the edge of the missile cone, laid out through set_state so
that one lane queues up to 1 launch + 9 cannon candidates + 2 fuses and a whole wave queues at once — run on every setting of the table of
kernel instances (kernel_instances.hl_settings(): the switches x general / default / 4v4) and on every call path the setting has: the phase
launches (hl_begin / hl_agents_act / hl_tick / hl_end), hh_hl_rollout and, 3-vs-3, the variant-row launches.  test_hier_crowded.py proves on the
CPU that the fixtures reach what they are built for (a lane past 8 entries whose ninth entry decides a kill, targets in slots 8 and 9, both
fuses, several kills by one shooter, mutual and friendly kills, an undecided launch that passes and one that is refused).

The six-slot settings run the 3-vs-3 fixture of their configuration; the ten-slot setting runs 4-vs-4, 5-vs-5 and 5-vs-4.  Compared: every
sub-tick's pilot rows and selector bytes of both sides, `running` and event masks on the phase path (variant rows: the agents' rows, that every
opponent's row is among its variants, `running`, event masks); behind every step on every path the four outputs, the full state (five-entry
target lists on ten slots), event masks, eval counters and the arena-tick count; at the end episode statistics and that no action faulted.
Unused unit slots stay empty, and the untouched arenas beside the crowded ones equal what the oracle gives them in a world where no arena is
laid out."""
import numpy as np
import pytest

import hier_crowded as H
import kernel_instances as KI
from test_gpu_kernel_instances import _check_names, _hl_id, _same_units, _set_switches

pytestmark = pytest.mark.gpu

FIXTURES = {"general": [((3, 3), False)], "default": [((3, 3), True)], "4v4": [((4, 4), False), ((5, 5), False), ((5, 4), False)]}
CASES = [(env, config, paths, key) for env, config, paths in KI.hl_settings() for key in FIXTURES[config]]


def _after_step(g, outs, want, untouched, nU, sel, what):
    for x, y, z, field in zip(outs, want["outs"], untouched["outs"], H.OUTS):
        x = x.cpu().numpy()
        assert np.array_equal(x, y), f"{what}: {field}"
        assert np.array_equal(x[sel], z[sel]), f"{what}: {field} of the untouched arenas"
    ev = g.event_masks()
    assert np.array_equal(ev, want["events"]), f"{what}: event masks"
    assert np.array_equal(ev[sel], untouched["events"][sel]), f"{what}: event masks of the untouched arenas"
    sg = g.get_state()
    for k, y in want["state"].items():
        if k == "ar_i":
            assert np.array_equal(sg[k], y), f"{what}: state {k}"
            assert np.array_equal(sg[k][sel], untouched["state"][k][sel]), f"{what}: state {k} of the untouched arenas"
        else:
            assert np.array_equal(sg[k][:, :nU], y), f"{what}: state {k}"
            assert np.array_equal(sg[k][sel][:, :nU], untouched["state"][k][sel]), f"{what}: state {k} of the untouched arenas"
    # an unused unit slot stays empty: never alive, no burst, nothing in flight, no targets (a reset leaves harmless operands in its type and magazine size)
    assert not sg["ac_i"][:, nU:][:, :, [0, 3, 8, 9]].any(), f"{what}: an unused unit slot is alive, fires, carries a missile or has a target"
    for k in ("rk_i", "rk_f", "tgt_id", "tgt_d"):
        assert not sg[k][:, nU:].any(), f"{what}: state {k}: an unused unit slot carries something"
    for x, y, field in zip(g.eval_info(), want["eval"], ("last", "total")):
        assert np.array_equal(x.cpu().numpy(), y), f"{what}: eval counters ({field})"
    assert g.hl_tick_count() == want["tick_count"], f"{what}: arena-ticks {g.hl_tick_count()}, the oracle ran {want['tick_count']}"


QUAD_ROWS = [("hh_k_world<4, 64, 1, false>", dict(HH_NO_QUAD="1")), ("hh_k_world<4, 64, 2, false>", dict(HH_NO_QUAD="1", HH_FORCE_W="2")),
             ("hh_k_world_quad", dict())]   # the last: the 2-vs-2 kernel a world of this size runs by default


@pytest.mark.parametrize("instance,env", QUAD_ROWS, ids=[",".join(f"{k[3:]}={v}" for k, v in sorted(e.items())) or "default" for _, e in QUAD_ROWS])
def test_crowded_quad_arenas_equal_oracle(oracle, monkeypatch, instance, env):
    """the 2-vs-2 fixture (1 launch + 3 cannon candidates + 2 fuses on one lane) through rollout on the generic kernel, W = 1 and 2, and on the
    2-vs-2 kernel a world of this size runs by default"""
    import torch
    import hhmarl_2d_amd.world as W
    want = H.quad_oracle_run()
    st, tape = H.quad_start()
    _set_switches(monkeypatch, env)
    g = W.World(H.quad_cfg(W))
    print(env, g.kernel_instance(0), "lane_entries_max", int(want["lane_max"].max()))
    if env:
        assert g.kernel_instance(0) == instance
    else:
        assert g.kernel_instance(0).startswith("hh_k_world_quad<")
    g.reset()
    g.set_state(H.copy_state(st))
    outs = [x.cpu().numpy() for x in g.rollout(torch.from_numpy(np.array(tape)).cuda())]
    for x, y, field in zip(outs, want["outs"], H.OUTS):
        assert np.array_equal(x, y), f"{instance}: {field}"
    assert np.array_equal(g.event_masks(), want["events"]), f"{instance}: event masks"
    got = g.get_state()
    for k in want["state"]:
        assert np.array_equal(got[k], want["state"][k]), f"{instance}: state {k}"
    assert np.array_equal(g.action_faults().cpu().numpy(), want["faults"]), f"{instance}: action faults"
    g.close()


@pytest.mark.parametrize("env,config,paths,key", CASES, ids=[f"{_hl_id(e, c)}-{H.key_id(k)}" for e, c, _, k in CASES])
def test_crowded_arenas_equal_oracle(oracle, monkeypatch, env, config, paths, key):
    import torch
    from hhmarl_2d_amd.world import World, make_config
    sides, default = key
    nA, nU = sides[0], sum(sides)
    assert H.cfg_kwargs(key)["horizon"] == KI.HL_CONFIGS[config]["horizon"], "the fixture runs the configuration the setting's instances are compiled for"
    want, untouched = H.oracle_run(sides, default), H.untouched_run(sides, default)
    _, cmds, tape = H.start(sides, default)
    sel = np.arange(H.N) % 7 == 6
    _set_switches(monkeypatch, env)
    worlds = {p: World(make_config(**H.cfg_kwargs(key))) for p in paths}
    A = next(iter(worlds.values())).A
    assert A == H.slots_of(key) and ("variant-rows" not in worlds or sides == (3, 3))
    name = f"{_hl_id(env, config)} / {H.key_id(key)}"
    for p, g in worlds.items():
        _check_names(g, paths[p], f"{name} / {p}")
        g.reset()
    print(name, {p: g.kernel_instance(paths[p]["which"]) for p, g in worlds.items()}, "lane_entries_max", int(want["lane_max"].max()),
          "arena-ticks", want["steps"][-1]["tick_count"])
    for step in range(H.STEPS):
        ws = want["steps"][step]
        cmd, tp = torch.from_numpy(np.array(cmds[step])).cuda(), torch.from_numpy(np.array(tape[step])).cuda()
        if step < 2:
            for g in worlds.values():
                g.set_state(H.pad_state(want["injected"][step], A))
        if "phases" in worlds:
            po, pm = worlds["phases"].hl_begin(cmd)
        if "variant-rows" in worlds:
            vo, vm = worlds["variant-rows"].hl_begin_variants(cmd)
        for k, wt in enumerate(ws["ticks"]):
            what = f"{name}: step {step} sub-step {k}"
            if "phases" in worlds:
                g = worlds["phases"]
                _same_units(pm.cpu().numpy(), wt["pm_a"], nU, f"{what}: agents' selector bytes")
                _same_units(po.cpu().numpy(), wt["po_a"], nU, f"{what}: agents' pilot rows")
                po, pm = g.hl_agents_act(tp[k])
                _same_units(pm.cpu().numpy(), wt["pm_o"], nU, f"{what}: opponents' selector bytes")
                _same_units(po.cpu().numpy(), wt["po_o"], nU, f"{what}: opponents' pilot rows")
                po, pm, running = g.hl_tick(tp[k])
                assert running == wt["running"], f"{what}: running {running}, oracle {wt['running']}"
                assert np.array_equal(g.event_masks(), wt["events"]), f"{what}: event masks"
            if "variant-rows" in worlds:         # 3-vs-3 only: rows 0..2 the agents, opponent j's variant v at 3 + 4 j + v
                g = worlds["variant-rows"]
                vm_h, vo_h = vm.cpu().numpy(), vo.cpu().numpy()
                pm_a, po_a, pm_o, po_o = wt["pm_a"], wt["po_a"], wt["pm_o"], wt["po_o"]
                live = pm_a[:, :nA] != 0
                assert np.array_equal(vm_h[:, :nA], pm_a[:, :nA]) and np.array_equal(vo_h[:, :nA][live], po_a[:, :nA][live]), f"{what}: variant rows of the agents"
                ovo, ovm = vo_h[:, 3:].reshape(H.N, 3, 4, 30), vm_h[:, 3:].reshape(H.N, 3, 4)
                for j in range(nU - nA):         # the row the opponent's pilot sees once the agents acted is one of its variants
                    on = pm_o[:, nA + j] != 0
                    match = (ovo[:, j] == po_o[:, nA + j][:, None, :]).all(-1) & (ovm[:, j] == pm_o[:, nA + j][:, None])
                    assert match[on].any(-1).all(), f"{what}: opponent {j}: its row is not among the variants"
                vact = np.zeros((H.N, 15, 4), dtype=np.int8)
                vact[:, :3] = tape[step][k][:, :3]
                for j in range(3):
                    vact[:, 3 + 4 * j:7 + 4 * j] = tape[step][k][:, 3 + j][:, None, :]   # the same action whichever variant matches
                vo, vm, running = g.hl_act_tick(torch.from_numpy(vact).cuda())
                assert running == wt["running"], f"{what}: variant rows: running {running}, oracle {wt['running']}"
                assert np.array_equal(g.event_masks(), wt["events"]), f"{what}: variant rows: event masks"
        for p, g in worlds.items():
            outs = g.hl_rollout(cmd, tp) if p == "hl_rollout" else g.hl_end()
            _after_step(g, outs, ws, untouched["steps"][step], nU, sel, f"{name} / {p}: step {step}")
    for p, g in worlds.items():
        for x, y, z in zip(g.episode_stats(), want["stats"], untouched["stats"]):
            assert np.array_equal(x.cpu().numpy(), y), f"{name} / {p}: episode statistics"
            assert np.array_equal(x.cpu().numpy()[sel], z[sel]), f"{name} / {p}: episode statistics of the untouched arenas"
        assert not g.action_faults().any() and not want["faults"].any(), f"{name} / {p}: action faults"
        g.close()
