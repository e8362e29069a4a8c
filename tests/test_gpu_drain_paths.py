"""The draw-first drain of the envelope queue changes no bit: the fixtures of test_drain_paths.py (which proves on the CPU that every class of queue
entry the new order treats differently is reached) run on the GPU in every form that compiles drain_envelope_queue_t — the 2-vs-2 worlds in the
default two-wave form, single-wave (HH_NO_TWO=1), the 16-arena two-wave form (HH_APW=16), two waves per SIMD (HH_FORCE_W=2) and on the generic
LDS-exchange kernel (HH_NO_QUAD=1); the HighLevelEnv world on the register-exchange kernels and on the LDS-exchange ones (HH_NO_OCT=1), phase
launches and hh_hl_rollout each — and every tick's obs, reward, valid and done, the event masks, the final state and the action faults are compared
with array_equal against the CPU oracle."""
import numpy as np
import pytest

import hier_crowded as H
import kernel_instances as KI
from test_drain_paths import HL_STEPS, QUAD_CONFIGS, TICKS, copy_state, hier_cfg, hier_oracle_run, hier_start, quad_cfg, quad_oracle_run, quad_start
from test_gpu_kernel_instances import _same_units, _set_switches

pytestmark = pytest.mark.gpu

PRE = {"l3": 1, "l3-general": 0}
FORMS = {
    "default": (dict(), lambda pre: KI._q(1, pre, True, 8, True, pre != 0)),
    "single-wave": (dict(HH_NO_TWO="1"), lambda pre: KI._q(1, pre, False, 16, False, True)),
    "apw16": (dict(HH_APW="16"), lambda pre: KI._q(1, pre, True, 16, False, pre != 0)),
    "force-w2": (dict(HH_FORCE_W="2"), lambda pre: KI._q(2, pre, False, 16, False, True)),
    "no-quad": (dict(HH_NO_QUAD="1"), lambda pre: "hh_k_world<4, 64, 1, false>"),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cfg", list(QUAD_CONFIGS))
def test_quad_drain_changes_no_bit(oracle, monkeypatch, cfg, form):
    import torch
    import hhmarl_2d_amd.world as W
    want = quad_oracle_run(cfg)
    st, tape = quad_start(cfg)
    env, name = FORMS[form]
    _set_switches(monkeypatch, env)
    g = W.World(quad_cfg(W, cfg))
    kernel = g.kernel_instance()
    print(cfg, form, kernel)
    assert kernel == name(PRE[cfg]), f"{cfg}, {form}: the world runs {kernel}"
    g.reset()
    g.set_state(copy_state(st))
    dev = torch.from_numpy(np.array(tape)).cuda()
    what = f"{cfg}, {form} ({kernel})"
    for k in range(2):
        outs = [x.cpu().numpy() for x in g.rollout(dev[k * TICKS:(k + 1) * TICKS].contiguous())]
        for x, y, field in zip(outs, want["launches"][k]["outs"], H.OUTS):
            assert np.array_equal(x, y), f"{what}: launch {k}: {field}"
        assert np.array_equal(g.event_masks(), want["launches"][k]["events"]), f"{what}: launch {k}: event masks"
    got = g.get_state()
    for k in want["state"]:
        assert np.array_equal(got[k], want["state"][k]), f"{what}: state {k}"
    assert np.array_equal(g.action_faults().cpu().numpy(), want["faults"]), f"{what}: action faults"
    g.close()


HIER_FORMS = {
    "oct": (dict(), "hh_k_hier_oct<1, phase>", "hh_k_hier_macro_oct<1, "),
    "lds": (dict(HH_NO_OCT="1"), "hh_k_hier<6, 64, 1>", "hh_k_hier_macro<6, 64, 1, "),
}   # (the macro kernels' last parameters follow the configuration and the arena count: the family and W are what the form selects)


def _after_step(g, outs, ws, what):
    for x, y, field in zip(outs, ws["outs"], H.OUTS):
        assert np.array_equal(x.cpu().numpy(), y), f"{what}: {field}"
    assert np.array_equal(g.event_masks(), ws["events"]), f"{what}: event masks"
    sg = g.get_state()
    for k, y in ws["state"].items():
        assert np.array_equal(sg[k], y), f"{what}: state {k}"


@pytest.mark.parametrize("path", ["phases", "hl_rollout"])
@pytest.mark.parametrize("form", list(HIER_FORMS))
def test_hier_drain_changes_no_bit(oracle, monkeypatch, form, path):
    import torch
    from hhmarl_2d_amd.world import World
    import hhmarl_2d_amd.world as W
    want = hier_oracle_run()
    cmds, tape = hier_start()
    env, phase_name, macro_name = HIER_FORMS[form]
    _set_switches(monkeypatch, env)
    g = World(hier_cfg(W))
    which = 1 if path == "hl_rollout" else 0
    kernel = g.kernel_instance(which)
    print(form, path, kernel)
    assert kernel.startswith(macro_name) if which else kernel == phase_name, f"{form}, {path}: the world runs {kernel}"
    g.reset()
    what = f"hier, {form}, {path} ({kernel})"
    for step in range(2 * HL_STEPS):
        ws = want["steps"][step]
        cmd, tp = torch.from_numpy(np.array(cmds[step])).cuda(), torch.from_numpy(np.array(tape[step])).cuda()
        if path == "hl_rollout":
            outs = g.hl_rollout(cmd, tp)
        else:
            po, pm = g.hl_begin(cmd)
            for k, wt in enumerate(ws["ticks"]):
                _same_units(pm.cpu().numpy(), wt["pm_a"], 6, f"{what}: step {step} sub-step {k}: agents' selector bytes")
                _same_units(po.cpu().numpy(), wt["po_a"], 6, f"{what}: step {step} sub-step {k}: agents' pilot rows")
                po, pm = g.hl_agents_act(tp[k])
                _same_units(pm.cpu().numpy(), wt["pm_o"], 6, f"{what}: step {step} sub-step {k}: opponents' selector bytes")
                _same_units(po.cpu().numpy(), wt["po_o"], 6, f"{what}: step {step} sub-step {k}: opponents' pilot rows")
                po, pm, running = g.hl_tick(tp[k])
                assert running == wt["running"], f"{what}: step {step} sub-step {k}: running"
                assert np.array_equal(g.event_masks(), wt["events"]), f"{what}: step {step} sub-step {k}: event masks"
            outs = g.hl_end()
        _after_step(g, outs, ws, f"{what}: step {step}")
    for x, y in zip(g.episode_stats(), want["stats"]):
        assert np.array_equal(x.cpu().numpy(), y), f"{what}: episode statistics"
    assert not g.action_faults().any() and not want["faults"].any(), f"{what}: action faults"
    g.close()
