"""The select-form sites of the 2-vs-2 tick in front of barrier X change no bit: every fixture of test_quad_select_paths.py (which proves on the
CPU that each rewritten site is reached) runs on the GPU in two launches, in the default form, single-wave (HH_NO_TWO=1) and in the 16-arena
two-wave form (HH_APW=16), and every tick's obs, reward, valid and done, the event masks behind each launch, the final state and the action
faults are compared with array_equal against the CPU oracle."""
import numpy as np
import pytest

from test_quad_select_paths import CASES, LAUNCH, copy_state, make_cfg, oracle_run, start

FORMS = {"default": dict(HH_NO_TWO="0", HH_APW="0"), "single-wave": dict(HH_NO_TWO="1", HH_APW="0"), "apw16": dict(HH_NO_TWO="0", HH_APW="16")}


def _gpu_run(cfg, N):
    import torch
    import hhmarl_2d_amd.world as W
    st, tape = start(cfg, N)
    g = W.World(make_cfg(W, cfg, N))
    g.reset()
    g.set_state(copy_state(st))
    dev = torch.from_numpy(np.array(tape)).cuda()
    launches = []
    for k in range(2):
        outs = [x.cpu().numpy() for x in g.rollout(dev[k * LAUNCH:(k + 1) * LAUNCH].contiguous())]
        launches.append(dict(outs=outs, events=np.array(g.event_masks())))
    res = dict(launches=launches, state=g.get_state(), faults=g.action_faults().cpu().numpy(), kernel=g.kernel_instance())
    g.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cfg,N", CASES)
def test_select_paths_change_no_bit(oracle, monkeypatch, cfg, N, form):
    want = oracle_run(cfg, N)
    monkeypatch.setenv("HH_FORCE_W", "0")
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    got = _gpu_run(cfg, N)
    print(cfg, N, form, got["kernel"])
    if form == "default":
        assert ", true, 8, true, " in got["kernel"], "the 8-arena two-wave form"
        if cfg in ("l3", "l3-stay-done"):
            assert got["kernel"] == "hh_k_world_quad<1, 1, true, 8, true, true>", "the headline instance"
        if cfg == "l3-general":
            assert got["kernel"].startswith("hh_k_world_quad<1, 0, "), "PRE = 0"
    elif form == "single-wave":
        assert ", false, " in got["kernel"], "single-wave form"
    else:
        assert ", true, 16, " in got["kernel"], "the 16-arena two-wave form"
    what = f"{cfg}, {N} arenas, {form} ({got['kernel']})"
    for k in range(2):
        for x, y, field in zip(got["launches"][k]["outs"], want["launches"][k]["outs"], ("obs", "reward", "valid", "done")):
            assert np.array_equal(x, y), f"{what}: launch {k}: {field}"
        assert np.array_equal(got["launches"][k]["events"], want["launches"][k]["events"]), f"{what}: launch {k}: event masks"
    for k in want["state"]:
        assert np.array_equal(got["state"][k], want["state"][k]), f"{what}: state {k}"
    assert np.array_equal(got["faults"], want["faults"]), f"{what}: action faults"
