"""Gradient clipping by global norm without a GPU: the sequential float64 restatement (tests/grad_clip_ref.py) against
torch.nn.utils.clip_grad_norm_, the torch-op forms against the restatement, the learners' grad_clip validation, and the C ABI's
declarations against include/hh_learner.h and the library."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import grad_clip_ref as GR
from hhmarl_2d_amd import _lib
from hhmarl_2d_amd import learner as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEARNERS = [(LR.CommanderLearner, (None, "cpu")), (LR.PPOLearner, ((0, 1), None, "cpu"))]


@pytest.fixture(scope="module")
def grads():
    return GR.grad_list(60, seed=21)


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("frac", (0.5, 2.0))
def test_restatement_equals_clip_grad_norm_in_float64(grads, frac):
    """the norm within n x 2^-53 relative (a float64 sum of non-negative terms in any order), the scaled gradients within the same bound"""
    n = sum(g.size for g in grads)
    assert n > 20000 and GR.bound(grads) == n * 2.0 ** -53
    norm0, _ = GR.norm_coef(grads, 1.0)
    max_norm = frac * norm0
    norm, coef = GR.norm_coef(grads, max_norm)
    params = [torch.nn.Parameter(torch.zeros(g.size, dtype=torch.float64)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.astype(np.float64))
    got = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    assert _rel(norm, got) <= GR.bound(grads)
    assert (coef < 1.0) == (frac < 1.0)
    for p, g in zip(params, grads):
        want = g.astype(np.float64) * coef
        assert np.all(np.abs(p.grad.numpy() - want) <= GR.bound(grads) * np.abs(want))


def test_grad_norm_torch_equals_the_restatement(grads):
    for max_norm in (1.0, 1e9):
        norm, coef = LR.grad_norm_torch([torch.from_numpy(g) for g in grads], max_norm)
        want_norm, want_coef = GR.norm_coef(grads, max_norm)
        assert norm.dtype == torch.float64 and coef.dtype == torch.float64
        assert _rel(float(norm), want_norm) <= GR.bound(grads)
        assert _rel(float(coef), want_coef) <= GR.bound(grads) + 4 * GR.U
    assert float(coef) == 1.0
    norm, coef = LR.grad_norm_torch([torch.zeros(5), torch.zeros(0)], 1.0)
    assert (float(norm), float(coef)) == (0.0, 1.0)
    norm, coef = LR.grad_norm_torch([], 1.0)
    assert (float(norm), float(coef)) == (0.0, 1.0)


def test_adam_step_torch_with_clip_equals_scaled_gradients(grads):
    gs = grads[:12]
    clip = LR.grad_norm_torch([torch.from_numpy(g) for g in gs], 0.25 * GR.norm_coef(gs, 1.0)[0])
    assert float(clip[1]) < 1.0

    def state():
        rng = np.random.default_rng(5)
        return ([torch.from_numpy((0.1 * rng.standard_normal(g.size)).astype(np.float32)) for g in gs],
                [torch.zeros(g.size) for g in gs], [torch.zeros(g.size) for g in gs])
    (pa, ma, va), (pb, mb, vb) = state(), state()
    tg = [torch.from_numpy(g.copy()) for g in gs]
    for t in range(3):
        LR.adam_step_torch(pa, tg, ma, va, t, lr=1e-3, clip=clip)
        LR.adam_step_torch(pb, [torch.from_numpy(s) for s in GR.scaled(gs, float(clip[1]))], mb, vb, t, lr=1e-3)
    for a, b in zip(pa + ma + va, pb + mb + vb):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    assert all(np.array_equal(t_.numpy(), g) for t_, g in zip(tg, gs)), "the gradients keep their unscaled values"


@pytest.mark.parametrize("learner,args", LEARNERS)
def test_grad_clip_is_validated_after_the_modes(learner, args):
    for bad in (0, -1.0, float("inf"), float("nan"), "1"):
        with pytest.raises(ValueError, match="grad_clip"):
            learner(*args, grad_clip=bad)
        with pytest.raises(ValueError, match="grad_clip"):
            learner(*args, optimizer="fused", step="graph", grad_clip=bad)
    with pytest.raises(ValueError, match="optimizer is one of"):
        learner(*args, optimizer="adam", grad_clip=-1)
    with pytest.raises(ValueError, match='needs optimizer="fused"'):
        learner(*args, step="graph", grad_clip=-1)
    params = list(inspect.signature(learner.__init__).parameters.values())
    assert params[-1].name == "grad_clip" and params[-1].default is None
    assert LR._grad_clip(None) is None and LR._grad_clip(2) == 2.0 and LR._grad_clip(0.5) == 0.5


def test_device_adam_takes_max_norm_last():
    params = list(inspect.signature(LR.DeviceAdam.__init__).parameters.values())
    assert [p.name for p in params] == ["self", "params", "lr", "betas", "eps", "max_norm"] and params[-1].default is None
    for f in (LR.adam_step, LR.adam_step_torch):
        assert inspect.signature(f).parameters["clip"].default is None
    assert list(inspect.signature(LR.grad_norm).parameters)[:5] == ["grads", "max_norm", "clip", "cursor", "table"]


def test_the_header_declares_the_three_functions_and_the_library_exports_them():
    txt = open(os.path.join(ROOT, "include", "hh_learner.h")).read()
    assert re.search(r"^#define HH_CLIP_OUT 2\b", txt, re.M) and _lib.CLIP_OUT == 2
    assert int(re.search(r"#define HH_PPO_STATS (\d+)", txt).group(1)) == 6 == len(_lib.PPO_STATS)
    want = {"hh_grad_norm_scratch_bytes": 3, "hh_grad_norm": 10, "hh_adam_step_clipped": 9}
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for sym, n_args in want.items():
        m = re.search(r"^int " + sym + r"\((.*?)\);", txt, re.M | re.S)
        assert m and len(m.group(1).split(",")) == n_args, sym
        assert sym in _lib.LEARNER_EXPORTS and hasattr(lib, sym), f"libhh_world.so does not export {sym}"
        assert len(getattr(L, sym).argtypes) == n_args
    src = open(os.path.join(ROOT, "hhmarl_2d_amd", "csrc", "hh_world.hip")).read()
    assert src.index('#include "hh_train_step.h"') < src.index('#include "hh_grad_clip.h"')
