"""hh_chunk_attn_forward / _backward and hh_residual_normalize_forward / _backward on the MI355X (include/hh_learner.h) through
learner.chunk_attention / residual_normalize: results and gradients against float64 CPU autograd of the torch-op restatements
(tests/chunk_attn_ref.py), the same bytes on every run, nothing written past the last sequence / row, refused arguments.

The bound is the project's (test_gpu_ppo_loss.py, test_gpu_gru_seq.py): per compared tensor, errors as max |difference| / max |reference|,
e32 = the error of the float32 torch-op restatement on the device on the same inputs, and the kernel may be at most 4 x e32 away.
Where e32 is 0 (one key: softmax is exactly 1.0f) ctx must equal the v columns bit for bit."""
import ctypes as C

import pytest
import torch

import chunk_attn_ref as REF

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5


def _lib():
    from hhmarl_2d_amd import _lib as L
    return L, L.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


_p = lambda t: C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("scale", REF.SCALES)
@pytest.mark.parametrize("E", (100, 150))
@pytest.mark.parametrize("Lm", (1, 2, 19, 20, 32))
@pytest.mark.parametrize("S", (1, 3, 65, 1027))
def test_core_against_float64(S, Lm, E, scale):
    from hhmarl_2d_amd import learner as LR
    qkv, d_ctx = REF.core_inputs(S, Lm, E, scale)
    want = REF.core_reference(S, Lm, E, scale)
    t32 = REF.core_run(qkv, d_ctx, torch.float32, "cuda")
    got = REF.core_run(qkv, d_ctx, torch.float32, "cuda", fn=LR.chunk_attention)
    for name, k, c, w in zip(("ctx", "d_qkv"), got, t32, want):
        assert torch.isfinite(k).all()
        e_k, e_32 = REF.rel_err(k, w), REF.rel_err(c, w)
        print(f"S={S} L={Lm} E={E} scale={scale} {name}: max |ref| {w.abs().max().item():.3e}; relative error of the float32 torch ops {e_32:.3e}, "
              f"of the kernel {e_k:.3e}")
        assert e_k <= 4.0 * e_32, f"{name}: kernel error {e_k:.3e} above 4 x {e_32:.3e}"
    if Lm == 1:
        assert torch.equal(got[0].float().view(torch.int32), qkv[..., 2 * E:].contiguous().view(torch.int32)), "one key: ctx is the v columns, bit for bit"


def _norm_check(R, E, zero_row):
    from hhmarl_2d_amd import learner as LR
    x, a, d_y = REF.norm_inputs(R, E, zero_row)
    want = REF.norm_reference(R, E, zero_row)
    t32 = REF.norm_run(x, a, d_y, torch.float32, "cuda")
    got = REF.norm_run(x, a, d_y, torch.float32, "cuda", fn=LR.residual_normalize)
    keep = torch.ones(R, dtype=torch.bool)
    if zero_row is not None:
        keep[zero_row] = False
        assert torch.equal(got[0][zero_row], torch.zeros(E, dtype=torch.float64)), "a = -x: y is exactly 0"
        assert torch.isfinite(got[1][zero_row]).all() and got[1][zero_row].abs().max().item() > 0
    assert torch.equal(got[1], got[2]), "x and a receive the same gradient"
    if not keep.any():
        return
    for name, k, c, w in zip(("y", "d_s"), got[:2], t32[:2], want[:2]):
        assert torch.isfinite(k).all()
        e_k, e_32 = REF.rel_err(k[keep], w[keep]), REF.rel_err(c[keep], w[keep])
        print(f"R={R} E={E} zero row {zero_row} {name}: relative error of the float32 torch ops {e_32:.3e}, of the kernel {e_k:.3e}")
        assert e_k <= 4.0 * e_32, f"{name}: kernel error {e_k:.3e} above 4 x {e_32:.3e}"


@pytest.mark.parametrize("E", (100, 150))
@pytest.mark.parametrize("R", (1, 63, 1300))
def test_normalize_against_float64(R, E):
    """one row has a = -x (y exactly 0.0, a finite d_s; that row alone is left out of the ratio).  At R = 1 that row would be the whole
    case, so R = 1 runs twice: with the zero row, and without it for the ratio"""
    _norm_check(R, E, R // 2)
    if R == 1:
        _norm_check(R, E, None)


def test_normalize_keeps_leading_dimensions():
    from hhmarl_2d_amd import learner as LR
    x, a, _ = REF.norm_inputs(63, 150, 31)
    x3, a3 = x[:60].reshape(3, 20, 150).cuda(), a[:60].reshape(3, 20, 150).cuda()
    assert torch.equal(LR.residual_normalize(x3, a3).reshape(60, 150), LR.residual_normalize(x[:60].cuda(), a[:60].cuda()))


# ---------------------------------------------------------------------------------------------------------------- bytes
@pytest.mark.parametrize("S,Lm,E", [(3, 19, 150), (65, 20, 100), (1027, 32, 150)])
def test_core_two_runs_same_bytes_and_nothing_past_the_last_sequence(S, Lm, E):
    L, lib, st = _lib()
    qkv, d_ctx = (t.cuda() for t in REF.core_inputs(S, Lm, E, 3.0))
    runs = []
    for _ in range(2):
        ctx = torch.full((S + 1, Lm, E), SENTINEL, device="cuda")
        d_qkv = torch.full((S + 1, Lm, 3 * E), SENTINEL, device="cuda")
        L.check(lib.hh_chunk_attn_forward(S, Lm, E, _p(qkv), _p(ctx), st))
        L.check(lib.hh_chunk_attn_backward(S, Lm, E, _p(qkv), _p(d_ctx), _p(d_qkv), st))
        torch.cuda.synchronize()
        for t in (ctx, d_qkv):
            assert (t[S] == SENTINEL).all() and (t[:S] != SENTINEL).all() and torch.isfinite(t).all()
        runs.append((ctx, d_qkv))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs))


@pytest.mark.parametrize("R,E", [(1, 100), (63, 150), (1300, 100)])
def test_normalize_two_runs_same_bytes_and_nothing_past_the_last_row(R, E):
    L, lib, st = _lib()
    x, a, d_y = (t.cuda() for t in REF.norm_inputs(R, E, R // 2))
    runs = []
    for _ in range(2):
        y, d_s = torch.full((R + 1, E), SENTINEL, device="cuda"), torch.full((R + 1, E), SENTINEL, device="cuda")
        norm = torch.full((R + 1,), SENTINEL, device="cuda")
        L.check(lib.hh_residual_normalize_forward(R, E, _p(x), _p(a), _p(y), _p(norm), st))
        L.check(lib.hh_residual_normalize_backward(R, E, _p(y), _p(norm), _p(d_y), _p(d_s), st))
        torch.cuda.synchronize()
        for t in (y, d_s, norm):
            assert (t[R] == SENTINEL).all() and (t[:R] != SENTINEL).all() and torch.isfinite(t).all()
        runs.append((y, d_s, norm))
    assert all(torch.equal(a_.view(torch.int32), b_.view(torch.int32)) for a_, b_ in zip(*runs))


# ---------------------------------------------------------------------------------------------------------------- refused arguments
def test_bad_arguments_are_refused_and_launch_nothing():
    from hhmarl_2d_amd import learner as LR
    L, lib, st = _lib()
    S, Lm = 3, 20
    qkv = torch.randn((S, 32, 450), device="cuda")            # large enough for every shape tried below
    d_ctx = torch.randn((S, 32, 150), device="cuda")
    ctx, d_qkv = torch.full_like(d_ctx, SENTINEL), torch.full_like(qkv, SENTINEL)
    for embed, ln in ((96, Lm), (100, 0), (150, 33), (128, Lm), (100, -1)):
        assert lib.hh_chunk_attn_forward(S, ln, embed, _p(qkv), _p(ctx), st) == -1             # HH_E_ARG
        assert b"hh_chunk_attn_forward" in lib.hh_last_error()
        assert lib.hh_chunk_attn_backward(S, ln, embed, _p(qkv), _p(d_ctx), _p(d_qkv), st) == -1
        assert b"hh_chunk_attn_backward" in lib.hh_last_error()
    assert lib.hh_chunk_attn_forward(-1, Lm, 100, _p(qkv), _p(ctx), st) == -1
    assert lib.hh_chunk_attn_forward(S, Lm, 100, None, _p(ctx), st) == -1 and lib.hh_chunk_attn_forward(S, Lm, 100, _p(qkv), _p(qkv), st) == -1
    assert lib.hh_chunk_attn_backward(S, Lm, 100, _p(qkv), _p(d_ctx), None, st) == -1
    x, y, norm = torch.randn((8, 150), device="cuda"), torch.full((8, 150), SENTINEL, device="cuda"), torch.full((8,), SENTINEL, device="cuda")
    for width in (128, 96, 0):
        assert lib.hh_residual_normalize_forward(8, width, _p(x), _p(x), _p(y), _p(norm), st) == -1
        assert b"hh_residual_normalize_forward" in lib.hh_last_error()
        assert lib.hh_residual_normalize_backward(8, width, _p(x), _p(norm), _p(x), _p(y), st) == -1
        assert b"hh_residual_normalize_backward" in lib.hh_last_error()
    assert lib.hh_residual_normalize_forward(8, 150, _p(x), _p(x), _p(x), _p(norm), st) == -1        # the output over an input
    assert lib.hh_residual_normalize_forward(8, 150, _p(x), None, _p(y), _p(norm), st) == -1
    torch.cuda.synchronize()
    for t in (ctx, d_qkv, y, norm):
        assert (t == SENTINEL).all(), "a refused call wrote something"
    # zero sequences / rows: success without a launch, pointers not even looked at
    assert lib.hh_chunk_attn_forward(0, Lm, 100, None, None, st) == 0 and lib.hh_chunk_attn_backward(0, Lm, 150, None, None, None, st) == 0
    assert lib.hh_residual_normalize_forward(0, 100, None, None, None, None, st) == 0
    assert lib.hh_residual_normalize_backward(0, 150, None, None, None, None, st) == 0
    out = LR.chunk_attention(torch.zeros((0, 20, 300), device="cuda"))
    assert tuple(out.shape) == (0, 20, 100) and out.dtype == torch.float32
    # the Python wrappers: contiguous float32 CUDA tensors of a compiled width only
    good = torch.randn((4, 20, 300), device="cuda")
    for bad in (good.double(), good.transpose(0, 1), good[..., :297], good.cpu(), torch.randn((4, 20, 288), device="cuda"),
                torch.randn((4, 33, 300), device="cuda"), good[0]):
        with pytest.raises(ValueError):
            LR.chunk_attention(bad)
    h = torch.randn((4, 20, 100), device="cuda")
    for bx, ba in ((h.double(), h.double()), (h.transpose(0, 1), h.transpose(0, 1)), (h, h[:2]), (h.cpu(), h.cpu()), (h, h.double()),
                   (torch.randn((4, 128), device="cuda"),) * 2):
        with pytest.raises(ValueError):
            LR.residual_normalize(bx, ba)
