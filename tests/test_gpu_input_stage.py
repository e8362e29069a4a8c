"""hh_input_stage_forward / _backward on the MI355X (include/hh_learner.h), through learner.input_stage and through the C ABI: the ten
stages of the trainable networks against float64 CPU autograd of the torch-op restatement (tests/input_stage_ref.py), a row count that
makes the grid-stride walk and the partial-sum cap wrap, the same bytes on every run, nothing written outside a group's columns and
rows, a strided source, refused arguments.

The bound is the project's (test_gpu_ppo_loss.py, test_gpu_chunk_attention.py): per compared tensor, errors as max |difference| /
max |reference|, e32 = the error of the float32 torch-op restatement on the device on the same inputs, and the kernel may be at most
4 x e32 away; where e32 is 0 the kernel must match the float32 restatement bit for bit."""
import ctypes as C

import pytest
import torch

import input_stage_ref as REF

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
E_ARG = -1


def _lib():
    from hhmarl_2d_amd import _lib as L
    return L, L.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


_p = lambda t: C.c_void_p(t.data_ptr())


def _check_against_float64(net, side, R):
    from hhmarl_2d_amd import learner as LR
    inp = REF.inputs(net, side, R)
    want = REF.reference(net, side, R)
    t32 = REF.run(net, side, inp, torch.float32, "cuda")
    got = REF.run(net, side, inp, torch.float32, "cuda", fn=LR.input_stage)
    worst = 0.0
    for name, ks, cs, ws in zip(("y", "d_w", "d_b"), got, t32, want):
        for layer, k, c, w in zip(REF.case(net, side)["layers"], ks, cs, ws):
            assert k.shape == w.shape and torch.isfinite(k).all()
            e_k, e_32 = REF.rel_err(k, w), REF.rel_err(c, w)
            print(f"{net} {side} R={R} {layer} {name}: max |ref| {w.abs().max().item():.3e}; relative error of the float32 torch ops {e_32:.3e}, "
                  f"of the kernel {e_k:.3e}")
            if e_32 == 0.0:
                assert torch.equal(k, c), f"{layer} {name}: the float32 torch ops are exact here and the kernel is not"
            else:
                assert e_k <= 4.0 * e_32, f"{layer} {name}: kernel error {e_k:.3e} above 4 x {e_32:.3e}"
                worst = max(worst, e_k / e_32)
    print(f"{net} {side} R={R}: worst ratio to the float32 torch error {worst:.2f}")


@pytest.mark.parametrize("R", REF.ROWS)
@pytest.mark.parametrize("net,side", REF.CASES)
def test_against_float64(net, side, R):
    _check_against_float64(net, side, R)


def test_against_float64_where_the_grid_wraps():
    """71200 rows = 2225 row tiles: the forward's workgroups and the backward's 64 partial sums per element each take more than one tile"""
    _check_against_float64("Fight1", "actor", REF.WRAP_ROWS)


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
def _raw(net, side, R, pad=0, src_ld=None, seed=0):
    """device tensors and the hh_input_group array of a case; every pack and gradient `pad` columns wider than it needs and one row longer,
    all filled with the sentinel -> (io, keep: everything io points into, packs, d_ws, d_bs, src)"""
    L, _, _ = _lib()
    c = REF.case(net, side)
    src, ws, bs, d_packs = REF.inputs(net, side, R, seed, src_ld)
    src, ws, bs = src.cuda(), [w.cuda() for w in ws], [b.cuda() for b in bs]
    n = len(ws)
    io = (L.HHInputGroup * n)()
    packs, d_ys = [], []
    for p, d in zip(c["packs"], d_packs):
        wd = d.shape[1] + pad
        packs.append(torch.full((R + 1, wd), SENTINEL, device="cuda"))
        g = torch.zeros((R + 1, wd))
        g[:R, :d.shape[1]] = d
        d_ys.append(g.cuda())
    d_ws = [torch.full((w.shape[0] + 1, w.shape[1]), SENTINEL, device="cuda") for w in ws]
    d_bs = [torch.full((w.shape[0] + 1,), SENTINEL, device="cuda") for w in ws]
    for pi, p in enumerate(c["packs"]):
        col = 0
        for i in p:
            g = io[i]
            g.n_out, g.n_seg = c["shapes"][i][0], len(c["segments"][i])
            for s, (c0, ln) in enumerate(c["segments"][i]):
                g.seg_col[s], g.seg_len[s] = c0, ln
            g.w, g.b = ws[i].data_ptr(), bs[i].data_ptr()
            g.y, g.y_ld = packs[pi].data_ptr() + 4 * col, packs[pi].shape[1]
            g.d_y, g.d_y_ld = d_ys[pi].data_ptr() + 4 * col, d_ys[pi].shape[1]
            g.d_w, g.d_b = d_ws[i].data_ptr(), d_bs[i].data_ptr()
            col += g.n_out
    return io, (ws, bs, d_ys), packs, d_ws, d_bs, src


def _scratch(lib, L, io, n, R):
    nbytes = C.c_int64()
    L.check(lib.hh_input_stage_scratch_bytes(n, io, R, C.byref(nbytes)))
    return torch.full((nbytes.value // 4 + 8,), SENTINEL, device="cuda"), nbytes.value


@pytest.mark.parametrize("net,side,R", [("Fight1", "critic", 63), ("commander", "critic", 65), ("Esc2", "actor", 1300)])
def test_two_runs_same_bytes_and_nothing_written_outside(net, side, R):
    """packs 3 columns wider than their groups and one row longer: the extra columns, row R, and the element after every d_w / d_b and
    after the scratch keep the sentinel"""
    L, lib, st = _lib()
    c = REF.case(net, side)
    n = len(c["shapes"])
    runs = []
    for _ in range(2):
        io, keep, packs, d_ws, d_bs, src = _raw(net, side, R, pad=3)
        scratch, nbytes = _scratch(lib, L, io, n, R)
        L.check(lib.hh_input_stage_forward(R, _p(src), src.shape[1], src.shape[1], n, io, st))
        L.check(lib.hh_input_stage_backward(R, _p(src), src.shape[1], src.shape[1], n, io, _p(scratch), nbytes, st))
        torch.cuda.synchronize()
        for t in packs:
            assert (t[R] == SENTINEL).all() and (t[:R, -3:] == SENTINEL).all()
            assert (t[:R, :-3] != SENTINEL).all() and torch.isfinite(t).all()
        for t in d_ws + d_bs:
            assert (t[-1] == SENTINEL).all() and (t[:-1] != SENTINEL).all() and torch.isfinite(t).all()
        assert (scratch[nbytes // 4:] == SENTINEL).all()
        runs.append(packs + d_ws + d_bs)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs))
    # and they are the wrapper's results
    from hhmarl_2d_amd import learner as LR
    ys, d_w, d_b = REF.run(net, side, REF.inputs(net, side, R), torch.float32, "cuda", fn=LR.input_stage)
    for i in range(n):
        assert torch.equal(d_w[i], runs[0][len(c["packs"]) + i][:-1].double().cpu()) and torch.equal(d_b[i], runs[0][len(c["packs"]) + n + i][:-1].double().cpu())


def test_strided_source():
    """obs rows of 30 floats of which the Fight1 actor reads 26: src_ld = 30, src_width = 26 gives the bytes of the packed 26-wide source"""
    L, lib, st = _lib()
    net, side, R = "Fight1", "actor", 65
    n = len(REF.case(net, side)["shapes"])
    io_w, keep_w, packs_w, d_ws_w, d_bs_w, wide = _raw(net, side, R, src_ld=30)
    io_n, keep_n, packs_n, d_ws_n, d_bs_n, _ = _raw(net, side, R, src_ld=30)
    narrow = wide[:, :26].contiguous()
    assert tuple(wide.shape) == (R, 30)
    for io, src, ld in ((io_w, wide, 30), (io_n, narrow, 26)):
        scratch, nbytes = _scratch(lib, L, io, n, R)
        L.check(lib.hh_input_stage_forward(R, _p(src), ld, 26, n, io, st))
        L.check(lib.hh_input_stage_backward(R, _p(src), ld, 26, n, io, _p(scratch), nbytes, st))
    torch.cuda.synchronize()
    for a, b in zip(packs_w + d_ws_w + d_bs_w, packs_n + d_ws_n + d_bs_n):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert (packs_w[0][:R] != SENTINEL).all()


def test_widest_call():
    """four layers of HH_INSTAGE_MAX_K inputs and 125 outputs each: the largest staging tile the ABI admits, against float64"""
    from hhmarl_2d_amd import learner as LR
    L, _, _ = _lib()
    g = torch.Generator().manual_seed(5)
    R, K = 65, L.INSTAGE_MAX_K
    src = torch.rand((R, K + 3), generator=g)
    ws = [torch.randn((125, K), generator=g) / K ** 0.5 for _ in range(4)]
    bs = [0.1 * torch.randn((125,), generator=g) for _ in range(4)]
    segs = [((i, K),) for i in range(4)]
    d_y = torch.randn((R, 500), generator=g)

    def run(dtype, device, fn):
        w = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in ws]
        b = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in bs]
        y, = fn(src.to(device=device, dtype=dtype), list(zip(w, b, segs)))
        y.backward(d_y.to(device=device, dtype=dtype))
        return [y.detach().double().cpu()] + [t.grad.double().cpu() for t in w + b]

    want, t32, got = run(torch.float64, "cpu", LR.input_stage_torch), run(torch.float32, "cuda", LR.input_stage_torch), run(torch.float32, "cuda", LR.input_stage)
    for k, c, w in zip(got, t32, want):
        e_k, e_32 = REF.rel_err(k, w), REF.rel_err(c, w)
        print(f"widest call: relative error of the float32 torch ops {e_32:.3e}, of the kernel {e_k:.3e}")
        if e_32 == 0.0:
            assert torch.equal(k, c), "the float32 torch ops are exact here and the kernel is not"
        else:
            assert e_k <= 4.0 * e_32


def test_wrapper_keeps_leading_dimensions_and_an_unused_pack_has_zero_gradient():
    from hhmarl_2d_amd import learner as LR
    net, side = "Fight2", "critic"
    c = REF.case(net, side)
    src, ws, bs, _ = REF.inputs(net, side, 60)
    ws, bs = [w.cuda().requires_grad_(True) for w in ws], [b.cuda().requires_grad_(True) for b in bs]
    groups = list(zip(ws, bs, c["segments"]))
    flat = LR.input_stage(src.cuda(), groups, c["packs"])
    cube = LR.input_stage(src.cuda().reshape(3, 20, -1), groups, c["packs"])
    assert [tuple(t.shape) for t in cube] == [(3, 20, 350), (3, 20, 150)]
    assert all(torch.equal(a.reshape(60, -1), b) for a, b in zip(cube, flat))
    cube[0].sum().backward()                     # the second pack takes no part in the loss
    assert torch.equal(ws[2].grad, torch.zeros_like(ws[2])) and torch.equal(bs[2].grad, torch.zeros_like(bs[2]))
    assert ws[0].grad.abs().max().item() > 0
    empty = LR.input_stage(torch.zeros((0, src.shape[1]), device="cuda"), groups, c["packs"])
    assert [tuple(t.shape) for t in empty] == [(0, 350), (0, 150)]


# ---------------------------------------------------------------------------------------------------------------- refused arguments
def test_bad_arguments_are_refused_and_launch_nothing():
    from hhmarl_2d_amd import learner as LR
    L, lib, st = _lib()
    net, side, R = "Fight1", "critic", 65
    c = REF.case(net, side)
    n, width = len(c["shapes"]), c["width"]
    io, keep, packs, d_ws, d_bs, src = _raw(net, side, R)
    scratch, nbytes = _scratch(lib, L, io, n, R)
    fwd = lambda io_=io, n_=n, R_=R, src_=_p(src), ld=width, wd=width: lib.hh_input_stage_forward(R_, src_, ld, wd, n_, io_, st)
    bwd = lambda io_=io, n_=n, R_=R, src_=_p(src), ld=width, wd=width, sc=_p(scratch), nb=nbytes: lib.hh_input_stage_backward(
        R_, src_, ld, wd, n_, io_, sc, nb, st)

    def refused(**kw):
        assert fwd(**kw) == E_ARG and b"hh_input_stage_forward" in lib.hh_last_error()
        assert bwd(**kw) == E_ARG and b"hh_input_stage_backward" in lib.hh_last_error()

    def with_field(i, **fields):
        """a copy of the group array with fields of group i replaced"""
        cp = (L.HHInputGroup * L.INSTAGE_MAX_GROUPS)()
        for k in range(n):
            C.memmove(C.byref(cp[k]), C.byref(io[k]), C.sizeof(L.HHInputGroup))
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(cp[i], k)[v[0]] = v[1]
            else:
                setattr(cp[i], k, v)
        return cp

    refused(n_=0)
    refused(n_=5)
    refused(io_=None)
    refused(R_=-1)
    refused(src_=None)
    refused(ld=width - 1)                                        # src_ld < src_width
    refused(wd=width - 1)                                        # v2 and v3 reach column 57
    refused(io_=with_field(0, n_seg=0))
    refused(io_=with_field(0, n_seg=7))
    refused(io_=with_field(0, n_out=0))
    refused(io_=with_field(0, seg_len=(0, 0)))                   # an empty segment: K of the run is 0
    refused(io_=with_field(0, seg_col=(0, -1)))
    refused(io_=with_field(2, seg_len=(3, 3 + 56)))              # K = 113 > HH_INSTAGE_MAX_K, and past the source
    refused(io_=with_field(1, n_out=176))                        # 501 outputs
    refused(io_=with_field(1, y_ld=174))                         # y_ld < n_out
    # K above HH_INSTAGE_MAX_K inside a wide enough source
    wide = torch.rand((R, 200), device="cuda")
    refused(io_=with_field(2, n_seg=1, seg_col=(0, 0), seg_len=(0, 113)), src_=_p(wide), ld=200, wd=200)
    # pointers each pass needs
    for f in ("w", "b", "y"):
        assert fwd(io_=with_field(1, **{f: None})) == E_ARG
    for f in ("y", "d_y", "d_w", "d_b"):
        assert bwd(io_=with_field(1, **{f: None})) == E_ARG
    assert bwd(io_=with_field(1, d_y_ld=174)) == E_ARG
    assert bwd(sc=None) == E_ARG and bwd(nb=nbytes - 4) == E_ARG and bwd(nb=0) == E_ARG
    out = C.c_int64(-7)
    assert lib.hh_input_stage_scratch_bytes(0, io, R, C.byref(out)) == E_ARG and lib.hh_input_stage_scratch_bytes(n, io, R, None) == E_ARG
    assert lib.hh_input_stage_scratch_bytes(n, with_field(2, n_seg=7), R, C.byref(out)) == E_ARG and out.value == -7
    torch.cuda.synchronize()
    for t in packs + d_ws + d_bs + [scratch]:
        assert (t == SENTINEL).all(), "a refused call wrote something"
    # zero rows: success without a launch, the data pointers not even looked at
    assert fwd(R_=0, src_=None) == 0 and bwd(R_=0, src_=None, sc=None, nb=0) == 0
    torch.cuda.synchronize()
    for t in packs + d_ws + d_bs:
        assert (t == SENTINEL).all()
    # the scratch stops growing: the cap on the partial sums is reached long before 71200 rows
    a, b, small = C.c_int64(), C.c_int64(), C.c_int64()
    L.check(lib.hh_input_stage_scratch_bytes(n, io, REF.WRAP_ROWS, C.byref(a)))
    L.check(lib.hh_input_stage_scratch_bytes(n, io, 10 * REF.WRAP_ROWS, C.byref(b)))
    L.check(lib.hh_input_stage_scratch_bytes(n, io, 33, C.byref(small)))
    assert a.value == b.value > small.value > 0
    # the Python wrapper: contiguous float32 CUDA tensors only
    ws, bs, _ = keep
    groups = list(zip(ws, bs, c["segments"]))
    for bad in (src.double(), src.cpu(), src.t().contiguous().t(), src[:, :40]):
        with pytest.raises(ValueError):
            LR.input_stage(bad, groups, c["packs"])
    with pytest.raises(ValueError):
        LR.input_stage(src, [(ws[0].double(), bs[0].double(), c["segments"][0])])
    with pytest.raises(ValueError):
        LR.input_stage(src, groups, packs=((0, 1),))
    with pytest.raises(ValueError):
        LR.input_stage(src, groups * 2)
