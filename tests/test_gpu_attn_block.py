"""learner.attention_block (hh_attn_block_forward / hh_attn_block_backward) on the MI355X against the float64 restatement of
tests/attn_block_ref.py: every output at most 4 x as far from it as the torch-op twin run in float32 on the same inputs, at every tile
geometry hh_attn_block_tile names; the degenerate cases exactly; the same bytes on every run and whatever else the call holds; nothing
written outside the call's rows; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_block_ref as REF

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0


def _dev():
    return torch.device("cuda", 0)


def _counts(E, Lm):
    """1, 3, one tile, one tile + 1, and enough that workgroup 0 walks three tiles, the last one ragged (where a tile holds several)"""
    from hhmarl_2d_amd import _lib
    from hhmarl_2d_amd import learner as LR
    spt, _ = LR.attention_block_tile(1, Lm, E)
    assert spt == _lib.ATTN_BLOCK_ROWS // Lm
    cap = _lib.ATTN_BLOCK_MAX_WG
    many = 2 * cap * spt + max(1, spt // 2)
    assert LR.attention_block_tile(many, Lm, E) == (spt, cap) and LR.attention_block_tile(spt + 1, Lm, E) == (spt, 2)
    return [1, 3, spt, spt + 1, many]


def _run_block(args):
    """learner.attention_block on make_case's tensors in float32 -> {name: float64 tensor}"""
    from hhmarl_2d_amd import learner as LR
    x, in_w, in_b, out_w, out_b, d_y = (t.to(_dev(), torch.float32).contiguous() for t in args)
    leaves = [t.clone().requires_grad_(True) for t in (x, in_w, in_b, out_w, out_b)]
    y = LR.attention_block(*leaves)
    y.backward(d_y)
    return dict(zip(REF.NAMES, [y.detach().double()] + [t.grad.double() for t in leaves]))


def _run_twin(args):
    """learner.attention_block_torch under autograd in float32 on the GPU -> {name: float64 tensor}"""
    from hhmarl_2d_amd import learner as LR
    x, in_w, in_b, out_w, out_b, d_y = (t.to(_dev(), torch.float32) for t in args)
    leaves = [t.clone().requires_grad_(True) for t in (x, in_w, in_b, out_w, out_b)]
    y = LR.attention_block_torch(*leaves)
    y.backward(d_y)
    return dict(zip(REF.NAMES, [y.detach().double()] + [t.grad.double() for t in leaves]))


@pytest.mark.parametrize("Lm", (1, 7, 20, 32))
@pytest.mark.parametrize("E", (100, 150))
def test_block_against_float64_by_the_four_times_rule(E, Lm):
    for S in _counts(E, Lm):
        args = REF.make_case(E, Lm, S, 1000 * E + 10 * Lm + S % 7)
        ref = REF.reference(args, torch.float64, _dev())
        twin = _run_twin(args)
        got = _run_block(args)
        for name in REF.NAMES:
            e_block, e_twin = (got[name] - ref[name]).abs().max().item(), (twin[name] - ref[name]).abs().max().item()
            print(f"E={E} len={Lm} n_seq={S} {name}: max |ref| {ref[name].abs().max().item():.3e}, error block {e_block:.3e}, float32 torch ops {e_twin:.3e}")
            assert torch.isfinite(got[name]).all() and got[name].shape == ref[name].shape
            assert e_block <= 4.0 * e_twin, (E, Lm, S, name, e_block, e_twin)


@pytest.mark.parametrize("E", (100, 150))
def test_one_key_is_out_proj_of_the_v_columns_exactly(E):
    """len == 1 on integer-valued inputs whose every sum is exact in float32 in any order: y is normalize(x + out_proj(v)) row by row,
    bit for bit (sqrt and division are correctly rounded on both sides), whatever the q and k rows of the in-projection hold"""
    from hhmarl_2d_amd import learner as LR
    g = torch.Generator().manual_seed(E)
    S = 77
    sparse = lambda *shape: (torch.randint(-1, 2, shape, generator=g) * (torch.rand(shape, generator=g) < 0.03)).float()
    x = torch.randint(-2, 3, (S, 1, E), generator=g).float()
    in_w, in_b = torch.randn((3 * E, E), generator=g), torch.randn((3 * E,), generator=g)
    in_w[2 * E:], in_b[2 * E:] = sparse(E, E), torch.randint(-2, 3, (E,), generator=g).float()
    out_w, out_b = sparse(E, E), torch.randint(-2, 3, (E,), generator=g).float()
    v = x[:, 0].double() @ in_w[2 * E:].double().T + in_b[2 * E:].double()
    s = x[:, 0].double() + v @ out_w.double().T + out_b.double()
    ss = (s * s).sum(dim=1)
    assert ss.max().item() < 2 ** 24 and s.abs().max().item() > 2
    s32, ss32 = s.numpy().astype(np.float32), ss.numpy().astype(np.float32)
    want = np.stack([s32[r] / np.maximum(np.sqrt(ss32[r]), np.float32(1e-12)) for r in range(S)])
    dev = _dev()
    y = LR.attention_block(x.to(dev), in_w.to(dev), in_b.to(dev), out_w.to(dev), out_b.to(dev))
    assert np.array_equal(y[:, 0].cpu().numpy(), want)
    in_w[:2 * E] = 0.0
    y2 = LR.attention_block(x.to(dev), in_w.to(dev), in_b.to(dev), out_w.to(dev), out_b.to(dev))
    assert torch.equal(y, y2)


@pytest.mark.parametrize("E", (100, 150))
def test_zero_chunk_gives_zero_and_the_clamp_branch(E):
    """a chunk of all-zero rows under zero biases: y = 0 there, and with d_y non-zero in one row of it alone (every other row's d_s is
    then +-0) d_b_out, the column sums of d_s, is that row's d_y / 1e-12 bit for bit; ctx is 0 there, so d_out_w is 0"""
    from hhmarl_2d_amd import learner as LR
    dev = _dev()
    x, in_w, in_b, out_w, out_b, _ = (t.float() for t in REF.make_case(E, 20, 3, 7, padded=False))
    x[1] = 0.0
    in_b, out_b = torch.zeros_like(in_b), torch.zeros_like(out_b)
    d_y = torch.zeros_like(x)
    d_y[1, 5] = torch.randn(E, generator=torch.Generator().manual_seed(3))
    leaves = [t.to(dev).requires_grad_(True) for t in (x, in_w, in_b, out_w, out_b)]
    y = LR.attention_block(*leaves)
    y.backward(d_y.to(dev))
    assert not y[1].any() and y[0].any() and y[2].any()
    want = d_y[1, 5].numpy() / np.float32(1e-12)
    assert np.array_equal(leaves[4].grad.cpu().numpy(), want)
    assert not leaves[3].grad.any() and all(torch.isfinite(t.grad).all() for t in leaves)
    assert not leaves[0].grad[0].any() and not leaves[0].grad[2].any() and leaves[0].grad[1].any()


@pytest.mark.parametrize("E,Lm", [(100, 20), (150, 7), (150, 1)])
def test_same_bytes_on_every_run_and_whatever_else_the_call_holds(E, Lm):
    from hhmarl_2d_amd import learner as LR
    spt, _ = LR.attention_block_tile(1, Lm, E)
    SA, SB = 2 * spt + 1, spt + 2
    args = REF.make_case(E, Lm, SA + SB, 11)
    a, b = _run_block(args), _run_block(args)
    for name in REF.NAMES:
        assert torch.equal(a[name], b[name]), name
    part = tuple(t[:SA] if i in (0, 5) else t for i, t in enumerate(args))
    alone = _run_block(part)
    assert torch.equal(alone["y"], a["y"][:SA]) and torch.equal(alone["d_x"], a["d_x"][:SA])


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("E,Lm", [(100, 20), (150, 7), (150, 1)])
def test_nothing_is_written_outside_the_call(E, Lm):
    """over-allocated y, d_x, save and scratch filled with a sentinel: the rows beyond n_seq and the bytes behind save's and scratch's
    stated sizes stay as they were"""
    from hhmarl_2d_amd import _lib
    from hhmarl_2d_amd import learner as LR
    dev, lib = _dev(), _lib.lib()
    spt, _ = LR.attention_block_tile(1, Lm, E)
    S, G = 2 * spt + 1, 64
    x, in_w, in_b, out_w, out_b, d_y = (t.to(dev, torch.float32).contiguous() for t in REF.make_case(E, Lm, S, 4))
    nb = C.c_int64()
    _lib.check(lib.hh_attn_block_save_bytes(S, Lm, E, C.byref(nb)))
    save_bytes = nb.value
    _lib.check(lib.hh_attn_block_scratch_bytes(S, Lm, E, C.byref(nb)))
    scratch_bytes = nb.value
    assert save_bytes % 16 == 0 and S * Lm * (4 * E + 1) * 4 <= save_bytes <= S * Lm * (4 * E + 1) * 4 + 48
    assert scratch_bytes == min(3, _lib.ATTN_BLOCK_MAX_WG) * (4 * E * E + 4 * E) * 4
    full = lambda *shape: torch.full(shape, SENTINEL, device=dev)
    y, d_x = full(S + 2, Lm, E), full(S + 2, Lm, E)
    save, scratch = full(save_bytes // 4 + G), full(scratch_bytes // 4 + G)
    d_w = [full(3 * E, E), full(3 * E), full(E, E), full(E)]
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.hh_attn_block_forward(S, Lm, E, _ptr(x), _ptr(in_w), _ptr(in_b), _ptr(out_w), _ptr(out_b), _ptr(y), _ptr(save), save_bytes, st))
    _lib.check(lib.hh_attn_block_backward(S, Lm, E, _ptr(x), _ptr(in_w), _ptr(out_w), _ptr(y), _ptr(save), save_bytes, _ptr(d_y), _ptr(d_x),
                                          *[_ptr(t) for t in d_w], _ptr(scratch), scratch_bytes, st))
    torch.cuda.synchronize()
    for t in (y, d_x):
        assert (t[S:] == SENTINEL).all() and not (t[:S] == SENTINEL).any()
    assert (save[save_bytes // 4:] == SENTINEL).all() and (scratch[scratch_bytes // 4:] == SENTINEL).all()
    assert not any((t == SENTINEL).any() for t in d_w)
    want = _run_block((x, in_w, in_b, out_w, out_b, d_y))
    assert torch.equal(y[:S].double(), want["y"]) and torch.equal(d_x[:S].double(), want["d_x"])
    for t, name in zip(d_w, REF.NAMES[2:]):
        assert torch.equal(t.double(), want[name]), name


def test_arguments():
    """n_seq == 0 succeeds and writes nothing; embed = 120, len = 33, a short save or scratch, a misaligned pointer and an output that
    overlaps an input are HH_E_ARG with nothing written"""
    from hhmarl_2d_amd import _lib
    from hhmarl_2d_amd import learner as LR
    dev, lib = _dev(), _lib.lib()
    E, Lm, S = 100, 20, 2
    x, in_w, in_b, out_w, out_b, d_y = (t.to(dev, torch.float32).contiguous() for t in REF.make_case(E, Lm, S, 4))
    full = lambda *shape: torch.full(shape, SENTINEL, device=dev)
    y, d_x, save, scratch = full(S, Lm, E), full(S, Lm, E), full(1 << 16), full(1 << 16)
    d_w = [full(3 * E, E), full(3 * E), full(E, E), full(E)]
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    big = 4 << 16

    def fwd(n_seq, ln, embed, yy=y, sb=big, xx=x):
        return lib.hh_attn_block_forward(n_seq, ln, embed, _ptr(xx), _ptr(in_w), _ptr(in_b), _ptr(out_w), _ptr(out_b), _ptr(yy), _ptr(save), sb, st)

    def bwd(n_seq, ln, embed, dx=d_x, sb=big, cb=big):
        return lib.hh_attn_block_backward(n_seq, ln, embed, _ptr(x), _ptr(in_w), _ptr(out_w), _ptr(y), _ptr(save), sb, _ptr(d_y), _ptr(dx),
                                          *[_ptr(t) for t in d_w], _ptr(scratch), cb, st)

    assert fwd(0, Lm, E) == 0 and bwd(0, Lm, E) == 0
    assert lib.hh_attn_block_forward(0, Lm, 150, None, None, None, None, None, None, None, 0, st) == 0
    for rc in (fwd(S, Lm, 120), bwd(S, Lm, 120), fwd(S, 33, E), bwd(S, 33, E), fwd(S, 0, E), fwd(-1, Lm, E), fwd(S, Lm, E, sb=64), bwd(S, Lm, E, sb=64),
               bwd(S, Lm, E, cb=64), fwd(S, Lm, E, yy=x), bwd(S, Lm, E, dx=d_y), fwd(S, Lm, E, xx=x.reshape(-1)[1:])):
        assert rc < 0
    spt, nwg = C.c_int32(), C.c_int32()
    assert lib.hh_attn_block_tile(S, Lm, 120, C.byref(spt), C.byref(nwg)) < 0 and lib.hh_attn_block_tile(S, 33, E, C.byref(spt), C.byref(nwg)) < 0
    torch.cuda.synchronize()
    for t in [y, d_x, save, scratch] + d_w:
        assert (t == SENTINEL).all(), "a refused or empty call wrote something"
    # the Python wrapper: zero sequences, and contiguous float32 CUDA tensors of a compiled width only
    out = LR.attention_block(torch.zeros((0, Lm, E), device=dev), in_w, in_b, out_w, out_b)
    assert tuple(out.shape) == (0, Lm, E) and out.dtype == torch.float32
    for bad in (x.double(), x.transpose(0, 1), x.cpu(), x[..., :96], torch.zeros((2, 33, E), device=dev), x[0], torch.zeros((2, Lm, 120), device=dev)):
        with pytest.raises(ValueError):
            LR.attention_block(bad, in_w, in_b, out_w, out_b)
    for bad_w in (in_w.double(), in_w[:, :96], in_w.cpu()):
        with pytest.raises(ValueError):
            LR.attention_block(x, bad_w, in_b, out_w, out_b)
