"""hh_gru_seq_forward / hh_gru_seq_backward on the MI355X (include/hh_learner.h) through learner.gru_sequence / gru_sequence_pair: y and all
four gradients against float64 CPU autograd of the same cell, exact zeros in the padding, the same bytes on every run, bad arguments.

The bound is relative to the format: per compared tensor, e32 = the error of the float32 torch-op cell (tests/commander_ref._gru stepped
on the device, through autograd; its W_ih is the identity, so its `x` is the kernel's gi, bit for bit) against the float64 reference on
the same inputs, and the kernel may be at most 4 x e32 away (errors as max |difference| / max |reference|).  4 x: a three-pass split-fp16
product drops the lo x lo term and keeps about 22 bits where fp32 keeps 24; the float32 fmaf kernel that ships has no such term."""
import ctypes as C

import pytest
import torch

import commander_ref as REF

pytestmark = pytest.mark.gpu
LEN, H = 20, 200
MAX_LEN = 32                                     # HH_GRU_MAX_LEN
TILE = 16                                        # HHG_TILE
SIZES = (1, TILE - 1, TILE, TILE + 1, 1000)
NAMES = ("y", "d_gi", "d_h0", "d_w_hh", "d_b_hh")


def _inputs(S, seed, max_len=LEN):
    g = torch.Generator().manual_seed(seed)
    seq_len = torch.randint(1, max_len + 1, (S,), generator=g).to(torch.int32)
    seq_len[0] = max_len if S > 1 else min(13, max_len)
    return dict(gi=torch.randn((S, max_len, 3 * H), generator=g), h0=0.5 * torch.randn((S, H), generator=g),
                w_hh=torch.randn((3 * H, H), generator=g) / H ** 0.5, b_hh=0.1 * torch.randn((3 * H,), generator=g),
                wy=torch.randn((S, max_len, H), generator=g), seq_len=seq_len)


def _pattern(name, S, max_len, seq_len):
    """the length patterns a tile of 16 sequences can meet, written over the random lengths `seq_len` [S] of S = 2 TILE + 1 sequences"""
    out = seq_len.clone()
    if name == "all-one":                        # no tile runs past step 0
        out[:] = 1
    elif name == "all-full":                     # no padding anywhere
        out[:] = max_len
    elif name == "short-tile-then-full-tile":    # the first tile stops at step 3 at the latest, the second runs all max_len steps with every lane on
        out[:TILE] = 1 + torch.arange(TILE, dtype=torch.int32) % 3
        out[TILE:2 * TILE] = max_len
    elif name == "one-full-among-ones":          # the second tile runs max_len steps for one sequence; its other 15 stopped after step 0
        out[TILE:] = 1
        out[TILE + 5] = max_len
    else:
        raise KeyError(name)
    assert S == 2 * TILE + 1 and int(out.min()) >= 1 and int(out.max()) <= max_len
    return out


def _cell_path(inp, dtype, device):
    """commander_ref._gru stepped over the sequences with autograd -> (y, d_gi, d_h0, d_w_hh, d_b_hh)"""
    t = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in inp.items() if k in ("gi", "h0", "w_hh", "b_hh")}
    sd = {"g.weight_ih_l0": torch.eye(3 * H, dtype=dtype, device=device), "g.bias_ih_l0": torch.zeros(3 * H, dtype=dtype, device=device),
          "g.weight_hh_l0": t["w_hh"], "g.bias_hh_l0": t["b_hh"]}
    seq_len = inp["seq_len"].to(device)
    h, ys = t["h0"], []
    for s in range(inp["gi"].shape[1]):
        on = (seq_len > s)[:, None]
        hn = REF._gru(sd, "g", t["gi"][:, s], h)
        h = torch.where(on, hn, h)
        ys.append(torch.where(on, hn, torch.zeros_like(hn)))
    y = torch.stack(ys, dim=1)
    (y * inp["wy"].to(device=device, dtype=dtype)).sum().backward()
    return [y.detach()] + [t[k].grad for k in ("gi", "h0", "w_hh", "b_hh")]


def _kernel_path(inps):
    """learner.gru_sequence (one GRU) or gru_sequence_pair (two) with autograd -> per GRU (y, d_gi, d_h0, d_w_hh, d_b_hh)"""
    from hhmarl_2d_amd import learner as LR
    ts = [{k: v.cuda().requires_grad_(True) for k, v in inp.items() if k in ("gi", "h0", "w_hh", "b_hh")} for inp in inps]
    seq_len = inps[0]["seq_len"].cuda()
    parts = [(t["gi"], t["h0"], t["w_hh"], t["b_hh"]) for t in ts]
    ys = [LR.gru_sequence(*parts[0], seq_len)] if len(inps) == 1 else list(LR.gru_sequence_pair(parts[0], parts[1], seq_len))
    sum((y * inp["wy"].cuda()).sum() for y, inp in zip(ys, inps)).backward()
    return [[y.detach()] + [t[k].grad for k in ("gi", "h0", "w_hh", "b_hh")] for y, t in zip(ys, ts)]


@pytest.mark.parametrize("n_gru", (1, 2))
@pytest.mark.parametrize("S", SIZES)
def test_forward_and_gradients_against_float64(S, n_gru):
    _check_against_float64(S, n_gru, LEN)


@pytest.mark.parametrize("n_gru", (1, 2))
@pytest.mark.parametrize("S", (TILE - 1, TILE + 1))
@pytest.mark.parametrize("max_len", (1, MAX_LEN))
def test_forward_and_gradients_at_the_shortest_and_the_longest_max_len(max_len, S, n_gru):
    """hh_gru_seq_* accept 1 <= max_len <= 32: one step only (every sequence has length 1, dW_hh sees h0 alone) and all 32"""
    _check_against_float64(S, n_gru, max_len)


@pytest.mark.parametrize("n_gru", (1, 2))
@pytest.mark.parametrize("pattern", ("all-one", "all-full", "short-tile-then-full-tile", "one-full-among-ones"))
def test_forward_and_gradients_at_length_patterns(pattern, n_gru):
    """a tile runs to the longest of ITS sequences: tiles whose longest sequence is short of max_len beside tiles that run all of it"""
    _check_against_float64(2 * TILE + 1, n_gru, LEN, pattern)


def _check_against_float64(S, n_gru, max_len, pattern=None):
    inps = [_inputs(S, 100 * g + S, max_len) for g in range(n_gru)]
    if pattern is not None:
        inps[0]["seq_len"] = _pattern(pattern, S, max_len, inps[0]["seq_len"])
    for inp in inps[1:]:
        inp["seq_len"] = inps[0]["seq_len"]
    got = _kernel_path(inps)
    torch.cuda.synchronize()
    for g, inp in enumerate(inps):
        want = _cell_path(inp, torch.float64, "cpu")
        t32 = _cell_path(inp, torch.float32, "cuda")
        pad = ~(torch.arange(max_len)[None, :] < inp["seq_len"][:, None])
        for name, k, c, w in zip(NAMES, got[g], t32, want):
            k, c = k.double().cpu(), c.double().cpu()
            assert torch.isfinite(k).all()
            scale = w.abs().max().item()
            e_k, e_32 = (k - w).abs().max().item() / scale, (c - w).abs().max().item() / scale
            print(f"S={S} L={max_len}{'' if pattern is None else ' ' + pattern} n_gru={n_gru} gru {g} {name}: max |ref| {scale:.3e}; relative error of the float32 torch-op cell {e_32:.3e}, of the kernel {e_k:.3e}")
            assert e_k <= 4.0 * e_32, f"{name}: kernel error {e_k:.3e} above 4 x {e_32:.3e}"
            if name in ("y", "d_gi") and pad.any():
                assert torch.equal(k[pad], torch.zeros_like(k[pad])), f"{name}: not exactly zero past seq_len"


def _raw(S, n_gru, seed=7, max_len=LEN):
    from hhmarl_2d_amd import learner as LR
    inps = [_inputs(S, seed + g, max_len) for g in range(n_gru)]
    seq_len = inps[0]["seq_len"].cuda()
    parts = [tuple(inp[k].cuda().contiguous() for k in ("gi", "h0", "w_hh", "b_hh")) for inp in inps]
    dys = [inp["wy"].cuda().contiguous() for inp in inps]

    def run():
        ys, scratch = LR.gru_seq_forward(parts, seq_len)
        out = LR.gru_seq_backward(parts, ys, dys, seq_len, scratch)
        torch.cuda.synchronize()
        return [t for y, o in zip(ys, out) for t in (y,) + o]
    return run, inps[0]["seq_len"], parts, dys


@pytest.mark.parametrize("S,n_gru", [(1000, 2), (TILE + 1, 1)])
def test_padding_is_exactly_zero_and_two_runs_give_the_same_bytes(S, n_gru):
    run, seq_len, _, _ = _raw(S, n_gru)
    first, second = run(), run()
    pad = (~(torch.arange(LEN)[None, :] < seq_len[:, None])).cuda()
    assert pad.any()
    for g in range(n_gru):
        y, d_gi, d_gh, d_h0 = first[4 * g:4 * g + 4]
        for name, t in (("y", y), ("d_gi", d_gi), ("d_gh", d_gh)):
            assert torch.equal(t[pad], torch.zeros_like(t[pad])), name
            assert t[~pad].abs().max().item() > 0
        assert torch.isfinite(d_h0).all()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))


@pytest.mark.parametrize("max_len,S,n_gru", [(1, TILE + 1, 2), (MAX_LEN, TILE + 1, 1)])
def test_two_runs_give_the_same_bytes_at_the_shortest_and_the_longest_max_len(max_len, S, n_gru):
    run, seq_len, _, _ = _raw(S, n_gru, max_len=max_len)
    first, second = run(), run()
    pad = (~(torch.arange(max_len)[None, :] < seq_len[:, None])).cuda()
    assert bool(pad.any()) == (max_len > 1)
    for g in range(n_gru):
        for name, t in zip(("y", "d_gi", "d_gh"), first[4 * g:4 * g + 3]):
            assert torch.equal(t[pad], torch.zeros_like(t[pad])), name
            assert torch.isfinite(t).all() and t[~pad].abs().max().item() > 0
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))


def test_bad_arguments_are_refused():
    from hhmarl_2d_amd import _lib as L
    lib = L.lib()
    S = 5
    _, _, parts, dys = _raw(S, 1)
    seq_len = torch.full((S,), LEN, dtype=torch.int32, device="cuda")
    nb = C.c_int64()
    assert lib.hh_gru_seq_scratch_bytes(1, S, 33, C.byref(nb)) == -1 and lib.hh_gru_seq_scratch_bytes(3, S, LEN, C.byref(nb)) == -1   # HH_E_ARG
    L.check(lib.hh_gru_seq_scratch_bytes(1, S, LEN, C.byref(nb)))
    scratch = torch.empty((nb.value // 4 + 4,), dtype=torch.float32, device="cuda")
    y = torch.empty((S, LEN, H), device="cuda")
    d_gi, d_gh, d_h0 = torch.empty((S, LEN, 3 * H), device="cuda"), torch.empty((S, LEN, 3 * H), device="cuda"), torch.empty((S, H), device="cuda")
    gi, h0, w_hh, b_hh = parts[0]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def io(**kw):
        a = (L.HHGruSeqIO * 1)()
        base = dict(gi=gi.data_ptr(), h0=h0.data_ptr(), w_hh=w_hh.data_ptr(), b_hh=b_hh.data_ptr(), y=y.data_ptr(), dy=dys[0].data_ptr(),
                    d_gi=d_gi.data_ptr(), d_gh=d_gh.data_ptr(), d_h0=d_h0.data_ptr())
        base.update(kw)
        for k, v in base.items():
            setattr(a[0], k, v)
        return a

    fwd = lambda a, Lm=LEN, sc=scratch, nbytes=nb.value: lib.hh_gru_seq_forward(1, S, Lm, a, p(seq_len), p(sc), nbytes, st)
    bwd = lambda a, Lm=LEN: lib.hh_gru_seq_backward(1, S, Lm, a, p(seq_len), p(scratch), nb.value, st)
    assert fwd(io()) == 0 and bwd(io()) == 0
    assert fwd(io(), Lm=33) == -1 and fwd(io(), Lm=0) == -1 and bwd(io(), Lm=33) == -1            # L out of range
    assert fwd(io(gi=None)) == -1 and fwd(io(y=None)) == -1 and bwd(io(dy=None)) == -1 and bwd(io(d_h0=None)) == -1   # null
    assert fwd(io(gi=gi.data_ptr() + 4)) == -1 and bwd(io(d_gi=d_gi.data_ptr() + 4)) == -1          # misaligned
    assert fwd(io(y=gi.data_ptr())) == -1 and bwd(io(d_gh=d_gi.data_ptr())) == -1                   # an output over another tensor
    assert fwd(io(), nbytes=nb.value - 4) == -1                                                    # scratch too small
    assert lib.hh_gru_seq_forward(1, S, LEN, io(), None, p(scratch), nb.value, st) == -1
    assert b"hh_gru_seq" in lib.hh_last_error()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        from hhmarl_2d_amd import learner as LR
        LR.gru_sequence(gi.double(), h0, w_hh, b_hh, seq_len)
