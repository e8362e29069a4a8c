"""learner.grad_norm (hh_grad_norm) and learner.adam_step(clip=...) (hh_adam_step_clipped) on the MI355X: the norm and the coefficient
against the sequential float64 restatement of tests/grad_clip_ref.py, the per-step table, and the clipped Adam step bit for bit against
hh_adam_step on gradients scaled on the host.  All buffers stand between sentinel guards."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_clip_ref as GR
import train_step_ref as TR

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e11
GUARD = 4            # elements in front of and behind every buffer: a guarded float32 view keeps the allocation's 16-byte alignment
LR_ = 1e-4
MISALIGNED_G = 6     # grad_list's tensor of 4097 elements starts 4 bytes into its allocation's 16-byte grid


def _guarded(values, shift=0, dtype=torch.float32):
    """a CUDA view of len(values) elements inside an allocation filled with SENTINEL, `shift` extra elements in"""
    n = len(values)
    big = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=dtype, device="cuda")
    view = big[GUARD + shift:GUARD + shift + n]
    view.copy_(torch.from_numpy(np.asarray(values, dtype=np.float32 if dtype == torch.float32 else np.float64)))
    return big, view


def _guards_intact(big, view):
    n = view.numel()
    off = (view.data_ptr() - big.data_ptr()) // view.element_size()
    return bool((big[:off] == SENTINEL).all() and (big[off + n:] == SENTINEL).all())


def _ulps(got, want):
    return abs(got - want) / np.spacing(abs(want))


def _host_coef(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def _device_norm(grads, max_norm, shifts=None):
    """grad_norm on guarded copies of the float32 arrays -> (clip as two floats, the bytes of clip and of the scratch, guards intact)"""
    from hhmarl_2d_amd import learner as LR
    gb = [_guarded(g, (shifts or {}).get(i, 0)) for i, g in enumerate(grads)]
    tiles = sum((len(g) + 4095) // 4096 for g in grads)
    clip_big, clip = _guarded([SENTINEL, SENTINEL], dtype=torch.float64)
    scr_big, scratch = _guarded([SENTINEL] * max(tiles, 1), dtype=torch.float64)
    out = LR.grad_norm([b[1] for b in gb], max_norm, clip, scratch=scratch)
    torch.cuda.synchronize()
    assert out is clip
    ok = all(_guards_intact(*b) for b in gb) and _guards_intact(clip_big, clip) and _guards_intact(scr_big, scratch)
    same = all(np.array_equal(b[1].cpu().numpy(), g) for b, g in zip(gb, grads))      # the gradients are only read
    c = clip.cpu().numpy()
    return (float(c[0]), float(c[1])), (c.tobytes(), scratch[:tiles].cpu().numpy().tobytes()), ok and same, gb


@pytest.mark.parametrize("n_small", (60, 121))
def test_norm_and_coefficient_of_a_list_that_needs_several_launches(n_small):
    """69 and 130 tensors (capacity 64 per launch: two and three partial launches, ONE final), sizes around the float4 group and the
    4096-element tile, an empty tensor, one g only 4-byte aligned, and the largest gradients in the LAST tensor: a norm per launch, or one
    that loses a launch's slots, is far outside the bound"""
    from hhmarl_2d_amd import _lib as L
    grads = GR.grad_list(n_small, seed=21 + n_small)
    assert len(grads) == 9 + n_small and len(grads) > L.ADAM_MAX_TENSORS * (1 if n_small == 60 else 2)
    assert max(np.abs(g).max() for g in grads[:-1] if g.size) < 10 < np.abs(grads[-1]).max()
    want_norm, _ = GR.norm_coef(grads, 1.0)
    (norm, coef), raw, ok, gb = _device_norm(grads, 1.0, shifts={MISALIGNED_G: 1})
    assert gb[MISALIGNED_G][1].data_ptr() % 16 == 4 and gb[0][1].data_ptr() % 16 == 0
    print(f"{len(grads)} tensors: device norm {norm!r}, restatement {want_norm!r}, relative difference {abs(norm - want_norm) / want_norm:.3e} "
          f"(bound {GR.bound(grads):.3e}); coefficient {coef!r}, {_ulps(coef, _host_coef(norm, 1.0)):.1f} ulps from the host's")
    assert ok, "guards intact, gradients unchanged"
    assert abs(norm - want_norm) <= GR.bound(grads) * want_norm
    assert coef < 1.0 and _ulps(coef, _host_coef(norm, 1.0)) <= 2
    # the same bytes on a second run, and the same norm whatever the alignment of g
    (norm2, coef2), raw2, ok2, _ = _device_norm(grads, 1.0, shifts={MISALIGNED_G: 1})
    assert raw2 == raw and ok2
    (norm3, _), _, _, _ = _device_norm(grads, 1.0)
    assert norm3 == norm


def test_threshold_cases_and_zero_gradients():
    grads = GR.grad_list(3, seed=5)
    (norm, _), _, ok, _ = _device_norm(grads, 1.0)
    assert ok and abs(norm - GR.norm_coef(grads, 1.0)[0]) <= GR.bound(grads) * norm
    for max_norm, binds in ((2.0 * norm, False), (0.5 * norm, True), (norm * (1.0 + 5e-10), None), (norm * (1.0 - 5e-10), True), (norm, True)):
        (n2, coef), _, ok, _ = _device_norm(grads, max_norm)
        want = _host_coef(norm, max_norm)
        print(f"max_norm / norm = {max_norm / norm!r}: coefficient {coef!r}, host {want!r}")
        assert ok and n2 == norm and _ulps(coef, want) <= 2 and coef <= 1.0
        if binds is not None:
            assert (coef < 1.0) == binds
    zeros = [np.zeros(n, dtype=np.float32) for n in (5, 4097, 0)]
    for z in (zeros, [np.zeros(0, dtype=np.float32)], []):
        clip, _, ok, _ = _device_norm(z, 1.0)
        assert ok and clip == (0.0, 1.0)


def test_gradients_whose_float32_squares_overflow_or_vanish():
    rng = np.random.default_rng(8)
    big = [(10.0 ** rng.uniform(19.0, 21.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for n in (5, 4097, 300)]
    with np.errstate(over="ignore"):
        assert all(np.isinf(np.square(x)).mean() > 0.8 for x in big[1:]), "above 1.85e19 a float32 square is inf: nearly all of them"
    (norm, coef), _, ok, _ = _device_norm(big, 1.0)
    want = GR.norm_coef(big, 1.0)[0]
    print(f"gradients in [1e19, 1e21]: device norm {norm!r}, restatement {want!r}, coefficient {coef!r}")
    assert ok and np.isfinite(norm) and abs(norm - want) <= GR.bound(big) * want
    assert 0.0 < coef < 1e-19 and _ulps(coef, _host_coef(norm, 1.0)) <= 2
    tiny = [np.full(n, 1e-25, dtype=np.float32) for n in (4097, 7)]
    assert not np.square(tiny[0]).any()
    (norm, coef), _, ok, _ = _device_norm(tiny, 1.0)
    want = GR.norm_coef(tiny, 1.0)[0]
    print(f"gradients of 1e-25: device norm {norm!r}, restatement {want!r}")
    assert ok and norm > 0.0 and abs(norm - want) <= GR.bound(tiny) * want and coef == 1.0


def test_the_table_fills_by_the_cursor_and_the_cursor_is_only_read():
    from hhmarl_2d_amd import learner as LR
    rng = np.random.default_rng(3)
    cursor = torch.zeros((1,), dtype=torch.int32, device="cuda")
    t = torch.zeros((1,), dtype=torch.int32, device="cuda")
    stats = torch.zeros((6,), dtype=torch.float64, device="cuda")
    stats_table = torch.zeros((5, 6), dtype=torch.float64, device="cuda")
    big, table = _guarded([SENTINEL] * 5, dtype=torch.float64)
    clip = torch.zeros((2,), dtype=torch.float64, device="cuda")
    norms = []
    for s in range(5):
        g = [torch.from_numpy(rng.standard_normal(n).astype(np.float32) * (s + 1)).cuda() for n in (7, 4099)]
        LR.grad_norm(g, 1.0, clip, cursor, table)
        assert int(cursor.item()) == s, "the cursor is not written by the norm"
        norms.append(float(clip[0].item()))
        LR.train_commit(stats, stats_table, cursor, t)
    assert table.cpu().numpy().tolist() == norms and len(set(norms)) == 5 and _guards_intact(big, table)
    for outside in (-1, 5):
        cursor.fill_(outside)
        LR.grad_norm(g, 1.0, clip, cursor, table)
        torch.cuda.synchronize()
        assert int(cursor.item()) == outside and table.cpu().numpy().tolist() == norms and _guards_intact(big, table)
    assert float(clip[0].item()) == norms[-1]
    with pytest.raises(ValueError):
        LR.grad_norm(g, 1.0, clip, cursor, None)


# ---------------------------------------------------------------------------------------------------------------- the clipped Adam step
ADAM_SIZES = (1, 3, 5, 4095, 4096, 4097, 8193, 40)       # across the 4096-element tile edge and the float4 group
ADAM_SHIFT = {3: ("g",), 5: ("p", "g", "m", "v")}        # tensor index -> buffers that are only 4-byte aligned (the tensor goes scalar)
COEF = 0.37


def _five_steps(inputs, clip_value, scale_on_host=None):
    """five Adam steps of every tensor from zero state, t advanced by train_commit -> (bytes of p, m, v per step, guards intact)"""
    from hhmarl_2d_amd import learner as LR
    sh = lambda i, k: 1 if k in ADAM_SHIFT.get(i, ()) else 0
    bufs = {k: [_guarded(p if k == "p" else np.zeros_like(p), sh(i, k)) for i, (p, _) in enumerate(inputs)] for k in "pmv"}
    t = torch.zeros((1,), dtype=torch.int32, device="cuda")
    cursor = torch.zeros((1,), dtype=torch.int32, device="cuda")
    table = torch.zeros((5, 6), dtype=torch.float64, device="cuda")
    stats = torch.zeros((6,), dtype=torch.float64, device="cuda")
    clip = None if clip_value is None else torch.tensor(clip_value, dtype=torch.float64, device="cuda")
    out, ok = [], True
    for s in range(5):
        gs = [g[s] for _, g in inputs]
        if scale_on_host is not None:
            gs = GR.scaled(gs, scale_on_host)
        gb = [_guarded(g, sh(i, "g")) for i, g in enumerate(gs)]
        LR.adam_step([b[1] for b in bufs["p"]], [b[1] for b in gb], [b[1] for b in bufs["m"]], [b[1] for b in bufs["v"]], t, lr=LR_, clip=clip)
        LR.train_commit(stats, table, cursor, t)
        torch.cuda.synchronize()
        ok = ok and all(_guards_intact(*b) for b in gb) and all(np.array_equal(b[1].cpu().numpy(), g) for b, g in zip(gb, gs))
        out.append(b"".join(b[1].cpu().numpy().tobytes() for k in "pmv" for b in bufs[k]))
    ok = ok and all(_guards_intact(*b) for k in "pmv" for b in bufs[k]) and int(t.item()) == 5
    assert bufs["p"][5][1].data_ptr() % 16 == 4 and bufs["p"][3][1].data_ptr() % 16 == 0
    return out, ok


@pytest.fixture(scope="module")
def adam_inputs():
    inputs = TR.adam_inputs(ADAM_SIZES, seed=17)        # |g| in {0} u [1e-6, 1e3]: scaled by 0.37 every value is 0 or a normal float32
    for _, gs in inputs:
        for g in gs:
            sc = np.abs(g.astype(np.float64) * COEF)
            assert ((sc == 0) | (sc >= 1e-30)).all()
    return inputs


def test_a_coefficient_of_one_leaves_the_unclipped_kernels_bytes(adam_inputs):
    plain, ok0 = _five_steps(adam_inputs, None)
    one, ok1 = _five_steps(adam_inputs, (123.5, 1.0))
    assert ok0 and ok1 and plain == one


def test_a_coefficient_below_one_is_the_unclipped_kernel_on_host_scaled_gradients(adam_inputs):
    clipped, ok0 = _five_steps(adam_inputs, (5.0, COEF))
    scaled, ok1 = _five_steps(adam_inputs, None, scale_on_host=COEF)
    plain, _ = _five_steps(adam_inputs, None)
    assert ok0 and ok1, "guards intact, the gradients keep their unscaled values"
    assert clipped == scaled and clipped[0] != plain[0]
    again, ok2 = _five_steps(adam_inputs, (5.0, COEF))
    assert ok2 and again == clipped, "the same bytes on two runs"


def test_norm_then_clipped_step_is_clip_grad_norm_then_adam():
    """the chain as DeviceAdam issues it, on one list: p, m, v equal hh_adam_step on the gradients scaled by the device's own coefficient"""
    from hhmarl_2d_amd import learner as LR
    grads = GR.grad_list(60, seed=2)

    def run(clipped):
        g = [torch.from_numpy(x).cuda() for x in grads]
        p, m, v = ([torch.zeros_like(x) for x in g] for _ in range(3))
        t = torch.zeros((1,), dtype=torch.int32, device="cuda")
        clip = LR.grad_norm(g, 0.5)
        if clipped:
            LR.adam_step(p, g, m, v, t, lr=LR_, clip=clip)
        else:
            LR.adam_step(p, [torch.from_numpy(x).cuda() for x in GR.scaled(grads, float(clip[1].item()))], m, v, t, lr=LR_)
        torch.cuda.synchronize()
        return b"".join(x.cpu().numpy().tobytes() for x in p + m + v), clip.cpu().numpy()
    (a, clip_a), (b, clip_b) = run(True), run(False)
    assert clip_a.tobytes() == clip_b.tobytes() and clip_a[1] < 1e-2 and a == b


def test_refused_arguments_enqueue_nothing():
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    lib = L.lib()
    full = lambda n, dt=torch.float64: torch.full((n,), SENTINEL, dtype=dt, device="cuda")
    p, g, m, v = (torch.full((48,), val, dtype=torch.float32, device="cuda") for val in (1.5, 1.0, 0.25, 0.5))
    clip, table, scratch = full(2), full(3), full(4)
    cursor = torch.zeros((1,), dtype=torch.int32, device="cuda")
    t = torch.zeros((1,), dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def desc(**kw):
        d = (L.HHAdamTensor * 1)()
        d[0].p, d[0].g, d[0].m, d[0].v, d[0].n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 40
        for k, val in kw.items():
            setattr(d[0], k, val)
        return d
    E = -1      # HH_E_ARG
    norm = lambda n=1, d=None, mx=1.0, cl=ptr(clip), cu=ptr(cursor), tb=ptr(table), rows=3, sc=ptr(scratch), nb=32: lib.hh_grad_norm(
        n, desc() if d is None else d, mx, cl, cu, tb, rows, sc, nb, st)
    assert norm(cl=None) == E and norm(n=-1) == E and lib.hh_grad_norm(1, None, 1.0, ptr(clip), None, None, 0, ptr(scratch), 32, st) == E
    assert norm(d=desc(g=None)) == E and norm(d=desc(n=-4)) == E and norm(d=desc(g=g.data_ptr() + 2)) == E
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert norm(mx=bad) == E
    assert norm(cu=None) == E and norm(tb=None) == E and norm(rows=-1) == E
    assert norm(nb=0) == E and norm(sc=None) == E
    nbytes = C.c_int64(-5)
    assert lib.hh_grad_norm_scratch_bytes(1, desc(), None) == E and lib.hh_grad_norm_scratch_bytes(-1, desc(), C.byref(nbytes)) == E
    assert lib.hh_grad_norm_scratch_bytes(1, desc(n=-4), C.byref(nbytes)) == E and nbytes.value == -5
    assert lib.hh_grad_norm_scratch_bytes(1, desc(n=4097, p=None, m=None, v=None), C.byref(nbytes)) == 0 and nbytes.value == 16
    step = lambda n=1, d=None, tt=ptr(t), cl=ptr(clip): lib.hh_adam_step_clipped(n, desc() if d is None else d, tt, cl, LR_, 0.9, 0.999, 1e-8, st)
    assert step(cl=None) == E and step(tt=None) == E and step(n=-1) == E
    assert lib.hh_adam_step_clipped(1, None, ptr(t), ptr(clip), LR_, 0.9, 0.999, 1e-8, st) == E
    for field in "pgmv":
        assert step(d=desc(**{field: None})) == E
        assert step(d=desc(**{field: getattr(desc()[0], field) + 2})) == E
    assert step(d=desc(n=-4)) == E
    torch.cuda.synchronize()
    assert all(bool((x == SENTINEL).all()) for x in (clip, table, scratch))
    assert bool((p == 1.5).all() and (g == 1.0).all() and (m == 0.25).all() and (v == 0.5).all()) and int(t.item()) == 0 and int(cursor.item()) == 0
    # an empty list and a list of empty tensors succeed: the final launch alone writes clip = (0, 1); p, m, v may be NULL for the norm
    assert lib.hh_grad_norm(0, None, 1.0, ptr(clip), None, None, 0, None, 0, st) == 0
    torch.cuda.synchronize()
    assert clip.tolist() == [0.0, 1.0]
    clip.fill_(SENTINEL)
    assert norm(d=desc(n=0), cu=None, tb=None, rows=0, sc=None, nb=0) == 0
    torch.cuda.synchronize()
    assert clip.tolist() == [0.0, 1.0]
    assert norm(d=desc(p=None, m=None, v=None)) == 0
    torch.cuda.synchronize()
    assert abs(clip.tolist()[0] - np.sqrt(40.0)) <= 40 * GR.U * np.sqrt(40.0) and table.tolist()[0] == clip.tolist()[0] and bool((table[1:] == SENTINEL).all())
    assert step(n=0, d=desc()) == 0 and step(d=desc(n=0)) == 0
    for bad in (0, -1.0, float("inf"), float("nan"), "1", None):
        with pytest.raises(ValueError):
            LR.grad_norm([g], bad)
    with pytest.raises(ValueError):
        LR.grad_norm([g.double()], 1.0)
    with pytest.raises(ValueError):
        LR.adam_step([p], [g], [m], [v], t, lr=LR_, clip=clip.float())
    with pytest.raises(ValueError):
        LR.grad_norm([g], 1.0, scratch=torch.zeros((0,), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert bool((p == 1.5).all() and (m == 0.25).all() and (v == 0.5).all())
