"""hh_dense_tanh_forward / hh_dense_tanh_backward (the learners' shared layer as split-fp16 MFMA, include/hh_learner.h) on the MI355X, through
the C ABI and through learner.dense_tanh: every output inside the derived bound of tests/dense_tanh_ref.py against float64 on shapes
around the row tile, the MFMA's 16 / 32, the 128-wide block and the partial-sum cap, strided inputs, gradients far below fp16's range,
the input families of the reference module (every scale table non-uniform, exact zeros, dynamic range inside rows: the last inside
the extended bound), exact zeros where the inputs have them, power-of-two changes of a row or column bit for bit, the same bytes on
every run, guard words, and refused arguments."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dense_tanh_ref as REF
from hhmarl_2d_amd import _lib as L

pytestmark = pytest.mark.gpu
T, P = L.DENSE_ROW_TILE, L.DENSE_MAX_PARTS
SHAPES = [(K, N, R) for K, N in REF.DIMS for R in REF.row_counts(K, N, T, P)]
EDGE_SHAPES = [(K, N, R) for K, N in REF.EDGE_DIMS for R in REF.row_counts(K, N, T, P)]
CAP_ROWS = ((1, P * T + 1), (T + 1, P * T - T))          # 500 x 500: a small block 0, then a block 1 with more tiles than partial sums
GUARD, MARK = 64, 12345.0
HH_E_ARG = -1


def _dev():
    return torch.device("cuda", 0)


class _Buf:
    """n floats between two guard runs of MARK; `init` = the value the payload starts from"""

    def __init__(self, n, init=MARK):
        self.n = int(n)
        self.t = torch.full((self.n + 2 * GUARD,), MARK, dtype=torch.float32, device=_dev())
        self.t[GUARD:GUARD + self.n] = init

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def get(self, shape):
        return self.t[GUARD:GUARD + self.n].reshape(shape).cpu().numpy()

    def guards_ok(self):
        return bool((self.t[:GUARD] == MARK).all() and (self.t[GUARD + self.n:] == MARK).all())


def _put(a):
    return torch.from_numpy(np.array(a)).to(_dev())      # a copy: the cases are read-only


def _scratch_bytes(K, N, rows):
    io = (L.HHDenseSrc * len(rows))()
    for i, r in enumerate(rows):
        io[i].n_rows = r
    n = C.c_int64()
    L.check(L.lib().hh_dense_tanh_scratch_bytes(K, N, len(rows), io, C.byref(n)))
    return n.value


def _run(c, pad=0, dys=None, ys_in=None):
    """one forward and one backward (from the forward's own y, or from the fixed ys_in) through the C ABI -> dict of numpy outputs, `bufs`
    and the raw bytes.  pad > 0: x rows of K + pad floats, the pad columns NaN."""
    K, N, rows = c["K"], c["N"], c["rows"]
    dys = c["dys"] if dys is None else dys
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    xs = []
    for x in c["xs"]:
        wide = np.full((x.shape[0], K + pad), np.nan, dtype=np.float32)
        wide[:, :K] = x
        xs.append(_put(wide))
    w, b, dyt = _put(c["w"]), _put(c["b"]), [_put(d) for d in dys]
    ys, dxs = [_Buf(r * N) for r in rows], [_Buf(r * K) for r in rows]
    dw, db = _Buf(N * K), _Buf(N)
    nbytes = _scratch_bytes(K, N, rows)
    scratch = _Buf(nbytes // 4)
    io = (L.HHDenseSrc * len(rows))()
    for i, r in enumerate(rows):
        io[i].n_rows, io[i].x, io[i].ld, io[i].y, io[i].d_y, io[i].d_x = r, xs[i].data_ptr(), K + pad, ys[i].ptr, dyt[i].data_ptr(), dxs[i].ptr
    vp = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.hh_dense_tanh_forward(K, N, len(rows), io, vp(w), vp(b), C.c_void_p(scratch.ptr), nbytes, st))
    saved = [] if ys_in is None else [_put(y) for y in ys_in]          # the backward reads these in place of the forward's y, which stays as it is
    for i, y in enumerate(saved):
        io[i].y = y.data_ptr()
    L.check(lib.hh_dense_tanh_backward(K, N, len(rows), io, vp(w), C.c_void_p(dw.ptr), C.c_void_p(db.ptr), C.c_void_p(scratch.ptr), nbytes, st))
    torch.cuda.synchronize()
    bufs = ys + dxs + [dw, db, scratch]
    out = dict(ys=[y.get((r, N)) for y, r in zip(ys, rows)], d_xs=[d.get((r, K)) for d, r in zip(dxs, rows)], d_w=dw.get((N, K)), d_b=db.get((N,)))
    return out, bufs, [bf.t.cpu().numpy().tobytes() for bf in bufs[:-1]]


def _check(name, c, out, dys=None, ys_in=None, ext=False, formed=False):
    """every output against float64 inside the bound; the backward's reference starts from the y the kernel saved, or from ys_in where the
    backward ran from it -> the four ratios.  ext: the extended bound, which includes REF.formation_terms; formed: the componentwise
    bound with them (the edge shapes with K = 1: the bias is U(-1, 1) there, y^2 passes 1/2, and the float32 restatement itself is
    1.3 x outside without them)"""
    formed = formed or ext
    dys = c["dys"] if dys is None else dys
    saved = out["ys"] if ys_in is None else ys_in
    y64 = REF.forward(c["xs"], c["w"], c["b"])
    b_y = (REF.forward_bound_ext if ext else REF.forward_bound)(c["xs"], c["w"], c["b"])
    ratios = {"y": max(REF.check(f"{name} y[{i}]", g, w_, b_) for i, (g, w_, b_) in enumerate(zip(out["ys"], y64, b_y)))}
    dx64, dw64, db64, dp64 = REF.backward(c["xs"], saved, dys, c["w"])
    b_dx, b_dw, b_db = (REF.backward_bounds_ext if ext else REF.backward_bounds)(c["xs"], dp64, c["w"], (saved, dys) if formed else None)
    ratios["d_x"] = max(REF.check(f"{name} d_x[{i}]", g, w_, b_) for i, (g, w_, b_) in enumerate(zip(out["d_xs"], dx64, b_dx)))
    ratios["d_w"] = REF.check(f"{name} d_w", out["d_w"], dw64, b_dw)
    ratios["d_b"] = REF.check(f"{name} d_b", out["d_b"], db64, b_db)
    print(name, {k: round(v, 4) for k, v in ratios.items()})
    return ratios


@pytest.mark.parametrize("K,N,R", SHAPES)
def test_every_output_inside_the_bound(K, N, R):
    """one block of R rows, and two blocks of (R, 1) rows; guard words around every output and the scratch stay"""
    for rows in ((R,), (R, 1)):
        c = REF.case(K, N, rows)
        out, bufs, _ = _run(c)
        assert all(bf.guards_ok() for bf in bufs), "a guard word changed"
        _check(f"K={K} N={N} rows={rows}", c, out)


@pytest.mark.parametrize("rows", [(2 * T - 1,), (2 * T, 2 * T + 1)])
def test_rows_around_two_tiles(rows):
    """the forward and d_x take 2 T rows per workgroup: the same bound on either side of that edge, at widths that are no multiple of 16"""
    c = REF.case(481, 497, rows)
    out, bufs, _ = _run(c)
    assert all(bf.guards_ok() for bf in bufs), "a guard word changed"
    _check(f"K=481 N=497 rows={rows}", c, out)


@pytest.mark.parametrize("K,N", REF.DIMS)
def test_strided_rows_do_not_leak(K, N):
    """ld = K + 12 with NaN beyond column K: the same bytes as from contiguous rows"""
    c = REF.case(K, N, (T + 1, 1))
    plain, _, raw = _run(c)
    wide, bufs, raw_w = _run(c, pad=12)
    assert all(bf.guards_ok() for bf in bufs)
    assert raw == raw_w
    _check(f"K={K} N={N} ld=K+12", c, wide)


@pytest.mark.parametrize("K,N,rows", [(500, 500, (T + 1, 1)), (500, 500, (3 * T + 5,)), (33, 17, (T + 1, 1)), (1, 1, (T + 1,))])
def test_gradient_range(K, N, rows):
    """d_y times 2^-40, and one row of magnitude 1 among rows of magnitude 1e-8: the same bound, which is relative to |A| |B|"""
    c = REF.case(K, N, rows)
    tiny = [(d * np.float32(2.0 ** -40)).astype(np.float32) for d in c["dys"]]
    out, _, _ = _run(c, dys=tiny)
    _check(f"K={K} N={N} rows={rows} d_y 2^-40", c, out, dys=tiny)
    mixed = [(d * np.float32(1e-8)).astype(np.float32) for d in c["dys"]]
    mixed[0][rows[0] // 2] = c["dys"][0][rows[0] // 2]
    out, _, _ = _run(c, dys=mixed)
    _check(f"K={K} N={N} rows={rows} one large row", c, out, dys=mixed)


@pytest.mark.parametrize("K,N,rows", [(500, 500, (P * T + 1, 1)), (481, 497, (T + 1, T - 1))] + [(500, 500, rows) for rows in CAP_ROWS])
def test_two_runs_give_the_same_bytes(K, N, rows):
    c = REF.case(K, N, rows)
    _, bufs_a, raw_a = _run(c)
    _, bufs_b, raw_b = _run(c)
    assert raw_a == raw_b
    assert all(bf.guards_ok() for bf in bufs_a + bufs_b)


@pytest.mark.parametrize("K,N,R", EDGE_SHAPES)
def test_edge_shapes_inside_the_bound(K, N, R):
    """K or N at 128 / 129 (a second P or Q block of one index), K next to the chunk of 32 with N across 16, 1 against 512: one block
    of R rows and two of (R, 1), guard words; at K = 1, where |b| goes up to 1, the bound has the term for forming d_pre where tanh is steep"""
    for rows in ((R,), (R, 1)):
        c = REF.case(K, N, rows)
        out, bufs, _ = _run(c)
        assert all(bf.guards_ok() for bf in bufs), "a guard word changed"
        _check(f"K={K} N={N} rows={rows}", c, out, formed=K == 1)


@pytest.mark.parametrize("K,N", REF.EDGE_DIMS)
def test_edge_shapes_strided_rows_do_not_leak(K, N):
    c = REF.case(K, N, (T + 1, 1))
    _, _, raw = _run(c)
    wide, bufs, raw_w = _run(c, pad=12)
    assert all(bf.guards_ok() for bf in bufs)
    assert raw == raw_w
    _check(f"K={K} N={N} ld=K+12", c, wide, formed=K == 1)


@pytest.mark.parametrize("rows", CAP_ROWS)
def test_walk_from_a_small_block_into_a_long_one(rows):
    """500 x 500: block 0 is one or two row tiles, block 1 has more tiles than there are partial sums, so d_W's walk wraps inside block 1"""
    c = REF.case(500, 500, rows)
    out, bufs, _ = _run(c)
    assert all(bf.guards_ok() for bf in bufs), "a guard word changed"
    _check(f"K=500 N=500 rows={rows}", c, out)


@pytest.mark.parametrize("family,K,N,rows", REF.family_grid(T))
def test_input_families(family, K, N, rows):
    """"scales" (all six scale tables non-uniform) and "zeros" inside the componentwise bound, "range" and "picked" inside the extended
    one; guard words.  "zeros": what is exactly zero in float64 is +-0 here, the zero x rows of the two blocks give the same y
    bytes, and everything is finite."""
    c = REF.case(K, N, rows, family=family)
    out, bufs, _ = _run(c)
    assert all(bf.guards_ok() for bf in bufs), "a guard word changed"
    _check(f"{family} K={K} N={N} rows={rows}", c, out, ext=family in REF.EXT_FAMILIES)
    if family != "zeros":
        return
    z = c["zeros"]
    assert all(np.isfinite(a).all() for a in out["ys"] + out["d_xs"] + [out["d_w"], out["d_b"]])
    for dx, dr, dt in zip(out["d_xs"], z["dy_rows"], z["dy_tiles"]):
        assert dr is None or not dx[dr].any(), "d_x of a zero d_y row"
        assert dt is None or not dx[dt[0]:dt[1]].any(), "d_x of a zero d_y tile"
        assert not dx[:, z["w_col"]].any(), "d_x of a zero W column"
    assert not out["d_w"][z["dy_col"]].any() and out["d_b"][z["dy_col"]] == 0, "d_w, d_b of a zero d_y column"
    assert not out["d_w"][:, z["x_col"]].any(), "d_w of a zero x column"
    y_rows = [y[xr] for y, xr in zip(out["ys"], z["x_rows"])]
    assert all(REF.same_bits(y_rows[0], y) for y in y_rows[1:]) and len(y_rows) == 2, "the y rows of zero x rows differ"


@functools.lru_cache(maxsize=None)
def _pow2_baseline(K, N):
    """the default case, the fixed y its backward runs from (float32 of the float64 forward), and the kernels' outputs for it"""
    c = REF.case(K, N, (T + 1, T - 1))
    y_in = [y.astype(np.float32) for y in REF.forward(c["xs"], c["w"], c["b"])]
    out, bufs, _ = _run(c, ys_in=y_in)
    assert all(bf.guards_ok() for bf in bufs)
    _check(f"K={K} N={N} fixed y", c, out, ys_in=y_in)
    return c, y_in, out


@pytest.mark.parametrize("s", (30, -30))
@pytest.mark.parametrize("K,N", ((500, 500), (481, 497)))
def test_power_of_two_changes_bit_for_bit(K, N, s):
    """The design scales by powers of two and undoes the scale on the float32 result, "both exact".  Then a change of one row or column by
    2^s (nothing clamps or leaves the normal range at s = +-30) moves the matching outputs by exactly 2^s: REF.pow2_variants, the
    backward from a fixed y.  The marked outputs are compared as int32 with numpy.ldexp of the baseline; an output the change does
    not reach keeps its bytes (inside `exact` too: only the marked row or column of it is scaled); the outputs it does reach for
    real (d_w and d_b under a d_y row; d_x under a d_y column; y under a column of W or x, whose row maxima change: the extended
    bound) are held to the bound."""
    c, y_in, base = _pow2_baseline(K, N)
    for name, c2, scaled, exact in REF.pow2_variants(c, s):
        out, bufs, _ = _run(c2, ys_in=y_in)
        assert all(bf.guards_ok() for bf in bufs), "a guard word changed"
        want = scaled(base)
        for key in exact:
            got, w_ = (out[key], want[key]) if isinstance(out[key], list) else ([out[key]], [want[key]])
            for i, (g, w1) in enumerate(zip(got, w_)):
                diff = int((g.view(np.int32) != w1.view(np.int32)).sum())
                assert diff == 0, f"K={K} N={N} {name}: {key}[{i}] differs from the baseline times 2^s in {diff} of {g.size} elements"
        _check(f"K={K} N={N} {name}", c2, out, ys_in=y_in, ext="ys" not in exact)


def test_bad_arguments_launch_nothing_and_zero_rows_succeed():
    K, N, R = 33, 17, 5
    c = REF.case(K, N, (R,))
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    x, w, b, dy = _put(c["xs"][0]), _put(c["w"]), _put(c["b"]), _put(c["dys"][0])
    y, dx, dw, db = _Buf(R * N), _Buf(R * K), _Buf(N * K), _Buf(N)
    nbytes = _scratch_bytes(K, N, (R,))
    tail = L.DENSE_FWD_SCRATCH_BYTES             # in front of the slots: the scales of w
    assert nbytes == (N * K + N) * 4 + tail and _scratch_bytes(500, 500, (P * T + 1, 1)) == P * (500 * 500 + 500) * 4 + tail == _scratch_bytes(500, 500, (10 ** 6,))
    scratch = _Buf(nbytes // 4)
    vp = lambda t: C.c_void_p(t.data_ptr())

    def io(n_rows=R, ld=K, xp=x.data_ptr(), yp=y.ptr, dyp=dy.data_ptr(), dxp=dx.ptr, n=1):
        a = (L.HHDenseSrc * 2)()
        for i in range(2):
            a[i].n_rows, a[i].x, a[i].ld, a[i].y, a[i].d_y, a[i].d_x = (n_rows if i == 0 else 0), xp, ld, yp, dyp, dxp
        return a

    fwd = lambda a, k=K, n_=N, n_src=1, wp=vp(w), bp=vp(b), sp=C.c_void_p(scratch.ptr), sb=nbytes: lib.hh_dense_tanh_forward(k, n_, n_src, a, wp, bp, sp, sb, st)
    bwd = lambda a, k=K, n_=N, n_src=1, wp=vp(w), dwp=C.c_void_p(dw.ptr), dbp=C.c_void_p(db.ptr), sp=C.c_void_p(scratch.ptr), sb=nbytes: \
        lib.hh_dense_tanh_backward(k, n_, n_src, a, wp, dwp, dbp, sp, sb, st)
    bad = [fwd(io(), k=0), fwd(io(), k=513), fwd(io(), n_=0), fwd(io(), n_=513), fwd(io(), n_src=0), fwd(io(), n_src=3), fwd(None),
           fwd(io(n_rows=-1)), fwd(io(ld=K - 1)), fwd(io(xp=None)), fwd(io(yp=None)), fwd(io(), wp=None), fwd(io(), bp=None), fwd(io(), sp=None), fwd(io(), sb=tail - 4),
           bwd(io(), k=0), bwd(io(), n_=513), bwd(io(), n_src=3), bwd(io(n_rows=-1)), bwd(io(ld=K - 1)), bwd(io(xp=None)), bwd(io(yp=None)),
           bwd(io(dyp=None)), bwd(io(dxp=None)), bwd(io(), wp=None), bwd(io(), dwp=None), bwd(io(), dbp=None), bwd(io(), sp=None),
           bwd(io(), sb=nbytes - 4)]
    assert bad == [HH_E_ARG] * len(bad), bad
    n = C.c_int64(-7)
    assert lib.hh_dense_tanh_scratch_bytes(K, N, 1, io(), None) == HH_E_ARG and lib.hh_dense_tanh_scratch_bytes(K, 0, 1, io(), C.byref(n)) == HH_E_ARG
    assert lib.hh_last_error()
    # zero rows: success, with null pointers, and with a second block of zero rows beside a real one
    assert fwd(io(n_rows=0, xp=None, yp=None), sp=None, sb=0) == 0 and bwd(io(n_rows=0, xp=None, yp=None, dyp=None, dxp=None), sp=None, sb=0) == 0
    assert fwd(io(n_rows=0), n_src=2) == 0
    torch.cuda.synchronize()
    for bf in (y, dx, dw, db, scratch):
        assert bool((bf.t == MARK).all()), "a refused or empty call wrote something"
    assert fwd(io(), n_src=2) == 0 and bwd(io(), n_src=2) == 0          # block 1 has 0 rows: its pointers are not used
    torch.cuda.synchronize()
    out = dict(ys=[y.get((R, N))], d_xs=[dx.get((R, K))], d_w=dw.get((N, K)), d_b=db.get((N,)))
    _check("second block of 0 rows", c, out)
    assert all(bf.guards_ok() for bf in (y, dx, dw, db, scratch))


@pytest.mark.parametrize("K,N", REF.DIMS)
def test_autograd_function(K, N):
    """learner.dense_tanh over two inputs with leading dimensions, one of them a column slice of a wider tensor: outputs keep the leading
    dimensions, every gradient inside the bound; a single tensor gives a single tensor with the same bytes"""
    from hhmarl_2d_amd import learner as LR
    c = REF.case(K, N, (3 * 22, 5), seed=2)
    wide = torch.full((3, 22, K + 7), float("nan"), device=_dev())
    wide[..., 3:3 + K] = _put(c["xs"][0]).reshape(3, 22, K)
    xa = wide[..., 3:3 + K].requires_grad_()
    xb = _put(c["xs"][1]).requires_grad_()
    w, b = _put(c["w"]).requires_grad_(), _put(c["b"]).requires_grad_()
    ya, yb = LR.dense_tanh((xa, xb), w, b)
    assert tuple(ya.shape) == (3, 22, N) and tuple(yb.shape) == (5, N)
    (ya * _put(c["dys"][0]).reshape(3, 22, N)).sum().add((yb * _put(c["dys"][1])).sum()).backward()
    out = dict(ys=[ya.detach().reshape(-1, N).cpu().numpy(), yb.detach().cpu().numpy()],
               d_xs=[xa.grad.reshape(-1, K).cpu().numpy(), xb.grad.cpu().numpy()], d_w=w.grad.cpu().numpy(), d_b=b.grad.cpu().numpy())
    assert tuple(xa.grad.shape) == (3, 22, K)
    _check(f"autograd K={K} N={N}", c, out)
    single = LR.dense_tanh(xb.detach(), w.detach(), b.detach())
    assert isinstance(single, torch.Tensor) and torch.equal(single, yb.detach())
    with pytest.raises(ValueError):
        LR.dense_tanh(xb.detach().double(), w.detach(), b.detach())
    with pytest.raises(ValueError):
        LR.dense_tanh(xb.detach().cpu(), w.detach(), b.detach())
    with pytest.raises(ValueError):
        LR.dense_tanh((xb.detach(),) * 3, w.detach(), b.detach())
    # an output that is not used gets a zero gradient, not garbage
    w2 = w.detach().clone().requires_grad_()
    y1, y2 = LR.dense_tanh((xb.detach(), xb.detach()), w2, b.detach())
    y1.sum().backward()
    w1 = w.detach().clone().requires_grad_()
    LR.dense_tanh(xb.detach(), w1, b.detach()).sum().backward()
    assert torch.equal(w2.grad, w1.grad)
