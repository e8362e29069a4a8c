"""float64 restatement of hh_dense_tanh_* (include/hh_learner.h) and the error bound the tests hold the kernels to.  No test in here.

The bound is derived, not measured.  For a product C = A B with a sum of length n, computed with both operands as fp16 (hi, lo) pairs
(hi hi + lo hi + hi lo, float32 accumulators):

    |C - C64| <= (4 * 2^-22 + (n + 2) * 2^-24) (|A| |B|)        componentwise

  2^-22 for each of the two operands' 11 + 11-bit representation, 2^-22 for the dropped lo lo product, 3 * 2^-24 for forming
  d_pre = d_y (1 - y^2) in float32 (together 3 * 2^-22 + 3 * 2^-24 < 4 * 2^-22), and (n + 2) * 2^-24 for float32 accumulation of n
  terms in any order and the final rounding.
Forward: the right-hand side gets |b| added (the bias joins the sum), and 4 * 2^-24 absolute for tanhf (<= 2 ulp of a result <= 1, and
tanh is 1-Lipschitz, so the pre-activation's error carries over as it is).
d_b: (R + 2) * 2^-24 * sum |d_pre| (a plain sum of R terms).

Forming d_pre where tanh is steep no longer (formation_terms; the backward bounds take it with `saved=(ys, dys)`).  "3 * 2^-24 for
forming d_pre" above counts three relative roundings.  The first of them is y^2's, and 1 - y^2 cancels: with t = fl(y y),
u = fl(1 - t), d = fl(d_y u) the error is |d - d_y (1 - y^2)| <= 2^-24 |d_y| (2 (1 - y^2) + y^2) = 2^-24 |d_y| (2 - y^2), which is
3 * 2^-24 |d_pre| only while y^2 <= 1/2.  Beyond that the float32 restatement itself leaves the bound above (1.3 x in d_b at K = 1,
where |b| goes up to 1; 8 x in d_x on the family "range", whose pre-activations saturate).  What is missing is, per element of d_pre,
    products:  2^-24 |d_y| max(0, 2 y^2 - 1)      (= 2^-24 |d_y| (2 - y^2) - 3 * 2^-24 |d_pre|, where positive)
    d_b:       2^-24 |d_y| y^2                    (its (R + 2) counts two roundings for d_pre: 2 - y^2 - 2 (1 - y^2) = y^2)
carried through |W|, |x| or the column sum like d_pre itself.  The tests that were here before the families run without it, as before.

The extended bound (forward_bound_ext, backward_bounds_ext).  "2^-22 for an operand's 11 + 11 bits" holds for an element whose lo half
is a normal fp16.  The kernels multiply all elements that share a scale (a row of x, of W or of d_pre for the forward and d_x; a
column of a 64-row tile for d_W) by the power of two S that takes the largest of them, amax, to [2^14, 2^15), and split v = a S:
    hi = fp16(v), lo = fp16(v - hi).  fp16's normal numbers start at 2^-14, below them the spacing is 2^-24.
    |v| >= 2^-14 and |v - hi| >= 2^-14:  both roundings are relative, |v - hi - lo| <= 2^-22 |v|
    otherwise:                           the last rounding is to a multiple of 2^-24 at the worst, |v - hi - lo| <= 2^-25
  and S amax >= 2^14, so in the operand's own units every staged element is off by at most
    max(2^-22 |a|, 2^-39 amax)                      (scale_exp's clamp aside: amax < 2^-111 is outside the domain)
The first alternative is what the componentwise bound already holds.  The second adds, to element (i, j) of a product A B, at most
    2^-39 (amax_i sum_k |b_kj| + bmax_j sum_k |a_ik|)
and the second-order terms (the two errors' product, the same errors inside the accumulation term, the lo lo product of a floored
element) are below that by 2^-11 or more; one factor of 2 covers them:
    floor (i, j) = 2^-38 (amax_i sum_k |b_kj| + bmax_j sum_k |a_ik|)
  forward: i = a row of x, j = a row n of W, k = the columns.  d_x: i = a row of d_pre, j = a column k of W, summed over n.
  d_W: per 64-row tile, i = column n of the tile's d_pre, j = column k of the tile's x, summed over the tile's rows; the tiles'
  terms add up, because every tile has scales of its own.
Where the elements that share a scale lie within 2^17 of each other the floor never applies and the bound is the componentwise one;
where they do not, the guarantee is relative to the largest element of the row or tile column, not to the element.  A long dense sum
hides that (the default inputs: an x of 2^-20 sits among 500 of order 1 and W is dense); a W that picks the small column does not
(family "picked").

Input families (case(family=...)), every one from the draws of the default:
  "scales"  every one of the six scale tables non-uniform: x[r, k] 2^(e_r + h_k), W[n, k] 2^(f_n - h_k), d_y[r, n] 2^(p_r + q_n)
  "zeros"   exact zeros: rows and columns of x, W and d_y, and a whole row tile of d_y
  "range"   the dynamic range inside rows: every element of x and W times 2^U{-12 .. 12} (and W as a whole by one power of two
            that keeps tanh out of saturation)
  "picked"  column 1 of x times 2^-30, and W = 1 in column 1, 0 elsewhere: the forward sum consists of the floored element alone
"scales" and "zeros" are held to the componentwise bound, "range" and "picked" to the extended one."""
import functools

import numpy as np

U22, U24 = 2.0 ** -22, 2.0 ** -24
FLOOR = 2.0 ** -38
DIMS = ((500, 500), (512, 512), (481, 497), (1, 1), (33, 17))       # (K, N)
# next to the kernels' 128-wide P / Q block (129: a second block of one index), next to the 32-wide chunk with N across 16, 1 against 512
EDGE_DIMS = ((128, 128), (129, 128), (128, 129), (32, 16), (31, 15), (1, 512), (512, 1))
FAMILIES = ("default", "scales", "zeros", "range", "picked")
EXT_FAMILIES = ("range", "picked")                                  # held to the extended bound
TABLES = ("w_rows", "x_rows", "w_cols", "dp_rows", "dp_tile_cols", "x_tile_cols")
# "scales": the ranges of the exponents.  h_k is +-9, not the +-12 first planned: x carries 2^h_k and W 2^-h_k, so every term of the
# forward sum has the same size while a row's scale follows its largest h_k, and the floor term grows like 2^(2 H) against the
# componentwise bound: at H = 12 it is 11 times that bound at K = 33 and the family would test the floor, which is "range"'s job.
# H = 9 is the largest at which the floor term stays below a quarter of the componentwise bound for every output on every shape of
# family_grid (0.13 at K = 33); case() asserts that quarter.  Both are figures of the two derived bounds, not of any kernel.
SCALES_E, SCALES_H, SCALES_PQ = (-6, 0), (-9, 9), (-20, 20)


def row_counts(K, N, tile, parts):
    """the row counts of the first block that the tests run for (K, N): around one tile; at 500 x 500 also past the partial-sum cap"""
    return (1, tile - 1, tile, tile + 1) + ((parts * tile + 1,) if (K, N) == (500, 500) else ())


def family_grid(tile):
    """(family, K, N, rows) of the family runs, on the host and on the GPU"""
    g = [(f, K, N, rows) for f in ("scales", "zeros") for K, N in ((500, 500), (481, 497), (33, 17)) for rows in ((tile + 1, 1), (2 * tile + 1, tile - 1))]
    return g + [(f, K, N, (tile + 1,)) for f in EXT_FAMILIES for K, N in ((500, 500), (33, 17))]


def factor(n):
    return 4 * U22 + (n + 2) * U24


def forward(xs, w, b, dtype=np.float64):
    """xs: list of [R_i, K]; -> list of tanh(x W^T + b) [R_i, N] in `dtype`"""
    w, b = w.astype(dtype), b.astype(dtype)
    return [np.tanh(x.astype(dtype) @ w.T + b) for x in xs]


def backward(xs, ys, dys, w, dtype=np.float64):
    """from the saved ys -> (d_xs, d_w, d_b, d_pres) in `dtype`"""
    w = w.astype(dtype)
    d_pres = [dy.astype(dtype) * (1 - y.astype(dtype) * y.astype(dtype)) for y, dy in zip(ys, dys)]
    d_xs = [dp @ w for dp in d_pres]
    d_w = sum(dp.T @ x.astype(dtype) for dp, x in zip(d_pres, xs))
    d_b = sum(dp.sum(axis=0) for dp in d_pres)
    return d_xs, d_w, d_b, d_pres


def forward_bound(xs, w, b):
    K = w.shape[1]
    aw, ab = np.abs(w.astype(np.float64)), np.abs(b.astype(np.float64))
    return [factor(K) * (np.abs(x.astype(np.float64)) @ aw.T + ab) + 4 * U24 for x in xs]


def formation_terms(ys, dys):
    """what forming d_pre = d_y (1 - y^2) in float32 adds beyond the three relative roundings the bounds count (module docstring)
    -> (per block the term of the products, per block the term of d_b)"""
    y2 = [y.astype(np.float64) ** 2 for y in ys]
    ady = [np.abs(dy.astype(np.float64)) for dy in dys]
    return [U24 * a * np.maximum(0.0, 2 * q - 1) for a, q in zip(ady, y2)], [U24 * a * q for a, q in zip(ady, y2)]


def backward_bounds(xs, d_pres64, w, saved=None):
    """-> (bounds of d_xs, of d_w, of d_b) from the float64 d_pre; saved = (ys, dys): with formation_terms"""
    N = w.shape[0]
    R = sum(x.shape[0] for x in xs)
    aw = np.abs(w.astype(np.float64))
    b_dx = [factor(N) * (np.abs(dp) @ aw) for dp in d_pres64]
    b_dw = factor(R) * sum(np.abs(dp).T @ np.abs(x.astype(np.float64)) for dp, x in zip(d_pres64, xs))
    b_db = (R + 2) * U24 * sum(np.abs(dp).sum(axis=0) for dp in d_pres64)
    if saved is not None:
        e_p, e_b = formation_terms(*saved)
        b_dx = [bd + e @ aw for bd, e in zip(b_dx, e_p)]
        b_dw = b_dw + sum(e.T @ np.abs(x.astype(np.float64)) for e, x in zip(e_p, xs))
        b_db = b_db + sum(e.sum(axis=0) for e in e_b)
    return b_dx, b_dw, b_db


def _floor(a, b):
    """the floor term of a product a [I, n] b^T [J, n] whose rows share a scale: [I, J]"""
    a, b = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(b, dtype=np.float64))
    if a.shape[1] == 0:
        return np.zeros((a.shape[0], b.shape[0]))
    return FLOOR * (np.outer(a.max(axis=1), b.sum(axis=1)) + np.outer(a.sum(axis=1), b.max(axis=1)))


def forward_floor(xs, w):
    """the floor term of the pre-activations (module docstring)"""
    return [_floor(x, w) for x in xs]


def forward_bound_ext(xs, w, b):
    return [bd + fl for bd, fl in zip(forward_bound(xs, w, b), forward_floor(xs, w))]


def backward_floors(xs, d_pres64, w, tile=64):
    """-> (floor terms of d_xs, of d_w); d_b has none (it is a plain sum)"""
    f_dx = [_floor(dp, w.T) for dp in d_pres64]
    f_dw = sum(_floor(dp[r:r + tile].T, x[r:r + tile].T) for dp, x in zip(d_pres64, xs) for r in range(0, x.shape[0], tile))
    return f_dx, f_dw


def backward_bounds_ext(xs, d_pres64, w, saved=None, tile=64):
    b_dx, b_dw, b_db = backward_bounds(xs, d_pres64, w, saved)
    f_dx, f_dw = backward_floors(xs, d_pres64, w, tile)
    return [bd + fl for bd, fl in zip(b_dx, f_dx)], b_dw + f_dw, b_db


def floor_share(c):
    """the largest floor term / componentwise bound of y, d_x and d_w for a case (backward from the float32 of the float64 y)"""
    y_in = [y.astype(np.float32) for y in forward(c["xs"], c["w"], c["b"])]
    dp64 = backward(c["xs"], y_in, c["dys"], c["w"])[3]
    b_dx, b_dw, _ = backward_bounds(c["xs"], dp64, c["w"])
    f_dx, f_dw = backward_floors(c["xs"], dp64, c["w"])
    r = lambda fl, bd: float(np.max(np.where(fl > 0, fl / np.maximum(bd, 1e-300), 0.0))) if fl.size else 0.0
    return dict(y=max(r(fl, bd) for fl, bd in zip(forward_floor(c["xs"], c["w"]), forward_bound(c["xs"], c["w"], c["b"]))),
                d_x=max(r(fl, bd) for fl, bd in zip(f_dx, b_dx)), d_w=r(f_dw, b_dw))


def scale_exp(m):
    """hdt_sf's rule: from the largest magnitudes m (float32) the exponents e of the scales 2^e that take them to [2^14, 2^15), from
    the exponent field, clamped to 253 - 127 (a zero or tiny maximum)"""
    ex = (np.ascontiguousarray(m, dtype=np.float32).view(np.uint32) >> 23) & 0xff
    return np.minimum(268 - ex.astype(np.int64), 253) - 127


def d_pre32(y_in, dys):
    """d_pre as the kernels form it, in float32"""
    return [(dy * (np.float32(1) - y * y)).astype(np.float32) for y, dy in zip(y_in, dys)]


def _amax(a, axis):
    return np.abs(a).max(axis=axis) if a.shape[axis] else np.zeros(a.shape[1 - axis], dtype=np.float32)


def scale_tables(c, y_in, tile=64):
    """the six scale tables of one call as exponents: w_rows [N] and w_cols [K]; x_rows and dp_rows: one array per block;
    dp_tile_cols and x_tile_cols: per block a list of one array per row tile"""
    dps = d_pre32(y_in, c["dys"])
    tiles = lambda a: [scale_exp(_amax(a[r:r + tile], 0)) for r in range(0, a.shape[0], tile)]
    return dict(w_rows=scale_exp(_amax(c["w"], 1)), w_cols=scale_exp(_amax(c["w"], 0)),
                x_rows=[scale_exp(_amax(x, 1)) for x in c["xs"]], dp_rows=[scale_exp(_amax(dp, 1)) for dp in dps],
                dp_tile_cols=[tiles(dp) for dp in dps], x_tile_cols=[tiles(x) for x in c["xs"]])


def distinct_scales(c, y_in=None):
    """how many distinct exponents each table holds; the row tables over block 0, the tile tables within block 0's first row tile"""
    if y_in is None:
        y_in = [y.astype(np.float32) for y in forward(c["xs"], c["w"], c["b"])]
    tb = scale_tables(c, y_in)
    first = dict(w_rows=tb["w_rows"], w_cols=tb["w_cols"], x_rows=tb["x_rows"][0], dp_rows=tb["dp_rows"][0],
                 dp_tile_cols=tb["dp_tile_cols"][0][0], x_tile_cols=tb["x_tile_cols"][0][0])
    return {k: len(np.unique(first[k])) for k in TABLES}


def _exps(rng, n, lo, hi):
    """n integer exponents from lo .. hi: every value as often as the others (so small n still get distinct ones), in random order"""
    return (lo + rng.permutation(n) % (hi - lo + 1)).astype(np.int64)


def _pow2(e):
    return np.ldexp(np.float32(1), e).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(K, N, rows, seed=0, dy_scale=1.0, family="default"):
    """inputs of one call, float32, read-only: rows = tuple of the blocks' row counts.  |x| <= 1 (the networks feed tanh and normalize
    outputs), weights and biases of nn.Linear's size, d_y of order 1 times dy_scale.  family: module docstring; every family starts
    from the default's draws, and multiplies by powers of two only (exact)."""
    assert family in FAMILIES, family
    rng = np.random.default_rng([seed, K, N] + list(rows))
    k = 1.0 / np.sqrt(K)
    w = rng.uniform(-k, k, (N, K)).astype(np.float32)
    b = rng.uniform(-k, k, (N,)).astype(np.float32)
    xs = [rng.uniform(-1, 1, (r, K)).astype(np.float32) for r in rows]
    dys = [(rng.standard_normal((r, N)) * dy_scale).astype(np.float32) for r in rows]
    extra = {}
    if family == "scales":
        h = _exps(rng, K, *SCALES_H)
        w = w * _pow2(_exps(rng, N, *SCALES_E)[:, None] - h[None, :])
        xs = [x * _pow2(_exps(rng, x.shape[0], *SCALES_E)[:, None] + h[None, :]) for x in xs]
        q = _exps(rng, N, *SCALES_PQ)
        dys = [d * _pow2(_exps(rng, d.shape[0], *SCALES_PQ)[:, None] + q[None, :]) for d in dys]
    elif family == "zeros":
        z = dict(x_rows=[r // 2 for r in rows], x_col=K // 3, w_row=N // 3, w_col=(2 * K) // 3, dy_col=(2 * N) // 3,
                 dy_rows=[r // 3 if r >= 3 else None for r in rows],
                 dy_tiles=[((r // 64 - 1) * 64, (r // 64) * 64) if r >= 128 else None for r in rows])       # the last whole row tile
        w[z["w_row"], :] = 0
        w[:, z["w_col"]] = 0
        for x, d, xr, dr, dt in zip(xs, dys, z["x_rows"], z["dy_rows"], z["dy_tiles"]):
            x[xr, :] = 0
            x[:, z["x_col"]] = 0
            d[:, z["dy_col"]] = 0
            if dr is not None:
                d[dr, :] = 0
            if dt is not None:
                d[dt[0]:dt[1], :] = 0
        extra["zeros"] = z
    elif family == "range":
        w = w * _pow2(rng.integers(-12, 13, w.shape))
        xs = [x * _pow2(rng.integers(-12, 13, x.shape)) for x in xs]
        # then all of W by ONE more power of two, which takes the largest |x W^T| to [1/2, 1): without it the sums are of order 2^20,
        # every y is +-1 exactly, every d_pre is 0, and the case would pass whatever the kernels did with it
        top = max(float(np.abs(x.astype(np.float64) @ w.astype(np.float64).T).max()) for x in xs)
        w = w * _pow2(-int(np.frexp(top)[1]))
    elif family == "picked":
        assert K >= 2
        for x in xs:
            x[:, 1] *= np.float32(2.0 ** -30)
        w = np.zeros_like(w)
        w[:, 1] = 1
    for a in [w, b] + xs + dys:
        assert a.dtype == np.float32 and np.isfinite(a).all()
        a.setflags(write=False)
    c = dict(K=K, N=N, rows=rows, w=w, b=b, xs=xs, dys=dys, family=family, **extra)
    if family == "scales":
        counts = distinct_scales(c)
        assert min(counts.values()) >= 4, f"a scale table of the scales family is nearly uniform: {counts}"
        # the family tests the scale plumbing, not the floor: the floor term stays below a quarter of the componentwise bound (SCALES_H)
        assert max(floor_share(c).values()) <= 0.25, f"scales: the exponents' ranges are too wide: {floor_share(c)}"
    return c


def pow2_variants(c, s):
    """the four power-of-two changes of one row or column of a case -> list of (name, changed case, scaled, exact): `scaled` maps an
    output (ys, d_xs, d_w, d_b as lists / arrays of the baseline) to what a kernel that scales and unscales exactly must return,
    bit for bit, for the outputs named in `exact`; the remaining outputs change for real and are held to the bound.
      d_y[r, :] 2^s (a row of block 0)  -> d_x[r, :] 2^s; y and every other row of d_x keep their bytes; d_w, d_b: the bound
      d_y[:, n] 2^s (every block)       -> d_w[n, :] 2^s, d_b[n] 2^s; y, the other rows of d_w and the rest of d_b keep their bytes
                                           (d_x sums over n and changes for real: the bound)
      W[:, k] 2^s                       -> d_x[:, k] 2^s; the other columns of d_x, d_w, d_b keep their bytes (y changes: the bound)
      x[:, k] 2^s (every block)         -> d_w[:, k] 2^s; the other columns of d_w, d_b, d_x keep their bytes (y changes: the bound)
    The backward is meant to run from a FIXED saved y (not the changed forward's)."""
    K, N, rows = c["K"], c["N"], c["rows"]
    f = np.float32(2.0 ** s)
    r, n, kw, kx = rows[0] // 2, (2 * N) // 3, K // 3, (2 * K) // 3

    def changed(key, fn):
        """the case with fn applied to a copy of c[key] (to every array of a list)"""
        v = [np.array(a) for a in c[key]] if isinstance(c[key], list) else np.array(c[key])
        for a in (v if isinstance(v, list) else [v]):
            fn(a)
        d = dict(c)
        d[key] = v
        return d

    def scaled(fn):
        """base outputs -> a copy of them with fn(copy) applied"""
        def go(base):
            o = {k_: ([np.array(a) for a in v] if isinstance(v, list) else np.array(v)) for k_, v in base.items()}
            fn(o)
            return o
        return go

    def in_row(a):
        a[r, :] *= f

    def in_col(k_):
        def fn(a):
            a[:, k_] *= f
        return fn

    def out_dx_row(o):
        o["d_xs"][0][r, :] = np.ldexp(o["d_xs"][0][r, :], s)

    def out_dw_row(o):
        o["d_w"][n, :] = np.ldexp(o["d_w"][n, :], s)
        o["d_b"][n] = np.ldexp(o["d_b"][n], s)

    def out_dx_col(o):
        for a in o["d_xs"]:
            a[:, kw] = np.ldexp(a[:, kw], s)

    def out_dw_col(o):
        o["d_w"][:, kx] = np.ldexp(o["d_w"][:, kx], s)

    row_case = changed("dys", lambda a: None)
    in_row(row_case["dys"][0])
    return [(f"d_y[{r}, :] 2^{s}", row_case, scaled(out_dx_row), ("ys", "d_xs")),
            (f"d_y[:, {n}] 2^{s}", changed("dys", in_col(n)), scaled(out_dw_row), ("ys", "d_w", "d_b")),
            (f"W[:, {kw}] 2^{s}", changed("w", in_col(kw)), scaled(out_dx_col), ("d_xs", "d_w", "d_b")),
            (f"x[:, {kx}] 2^{s}", changed("xs", in_col(kx)), scaled(out_dw_col), ("d_xs", "d_w", "d_b"))]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int32), b.view(np.int32)))


def check(name, got, want64, bound):
    """-> the largest error / bound of the array (0 / 0 counts as 0); asserts it is <= 1"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want64)
    assert np.isfinite(err).all(), f"{name}: not finite"
    ratio = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0
    assert ratio <= 1.0, f"{name}: error {ratio:.3f} x the bound"
    return ratio
