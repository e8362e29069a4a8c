"""float64 restatement of hh_dense_tanh_* (include/hh_learner.h) and the error bound the tests hold the kernels to.  No test in here.

The bound is derived, not measured.  For a product C = A B with a sum of length n, computed with both operands as fp16 (hi, lo) pairs
(hi hi + lo hi + hi lo, float32 accumulators):

    |C - C64| <= (4 * 2^-22 + (n + 2) * 2^-24) (|A| |B|)        componentwise

  2^-22 for each of the two operands' 11 + 11-bit representation, 2^-22 for the dropped lo lo product, 3 * 2^-24 for forming
  d_pre = d_y (1 - y^2) in float32 (together 3 * 2^-22 + 3 * 2^-24 < 4 * 2^-22), and (n + 2) * 2^-24 for float32 accumulation of n
  terms in any order and the final rounding.
Forward: the right-hand side gets |b| added (the bias joins the sum), and 4 * 2^-24 absolute for tanhf (<= 2 ulp of a result <= 1, and
tanh is 1-Lipschitz, so the pre-activation's error carries over as it is).
d_b: (R + 2) * 2^-24 * sum |d_pre| (a plain sum of R terms)."""
import functools

import numpy as np

U22, U24 = 2.0 ** -22, 2.0 ** -24
DIMS = ((500, 500), (512, 512), (481, 497), (1, 1), (33, 17))       # (K, N)


def row_counts(K, N, tile, parts):
    """the row counts of the first block that the tests run for (K, N): around one tile; at 500 x 500 also past the partial-sum cap"""
    return (1, tile - 1, tile, tile + 1) + ((parts * tile + 1,) if (K, N) == (500, 500) else ())


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


def backward_bounds(xs, d_pres64, w):
    """-> (bounds of d_xs, of d_w, of d_b) from the float64 d_pre"""
    N = w.shape[0]
    R = sum(x.shape[0] for x in xs)
    aw = np.abs(w.astype(np.float64))
    b_dx = [factor(N) * (np.abs(dp) @ aw) for dp in d_pres64]
    b_dw = factor(R) * sum(np.abs(dp).T @ np.abs(x.astype(np.float64)) for dp, x in zip(d_pres64, xs))
    b_db = (R + 2) * U24 * sum(np.abs(dp).sum(axis=0) for dp in d_pres64)
    return b_dx, b_dw, b_db


@functools.lru_cache(maxsize=None)
def case(K, N, rows, seed=0, dy_scale=1.0):
    """inputs of one call, float32, read-only: rows = tuple of the blocks' row counts.  |x| <= 1 (the networks feed tanh and normalize
    outputs), weights and biases of nn.Linear's size, d_y of order 1 times dy_scale."""
    rng = np.random.default_rng([seed, K, N] + list(rows))
    k = 1.0 / np.sqrt(K)
    w = rng.uniform(-k, k, (N, K)).astype(np.float32)
    b = rng.uniform(-k, k, (N,)).astype(np.float32)
    xs = [rng.uniform(-1, 1, (r, K)).astype(np.float32) for r in rows]
    dys = [(rng.standard_normal((r, N)) * dy_scale).astype(np.float32) for r in rows]
    for a in [w, b] + xs + dys:
        a.setflags(write=False)
    return dict(K=K, N=N, rows=rows, w=w, b=b, xs=xs, dys=dys)


def check(name, got, want64, bound):
    """-> the largest error / bound of the array (0 / 0 counts as 0); asserts it is <= 1"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want64)
    assert np.isfinite(err).all(), f"{name}: not finite"
    ratio = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0
    assert ratio <= 1.0, f"{name}: error {ratio:.3f} x the bound"
    return ratio
