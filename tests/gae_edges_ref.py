"""Case tables for the edge tests of hh_gae and hh_gae_rllib (csrc/hh_gae.h): shapes either side of the 256-lane block, T from 1, done
patterns that an index taken from the wrong quotient cannot pass, gamma and lambda at 0 and 1, and a table on which the masked recursion
is exact in float32.  The yardsticks: oracle/gae_ref.py's rllib_stream (bit for bit) for hh_gae_rllib, and for hh_gae the masked recursion
restated here in float64, with the same in float32 for e32, the cost of the format (tests/test_gae_edges_host.py shows that this float32
form is gae_ref.masked_stream bit for bit)."""
import functools
import zlib

import numpy as np

# (N, nA): N * nA = 1, 255, 256, 257, 513 where nA divides it, and the nearest counts either side of 256 where it does not
SHAPES = ((1, 1), (255, 1), (256, 1), (257, 1), (513, 1), (127, 2), (128, 2), (129, 2), (85, 3), (86, 3), (171, 3))
TS = (1, 2, 97)
DONES = ("none", "every", "first", "last", "ragged")
GAMMA_LAMBDA = ((0.99, 0.95), (0.99, 1.0), (1.0, 1.0), (0.0, 0.95), (0.99, 0.0))
GL_SHAPES = ((257, 1), (128, 2), (85, 3))            # the shapes that run every (gamma, lambda)


def cases():
    """(N, nA, T, done pattern, gamma, lambda)"""
    out = [(N, nA, T, d) + GAMMA_LAMBDA[0] for (N, nA) in SHAPES for T in TS for d in DONES]
    out += [(N, nA, T, d) + gl for gl in GAMMA_LAMBDA[1:] for (N, nA) in GL_SHAPES for T in TS for d in DONES]
    return out


def done_pattern(name, T, N, rng):
    done = np.zeros((T, N), dtype=np.uint8)
    if name == "every":
        done[:] = 1
    elif name == "first":
        done[0] = 1
    elif name == "last":
        done[T - 1] = 1
    elif name == "ragged":                           # differs from arena to arena, periodic in nothing
        done[:] = rng.random((T, N)) < 0.15
    return done


def masked(reward, valid, value, done, gamma, lam, dtype):
    """hh_gae's recursion (csrc/hh_gae.h) in `dtype`, on the float32 inputs and the float32 gamma and lambda the kernel is given:
         delta_t = r_t + gamma V_{t+1} (1 - done_t) - V_t,   A_t = delta_t + gamma lambda (1 - done_t) A_{t+1},   R_t = A_t + V_t
    a row with valid = 0 has A = R = 0, passes nothing on and its reward is not read"""
    T = reward.shape[0]
    g, l = dtype(np.float32(gamma)), dtype(np.float32(lam))
    r, v = reward.astype(dtype), value.astype(dtype)
    adv, ret = np.zeros(reward.shape, dtype=dtype), np.zeros(reward.shape, dtype=dtype)
    a_next, v_next = np.zeros(reward.shape[1:], dtype=dtype), v[T]
    with np.errstate(invalid="ignore"):
        for t in range(T - 1, -1, -1):
            nd = (1 - done[t].astype(dtype))[:, None]
            delta = r[t] + g * v_next * nd - v[t]
            a = delta + g * l * nd * a_next
            a = np.where(valid[t] > 0, a, dtype(0))
            adv[t], ret[t] = a, np.where(valid[t] > 0, a + v[t], dtype(0))
            a_next, v_next = a, v[t]
    return adv, ret


def errors(got, want):
    return tuple(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got, want))


FEW = 8


def e32_is_representative(want, e32):
    """at least a quarter ulp at the scale of the compared quantity, e32 >= 2^-25 max |float64 value|: half of the largest error that a
    single rounding, which is all that some of these cases hold, can leave (nothing of the kernel's enters)"""
    return all(e > 0.0 and e >= 2.0 ** -25 * float(np.abs(w).max()) for e, w in zip(e32, want))


def _draw(case, seed):
    N, nA, T, dname, gamma, lam = case
    rng = np.random.default_rng(zlib.crc32(repr((N, nA, T, dname, seed)).encode()))
    reward = rng.standard_normal((T, N, nA)).astype(np.float32)
    value = rng.standard_normal((T + 1, N, nA)).astype(np.float32)
    valid = (rng.random((T, N, nA)) < 0.85).astype(np.uint8)
    valid[T - 1, 0, 0] = 1
    return dict(reward=reward, value=value, valid=valid, done=done_pattern(dname, T, N, rng))


@functools.lru_cache(maxsize=None)
def general_case(case):
    """-> (inputs, float64 restatement (adv, ret), e32 (adv, ret)).  On a handful of elements e32 is a single draw and can be a small
    fraction of an ulp, or 0, by luck: up to FEW elements the seed is the first of 0..63 at which e32 is representative (see there),
    everywhere else 0; the host test asserts e32 > 0 everywhere and the representative e32 on the small cases."""
    N, nA, T = case[:3]
    for seed in range(64 if N * nA * T <= FEW else 1):
        x = _draw(case, seed)
        want = masked(x["reward"], x["valid"], x["value"], x["done"], case[4], case[5], np.float64)
        e32 = errors(masked(x["reward"], x["valid"], x["value"], x["done"], case[4], case[5], np.float32), want)
        if N * nA * T > FEW or e32_is_representative(want, e32):
            break
    return x, want, e32


# ---- the exact table: gamma = lambda = 0.5, rewards and values multiples of 1/64 in [-8, 8].  gamma V is a multiple of 2^-7 and each
# step of the recursion (gamma lambda = 2^-2) needs two more bits, so after k steps A is a multiple of 2^-(5 + 2 k) below 32: 24 bits
# at k = 7.  T = 8 takes multiples of 1/16.  The host test asserts float32 == float64 on every case.
EXACT_CASES = tuple((N, nA, T, 16 if T == 8 else 64) for (N, nA) in ((257, 1), (128, 2), (86, 3)) for T in (1, 2, 7, 8))


@functools.lru_cache(maxsize=None)
def exact_case(case):
    N, nA, T, den = case
    rng = np.random.default_rng(zlib.crc32(repr(("exact",) + case).encode()))
    reward = (rng.integers(-8 * den, 8 * den + 1, (T, N, nA)) / den).astype(np.float32)
    value = (rng.integers(-8 * den, 8 * den + 1, (T + 1, N, nA)) / den).astype(np.float32)
    valid = (rng.random((T, N, nA)) < 0.85).astype(np.uint8)
    return dict(reward=reward, value=value, valid=valid, done=done_pattern("ragged", T, N, rng))
