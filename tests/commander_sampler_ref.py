"""TEST INFRASTRUCTURE (no GPU) — one sampler step of the commander (hh_commander_sample: hh_k_commander) restated arena by arena from
tests/commander_ref.py, and the table of edge cases both tests/test_commander_sampler_edges_host.py (CPU: the reference alone meets the
conditions the exact comparisons rest on) and tests/test_gpu_commander_sampler_edges.py (the kernels against it) iterate over.

A call has N arenas = 3 N agent rows (row r = agent slot r % 3 of arena r // 3) and the kernel works on 32-row tiles, so an arena's three
rows straddle a tile edge wherever 3 N is no multiple of 32: `straddlers(N)`.  The value branch of row r reads the other two slots of its
arena, whichever tile they are in."""
import functools
import zlib

import numpy as np
import torch

from hhmarl_2d_amd.commander import random_weights
import commander_ref as CR

TILE = 32                                  # HHC_R
TOL = 1e-5                                 # the bound of tests/test_gpu_commander.py and tests/test_gpu_commander_chain.py
ONE_BELOW = 1.0 - 2.0 ** -53               # the largest double below 1
MIN_HALF_WIDTH = 1e-3                      # see test_commander_sampler_edges_host.py
MIN_GREEDY_GAP = 4e-5                      # twice the 2 x TOL by which the bound lets the gap between two logits move
EXACT_STEP = 1e-3                          # distance of the exact-logit table's uniforms from the CDF boundary they sit beside
EXACT_CLEAR = 1e-4                         # ... and the least distance from EVERY float64 boundary the host test holds them to
RAGGED_N = (1, 5, 10, 11, 21, 22, 32, 33, 43, 97)
RAGGED_ROWS = (3, 15, 30, 33, 63, 66, 96, 99, 129, 291)   # either side of one, two and three tiles; 33 = 2|1 and 66 = 1|2 across an edge
FRESH_PATTERNS = ("none", "all", "alternating", "straddle")
SEED = 4                                   # commander.random_weights; chosen for the greedy gap (test_commander_sampler_edges_host.py)
MAX_ROWS = 3 * 128
W_ACT_OUT, B_ACT_OUT = "act_out._model.0.weight", "act_out._model.0.bias"


@functools.lru_cache(maxsize=None)
def weights(seed=SEED):
    """the reference's state_dict as numpy float32 (hhmarl_2d_amd.commander.random_weights); read-only"""
    sd = random_weights(seed)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def torch_weights(sd, dtype):
    """commander_ref.to_torch of a state_dict of (read-only) numpy arrays"""
    return CR.to_torch({k: np.array(v) for k, v in sd.items()}, dtype)


@functools.lru_cache(maxsize=None)
def _sd(seed, dtype):
    return torch_weights(weights(seed), dtype)


def straddlers(N):
    """the arenas of an N-arena call whose three rows lie in two tiles"""
    n = np.arange(N)
    return n[(3 * n) // TILE != (3 * n + 2) // TILE]


def reference(sd, obs, h_given, fresh, crit_act):
    """hh_commander_sample's forward with torch ops in sd's dtype: the states of fresh arenas are zeros WHATEVER h_given holds there
    -> (logits [N, 3, 3], vf [N, 3], h_out [N, 3, 2, 200]) as numpy, and the state the forward used [N, 3, 2, 200] float32"""
    dtype = next(iter(sd.values())).dtype
    h0 = np.array(h_given, dtype=np.float32)
    if fresh is not None:
        h0[np.asarray(fresh).astype(bool)] = 0.0
    t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    with torch.no_grad():
        lg, v, h = CR.arena_forward(sd, t(obs), t(h0), t(crit_act))
    return lg.numpy(), v.numpy(), h.numpy(), h0


def targets(n_rows):
    """the target action of row r: (r + r // 3) % 3 — every action on every agent slot, and on both sides of a tile edge"""
    r = np.arange(n_rows)
    return (r + r // 3) % 3


def cdf64(logits):
    """the float64 softmax CDF of logits [..., 3] with a leading 0 -> [..., 4]"""
    lg = np.asarray(logits, dtype=np.float64)
    e = np.exp(lg - lg.max(axis=-1, keepdims=True))
    return np.concatenate((np.zeros(lg.shape[:-1] + (1,)), np.cumsum(e, axis=-1) / e.sum(axis=-1, keepdims=True)), axis=-1)


def midpoint_uniforms(ref_logits, tgt):
    """per row the u in the middle of the target's interval of the float64 softmax CDF -> (u [R], half-width of each interval [R])"""
    cdf = cdf64(np.asarray(ref_logits).reshape(-1, 3))
    rows = np.arange(cdf.shape[0])
    a, b = cdf[rows, tgt], cdf[rows, tgt + 1]
    return 0.5 * (a + b), 0.5 * (b - a)


def inverse_cdf_f32(logits, u):
    """hh_commander_sample's draw as include/hh_commander.h words it, in numpy float32 and the kernel's operation order: m = max l,
    S = (e_0 + e_1) + e_2 with e_i = exp(l_i - m), t = (float) u * S, the first i whose running sum exceeds t, the last if none does.
    logits [..., 3], u [...] -> action int64"""
    l = np.asarray(logits, dtype=np.float32)
    m = l.max(axis=-1, keepdims=True)
    with np.errstate(under="ignore"):
        e = np.exp((l - m).astype(np.float32)).astype(np.float32)
    S = ((e[..., 0] + e[..., 1]).astype(np.float32) + e[..., 2]).astype(np.float32)
    t = (np.asarray(u, dtype=np.float64).astype(np.float32) * S).astype(np.float32)
    c0 = e[..., 0]
    c1 = (c0 + e[..., 1]).astype(np.float32)
    return np.where(c0 > t, 0, np.where(c1 > t, 1, 2)).astype(np.int64)


def first_max(logits):
    """hhc_first_max = torch.argmax's first maximum"""
    return np.argmax(np.asarray(logits), axis=-1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------ the cases
# name, group, arenas n, fresh pattern ("random" | FRESH_PATTERNS), nan_states (h_in of fresh arenas holds NaN), crit_act ("distinct": the
# three slots of every arena hold 0, 0.5 and 1 in a random order | "random": each slot any of the three | "zero": NULL), uniforms
# ("midpoint" | "zero" | "one"), weight seed
def _cases():
    out = []
    for n in RAGGED_N:
        out.append(dict(name=f"ragged-{n}", group="ragged", n=n, fresh="random", nan_states=False, crit_act="distinct", uniforms="midpoint", seed=SEED))
    for n in (11, 22):
        for pat in FRESH_PATTERNS:
            out.append(dict(name=f"fresh-{n}-{pat}", group="fresh", n=n, fresh=pat, nan_states=True, crit_act="random", uniforms="midpoint", seed=SEED))
    for pat in ("zero", "one"):
        out.append(dict(name=f"draw-{pat}-11", group="draw-edges", n=11, fresh="random", nan_states=False, crit_act="zero", uniforms=pat, seed=SEED))
    return out


CASES = _cases()
CASE_BY_NAME = {c["name"]: c for c in CASES}


def names(group):
    return [c["name"] for c in CASES if c["group"] == group]


def row_counts(cases):
    """the set of 3 N over the `ragged` cases among `cases`"""
    return {3 * c["n"] for c in cases if c["group"] == "ragged"}


def case_fresh(case):
    N, pat = case["n"], case["fresh"]
    f = np.zeros(N, dtype=np.uint8)
    if pat == "random":
        f[:] = np.random.default_rng([zlib.crc32(case["name"].encode()), 1]).random(N) < 0.3
    elif pat == "all":
        f[:] = 1
    elif pat == "alternating":
        f[0::2] = 1
    elif pat == "straddle":
        f[straddlers(N)] = 1
    else:
        assert pat == "none"
    return f


def make_inputs(name, N, crit="distinct"):
    """observations as tests/test_gpu_commander.py draws them (uniform [0, 1), the opponent block of a fifth of the rows and a tenth of
    the rows as a whole zeroed), one arena with all three rows zero (N >= 3), states uniform (-1, 1), crit_act in {0, 0.5, 1}"""
    rng = np.random.default_rng([zlib.crc32(name.encode()), 2])
    obs = rng.random((N, 3, 34), dtype=np.float32)
    obs[:, :, 4:24] *= rng.random((N, 3, 1)) > 0.2
    obs *= rng.random((N, 3, 1)) > 0.1
    if N >= 3:
        obs[(N - 1) // 2] = 0.0
    h = rng.uniform(-1.0, 1.0, (N, 3, 2, 200)).astype(np.float32)
    if crit == "distinct":
        ca = np.stack([rng.permutation(3) for _ in range(N)]).astype(np.float32) / 2.0
    elif crit == "random":
        ca = rng.integers(0, 3, (N, 3)).astype(np.float32) / 2.0
    else:
        ca = None
    return obs, h, ca


@functools.lru_cache(maxsize=None)
def _build(name):
    case = CASE_BY_NAME[name]
    N = case["n"]
    obs, h, ca = make_inputs(name, N, case["crit_act"])
    fresh = case_fresh(case)
    if case["nan_states"]:
        h[fresh.astype(bool)] = np.nan
    lg, vf, h_out, h0 = reference(_sd(case["seed"], torch.float64), obs, h, fresh, ca)
    lg32, vf32, h32, _ = reference(_sd(case["seed"], torch.float32), obs, h, fresh, ca)
    tgt = targets(3 * N)
    if case["uniforms"] == "midpoint":
        u, half = midpoint_uniforms(lg, tgt)
    else:
        u, half = np.full(3 * N, 0.0 if case["uniforms"] == "zero" else ONE_BELOW), np.full(3 * N, np.nan)
    u = u.reshape(N, 3)
    act, logp = CR.inverse_cdf(lg, u)
    top = np.sort(lg, axis=-1)
    ref = dict(logits=lg, vf=vf, h_out=h_out, actions=act, logp=logp, greedy=first_max(lg), gap=top[..., 2] - top[..., 1])
    f32 = dict(logits=lg32, vf=vf32, h_out=h32)
    e32 = {k: float(np.abs(f32[k].astype(np.float64) - ref[k]).max()) for k in f32}
    out = dict(case=case, n=N, obs=obs, h_in=h, h_used=h0, fresh=fresh, crit_act=ca, uniforms=u, targets=tgt.reshape(N, 3), half_width=half.reshape(N, 3),
               ref=ref, f32=f32, e32=e32)
    for d in (out, ref, f32):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def build(case):
    """the inputs and the references of a case, computed once per process and read-only:
        obs f32 [N, 3, 34], h_in f32 [N, 3, 2, 200] (NaN in fresh arenas where the case says so), h_used (zeros there: what h_in must hold after
        the call), fresh u8 [N], crit_act f32 [N, 3] or None, uniforms f64 [N, 3], targets [N, 3] and half_width [N, 3] (midpoint cases),
        ref = the float64 restatement (commander_ref.arena_forward / inverse_cdf): logits [N, 3, 3], vf [N, 3], h_out [N, 3, 2, 200], actions
              and logp of `uniforms`, greedy (first arg-max), gap (largest minus second largest logit),
        f32 = logits, vf, h_out of the same forward with float32 torch ops, e32 = max |f32 - ref| per output"""
    return _build(case["name"] if isinstance(case, dict) else case)


# ------------------------------------------------------------------------------------------------------------- the exact-logit table
# act_out._model.0.weight = 0: the kernel sums y * 0.0f, so its logits are the act_out bias bit for bit.  Gaps are at most 80 or at least 200:
# float32 exp is then a normal number or exactly 0, never a denormal.
TIES = ((0.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0))
BIAS_TRIPLES = TIES + ((0.0, -1.0, 1.0), (-200.0, 0.0, 0.0), (0.0, -200.0, 0.0), (0.0, 0.0, -200.0), (-200.0, 0.0, -200.0), (0.0, -80.0, 0.0))


def exact_weights(bias, seed=SEED):
    sd = dict(weights(seed))
    sd[W_ACT_OUT] = np.zeros_like(sd[W_ACT_OUT])
    sd[B_ACT_OUT] = np.asarray(bias, dtype=np.float32)
    return sd


@functools.lru_cache(maxsize=None)
def exact_table():
    """per bias triple: the uniforms 0, 1 - 2^-53 and, for every boundary b of the float64 softmax CDF, b - EXACT_STEP and b + EXACT_STEP
    where they lie inside (0, 1) (a boundary a float32 cannot tell from 0 or 1 — the e^-200 ones — keeps its inner neighbour only), with
        expected  the float32 restatement of the draw (inverse_cdf_f32) — what the kernel must return
        act64     the float64 restatement (commander_ref.inverse_cdf)
        logp64    float64 log-softmax at `expected`
        clear     the distance of u from the nearest float64 boundary (0 and 1 are none)
        greedy    the first arg-max"""
    rows = []
    for bias in BIAS_TRIPLES:
        b = np.asarray(bias, dtype=np.float64)
        inner = cdf64(b)[1:3]
        us = [0.0, ONE_BELOW] + [float(x + d) for x in inner for d in (-EXACT_STEP, EXACT_STEP) if 0.0 < x + d < 1.0]
        us = np.array(sorted(set(us)))
        lg = np.tile(b, (len(us), 1))
        expected = inverse_cdf_f32(lg, us)
        act64, _ = CR.inverse_cdf(lg, us)
        lsm = (b - b.max()) - np.log(np.exp(b - b.max()).sum())
        rows.append(dict(bias=tuple(float(x) for x in bias), uniforms=us, expected=expected, act64=act64, logp64=lsm[expected],
                         clear=np.abs(us[:, None] - inner[None, :]).min(axis=1), greedy=int(first_max(b))))
    return rows
