"""TEST INFRASTRUCTURE (no GPU) — the PPO sampler step (hh_policy_sample: hh_k_policy_ppo / hh_k_policy_w16_ppo) restated row by row from
oracle/policy_ref.py, and the table of edge cases both tests/test_sampler_edges_host.py (CPU: the reference alone meets the conditions the
exact comparisons rest on) and tests/test_gpu_sampler_edges.py (the kernels against it) iterate over.

A call is described per ROW: `kinds_by_row[r]` is the network kind row r flies (-1: none, the row is in no list).  Rows come in pairs
(arena n = rows 2 n, 2 n + 1): the value branch of row r takes the other agent's observation and action inputs from row r ^ 1, listed or not."""
import functools
import zlib

import numpy as np
import torch

from hhmarl_2d_amd import policy_nets as PN
import policy_ref as PR   # oracle/policy_ref.py

KINDS = (PN.FIGHT1, PN.FIGHT2, PN.ESC1, PN.ESC2)
SEL = {PN.FIGHT1: 5, PN.FIGHT2: 9, PN.ESC1: 6, PN.ESC2: 10}   # pilots.SEL_*: (1 fight | 2 escape) | aircraft type << 2
MODE_KINDS = {"fight": (PN.FIGHT1, PN.FIGHT2), "escape": (PN.ESC1, PN.ESC2)}
MODE_D = {"fight": 26, "escape": 30}      # the observation width of a LowLevelEnv world of that mode
EDGE_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97)   # around the 16-row wave, the 32-row tile and the 64-row tile
ONE_BELOW = 1.0 - 2.0 ** -53              # the largest double below 1
MIN_HALF_WIDTH = 1e-3                     # see test_sampler_edges_host.py


def n_comp(kind):
    return 4 if PN.N_OUT[kind] == 26 else 3


@functools.lru_cache(maxsize=None)
def weights(seed):
    """kind -> (actor tensors, value-branch tensors): per-slot shared layers (tie_shared = False)"""
    return {k: (PN.random_weights(k, seed), PN.random_critic_weights(k, seed)) for k in KINDS}


def sample_ref(kinds_by_row, weights, obs, crit_act, uniforms, greedy):
    """The sampler step on rows [R, D] (R even) -> dict of per-row arrays:
        logits float32 [R, 32]   policy_ref.torch_forward (fp32, CPU) in columns < N_OUT, 0 beyond; NaN on rows without a network
        vf     float32 [R]       policy_ref.torch_value, the other agent = row r ^ 1 (its first d2 observation columns and a2 action inputs)
        actions int8 [R, 4]      policy_ref.inverse_cdf_actions (float64) of `uniforms` [R, 4], or policy_ref.decode if greedy; 0 without a network
        logp, margin float64 [R] of that draw (greedy: the log-probability of the arg-max, margin = inf)
    weights: kind -> (sd, csd); crit_act [R, 4] or None (zeros)"""
    kinds_by_row = np.asarray(kinds_by_row).reshape(-1)
    R = len(kinds_by_row)
    assert R % 2 == 0
    o = torch.tensor(np.asarray(obs), dtype=torch.float32).reshape(R, -1)
    ca = torch.zeros((R, 4)) if crit_act is None else torch.tensor(np.asarray(crit_act), dtype=torch.float32).reshape(R, 4)
    out = dict(logits=np.full((R, 32), np.nan, dtype=np.float32), vf=np.full(R, np.nan, dtype=np.float32), actions=np.zeros((R, 4), dtype=np.int8),
               logp=np.full(R, np.nan), margin=np.full(R, np.nan))
    for kind in KINDS:
        idx = np.flatnonzero(kinds_by_row == kind)
        if not len(idx):
            continue
        sd, csd = weights[kind]
        n_out = PN.N_OUT[kind]
        lg = PR.torch_forward(kind, sd, o[idx])
        out["logits"][idx] = 0.0
        out["logits"][idx, :n_out] = lg.numpy()
        out["vf"][idx] = PR.torch_value(kind, sd, csd, o[idx], ca[idx], o[idx ^ 1], ca[idx ^ 1]).numpy()
        if greedy:
            act = PR.decode(lg, n_out).numpy()
            out["actions"][idx] = act
            out["logp"][idx] = PR.multicategorical_logp(lg, act, n_out).double().numpy()
            out["margin"][idx] = np.inf
        else:
            u = np.asarray(uniforms, dtype=np.float64).reshape(R, 4)[idx]
            out["actions"][idx], out["logp"][idx], out["margin"][idx] = PR.inverse_cdf_actions(lg.numpy(), u, n_out)
    return out


def cycle_targets(n_rows, n_out):
    """target action of list position `row`, component k: (row + k) % width — every index of every component in turn"""
    t = np.zeros((n_rows, 4), dtype=np.int64)
    for k, w in enumerate(PN.ACTION_SPLIT[: 4 if n_out == 26 else 3]):
        t[:, k] = (np.arange(n_rows) + k) % w
    return t


def midpoint_uniforms(ref_logits, n_out, targets):
    """per row and component the u in the middle of the target index's interval of the float64 softmax CDF of `ref_logits` (the CDF of
    policy_ref.inverse_cdf_actions) -> (u float64 [R, 4], the smallest half-width of an interval used).  A component the kind does not have: 0.5"""
    lg = np.asarray(ref_logits, dtype=np.float64)
    targets = np.asarray(targets)
    u = np.full((lg.shape[0], 4), 0.5)
    half = np.inf
    lo = 0
    rows = np.arange(lg.shape[0])
    for k, w in enumerate(PN.ACTION_SPLIT[: 4 if n_out == 26 else 3]):
        seg = lg[:, lo:lo + w]
        e = np.exp(seg - seg.max(axis=1, keepdims=True))
        cdf = np.concatenate((np.zeros((len(rows), 1)), np.cumsum(e, axis=1) / e.sum(axis=1, keepdims=True)), axis=1)
        a, b = cdf[rows, targets[:, k]], cdf[rows, targets[:, k] + 1]
        u[:, k] = 0.5 * (a + b)
        if len(rows):
            half = min(half, float((0.5 * (b - a)).min()))
        lo += w
    return u, half


# ------------------------------------------------------------------------------------------------------------------------ the cases
# name, mode (fight | escape | four), arenas N, selector pattern, crit_act, uniform pattern, weight seed
#   selectors: "uniform"    every arena flies the mode's two networks
#              "third_off"  selector 0 on a random third of the ROWS
#              "four_nets"  row 0 from {FIGHT1, ESC1, none}, row 1 from {FIGHT2, ESC2, none}
#   crit_act:  "scaled" = PN.scale_actions of random actions | "zero"
#   uniforms:  "midpoint" (cycle_targets) | "zero" (u = 0) | "one" (u = 1 - 2^-53)
def _cases():
    out = []
    for mode in ("fight", "escape"):
        for n in EDGE_LENGTHS:
            out.append(dict(name=f"ragged-{mode}-{n}", group="ragged", mode=mode, n=n, sel="uniform", crit_act="scaled", uniforms="midpoint", seed=5))
    for mode in ("fight", "escape"):
        for n in (97, 333):
            out.append(dict(name=f"no-network-{mode}-{n}", group="no-network", mode=mode, n=n, sel="third_off", crit_act="scaled", uniforms="midpoint", seed=9))
    out.append(dict(name="four-nets-333", group="four-nets", mode="four", n=333, sel="four_nets", crit_act="scaled", uniforms="midpoint", seed=9))
    for mode in ("fight", "escape"):
        for pat in ("zero", "one"):
            out.append(dict(name=f"draw-{pat}-{mode}-33", group="draw-edges", mode=mode, n=33, sel="uniform", crit_act="zero", uniforms=pat, seed=5))
    return out


CASES = _cases()
CASE_BY_NAME = {c["name"]: c for c in CASES}


def case_kinds(case):
    """kinds_by_row [N, 2] of a case (-1: no network)"""
    N = case["n"]
    rng = np.random.default_rng([zlib.crc32(case["name"].encode()), 1])
    if case["sel"] == "four_nets":
        k = np.stack((np.array([PN.FIGHT1, PN.ESC1, -1])[rng.integers(0, 3, N)], np.array([PN.FIGHT2, PN.ESC2, -1])[rng.integers(0, 3, N)]), axis=1)
    else:
        k = np.tile(np.array(MODE_KINDS[case["mode"]]), (N, 1))
        if case["sel"] == "third_off":
            k[rng.random((N, 2)) < 1.0 / 3.0] = -1
    return k.astype(np.int64)


def list_lengths(cases):
    """kind -> the set of per-network list lengths over `cases`"""
    out = {k: set() for k in KINDS}
    for c in cases:
        kk = case_kinds(c)
        for k in KINDS:
            if (kk == k).any():
                out[k].add(int((kk == k).sum()))
    return out


@functools.lru_cache(maxsize=None)
def _build(name):
    case = CASE_BY_NAME[name]
    N = case["n"]
    kinds = case_kinds(case)
    rng = np.random.default_rng([zlib.crc32(name.encode()), 2])
    obs = rng.uniform(-1.0, 1.0, (N, 2, 30)).astype(np.float32)
    obs[kinds == PN.FIGHT2, 24:] = 0.0          # the friend block a type-2 agent of a fight world does not have
    if case["crit_act"] == "scaled":
        a = np.stack([rng.integers(0, w, (N, 2)) for w in PN.ACTION_SPLIT], axis=-1).astype(np.int8)
        ca = PN.scale_actions(a)
    else:
        ca = np.zeros((N, 2, 4), dtype=np.float32)
    dead = (kinds < 0).all(axis=1)              # neither row listed: nothing may read the pair
    obs[dead] = np.nan
    ca[dead] = np.nan
    sel = np.zeros((N, 2), dtype=np.uint8)
    for k in KINDS:
        sel[kinds == k] = SEL[k]
    D = 30 if case["mode"] == "four" else MODE_D[case["mode"]]
    W = weights(case["seed"])
    flat = kinds.reshape(-1)
    base = sample_ref(flat, W, obs.reshape(2 * N, 30), ca.reshape(2 * N, 4), None, True)
    u = np.full((2 * N, 4), 0.5)
    targets = np.zeros((2 * N, 4), dtype=np.int64)
    half = np.inf
    if case["uniforms"] == "midpoint":
        for k in KINDS:
            idx = np.flatnonzero(flat == k)          # list position = rank among the kind's rows
            if len(idx):
                targets[idx] = cycle_targets(len(idx), PN.N_OUT[k])
                u[idx], h = midpoint_uniforms(base["logits"][idx, : PN.N_OUT[k]], PN.N_OUT[k], targets[idx])
                half = min(half, h)
    else:
        u[:] = 0.0 if case["uniforms"] == "zero" else ONE_BELOW
    ref = sample_ref(flat, W, obs.reshape(2 * N, 30), ca.reshape(2 * N, 4), u, False)
    for d in (base, ref):
        for v in d.values():
            v.setflags(write=False)
    for v in (kinds, sel, obs, ca, u, targets):
        v.setflags(write=False)
    return dict(case=case, kinds=kinds, sel=sel, obs30=obs, crit_act=ca, uniforms=u.reshape(N, 2, 4), targets=targets, half_width=half, D=D, ref=ref,
                greedy=base)


def build(case):
    """the inputs and the reference of a case, computed once per process and read-only:
        kinds [N, 2], sel uint8 [N, 2], obs30 f32 [N, 2, 30] (uniform(-1, 1); the case's own stride is D: obs30[..., :D]), crit_act f32 [N, 2, 4],
        uniforms f64 [N, 2, 4], targets [2 N, 4] (midpoint cases), half_width, ref = sample_ref of the draw, greedy = sample_ref(greedy = True)"""
    return _build(case["name"] if isinstance(case, dict) else case)


def with_garbage(inp):
    """obs30 of a case with NaN in every column a kernel must not read: at or beyond the row's own OBS_DIM and, where its partner is listed, at or
    beyond the partner's d2 — the larger of the two is the first column nobody reads"""
    kinds, obs = inp["kinds"], inp["obs30"].copy()
    for n in range(kinds.shape[0]):
        for s in range(2):
            own = PN.OBS_DIM[kinds[n, s]] if kinds[n, s] >= 0 else 0
            other = PN.CRITIC_DIMS[kinds[n, 1 - s]][2] if kinds[n, 1 - s] >= 0 else 0
            obs[n, s, max(own, other):] = np.nan
    return obs
