"""Restatements and input tables for hh_heads_loss (include/hh_learner.h, csrc/hh_heads_loss.h): the whole tail of a minibatch step behind
shared_layer's GEMM — tanh, act_out and val_out, RLlib 2.4's PPO loss, and the gradient of the total with respect to the pre-activations
za, zc and the four head parameters — written with torch ops and autograd in a chosen dtype.  float64 is the yardstick, float32 gives e32,
the cost of the format, per compared quantity; the kernel may be at most 4 x e32 away from float64 (the project's rule).

Nothing here imports the package's learner: the loss is spelled out again from include/hh_learner.h's formulas.

No row is ever left out of a comparison, so the tables keep every unmasked row at least KINK_MARGIN away from each kink (the ratio at
1 +- clip_param, the squared value error at vf_clip_param, and the two arguments of the surrogate's min where the ratio is clipped): a
last-bit difference in a logit cannot flip a branch.  tests/test_heads_loss_host.py asserts that on every table; the kinks themselves
are covered by tests/test_gpu_ppo_loss_edges.py, whose branch logic is the same device code."""
import ctypes as C
import functools

import torch

INSTANCES = (4, 3, 1)                                        # hh_ppo_loss_params.n_comp; 1 = the commander's Categorical
WIDTHS = {4: (13, 9, 2, 2), 3: (13, 9, 2), 1: (3,)}
N_OUT = {4: 26, 3: 24, 1: 3}
OLD_LD = {4: 32, 3: 32, 1: 4}
K = 500
CLIP = 0.25
KINK_MARGIN = 1e-3
U32, U64 = 2.0 ** -24, 2.0 ** -53
ROW_KEYS = ("za", "zc", "old_logits", "actions", "old_logp", "adv", "target")
WEIGHT_KEYS = ("w_act", "b_act", "w_val", "b_val")
GRADS = ("d_za", "d_zc", "d_w_act", "d_b_act", "d_w_val", "d_b_val")
QUANTITIES = ("stats",) + GRADS + ("logits", "vf")           # what is compared, each as one group


def kw(klc=0.2, ec=0.01, vclip=10.0, vfc=1.0):
    return dict(clip_param=CLIP, vf_clip_param=vclip, vf_loss_coeff=vfc, entropy_coeff=ec, kl_coeff=klc)


def n_valid_of(inp):
    return inp["za"].shape[0] if inp["mask"] is None else int(inp["mask"].sum())


def _rows(inp):
    R = inp["za"].shape[0]
    return torch.arange(R) if inp["mask"] is None else inp["mask"].nonzero()[:, 0]


def restate(inp, dtype, n_comp, k, n_valid=None):
    """the whole tail in `dtype`, on the rows the mask keeps only (so NaN in a masked row cannot enter) -> dict: stats (6 floats),
    the six gradients and logits [R, n_out], vf [R] as float64 tensors (zero in masked rows), and aux: per unmasked row the ratio, the
    squared value error, adv, vf, the four loss terms and d total / d logits"""
    R = inp["za"].shape[0]
    n_out = N_OUT[n_comp]
    idx = _rows(inp)
    n = float(n_valid_of(inp) if n_valid is None else n_valid)
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
    za, zc = leaf(inp["za"][idx]), leaf(inp["zc"][idx])
    w_act, b_act, w_val, b_val = (leaf(inp[key]) for key in WEIGHT_KEYS)
    logits = torch.tanh(za) @ w_act.T + b_act
    vf = torch.tanh(zc) @ w_val.reshape(-1) + b_val.reshape(())
    logits.retain_grad()
    old = inp["old_logits"][idx][:, :n_out].to(dtype)
    act = inp["actions"][idx].long().reshape(len(idx), -1)
    logp = ent = kl = torch.zeros(len(idx), dtype=dtype)
    lo = 0
    for c, wd in enumerate(WIDTHS[n_comp]):
        lp, lq = torch.log_softmax(logits[:, lo:lo + wd], dim=1), torch.log_softmax(old[:, lo:lo + wd], dim=1)
        logp = logp + lp.gather(1, act[:, c:c + 1]).squeeze(1)
        ent = ent - (lp.exp() * lp).sum(dim=1)
        kl = kl + (lq.exp() * (lq - lp)).sum(dim=1)
        lo += wd
    ratio = torch.exp(logp - inp["old_logp"][idx].to(dtype))
    A = inp["adv"][idx].to(dtype)
    surr = torch.minimum(A * ratio, A * ratio.clamp(1 - k["clip_param"], 1 + k["clip_param"]))
    sq = (vf - inp["target"][idx].to(dtype)) ** 2
    vl = sq.clamp(0, k["vf_clip_param"])
    want_kl = k["kl_coeff"] > 0.0
    total = (-surr + k["vf_loss_coeff"] * vl - k["entropy_coeff"] * ent).sum() / n
    if want_kl:
        total = total + k["kl_coeff"] * kl.sum() / n
    out = {}
    full = lambda t, shape: torch.zeros(shape, dtype=torch.float64).index_copy_(0, idx, t.detach().double())
    if len(idx):
        total.backward()
        out["d_za"], out["d_zc"] = full(za.grad, (R, K)), full(zc.grad, (R, K))
        for key, p in zip(GRADS[2:], (w_act, b_act, w_val, b_val)):
            out[key] = p.grad.double()
    else:
        out["d_za"], out["d_zc"] = torch.zeros((R, K), dtype=torch.float64), torch.zeros((R, K), dtype=torch.float64)
        for key, p in zip(GRADS[2:], (w_act, b_act, w_val, b_val)):
            out[key] = torch.zeros(p.shape, dtype=torch.float64)
    div = lambda t: float(t.detach().double().sum()) / n if n else float("nan")
    out["stats"] = [float(total.detach()) if n else float("nan"), div(-surr), div(vl), div(kl) if want_kl else 0.0, div(ent), n]
    out["logits"], out["vf"] = full(logits, (R, n_out)), full(vf, (R,))
    out["aux"] = {"ratio": ratio.detach().double(), "sq": sq.detach().double(), "adv": A.detach().double(), "vf": vf.detach().double(),
                  "terms": torch.stack([-surr, vl, kl, ent], dim=1).detach().double(),
                  "d_logits": (logits.grad if len(idx) else torch.zeros_like(logits)).detach().double()}
    return out


def errors(got, want):
    """{quantity: largest absolute difference} of `got` (tensors or lists, any float dtype) against the float64 `want`; the five
    statistics together"""
    err = {"stats": max(abs(float(a) - float(b)) for a, b in zip(list(got["stats"])[:5], want["stats"][:5]))}
    for key in QUANTITIES[1:]:
        if key in got and got[key] is not None:
            err[key] = (torch.as_tensor(got[key]).double().reshape(want[key].shape) - want[key]).abs().max().item()
    return err


def kink_distances(want, k):
    """per unmasked row of a float64 restatement: (distance of the ratio from 1 - clip and 1 + clip, distance of the squared value error
    from vf_clip_param, and |A ratio - A clamp(ratio)| where the ratio is outside the clip range, +inf inside, where the two are equal
    by construction and the gradient does not depend on which one min picks)"""
    a = want["aux"]
    lo, hi = 1 - k["clip_param"], 1 + k["clip_param"]
    d_ratio = torch.minimum((a["ratio"] - lo).abs(), (a["ratio"] - hi).abs())
    d_sq = (a["sq"] - k["vf_clip_param"]).abs()
    outside = (a["ratio"] < lo) | (a["ratio"] > hi)
    d_min = torch.where(outside, (a["adv"] * a["ratio"] - a["adv"] * a["ratio"].clamp(lo, hi)).abs(), torch.full_like(a["ratio"], float("inf")))
    return d_ratio, d_sq, d_min


def make_inputs(n_comp, R, masked, seed, nan=False, mask=None):
    """R rows for the instance: pre-activations of order 1, head weights of nn.Linear(500, .)'s scale, the sampler's logits 0.3 away from
    the learner's, old_logp 0.2 away from the learner's logp (ratios on both sides of the clip range), targets about 1.5 away from the
    value; then every row that the float64 restatement finds within 0.02 of a kink is moved: its old_logp to the learner's logp (ratio
    1), its target onto its value, its advantage to +-0.5.  masked: a ragged mask with row 0 kept (mask: that mask instead).  nan: NaN in
    every float column of the masked rows, za and zc among them, and out-of-range action bytes there."""
    g = torch.Generator().manual_seed(1000 * n_comp + 7919 * seed + R)
    n_out = N_OUT[n_comp]
    s = K ** -0.5
    inp = {"za": torch.randn((R, K), generator=g), "zc": torch.randn((R, K), generator=g),
           "w_act": (torch.rand((n_out, K), generator=g) * 2 - 1) * s, "b_act": (torch.rand((n_out,), generator=g) * 2 - 1) * s,
           "w_val": (torch.rand((1, K), generator=g) * 2 - 1) * 4 * s, "b_val": (torch.rand((1,), generator=g) * 2 - 1) * s}
    act = torch.stack([torch.randint(0, wd, (R,), generator=g) for wd in WIDTHS[n_comp]], dim=1).to(torch.int8)
    inp["actions"] = act[:, 0].contiguous() if n_comp == 1 else torch.cat([act, torch.zeros((R, 4 - act.shape[1]), dtype=torch.int8)], dim=1)
    if mask is None:
        mask = torch.rand((R,), generator=g) < 0.7 if masked else None
        if mask is not None:
            mask[0] = True
    inp["mask"] = mask
    z = torch.zeros(R)
    probe = dict(inp, old_logits=torch.zeros((R, OLD_LD[n_comp])), old_logp=z, adv=z, target=z, mask=None)
    w = restate(probe, torch.float64, n_comp, kw())
    old = torch.zeros((R, OLD_LD[n_comp]))
    old[:, :n_out] = (w["logits"] + 0.3 * torch.randn((R, n_out), generator=g).double()).float()
    inp["old_logits"] = old
    logp = torch.log(w["aux"]["ratio"])                      # the probe's old_logp is 0: its ratio is exp(logp)
    inp["old_logp"] = (logp + 0.2 * torch.randn((R,), generator=g).double()).float()
    inp["adv"] = torch.randn((R,), generator=g)
    inp["target"] = (w["vf"] + 1.5 * torch.randn((R,), generator=g).double()).float()
    k = kw()
    d_ratio, d_sq, d_min = kink_distances(restate(dict(inp, mask=None), torch.float64, n_comp, k), k)
    inp["old_logp"] = torch.where(d_ratio < 0.02, logp.float(), inp["old_logp"])
    inp["target"] = torch.where(d_sq < 0.02, w["vf"].float(), inp["target"])
    inp["adv"] = torch.where(d_min < 0.02, torch.where(inp["adv"] < 0, -0.5, 0.5), inp["adv"])
    if nan and mask is not None:
        off = ~mask
        for key in ROW_KEYS:
            if inp[key].dtype == torch.float32:
                inp[key] = inp[key].clone()
                inp[key][off] = float("nan")
        inp["actions"] = inp["actions"].clone()
        inp["actions"][off] = 77
    return inp


def geometry(n_rows, n_comp):
    """(tile_rows, n_workgroups) of a call, from the library (hh_heads_loss_geometry: host only, no GPU needed)"""
    from hhmarl_2d_amd import _lib as L
    tile, wgs = C.c_int32(), C.c_int32()
    L.check(L.lib().hh_heads_loss_geometry(n_rows, n_comp, C.byref(tile), C.byref(wgs)))
    return tile.value, wgs.value


def row_counts(n_comp):
    """the row counts of the grid: 1; either side of a tile; one tile more than one full round of the workgroups when the walk is
    grid-stride (the cap on the workgroups is what a call of very many rows reports); 280 = 14 chunks of 20; about 5000, ragged"""
    tile, _ = geometry(1, n_comp)
    cap = geometry(1 << 30, n_comp)[1]
    counts = [1, tile - 1, tile, tile + 1, 280, 5003]
    if cap < (1 << 30) // tile:                              # fewer workgroups than tiles at some size: the walk is grid-stride
        counts.append((cap + 1) * tile)
    return sorted(set(c for c in counts if c >= 1))


FEW_ROWS = 5


def representative(inp, want, e32, got32, k):
    """Whether a draw of the float32 restatement's error says something about the format.  A compared quantity that is a handful of
    numbers gives a single draw, which can land within a small fraction of an ulp of float64 by luck; 4 x that says nothing.  The floors,
    none of which looks at the kernel (U32 = 2^-24, half an ulp relative):
      * every quantity ends a chain — a 500-term dot product, an exp of a sum of logs — whose result float32 rounds once more at the
        least: e32 >= U32 / 2 x the quantity's largest float64 value, and e32 > 0;
      * with at most FEW_ROWS rows every quantity is a few draws, and tests/ppo_loss_edges_ref.py's reasoning applies: float32 holds
        logp - old_logp, two sums of about -8, to U32 x their size at best, and that absolute error is the relative error of the ratio,
        so of the surrogate (the statistics: U32 x max(1, |old_logp|) x the largest row's |surrogate| / n) and of everything d_logits
        feeds — d_za, d_w_act, d_b_act: e32 >= U32 x max(1, |old_logp|) x the largest value;
      * likewise vf - target is held to U32 x max(|vf|, |target|) at best, a relative error of U32 x max(|vf|, |target|) / |vf - target|
        in d_vf and so in d_zc, d_w_val and d_b_val (where the value gradient passes);
      * at any row count three quantities stay a handful of numbers, each the sum over the rows of per-row values: the statistics,
        d_b_val (one number) and d_b_act (3 numbers for the Categorical).  Their floor comes from the float32 restatement's own per-row
        errors (got32, the restatement that produced e32): taken as independent draws, the root of the sum of their squares is one
        standard deviation of the sum's error, and a seed whose e32 is below that is a lucky cancellation among the rows."""
    floor = {key: U32 / 2 * (max(abs(v) for v in want["stats"][:5]) if key == "stats" else want[key].abs().max().item()) for key in QUANTITIES}
    idx = _rows(inp)
    if 0 < len(idx) <= FEW_ROWS:
        amp = inp["old_logp"][idx].double().abs().clamp(min=1.0).max().item()
        for key in ("d_za", "d_w_act", "d_b_act"):
            floor[key] = 2 * amp * floor[key]
        floor["stats"] = max(floor["stats"], U32 * amp * want["aux"]["terms"][:, 0].abs().max().item() / max(want["stats"][5], 1.0))
        vf, tg = want["vf"][idx], inp["target"][idx].double()
        amp_v = (torch.maximum(vf.abs(), tg.abs()) / (vf - tg).abs().clamp(min=1e-30)).max().item()
        for key in ("d_zc", "d_w_val", "d_b_val"):
            floor[key] = 2 * max(amp_v, 0.5) * floor[key]
    n = max(want["stats"][5], 1.0)
    rss = lambda d: d.pow(2).sum(dim=0).sqrt()
    a32, a64 = got32["aux"], want["aux"]
    floor["stats"] = max(floor["stats"], (rss(a32["terms"] - a64["terms"]) / n).max().item())
    floor["d_b_act"] = max(floor["d_b_act"], rss(a32["d_logits"] - a64["d_logits"]).max().item())
    passing = (a64["sq"] <= k["vf_clip_param"]).double()
    floor["d_b_val"] = max(floor["d_b_val"], 2 * k["vf_loss_coeff"] / n * rss((a32["vf"] - a64["vf"]) * passing).item())
    return all(floor[key] == 0.0 or (e32[key] > 0.0 and e32[key] >= floor[key]) for key in QUANTITIES)


SEEDS = 256


def _representative_case(inp, n_comp, k):
    """(inputs, float64 restatement, e32) where the float32 restatement's error on these inputs is representative, else None"""
    want, got32 = restate(inp, torch.float64, n_comp, k), restate(inp, torch.float32, n_comp, k)
    e32 = errors(got32, want)
    return (inp, want, e32) if representative(inp, want, e32, got32, k) else None


@functools.lru_cache(maxsize=None)
def case(n_comp, R, masked, klc=0.2):
    """-> (inputs, float64 restatement, e32) at the first seed of 0..255 whose float32 error is representative (see there)"""
    k = kw(klc)
    for seed in range(SEEDS):
        inp = make_inputs(n_comp, R, masked, seed)
        found = _representative_case(inp, n_comp, k)
        if found:
            return found
    raise AssertionError(f"no representative seed for n_comp={n_comp} R={R} masked={masked}")


def grid():
    """(n_comp, R, masked): every row count unmasked, and the multi-tile ones with a ragged mask as well"""
    out = []
    for n_comp in INSTANCES:
        tile, _ = geometry(1, n_comp)
        for R in row_counts(n_comp):
            out.append((n_comp, R, False))
            if R > tile:
                out.append((n_comp, R, True))
    return out


@functools.lru_cache(maxsize=None)
def masked_tile_case(n_comp):
    """three tiles and a bit: the whole second tile masked, the rest ragged, at the first seed whose float32 error is representative
    -> (inputs, float64 restatement, e32, the same inputs with NaN in every float column of every masked row)"""
    tile, _ = geometry(1, n_comp)
    R = 3 * tile + 5
    g = torch.Generator().manual_seed(5)
    mask = torch.rand((R,), generator=g) < 0.7
    mask[0] = True
    mask[tile:2 * tile] = False
    for seed in range(SEEDS):
        found = _representative_case(make_inputs(n_comp, R, True, seed, mask=mask), n_comp, kw())
        if found:
            return found + (make_inputs(n_comp, R, True, seed, nan=True, mask=mask),)
    raise AssertionError(f"no representative seed for the masked tile of n_comp={n_comp}")


def stats_reorder_bound(want, k):
    """hh_heads_loss and hh_ppo_loss compute every row's four float64 terms from the same float32 values by the same device code, and
    differ only in the ORDER in which they add them (16-row tiles walked grid-stride against 256-row tiles).  Each computed sum of n terms
    t_i is within (n - 1) U64 sum|t_i| of the exact one (to first order), so two orders differ by at most 2 (n - 1) U64 sum|t_i|.  A mean
    is that sum over n, one more rounding; the total combines three or four sums with the coefficients, a few roundings more.
    -> per statistic 0..4 the bound on |difference|, with sum|t_i| taken from the float64 restatement and 1 % added for the float32
    terms' own distance from it."""
    t = want["aux"]["terms"].abs().sum(dim=0).tolist()       # sum|t| of -surrogate, vf_loss, kl, entropy
    n = max(len(want["aux"]["terms"]), 1)
    per = [1.01 * (2 * (n - 1) + 4) * U64 * s / n for s in t]
    kl_on = k["kl_coeff"] > 0.0
    total = per[0] + k["vf_loss_coeff"] * per[1] + k["entropy_coeff"] * per[3] + (k["kl_coeff"] * per[2] if kl_on else 0.0)
    total += 8 * U64 * (t[0] + k["vf_loss_coeff"] * t[1] + k["entropy_coeff"] * t[3] + (k["kl_coeff"] * t[2] if kl_on else 0.0)) / n
    return [total, per[0], per[1], per[2] if kl_on else 0.0, per[3]]
