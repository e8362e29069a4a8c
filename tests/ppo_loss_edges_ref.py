"""Case tables for the edge tests of hh_ppo_loss (n_comp 4 and 3) and hh_ppo_loss_categorical (n_comp 1 here): include/hh_learner.h,
csrc/hh_ppo_loss.h.  tests/test_ppo_loss_edges_host.py proves without a GPU what tests/test_gpu_ppo_loss_edges.py relies on; the
yardsticks are the existing restatements (tests/ppo_loss_ref.py for the MultiCategorical, tests/test_gpu_ppo_loss_categorical.py's for
the Categorical) in float64, and the same in float32 for e32, the cost of the format.

The tables are built so that no row has to be left out of a comparison: every row is either exactly ON a kink, where the header says what
the gradient is, or far from one (>= 0.01 in the ratio), so the float32 kernel and the float64 restatement are on the same side."""
import functools
import math

import torch

import ppo_loss_ref as REF
import test_gpu_ppo_loss_categorical as CAT

INSTANCES = (4, 3, 1)                                        # 1 = hh_ppo_loss_categorical
WIDTHS = {4: (13, 9, 2, 2), 3: (13, 9, 2), 1: (3,)}
N_OUT = {4: 26, 3: 24, 1: 3}
OLD_LD = {4: 32, 3: 32, 1: 4}
LDS = {4: tuple(range(26, 33)), 3: tuple(range(24, 33)), 1: (4,)}
CLIP = 0.25
ROW_KEYS = ("logits", "old_logits", "actions", "old_logp", "adv", "vf", "target")


def kw(klc=0.2, ec=0.01, vclip=10.0, vfc=1.0):
    return dict(clip_param=CLIP, vf_clip_param=vclip, vf_loss_coeff=vfc, entropy_coeff=ec, kl_coeff=klc)


def restate(inp, dtype, n_comp, k):
    """-> (stats [6], d_logits [R, ld], d_vf [R], ratio [R], squared value error [R]) of the restatement in `dtype`"""
    if n_comp == 1:
        return CAT.restatement(inp, dtype, **k)
    s, dl, dv, aux = REF.reference(inp, dtype, n_comp=n_comp, **k)
    return s, dl, dv, aux["ratio"], aux["vf_sq"]


def errors(got, want, rows=None):
    """largest absolute differences (statistics, d_logits, d_vf) of `got` = (stats, d_logits, d_vf, ...) against the float64 `want`,
    the gradients over `rows` (all rows when None)"""
    e_s = max(abs(float(a) - float(b)) for a, b in zip(got[0][:5], want[0][:5]))
    dl, dv = (got[1].double() - want[1]).abs(), (got[2].double() - want[2]).abs()
    if rows is not None:
        dl, dv = dl[rows], dv[rows]
    return e_s, (dl.max().item() if dl.numel() else 0.0), (dv.max().item() if dv.numel() else 0.0)


def near_kink(ratio, sq, vclip):
    return REF.near_kink({"ratio": ratio, "vf_sq": sq}, CLIP, vclip)


def base_inputs(n_comp, R, ld, masked, seed):
    """the existing generators' inputs"""
    if n_comp == 1:
        return CAT.make_inputs(R, masked, seed * 131 + R % 97)
    return REF.make_inputs(R, n_comp, ld, masked, seed)


def n_valid_of(inp):
    return inp["logits"].shape[0] if inp["mask"] is None else int(inp["mask"].sum())


# ---- the ragged grid: (R, ld, masked, kl_coeff, entropy_coeff)
TILE_R, SMALL_R, BIG_R = (255, 256, 257, 511, 512, 513), (1, 2, 3, 5, 257, 259), (65536, 65537)


def grid_cases(n_comp):
    lds = LDS[n_comp]
    cases = []
    for R in TILE_R:
        for ld in sorted({lds[0], lds[-1]}):
            cases += [(R, ld, False, 0.2, 0.01), (R, ld, True, 0.2, 0.01)]
        cases.append((R, lds[0], False, 0.0, 0.01))
    for R in SMALL_R:
        for ld in lds:
            c = (R, ld, R > 5 and ld % 2 == 0, 0.2, 0.01)
            if c not in cases:
                cases.append(c)
    cases += [(R, lds[0], True, 0.2, 0.01) for R in BIG_R]
    return cases


def e32_must_be_positive(inp):
    """(stats, d_logits, d_vf): where n_valid is a power of two the value gradient vf_coeff / n * 2 * (vf - target) is exact in float32
    whenever the subtraction is, e32 is then 0.0, and 4 x e32 asks the kernel for the exact value too"""
    n = n_valid_of(inp)
    return True, True, n & (n - 1) != 0


def e32_is_representative(inp, want, e32):
    """With thousands of rows the largest float32 error of a case is a stable figure.  With one to five rows it is a single draw: the
    float32 restatement can land within a small fraction of an ulp of float64 by luck, and 4 x that says nothing about the format.  A
    case of so few rows therefore has to show at least the error that float32 cannot avoid (u = 2^-24, half an ulp relative), in each
    quantity that e32_must_be_positive names:
      * the statistics: u x the largest float64 value;
      * d_vf, a single subtraction and scalings, one rounding whose error is u x the value at most: half of that;
      * what carries the ratio: float32 holds logp - old_logp, two sums of about -8, to u x their size at best, and that absolute error
        is the relative error of exp(.), so of the row's surrogate and of its whole d_logits row: u x max(1, |old_logp|) x the row's
        largest gradient element, and x the row's surrogate / n for the statistics.
    Nothing here looks at the kernel."""
    u = 2.0 ** -24
    n = max(n_valid_of(inp), 1)
    on = torch.ones(len(want[3]), dtype=torch.bool) if inp["mask"] is None else inp["mask"]
    amp = inp["old_logp"].double().abs().clamp(min=1.0)
    A, ratio = inp["adv"].double(), want[3]
    surr = torch.minimum(A * ratio, A * ratio.clamp(1 - CLIP, 1 + CLIP)).abs()
    floor = (u * max(max(abs(v) for v in want[0][:5]), (amp * surr)[on].max().item() / n),
             u * (amp[:, None] * want[1].abs()).max().item(),
             u / 2 * want[2].abs().max().item())
    return all(e > 0.0 and e >= f for e, f, must in zip(e32, floor, e32_must_be_positive(inp)) if must)


FEW_ROWS, SEEDS = 5, 256


def first_representative(make, n_comp, k):
    """the first seed of 0..255 whose inputs make(seed) pass e32_is_representative -> (seed, inputs, float64 restatement, e32)"""
    for seed in range(SEEDS):
        inp = make(seed)
        want = restate(inp, torch.float64, n_comp, k)
        e32 = errors(restate(inp, torch.float32, n_comp, k), want)
        if e32_is_representative(inp, want, e32):
            break
    return seed, inp, want, e32


@functools.lru_cache(maxsize=None)
def grid_case(n_comp, case):
    """-> (inputs, float64 restatement, e32 (stats, d_logits, d_vf)): make_inputs at seed 0, and at R <= 5 at the first seed whose e32
    is representative (see there); the host test asserts e32 > 0 on every case and the representative e32 on the small ones."""
    R, ld, masked, klc, ec = case
    if R <= FEW_ROWS:
        return first_representative(lambda seed: base_inputs(n_comp, R, ld, masked, seed), n_comp, kw(klc, ec))[1:]
    inp = base_inputs(n_comp, R, ld, masked, 0)
    want = restate(inp, torch.float64, n_comp, kw(klc, ec))
    return inp, want, errors(restate(inp, torch.float32, n_comp, kw(klc, ec)), want)


# ---- the kink table
KINK_R, KINK_VCLIP, KINK_VFC = 512, 4.0, 0.5               # n = 512 and vf_loss_coeff = 0.5: vf_coeff / n * 2 * dv is exact in float32
LOG_RATIOS = (-20.0, math.log(0.70), math.log(0.74), math.log(0.76), 0.0, math.log(1.24), math.log(1.26), math.log(1.30), 20.0, 80.0)
ADVS = (1.5, -1.5, 0.0, 1e-30)
RATIO_ADV = tuple((lr, a) for lr in LOG_RATIOS for a in ADVS if not (lr >= 20.0 and a < 0.0))    # e^20 and e^80 with adv >= 0: finite loss
DVS = (0.0, 2.0, -2.0, 2.0 - 2.0 ** -23, -(2.0 - 2.0 ** -23), 2.0 + 2.0 ** -22, -(2.0 + 2.0 ** -22), 3.0, -3.0)
KINK_DVS = tuple(d for d in DVS if abs(d) not in (0.0, 3.0))     # within near_kink's band of vf_clip_param: on the kink or one ulp off it


def kink_kw(klc, ec):
    return kw(klc, ec, vclip=KINK_VCLIP, vfc=KINK_VFC)


def _logp64(logits, actions, n_comp):
    lo, out = 0, torch.zeros(logits.shape[0], dtype=torch.float64)
    a = actions.long().reshape(logits.shape[0], -1)
    for i, w in enumerate(WIDTHS[n_comp]):
        out += torch.log_softmax(logits[:, lo:lo + w].double(), dim=1).gather(1, a[:, i:i + 1])[:, 0]
        lo += w
    return out


@functools.lru_cache(maxsize=None)
def kink_table(n_comp):
    """-> (inputs, meta).  logits == old_logits bit for bit; row i takes RATIO_ADV[i % 38] and DVS[i % 9] (38 and 9 are coprime: all 342
    pairs occur in 512 rows); the row width is odd (n_out + 1) for the MultiCategorical, with junk in the last column."""
    R, n_out = KINK_R, N_OUT[n_comp]
    ld = 4 if n_comp == 1 else n_out + 1
    g = torch.Generator().manual_seed(7000 + n_comp)
    old = torch.zeros((R, OLD_LD[n_comp]))
    old[:, :n_out] = torch.randn((R, n_out), generator=g) * 1.5
    logits = torch.randn((R, ld), generator=g)
    logits[:, :n_out] = old[:, :n_out]
    actions = torch.zeros((R, 4), dtype=torch.int8)
    for i, w in enumerate(WIDTHS[n_comp]):
        actions[:, i] = torch.randint(0, w, (R,), generator=g).to(torch.int8)
    if n_comp == 1:
        actions = actions[:, 0].contiguous()
    log_r = torch.tensor([RATIO_ADV[i % len(RATIO_ADV)][0] for i in range(R)], dtype=torch.float64)
    adv = torch.tensor([RATIO_ADV[i % len(RATIO_ADV)][1] for i in range(R)], dtype=torch.float64)
    dv = torch.tensor([DVS[i % len(DVS)] for i in range(R)], dtype=torch.float64)
    # exactly representable vf and target with an exact difference: a non-zero target only where vf = target + dv stays exact
    target = torch.tensor([float(i % 3 - 1) if abs(DVS[i % len(DVS)]) in (0.0, 2.0, 3.0) else 0.0 for i in range(R)], dtype=torch.float64)
    old_logp = (_logp64(logits[:, :n_out], actions, n_comp) - log_r).float()
    inp = dict(logits=logits, vf=(target + dv).float(), old_logits=old, actions=actions, old_logp=old_logp, adv=adv.float(),
               target=target.float(), mask=None)
    return inp, dict(log_r=log_r, adv=adv, dv=dv)


@functools.lru_cache(maxsize=None)
def kink_expect(n_comp):
    """per row, from the float64 autograd result at entropy_coeff = kl_coeff = 0 (not from the kernel's rule): does the policy gradient
    pass (any non-zero d_logits), does the value gradient pass (non-zero d_vf; dv = 0 has a zero gradient on either side)"""
    inp, _ = kink_table(n_comp)
    _, dl, dv, _, _ = restate(inp, torch.float64, n_comp, kink_kw(0.0, 0.0))
    return (dl != 0).any(dim=1), dv != 0


def ratio_side(ratio):
    return (ratio > 1 + CLIP).long() - (ratio < 1 - CLIP).long()          # -1 below, 0 inside (closed), +1 above


def value_side(sq, vclip):
    return (sq > vclip).long() - (sq < vclip).long()                      # -1 inside, 0 on the kink, +1 beyond


# ---- the wide-logit table
GAPS = (30, 80, 200)
WIDE_REPEATS = 8


@functools.lru_cache(maxsize=None)
def wide_table(n_comp, offsets):
    """-> (inputs, float64 tensors the float32 inputs were rounded from).  Every logit is a multiple of 1/8.  Per component one top logit
    and the others `gap + k/8` (k < 16) below it; the component's mode is 0: the chosen action is the top logit; 1: it is one of the
    others, whose probability underflows in float32 at the gaps 200 (to 0) and 80 (e^-80 is below the sum's rounding); 2: the learner's
    top logit has moved away from the sampler's, which the action sits on (ratio e^-gap, KL of about gap).  Row by row one featured
    component runs through (gap, mode), the others take mode 0 or 1.  With `offsets` each component of logits and of old_logits is
    shifted by +8192 or -8192, independently.  old_logp is the sampler's own log-probability, so log(ratio) is a multiple of 1/8 up to
    e^-30: at least 0.028 from either clip boundary."""
    g = torch.Generator().manual_seed(9100 + n_comp)
    widths, n_out = WIDTHS[n_comp], N_OUT[n_comp]
    ld = 4 if n_comp == 1 else n_out + 3
    rows = [(gap, mode, c) for _ in range(WIDE_REPEATS) for gap in GAPS for mode in (0, 1, 2) for c in range(len(widths))]
    R = len(rows)
    ri = lambda hi, shape=(): torch.randint(0, hi, shape, generator=g)
    new64, old64 = torch.zeros((R, ld), dtype=torch.float64), torch.zeros((R, OLD_LD[n_comp]), dtype=torch.float64)
    actions = torch.zeros((R, 4), dtype=torch.int8)
    for r, (gap, mode_f, cf) in enumerate(rows):
        lo = 0
        for c, w in enumerate(widths):
            mode = mode_f if c == cf else int(ri(2))
            top = int(ri(w))
            top_old = (top + 1 + int(ri(w - 1))) % w if mode == 2 else top
            x = -(gap + ri(16, (w,)).double() / 8)
            y = -(gap + ri(16, (w,)).double() / 8)
            x[top], y[top_old] = 0.0, 0.0
            a = top if mode == 0 else (top_old if mode == 2 else (top + 1 + int(ri(w - 1))) % w)
            sx, sy = (ri(65, (2,)).double() - 32) / 8
            if offsets:
                sx, sy = sx + 8192.0 * (2 * int(ri(2)) - 1), sy + 8192.0 * (2 * int(ri(2)) - 1)
            new64[r, lo:lo + w], old64[r, lo:lo + w] = x + sx, y + sy
            actions[r, c] = a
            lo += w
    if n_comp == 1:
        actions = actions[:, 0].contiguous()
    dv64 = (ri(41, (R,)).double() - 20) / 4                       # multiples of 1/4 in [-5, 5]: dv^2 is never within 0.2 of vf_clip_param = 10
    target64 = (ri(65, (R,)).double() - 32) / 8
    adv64 = (ri(33, (R,)).double() - 16) / 8
    old_logp = _logp64(old64[:, :n_out], actions, n_comp).float()
    raw = dict(logits=new64, old_logits=old64, vf=target64 + dv64, target=target64, adv=adv64)
    inp = {k: v.float() for k, v in raw.items()}
    inp.update(actions=actions, old_logp=old_logp, mask=None)
    return inp, raw


# ---- the action table
BAD_BYTE4 = (-128, -1, 1, 127)


@functools.lru_cache(maxsize=None)
def action_table(n_comp):
    """-> (inputs of 2 K rows, K): row i < K holds one out-of-range byte (-128, -1, W, 127 in one component), row K + i is the same row
    with the byte clamped into 0..W-1; for n_comp = 3, four more pairs differ only in the fourth byte (-128, -1, 1, 127 against 0).
    old_logp is the sampler's log-probability of the clamped action in both."""
    widths = WIDTHS[n_comp]
    bad = [(c, b) for c, w in enumerate(widths) for b in (-128, -1, w, 127)] + ([(3, b) for b in BAD_BYTE4] if n_comp == 3 else [])
    K = len(bad)
    ld = 4 if n_comp == 1 else N_OUT[n_comp] + 2
    base = base_inputs(n_comp, K, ld, False, 11)
    inp = {k: (None if v is None else torch.cat([v, v])) for k, v in base.items()}
    a = inp["actions"].reshape(2 * K, -1).clone()
    for i, (c, b) in enumerate(bad):
        a[i, c] = b
        a[K + i, c] = 0 if c >= len(widths) else min(max(b, 0), widths[c] - 1)
    inp["actions"] = a[:, 0].contiguous() if n_comp == 1 else a
    # the sampler's log-probability of the clamped action, as if it had drawn that one: the ratios stay those of the generator
    lp = _logp64(inp["old_logits"][:, :N_OUT[n_comp]], a[K:, :len(widths)].repeat(2, 1), n_comp).float()
    inp["old_logp"] = lp
    return inp, K


# ---- mask patterns over 769 rows (three tiles and one row)
MASK_R = 769
MASK_PATTERNS = ("tile1_off", "only_row0", "only_row768", "all_off")


def mask_pattern(name):
    m = torch.zeros(MASK_R, dtype=torch.bool)
    if name == "tile1_off":
        m[:256], m[512:] = True, True
    elif name == "only_row0":
        m[0] = True
    elif name == "only_row768":
        m[768] = True
    return m


def _mask_inputs(n_comp, name, nan, seed):
    inp = dict(base_inputs(n_comp, MASK_R, LDS[n_comp][0], False, seed))
    m = mask_pattern(name)
    inp["mask"] = m
    for k in ("logits", "old_logits", "old_logp", "adv", "vf", "target"):
        v = inp[k].clone()
        v[~m] = float("nan") if nan else 0.0
        inp[k] = v
    return inp


@functools.lru_cache(maxsize=None)
def mask_seed(n_comp, name):
    """3, and for the patterns with a single valid row the first seed whose e32 is representative (see e32_is_representative)"""
    if int(mask_pattern(name).sum()) != 1:
        return 3
    return first_representative(lambda seed: _mask_inputs(n_comp, name, False, seed), n_comp, kw())[0]


def mask_case(n_comp, name, nan):
    return _mask_inputs(n_comp, name, nan, mask_seed(n_comp, name))


def ignored_columns_case(n_comp, nan):
    """an unmasked case at the widest rows with NaN (or 0.0) in every column at or beyond n_out of logits and old_logits"""
    n_out = N_OUT[n_comp]
    inp = dict(base_inputs(n_comp, 257, LDS[n_comp][-1], False, 5))
    for k in ("logits", "old_logits"):
        v = inp[k].clone()
        v[:, n_out:] = float("nan") if nan else 0.0
        inp[k] = v
    return inp


def replace_row(inp, row, donor, donor_row):
    """`inp` with row `row` of every per-row input replaced by row `donor_row` of `donor` (the mask is kept)"""
    out = dict(inp)
    for k in ROW_KEYS:
        v = inp[k].clone()
        v[row] = donor[k][donor_row]
        out[k] = v
    return out


def permuted(inp, perm):
    return {k: (None if v is None else v[perm].contiguous()) for k, v in inp.items()}
