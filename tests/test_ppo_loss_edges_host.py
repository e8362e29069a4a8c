"""What tests/test_gpu_ppo_loss_edges.py rests on, proved without a GPU on the tables of tests/ppo_loss_edges_ref.py: no row of the
kink, wide-logit and action tables needs to be left out of a comparison, the float32 and float64 restatements agree on the side of every
kink, the tables reach what they claim to reach, the wide table's inputs are exact in float32, the float32 restatement's error e32 is
positive wherever 4 x e32 is the bound, and the float64 restatement alone is finite where the GPU test expects finite outputs."""
import math

import pytest
import torch

import ppo_loss_edges_ref as E

NC = pytest.mark.parametrize("n_comp", E.INSTANCES)


def _finite(res):
    return all(math.isfinite(v) for v in res[0]) and bool(torch.isfinite(res[1]).all()) and bool(torch.isfinite(res[2]).all())


@NC
def test_kink_table_rows_are_on_the_value_kink_or_far_from_every_kink(n_comp):
    inp, meta = E.kink_table(n_comp)
    n_out = E.N_OUT[n_comp]
    assert torch.equal(inp["logits"][:, :n_out].view(torch.int32), inp["old_logits"][:, :n_out].view(torch.int32))
    # vf, target and their difference are exact
    assert torch.equal(inp["vf"].double() - inp["target"].double(), meta["dv"])
    assert torch.equal((inp["vf"] - inp["target"]).double(), meta["dv"])
    k = E.kink_kw(0.2, 0.01)
    r64 = E.restate(inp, torch.float64, n_comp, k)
    r32 = E.restate(inp, torch.float32, n_comp, k)
    # near_kink flags the rows placed on the value kink or one ulp off it, and nothing else: no ratio is within 1e-4 of a boundary
    placed = torch.tensor([abs(d) in [abs(x) for x in E.KINK_DVS] for d in meta["dv"].tolist()])
    assert torch.equal(E.near_kink(r64[3], r64[4], E.KINK_VCLIP), placed)
    for lo_hi in (1 - E.CLIP, 1 + E.CLIP):
        assert (r64[3] - lo_hi).abs().min().item() >= 0.01 - 1e-6 and (r32[3].double() - lo_hi).abs().min().item() >= 0.01 - 1e-4
    # float32 and float64 on the same side of each kink, and that side is the one the table aims at
    assert torch.equal(E.ratio_side(r64[3]), E.ratio_side(r32[3]))
    assert torch.equal(E.value_side(r64[4], E.KINK_VCLIP), E.value_side(r32[4], E.KINK_VCLIP))
    want_r = torch.tensor([(lr > math.log(1.25)) - (lr < math.log(0.75)) for lr in meta["log_r"].tolist()])
    assert torch.equal(E.ratio_side(r64[3]), want_r)
    want_v = torch.tensor([(abs(d) > 2.0) - (abs(d) < 2.0) for d in meta["dv"].tolist()])
    assert torch.equal(E.value_side(r64[4], E.KINK_VCLIP), want_v)
    assert set(want_v.tolist()) == {-1, 0, 1}
    # every (ratio side, sign of the advantage) occurs, and so does every value error
    seen = {(int(s), (a > 0) - (a < 0)) for s, a in zip(want_r.tolist(), meta["adv"].tolist())}
    assert seen == {(s, a) for s in (-1, 0, 1) for a in (-1, 0, 1)}
    assert set(meta["dv"].tolist()) == set(E.DVS) and len(set(zip(meta["log_r"].tolist(), meta["adv"].tolist()))) == len(E.RATIO_ADV) == 38
    assert _finite(r64) and _finite(E.restate(inp, torch.float64, n_comp, E.kink_kw(0.0, 0.0)))
    e32 = E.errors(r32, r64)
    assert e32[0] > 0.0 and e32[1] > 0.0              # d_vf is held to its exact value instead


@NC
def test_kink_table_expectations_come_out_of_autograd_as_the_header_says(n_comp):
    inp, meta = E.kink_table(n_comp)
    pol, val = E.kink_expect(n_comp)
    adv, lr, dv = meta["adv"], meta["log_r"], meta["dv"]
    below, above = lr < math.log(0.75), lr > math.log(1.25)
    assert torch.equal(pol, (adv != 0) & ~((adv > 0) & above) & ~((adv < 0) & below))
    assert torch.equal(val, (dv.abs() <= 2.0) & (dv != 0))
    assert pol.any() and (~pol).any() and val.any() and (~val).any()
    # the exact value gradient: every factor is a power of two or exact in float32
    n = E.KINK_R
    exact = E.KINK_VFC / n * 2 * dv
    assert torch.equal(exact.float().double(), exact) and n & (n - 1) == 0
    _, _, dv64, _, _ = E.restate(inp, torch.float64, n_comp, E.kink_kw(0.0, 0.0))
    assert torch.equal(dv64[val], exact[val])


@NC
@pytest.mark.parametrize("offsets", (False, True))
def test_wide_table_is_exact_in_float32_and_far_from_every_kink(n_comp, offsets):
    inp, raw = E.wide_table(n_comp, offsets)
    for k, v in raw.items():
        assert torch.equal(inp[k].double(), v), k
        assert torch.equal(v * 8, (v * 8).round()), k
    n_out = E.N_OUT[n_comp]
    assert torch.isfinite(inp["logits"]).all() and torch.isfinite(inp["old_logits"]).all() and torch.isfinite(inp["old_logp"]).all()
    # the gaps, the underflow and the offsets are there
    lo = 0
    gaps = set()
    for w in E.WIDTHS[n_comp]:
        x = inp["logits"][:, lo:lo + w]
        gaps |= set(((x.max(dim=1)[0][:, None] - x).clamp(max=200).max(dim=1)[0]).tolist())
        lo += w
    assert 200.0 in gaps
    p_chosen = torch.exp((E._logp64(inp["logits"][:, :n_out], inp["actions"], n_comp)).float())
    assert (p_chosen == 0).any() and (p_chosen == 1).any()
    big = inp["logits"][:, :n_out].abs().max().item()
    assert (big > 8000) == offsets and (inp["old_logits"][:, :n_out].abs().max().item() > 8000) == offsets
    if offsets:
        assert (inp["logits"][:, 0] * inp["old_logits"][:, 0] < 0).any() and (inp["logits"][:, 0] * inp["old_logits"][:, 0] > 0).any()
    k = E.kw()
    r64 = E.restate(inp, torch.float64, n_comp, k)
    r32 = E.restate(inp, torch.float32, n_comp, k)
    assert not E.near_kink(r64[3], r64[4], 10.0).any()
    for lo_hi in (1 - E.CLIP, 1 + E.CLIP):
        assert (r64[3] - lo_hi).abs().min().item() >= 0.02 and (r32[3].double() - lo_hi).abs().min().item() >= 0.02
    assert torch.equal(E.ratio_side(r64[3]), E.ratio_side(r32[3])) and torch.equal(E.value_side(r64[4], 10.0), E.value_side(r32[4], 10.0))
    assert set(E.ratio_side(r64[3]).tolist()) == {-1, 0, 1} and set(E.value_side(r64[4], 10.0).tolist()) == {-1, 1}
    assert _finite(r64) and r64[0][3] > 1.0           # the moved top logits give a KL of the order of the gap
    assert min(E.errors(r32, r64)) > 0.0


@NC
def test_action_table_holds_every_clamp_value_and_no_kink(n_comp):
    inp, K = E.action_table(n_comp)
    a = inp["actions"].reshape(2 * K, -1).long()
    widths = E.WIDTHS[n_comp]
    for c, w in enumerate(widths):
        assert {-128, -1, w, 127} <= set(a[:K, c].tolist())
        assert int(a[K:, c].min()) >= 0 and int(a[K:, c].max()) <= w - 1 and {0, w - 1} <= set(a[K:, c].tolist())
    if n_comp == 3:
        assert set(a[:K, 3].tolist()) == set(E.BAD_BYTE4) | {0} and set(a[K:, 3].tolist()) == {0}
    assert ((a[:K] != a[K:]).sum(dim=1) == 1).all()
    for key in E.ROW_KEYS:
        if key != "actions":
            assert torch.equal(inp[key][:K], inp[key][K:])
    twin = dict(inp, actions=torch.cat([inp["actions"][K:], inp["actions"][K:]]))
    k = E.kw()
    r64 = E.restate(twin, torch.float64, n_comp, k)
    assert not E.near_kink(r64[3], r64[4], 10.0).any() and _finite(r64)
    assert min(E.errors(E.restate(twin, torch.float32, n_comp, k), r64)) > 0.0


@NC
def test_grid_covers_the_issue_and_e32_is_positive(n_comp):
    cases = E.grid_cases(n_comp)
    assert len(set(cases)) == len(cases)
    lds = E.LDS[n_comp]
    for R in E.TILE_R:
        assert {ld for (r, ld, *_rest) in cases if r == R} >= {lds[0], lds[-1]}
        assert any(r == R and klc == 0.0 for (r, _, _, klc, _) in cases)
    for R in E.SMALL_R:
        assert {ld for (r, ld, *_rest) in cases if r == R} == set(lds)
    assert all((R, lds[0], True, 0.2, 0.01) in cases for R in E.BIG_R)
    assert all(ec != 0.0 for (*_rest, ec) in cases)
    for case in cases:
        if case[0] in E.BIG_R:
            continue                                  # the same assertion runs in the GPU test, where the reference is computed anyway
        inp, want, e32 = E.grid_case(n_comp, case)
        assert inp["logits"].shape == (case[0], case[1]) and (inp["mask"] is not None) == case[2]
        assert all(e > 0.0 for e, must in zip(e32, E.e32_must_be_positive(inp)) if must), (case, e32)
        assert case[0] > E.FEW_ROWS or E.e32_is_representative(inp, want, e32), (case, e32)
        assert _finite(want)


@NC
@pytest.mark.parametrize("name", E.MASK_PATTERNS)
def test_mask_patterns(n_comp, name):
    m = E.mask_pattern(name)
    assert int(m.sum()) == {"tile1_off": 513, "only_row0": 1, "only_row768": 1, "all_off": 0}[name]
    zero, nan = E.mask_case(n_comp, name, False), E.mask_case(n_comp, name, True)
    for k in ("logits", "old_logits", "old_logp", "adv", "vf", "target"):
        assert torch.isnan(nan[k][~m]).all() and torch.isfinite(nan[k][m]).all() and (zero[k][~m] == 0).all()
        assert torch.equal(nan[k][m], zero[k][m])
    if name != "all_off":
        r64 = E.restate(zero, torch.float64, n_comp, E.kw())
        assert _finite(r64) and r64[0][5] == int(m.sum())
        e32 = E.errors(E.restate(zero, torch.float32, n_comp, E.kw()), r64)
        assert all(e > 0.0 for e, must in zip(e32, E.e32_must_be_positive(zero)) if must), e32
        assert int(m.sum()) != 1 or E.e32_is_representative(zero, r64, e32), e32


@NC
def test_ignored_columns_case(n_comp):
    n_out = E.N_OUT[n_comp]
    nan, zero = E.ignored_columns_case(n_comp, True), E.ignored_columns_case(n_comp, False)
    for k in ("logits", "old_logits"):
        assert nan[k].shape[1] > n_out and torch.isnan(nan[k][:, n_out:]).all() and torch.equal(nan[k][:, :n_out], zero[k][:, :n_out])
