"""CPU half of the sampler edge tests: the reference of tests/sampler_ref.py ALONE meets the conditions under which
tests/test_gpu_sampler_edges.py may compare the kernels' drawn actions exactly, on every row.

The half-width condition.  The kernels' documented logit bound is 1e-5 (include/hh_policy.h; TOL of tests/test_policy_value.py).  A logit error of
1e-5 moves a softmax CDF by at most 2e-5 (|d softmax| <= 2 |d logit| in the worst case of all the mass moving one way), and the kernels' (float) u
rounding adds 6e-8.  A uniform that sits 1e-3 = 50 x that away from both ends of its CDF interval therefore selects the same index on the device as in
the float64 restatement: no row needs to be excluded.  With the synthetic weights of seeds 5 and 9 on uniform(-1, 1) rows the smallest action
probability is about 0.0136 (half-width 6.8e-3)."""
import numpy as np
import pytest

from hhmarl_2d_amd import policy_nets as PN
import policy_ref as PR
import sampler_ref as SR

MIDPOINT = [c for c in SR.CASES if c["uniforms"] == "midpoint"]


def check_tile_edge_coverage(cases):
    """every kind meets every list length around the 16-row wave, the 32-row tile and the 64-row tile"""
    have = SR.list_lengths(cases)
    for kind in SR.KINDS:
        missing = sorted(set(SR.EDGE_LENGTHS) - have[kind])
        assert not missing, f"{PN.KIND_NAMES[kind]}: no case with a list of {missing} rows"


def check_action_coverage(case):
    """every action index of every component is some row's target.  A list of n rows has n targets per component, so a list shorter than a
    component is wide (the 1-row lists; 13 is the widest component) carries n distinct ones instead: the cycle of sampler_ref.cycle_targets
    repeats nothing before it has been through every index"""
    inp = SR.build(case)
    flat = inp["kinds"].reshape(-1)
    for kind in SR.KINDS:
        idx = np.flatnonzero(flat == kind)
        for k in range(SR.n_comp(kind) if len(idx) else 0):
            w = PN.ACTION_SPLIT[k]
            seen = set(inp["targets"][idx, k].tolist())
            assert seen <= set(range(w)) and len(seen) == min(len(idx), w), (case["name"], PN.KIND_NAMES[kind], k)


@pytest.mark.parametrize("case", MIDPOINT, ids=lambda c: c["name"])
def test_midpoint_uniforms_are_far_from_every_cdf_boundary(case):
    inp = SR.build(case)
    assert inp["half_width"] >= SR.MIN_HALF_WIDTH, inp["half_width"]
    flat = inp["kinds"].reshape(-1)
    live = flat >= 0
    # the float64 draw of those uniforms IS the target, with the same distance to spare
    for kind in SR.KINDS:
        idx = np.flatnonzero(flat == kind)
        nc = SR.n_comp(kind)
        assert np.array_equal(inp["ref"]["actions"][idx, :nc], inp["targets"][idx, :nc])
        assert (inp["ref"]["actions"][idx, nc:] == 0).all()
    assert inp["ref"]["margin"][live].min() >= SR.MIN_HALF_WIDTH
    assert np.isfinite(inp["ref"]["logp"][live]).all() and np.isnan(inp["ref"]["logp"][~live]).all()


@pytest.mark.parametrize("case", MIDPOINT, ids=lambda c: c["name"])
def test_targets_cover_every_action_index(case):
    check_action_coverage(case)


def test_tile_edge_coverage():
    check_tile_edge_coverage(SR.CASES)
    # the check notices a missing length and a missing kind
    with pytest.raises(AssertionError, match="Esc"):
        check_tile_edge_coverage([c for c in SR.CASES if c["name"] != "ragged-escape-17"])
    with pytest.raises(AssertionError, match="Fight"):
        check_tile_edge_coverage([c for c in SR.CASES if c["mode"] != "fight"])


def test_rows_without_a_network_come_in_every_pairing():
    for case in SR.CASES:
        if case["sel"] == "uniform":
            continue
        inp = SR.build(case)
        listed = inp["kinds"] >= 0
        both, one, none = listed.all(axis=1), listed.sum(axis=1) == 1, ~listed.any(axis=1)
        assert both.any() and none.any() and (listed[one][:, 0]).any() and (listed[one][:, 1]).any(), case["name"]
        # a pair nobody flies holds NaN everywhere; an unlisted row beside a listed one keeps the data its partner's critic reads
        assert np.isnan(inp["obs30"][none]).all() and np.isnan(inp["crit_act"][none]).all()
        assert np.isfinite(inp["obs30"][~none]).all() and np.isfinite(inp["crit_act"][~none]).all()
        assert np.isfinite(inp["ref"]["vf"][listed.reshape(-1)]).all()
        assert (inp["sel"][~listed] == 0).all() and (inp["sel"][listed] != 0).all()
    four = SR.build("four-nets-333")["kinds"]
    assert {tuple(p) for p in four.tolist()} == {(a, b) for a in (PN.FIGHT1, PN.ESC1, -1) for b in (PN.FIGHT2, PN.ESC2, -1)}


def test_draw_edge_references():
    """u = 0 draws the first index, u = 1 - 2^-53 the last one of every component the kind has"""
    for case in SR.CASES:
        if case["group"] != "draw-edges":
            continue
        inp = SR.build(case)
        for slot, kind in enumerate(SR.MODE_KINDS[case["mode"]]):
            a = inp["ref"]["actions"].reshape(-1, 2, 4)[:, slot]
            last = np.array([12, 8, 1, 1 if PN.N_OUT[kind] == 26 else 0])
            assert (a == (0 if case["uniforms"] == "zero" else last)).all()


def test_sample_ref_is_the_per_kind_restatement():
    """sample_ref on a mixed call = policy_ref's functions on each kind's rows, the other agent taken from row r ^ 1 whatever it flies"""
    inp = SR.build("four-nets-333")
    W = SR.weights(9)
    import torch
    o, ca = torch.from_numpy(inp["obs30"].reshape(-1, 30).copy()), torch.from_numpy(inp["crit_act"].reshape(-1, 4).copy())
    flat = inp["kinds"].reshape(-1)
    r = int(np.flatnonzero((flat == PN.ESC1) & (np.roll(flat, -1) == PN.FIGHT2))[0])     # an Esc1 agent beside a Fight2 agent: even row, r ^ 1 = r + 1
    assert r % 2 == 0
    v = PR.torch_value(PN.ESC1, *W[PN.ESC1], o[r:r + 1], ca[r:r + 1], o[r + 1:r + 2], ca[r + 1:r + 2])
    assert abs(float(v) - float(inp["ref"]["vf"][r])) <= 1e-6
    lg = PR.torch_forward(PN.FIGHT2, W[PN.FIGHT2][0], o[r + 1:r + 2])
    assert np.abs(lg.numpy()[0] - inp["ref"]["logits"][r + 1, :24]).max() <= 1e-6 and (inp["ref"]["logits"][r + 1, 24:] == 0).all()
    with_nan = SR.with_garbage(SR.build("ragged-fight-33"))
    assert np.isnan(with_nan[:, 0, 26:]).all() and np.isnan(with_nan[:, 1, 24:]).all() and np.isfinite(with_nan[:, 0, :26]).all() and np.isfinite(with_nan[:, 1, :24]).all()
    again = SR.sample_ref(SR.build("ragged-fight-33")["kinds"], SR.weights(5), with_nan, SR.build("ragged-fight-33")["crit_act"],
                          SR.build("ragged-fight-33")["uniforms"], False)
    assert all(np.array_equal(again[k], SR.build("ragged-fight-33")["ref"][k]) for k in again)
