"""CPU half of the commander sampler edge tests: the reference of tests/commander_sampler_ref.py ALONE meets the conditions under which
tests/test_gpu_commander_sampler_edges.py may compare the kernel's drawn and greedy actions exactly, on every row, and under which its
1e-5 bound says something about every stage of the network.

The half-width condition (the figure and derivation of tests/test_sampler_edges_host.py).  The commander's logit bound is TOL = 1e-5.  A logit
error of 1e-5 moves a softmax CDF by at most 2e-5 (|d softmax| <= 2 |d logit| in the worst case of all the mass moving one way), and the kernel's
(float) u rounding adds 6e-8.  A uniform that sits MIN_HALF_WIDTH = 1e-3 = 50 x that away from both ends of its CDF interval therefore selects the
same action on the device as in the float64 restatement: no row needs to be excluded.  With the synthetic weights of seed 4 the smallest action
probability over all cases is 0.19 (half-width 0.097).

The greedy gap.  Two logits that each move by TOL change their difference by at most 2 TOL = 2e-5; the reference's gap between its two largest
logits is held to MIN_GREEDY_GAP = 4e-5 = twice that on every row of every case whose greedy actions are compared with the float64 arg-max.
Seed 4 was chosen for it: the smallest gap over all cases is 8.0e-4 (seed 3: 2.6e-6, seed 5: 5.0e-4, seed 6: 7.2e-6).

The exact-logit table.  Away from u = 0 and u = 1 - 2^-53 every uniform lies 1e-3 from the boundary it was made from and at least 1e-4 from every
float64 CDF boundary, and there the float32 and the float64 restatement of the draw agree.  AT the two ends they need not, and the expectation is
the float32 restatement's, which follows include/hh_commander.h word for word ("t = (float)u * S, the action is the first i whose running sum
exceeds t (the last if none does)"): with bias (-200, 0, 0) float32 holds e_0 = exp(-200) = 0, the running sum 0 does not EXCEED t = 0, and u = 0
draws action 1 where float64 (e_0 = 1.4e-87 > 0) draws 0; with bias (0, 0, -200) u = 1 - 2^-53 rounds to 1.0f, t = S, no running sum exceeds it
and the draw is "the last", action 2, whose float32 probability is 0 (logp = -200.69, finite) where float64 draws 1.

Sensitivity of the bound.  Rounding any ONE of shared_layer, inp4, v4 and the four GRU matrices to fp16 in the float64 restatement (a lost lo
plane of the kernel's split-fp16 operands) moves a compared output by more than TOL.  Which output matters: on these inputs (97 arenas, seed 4)
                              logits     vf         h_out
    shared_layer              1.8e-4     1.2e-4     0
    inp4                      2.3e-5     0          2.3e-4
    v4                        0          2.2e-5     2.6e-4
    rnn_act.weight_ih_l0      9.3e-6     0          2.3e-4
    rnn_act.weight_hh_l0      1.3e-5     0          2.9e-4
    rnn_val.weight_ih_l0      0          8.6e-6     2.9e-4
    rnn_val.weight_hh_l0      0          8.8e-6     2.4e-4
A lost lo plane of a GRU matrix moves the network's outputs by about TOL itself — normalize(x_full + h') and the shared layer damp it; for
rnn_act.weight_hh_l0 7.5e-6 to 8.1e-6, INSIDE the bound, with the weights of seeds 3 and 5 — and the state by 2e-4 to 3e-4.  The logits and
vf do not pin the GRU stage; the state comparison does, which is why the GPU test compares h_out, both states, on every row."""
import os
import re

import numpy as np
import pytest
import torch

import commander_ref as CR
import commander_sampler_ref as SR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIDPOINT = [c for c in SR.CASES if c["uniforms"] == "midpoint"]
SENSITIVE = ("shared_layer._model.0.weight", "inp4._model.0.weight", "v4._model.0.weight", "rnn_act.weight_ih_l0", "rnn_act.weight_hh_l0",
             "rnn_val.weight_ih_l0", "rnn_val.weight_hh_l0")


def check_half_width(ref_logits, uniforms, targets):
    """every uniform at least MIN_HALF_WIDTH inside its target's interval of the float64 CDF -> the smallest distance"""
    cdf = SR.cdf64(np.asarray(ref_logits).reshape(-1, 3))
    u, t = np.asarray(uniforms).reshape(-1), np.asarray(targets).reshape(-1)
    rows = np.arange(len(u))
    d = np.minimum(u - cdf[rows, t], cdf[rows, t + 1] - u)
    assert d.min() >= SR.MIN_HALF_WIDTH, f"row {int(d.argmin())}: a uniform {d.min():.3e} from its interval's end"
    return float(d.min())


def check_row_counts(cases):
    missing = sorted(set(SR.RAGGED_ROWS) - SR.row_counts(cases))
    assert not missing, f"no ragged case with {missing} rows"


def check_action_coverage(case):
    """every action is some row's target on every agent slot"""
    t = SR.build(case)["targets"]
    for slot in range(3):
        assert set(t[:, slot].tolist()) == {0, 1, 2}, (case["name"], slot)


def moved_by_fp16(key, rounded=True):
    """the largest move of each compared output on the ragged inputs of 97 arenas when `key` is rounded to fp16 in the float64 restatement"""
    inp = SR.build("ragged-97")
    sd = dict(SR.weights())
    if rounded:
        sd[key] = sd[key].astype(np.float16).astype(np.float32)
    lg, vf, h_out, _ = SR.reference(SR.torch_weights(sd, torch.float64), inp["obs"], inp["h_in"], inp["fresh"], inp["crit_act"])
    return dict(logits=float(np.abs(lg - inp["ref"]["logits"]).max()), vf=float(np.abs(vf - inp["ref"]["vf"]).max()),
                h_out=float(np.abs(h_out - inp["ref"]["h_out"]).max()))


def check_sensitive(key, rounded=True):
    d = moved_by_fp16(key, rounded)
    assert max(d.values()) > SR.TOL, f"{key} rounded to fp16 moves no compared output by more than {SR.TOL}: {d}"
    return d


@pytest.mark.parametrize("case", MIDPOINT, ids=lambda c: c["name"])
def test_midpoint_uniforms_are_far_from_every_cdf_boundary(case):
    inp = SR.build(case)
    assert inp["half_width"].min() >= SR.MIN_HALF_WIDTH, inp["half_width"].min()
    assert check_half_width(inp["ref"]["logits"], inp["uniforms"], inp["targets"]) >= SR.MIN_HALF_WIDTH
    # the float64 draw of those uniforms IS the target, on every row
    assert np.array_equal(inp["ref"]["actions"], inp["targets"]) and np.isfinite(inp["ref"]["logp"]).all()


def test_half_width_check_notices_a_uniform_near_a_boundary():
    inp = SR.build("ragged-11")
    u = inp["uniforms"].copy()
    r, s = 10, 1                                                   # a row of the arena that straddles the tile edge
    u[r, s] = SR.cdf64(inp["ref"]["logits"][r, s])[inp["targets"][r, s]] + 0.5 * SR.MIN_HALF_WIDTH
    with pytest.raises(AssertionError, match="from its interval's end"):
        check_half_width(inp["ref"]["logits"], u, inp["targets"])


def test_row_count_and_action_coverage():
    check_row_counts(SR.CASES)
    assert {3 * n for n in SR.RAGGED_N} == set(SR.RAGGED_ROWS)
    for rows in SR.RAGGED_ROWS:                                    # the check notices every missing one
        with pytest.raises(AssertionError, match=f"{rows}"):
            check_row_counts([c for c in SR.CASES if 3 * c["n"] != rows or c["group"] != "ragged"])
    for case in SR.CASES:
        if case["group"] == "ragged" and case["n"] >= 3:
            check_action_coverage(case)
    # the arenas whose rows lie in two tiles: 2|1 at 33 rows, 2|1 and 1|2 at 66
    assert SR.straddlers(11).tolist() == [10] and SR.straddlers(22).tolist() == [10, 21] and len(SR.straddlers(32)) == 2
    assert (3 * 10 + 2) // 32 == 1 and (3 * 10 + 1) // 32 == 0 and (3 * 21) // 32 == 1 and (3 * 21 + 1) // 32 == 2
    # both sides of a tile edge see every action on every agent slot: the nine rows (three arenas' worth) before and after it
    t = SR.build("ragged-43")["targets"].reshape(-1)
    for edge in (32, 64, 96, 128):
        for rows in (range(edge - 9, edge), range(edge, edge + 9)):
            seen = {(r % 3, int(t[r])) for r in rows if r < len(t)}
            assert rows[-1] >= len(t) or seen == {(s, a) for s in range(3) for a in range(3)}, (edge, sorted(seen))


def test_inputs_are_what_the_cases_say():
    for case in SR.CASES:
        inp = SR.build(case)
        N = case["n"]
        assert inp["obs"].shape == (N, 3, 34) and inp["obs"].min() >= 0.0 and inp["obs"].max() < 1.0
        if N >= 3:
            assert (inp["obs"] == 0).all(axis=(1, 2)).any(), "an arena with all three rows zero"
        f = inp["fresh"].astype(bool)
        assert np.isfinite(inp["h_in"][~f]).all() and (np.abs(inp["h_in"][~f]) <= 1.0).all()
        assert np.isnan(inp["h_in"][f]).all() if case["nan_states"] else np.isfinite(inp["h_in"]).all()
        assert (inp["h_used"][f] == 0).all() and np.array_equal(inp["h_used"][~f], inp["h_in"][~f])
        if case["crit_act"] == "distinct":
            assert (np.sort(inp["crit_act"], axis=1) == np.array([0.0, 0.5, 1.0], dtype=np.float32)).all()
        elif case["crit_act"] == "random":
            assert set(np.unique(inp["crit_act"]).tolist()) <= {0.0, 0.5, 1.0}
        else:
            assert inp["crit_act"] is None
    pats = {p: SR.build(f"fresh-22-{p}")["fresh"] for p in SR.FRESH_PATTERNS}
    assert not pats["none"].any() and pats["all"].all() and pats["alternating"].tolist() == [1, 0] * 11
    assert np.flatnonzero(pats["straddle"]).tolist() == [10, 21]
    assert np.flatnonzero(SR.build("fresh-11-straddle")["fresh"]).tolist() == [10]
    assert 0 < SR.build("ragged-97")["fresh"].sum() < 97


@pytest.mark.parametrize("name", SR.names("ragged") + SR.names("fresh"))
def test_greedy_gap(name):
    """no row excluded: the float64 arg-max is unique by MIN_GREEDY_GAP on every row the GPU test compares greedy actions on"""
    gap = SR.build(name)["ref"]["gap"]
    print(f"{name}: smallest gap between the two largest reference logits {gap.min():.3e}")
    assert gap.min() >= SR.MIN_GREEDY_GAP


def test_exact_logit_table():
    with open(os.path.join(ROOT, "include", "hh_commander.h")) as f:
        header = re.sub(r"\s*\n \* ?", " ", f.read())                    # the comment's lines joined
    assert "m = max l, S = sum exp(l_i - m) in index order, t = (float)u * S, the action is the first i whose running sum exceeds t (the last if none does)" in header
    table = SR.exact_table()
    assert [r["bias"] for r in table] == [tuple(map(float, b)) for b in SR.BIAS_TRIPLES]
    for row in table:
        b = np.array(row["bias"])
        gaps = np.abs(b[:, None] - b[None, :])
        assert ((gaps <= 80.0) | (gaps >= 200.0)).all()                       # float32 exp: a normal number or exactly 0
        e = np.exp((b - b.max()).astype(np.float32))
        assert ((e == 0) | (e >= np.finfo(np.float32).tiny)).all()
        u = row["uniforms"]
        edge = (u == 0.0) | (u == SR.ONE_BELOW)
        assert edge.sum() == 2 and (~edge).sum() >= 2 and (u >= 0).all() and (u < 1).all()
        assert row["clear"][~edge].min() >= SR.EXACT_CLEAR, row["bias"]
        assert np.array_equal(row["expected"][~edge], row["act64"][~edge]), row["bias"]
        assert np.isfinite(row["logp64"]).all()
        assert row["greedy"] == int(np.flatnonzero(b == b.max())[0])
    by = {r["bias"]: r for r in table}
    at = lambda bias, u: int(by[bias]["expected"][np.flatnonzero(by[bias]["uniforms"] == u)[0]])
    assert at((-200.0, 0.0, 0.0), 0.0) == 1 and at((-200.0, 0.0, -200.0), 0.0) == 1        # the running sum 0 does not exceed t = 0
    assert at((0.0, 0.0, -200.0), SR.ONE_BELOW) == 2 and at((-200.0, 0.0, -200.0), SR.ONE_BELOW) == 2   # "the last if none does"
    assert all(at(tuple(map(float, b)), 0.0) == 0 for b in SR.TIES) and all(at(tuple(map(float, b)), SR.ONE_BELOW) == 2 for b in SR.TIES)
    assert [by[tuple(map(float, b))]["greedy"] for b in SR.TIES] == [0, 0, 1, 0]            # the first arg-max
    # the float32 restatement is the float64 one wherever a draw has room: the midpoint cases
    inp = SR.build("ragged-97")
    assert np.array_equal(SR.inverse_cdf_f32(inp["ref"]["logits"], inp["uniforms"]), inp["ref"]["actions"])


def test_draw_edge_references():
    for name, want in (("draw-zero-11", 0), ("draw-one-11", 2)):
        inp = SR.build(name)
        assert (inp["ref"]["actions"] == want).all() and (SR.inverse_cdf_f32(inp["ref"]["logits"], inp["uniforms"]) == want).all()
        assert (inp["uniforms"] == (0.0 if want == 0 else SR.ONE_BELOW)).all()


@pytest.mark.parametrize("key", SENSITIVE)
def test_bound_is_sensitive_to_a_lost_lo_plane(key):
    d = check_sensitive(key)
    print(f"{key} rounded to fp16: logits {d['logits']:.3e} vf {d['vf']:.3e} h_out {d['h_out']:.3e}")
    if key.startswith("rnn_"):
        # the state comparison is what pins the GRU stage: 20 x TOL there, about TOL itself in the network's outputs
        assert d["h_out"] > 20 * SR.TOL and max(d["logits"], d["vf"]) < 2 * SR.TOL
    with pytest.raises(AssertionError, match="moves no compared output"):     # the check pointed at an unrounded matrix
        check_sensitive(key, rounded=False)


@pytest.mark.parametrize("name", SR.names("fresh"))
def test_fresh_reference_ignores_what_the_state_held(name):
    inp = SR.build(name)
    sd = SR.torch_weights(SR.weights(), torch.float64)
    zeros = np.nan_to_num(inp["h_in"], nan=0.0)
    junk = np.nan_to_num(inp["h_in"], nan=0.75)
    for h in (zeros, junk):
        lg, vf, h_out, used = SR.reference(sd, inp["obs"], h, inp["fresh"], inp["crit_act"])
        assert np.array_equal(lg, inp["ref"]["logits"]) and np.array_equal(vf, inp["ref"]["vf"]) and np.array_equal(h_out, inp["ref"]["h_out"])
        assert np.array_equal(used, inp["h_used"])
    assert all(np.isfinite(inp["ref"][k]).all() for k in ("logits", "vf", "h_out", "logp"))
    if inp["fresh"].any() and not inp["fresh"].all():
        # ... and a state that is NOT fresh matters: the comparison would notice a kernel that zeroed too much
        lg, _, _, _ = SR.reference(sd, inp["obs"], zeros, np.ones_like(inp["fresh"]), inp["crit_act"])
        assert np.abs(lg - inp["ref"]["logits"])[~inp["fresh"].astype(bool)].min() > 0
