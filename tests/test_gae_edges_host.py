"""What tests/test_gpu_gae_edges.py rests on, without a GPU (tables: tests/gae_edges_ref.py): the float32 form of the masked recursion is
oracle/gae_ref.py's masked_stream bit for bit and does not read an invalid row's reward, e32 is positive on every general case, the exact
table is exact, and the ragged done pattern cannot be reproduced by an arena index taken as col % N or col % nA."""
import numpy as np
import pytest

import gae_edges_ref as G
import gae_ref


def test_the_cases_cover_the_issue():
    cases = G.cases()
    assert len(set(cases)) == len(cases)
    cols = {(N * nA, nA) for (N, nA, *_r) in cases}
    assert {(1, 1), (255, 1), (256, 1), (257, 1), (513, 1), (256, 2), (255, 3), (513, 3)} <= cols
    assert {(254, 2), (258, 2), (258, 3)} <= cols                     # either side of the block where nA does not divide 255 or 257
    for (N, nA) in G.SHAPES:
        assert {(T, d) for (n, a, T, d, *_r) in cases if (n, a) == (N, nA)} == {(T, d) for T in G.TS for d in G.DONES}
    for gl in G.GAMMA_LAMBDA:
        assert {a for (_n, a, _T, _d, *g) in cases if tuple(g) == gl} == {1, 2, 3}
    assert set(G.GAMMA_LAMBDA) == {(0.99, 0.95), (0.99, 1.0), (1.0, 1.0), (0.0, 0.95), (0.99, 0.0)}


def test_float32_form_is_masked_stream_and_e32_is_positive():
    for case in G.cases():
        x, want, e32 = G.general_case(case)
        a32, r32 = G.masked(x["reward"], x["valid"], x["value"], x["done"], case[4], case[5], np.float32)
        a_ms, r_ms = gae_ref.masked_stream(x["reward"], x["valid"], x["value"], x["done"], case[4], case[5])
        assert a32.dtype == np.float32 and np.array_equal(a32, a_ms) and np.array_equal(r32, r_ms), case
        assert min(e32) > 0.0, (case, e32)
        assert case[0] * case[1] * case[2] > G.FEW or G.e32_is_representative(want, e32), (case, e32)
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
        off = x["valid"] == 0
        assert (want[0][off] == 0).all() and (want[1][off] == 0).all()


def test_an_invalid_rows_reward_is_not_read_by_the_references():
    case = (129, 2, 97, "ragged", 0.99, 0.95)
    x, want, _ = G.general_case(case)
    off = x["valid"] == 0
    assert off.any() and off[:-1].any()
    r_nan = np.where(off, np.float32("nan"), x["reward"])
    for got in (G.masked(r_nan, x["valid"], x["value"], x["done"], 0.99, 0.95, np.float64),):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with np.errstate(invalid="ignore"):
        a_ms, r_ms = gae_ref.masked_stream(r_nan, x["valid"], x["value"], x["done"], 0.99, 0.95)
    a0, r0 = gae_ref.masked_stream(x["reward"], x["valid"], x["value"], x["done"], 0.99, 0.95)
    assert np.array_equal(a_ms, a0) and np.array_equal(r_ms, r0)
    # and an invalid row does not propagate: the rows before it see A_{t+1} = 0 (a reference that passed it on would differ)
    assert np.abs(want[0]).max() > 0


@pytest.mark.parametrize("case", G.EXACT_CASES)
def test_exact_table_is_exact(case):
    x = G.exact_case(case)
    den = case[3]
    for k in ("reward", "value"):
        assert np.array_equal(x[k] * den, np.round(x[k] * den)) and np.abs(x[k]).max() <= 8.0
    a64, r64 = G.masked(x["reward"], x["valid"], x["value"], x["done"], 0.5, 0.5, np.float64)
    a32, r32 = G.masked(x["reward"], x["valid"], x["value"], x["done"], 0.5, 0.5, np.float32)
    assert np.array_equal(a32.astype(np.float64), a64) and np.array_equal(r32.astype(np.float64), r64)
    if case[2] >= 7:                                                  # chains of 7 steps are there: this is the edge of 24 bits
        assert (x["done"][:-1].sum(axis=0) == 0).any()
        assert (np.abs(a64) * 2.0 ** 19 % 2 == 1).any() or case[3] == 16


def test_ragged_done_is_tied_to_the_arena():
    """the done of column col belongs to arena col // nA: the outputs with the index taken as col % N or col % nA differ"""
    for (N, nA) in ((128, 2), (85, 3), (129, 2)):
        case = (N, nA, 97, "ragged", 0.99, 0.95)
        x, want, e32 = G.general_case(case)
        col = np.arange(N * nA)
        for wrong in (col % N, col % nA):
            d = x["done"][:, wrong].reshape(97, N, nA)                # a per-column done, as the wrong index would read it
            right = x["done"][:, col // nA].reshape(97, N, nA)
            assert (d != right).mean() > 0.05
            assert np.array_equal(right, np.broadcast_to(x["done"][:, :, None], right.shape))
