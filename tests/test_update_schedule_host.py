"""update_schedule without a GPU: the one table that every step mode of both learners walks.  Unshuffled it is sequence_schedule's,
byte for byte, and its rows are the old eager loop's — passes outside, minibatch_order inside — restated here; shuffled it is
shuffled_schedule's pair.  `need` is the widest row's chunks."""
import numpy as np
import pytest

from hhmarl_2d_amd import learner as LR

KEYS = dict(seed=3, update=2, policy=1)
RAGGED = [20, 1, 20, 7, 20, 20, 3, 20, 12, 20, 20, 5, 20, 2]      # 190 rows: parts of >= 64 rows and a remainder of 47 (< 64)
CASES = {"one chunk": ([13], 64),
         "escape rows, S no multiple of the size": (np.ones(271, dtype=np.int64), 64),
         "ragged chunks with a remainder part": (RAGGED, 64),
         "a size above the whole batch": (RAGGED, 100000)}


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("passes", (1, 3))
@pytest.mark.parametrize("case", list(CASES))
def test_unshuffled_is_sequence_schedule_and_the_eager_order(case, passes):
    seq_len, size = CASES[case]
    order, sched, need = LR.update_schedule(seq_len, size, passes, **KEYS, shuffle=False)
    parts, want = LR.sequence_schedule(seq_len, size, passes, **KEYS)
    assert order is None
    assert sched.dtype == np.int32 and sched.shape == (passes * len(parts), 4) and _same_bytes(sched, want)
    assert need == max(s1 - s0 for s0, s1 in parts)
    # the eager loop as it was written: per pass the parts in minibatch_order's order, n_valid from the lengths' running sum
    csum = np.concatenate([[0], np.cumsum(np.asarray(seq_len, dtype=np.int64))])
    rows = []
    for sgd_pass in range(passes):
        for i in LR.minibatch_order(len(parts), KEYS["seed"], KEYS["update"], KEYS["policy"], sgd_pass):
            s0, s1 = parts[i]
            rows.append((s0, s1, int(csum[s1] - csum[s0]), 0))
    assert sched.tolist() == [list(r) for r in rows]


@pytest.mark.parametrize("passes", (1, 3))
@pytest.mark.parametrize("case", list(CASES))
def test_shuffled_is_shuffled_schedule(case, passes):
    seq_len, size = CASES[case]
    order, sched, need = LR.update_schedule(seq_len, size, passes, **KEYS, shuffle=True)
    want_order, want_sched = LR.shuffled_schedule(seq_len, size, passes, **KEYS)
    assert order.dtype == np.int32 and _same_bytes(order, want_order)
    assert sched.dtype == np.int32 and sched.ndim == 2 and sched.shape[1] == 4 and _same_bytes(sched, want_sched)
    assert need == int((sched[:, 1] - sched[:, 0]).max())


def test_the_cases_are_the_edges_they_claim():
    parts = LR.minibatch_partition(RAGGED, 64)
    tail = sum(RAGGED[parts[-1][0]:parts[-1][1]])
    assert len(parts) >= 3 and 0 < tail < 64, "the last part is a remainder smaller than the minibatch size"
    assert LR.minibatch_partition(RAGGED, 100000) == [(0, len(RAGGED))] and LR.minibatch_partition([13], 64) == [(0, 1)]
    assert 271 % 64 and LR.minibatch_partition(np.ones(271, dtype=np.int64), 64)[-1] == (256, 271)


def test_no_minibatch_needs_one_slot():
    """no pass: an empty table in either form; the staging capacity never falls below one chunk where there is no step"""
    order, sched, need = LR.update_schedule(RAGGED, 64, 0, **KEYS, shuffle=True)
    assert order.shape == (0,) and sched.shape == (0, 4) and need == 1
    order, sched, _ = LR.update_schedule(RAGGED, 64, 0, **KEYS, shuffle=False)
    assert order is None and sched.shape == (0, 4) and sched.dtype == np.int32
