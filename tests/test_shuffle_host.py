"""shuffle_sequences without a GPU: sequence_order and shuffled_schedule against their contract and the restatement of
tests/shuffle_ref.py, the torch-op gather against the restatement, both learners' validation of the flag, and the C ABI's declaration."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import shuffle_ref as SR
from hhmarl_2d_amd import _lib
from hhmarl_2d_amd import learner as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEARNERS = [(LR.CommanderLearner, (None, "cpu")), (LR.PPOLearner, ((0, 1), None, "cpu"))]
S, PASSES = 331, 3
SEQ_LEN = np.random.default_rng(5).integers(1, 21, S)       # 3442 rows: with seed 1 the first pass cuts 13 minibatches of 256, the others 14
KEYS = dict(seed=1, update=2, policy=1)


def test_sequence_order_is_a_keyed_permutation_of_its_own_stream():
    a = LR.sequence_order(S, 7, 2, 1, 0)
    assert a.dtype == np.int64 and a.shape == (S,) and sorted(a.tolist()) == list(range(S))
    assert np.array_equal(a, LR.sequence_order(S, 7, 2, 1, 0)) and np.array_equal(a, SR.sequence_order_ref(S, 7, 2, 1, 0))
    np.random.seed(0)
    np.random.random(5)                                   # the global generator is no key
    assert np.array_equal(a, LR.sequence_order(S, 7, 2, 1, 0))
    for other in ((8, 2, 1, 0), (7, 3, 1, 0), (7, 2, 0, 0), (7, 2, 1, 1)):
        assert not np.array_equal(a, LR.sequence_order(S, *other)), other
    assert not np.array_equal(a, LR.minibatch_order(S, 7, 2, 1, 0)), "a different stream from minibatch_order's for the same keys"
    assert LR.sequence_order(0, 1, 2, 3, 4).shape == (0,) and LR.sequence_order(1, 1, 2, 3, 4).tolist() == [0]


@pytest.mark.parametrize("size", (256, 100000, 1))
def test_shuffled_schedule_keeps_its_contract(size):
    order, sched = LR.shuffled_schedule(SEQ_LEN, size, PASSES, **KEYS)
    assert order.dtype == np.int32 and order.shape == (PASSES * S,)
    assert sched.dtype == np.int32 and sched.ndim == 2 and sched.shape[1] == 4 and not sched[:, 3].any()
    want_order, want_sched = SR.schedule_ref(SEQ_LEN, size, PASSES, **KEYS)
    assert np.array_equal(order, want_order) and np.array_equal(sched, want_sched)
    firsts, counts, at = [], [], 0
    for p in range(PASSES):
        perm = order[p * S:(p + 1) * S]
        assert np.array_equal(perm, LR.sequence_order(S, KEYS["seed"], KEYS["update"], KEYS["policy"], p))
        assert sorted(perm.tolist()) == list(range(S)), "every sequence once per pass"
        rows = [r for r in sched.tolist() if p * S <= r[0] < (p + 1) * S]
        assert rows == sched[at:at + len(rows)].tolist(), "the passes follow each other, their minibatches in position order"
        at += len(rows)
        assert rows[0][0] == p * S and rows[-1][1] == (p + 1) * S, "inside the pass's own range"
        assert all(a[1] == b[0] for a, b in zip(rows, rows[1:])) and all(r[0] < r[1] for r in rows), "no gap, no overlap, nothing empty"
        for i, (o0, o1, nv, _) in enumerate(rows):
            lens = SEQ_LEN[order[o0:o1]]
            assert nv == int(lens.sum())
            if i < len(rows) - 1:
                assert nv >= size and nv - int(lens[-1]) < size, "at least `size` rows, and fewer without the final chunk"
        assert sum(r[2] for r in rows) == int(SEQ_LEN.sum())
        firsts.append(frozenset(order[rows[0][0]:rows[0][1]].tolist()))
        counts.append(len(rows))
    assert at == len(sched)
    if size == 256:
        assert firsts[0] != firsts[1] and firsts[1] != firsts[2], "two passes have different first minibatches"
        assert counts == [13, 14, 14], "the passes may differ in their number of steps"
    elif size == 1:
        assert counts == [S] * PASSES
    else:
        assert counts == [1] * PASSES and firsts[0] == frozenset(range(S))


def test_shuffled_schedule_edges():
    order, sched = LR.shuffled_schedule([], 256, 3, 0, 0, 0)
    assert order.shape == (0,) and sched.shape == (0, 4) and order.dtype == np.int32 and sched.dtype == np.int32
    order, sched = LR.shuffled_schedule([5], 256, 2, 0, 0, 0)
    assert order.tolist() == [0, 0] and sched.tolist() == [[0, 1, 5, 0], [1, 2, 5, 0]]
    order, sched = LR.shuffled_schedule(np.ones(10, dtype=np.int64), 4, 0, 0, 0, 0)
    assert order.shape == (0,) and sched.shape == (0, 4)
    huge = np.broadcast_to(np.int64(1), (1 << 27,))      # a view of one element: 2^27 chunks x 30 passes do not fit int32 positions
    with pytest.raises(ValueError, match="int32"):
        LR.shuffled_schedule(huge, 256, 30, 0, 0, 0)      # refused before anything of that size is built


def test_the_unshuffled_definitions_stay():
    """minibatch_order's stream and minibatch_schedule's rows are what they were: values pinned from the four-entry key"""
    assert np.array_equal(LR.minibatch_order(6, 7, 2, 1, 0), np.random.default_rng([7, 2, 1, 0]).permutation(6))
    parts, sched = LR.sequence_schedule(SEQ_LEN, 256, 2, 7, 2, 1)
    assert parts == LR.minibatch_partition(SEQ_LEN, 256) and sched.shape == (2 * len(parts), 4) and not sched[:, 3].any()
    assert sorted(tuple(r[:2]) for r in sched[:len(parts)].tolist()) == sorted(parts)


def test_the_torch_gather_equals_the_restatement():
    g = torch.Generator().manual_seed(3)
    cols = [torch.randn((12, 20, 7), generator=g), torch.randint(0, 9, (12, 20, 4), generator=g).to(torch.int8), torch.randn((12,), generator=g),
            torch.randint(0, 2, (12, 20), generator=g).to(torch.uint8)]
    cols[0][3, 2, 1] = float("nan")
    for idx in ([3, 0, 11], list(range(11, -1, -1)), [3, 3, 3, 0], [], [-1, 12, 2 ** 31 - 1, -2 ** 31, 5], [3, -1, 4]):
        got = LR.minibatch_stage_gather_torch(cols, 13, idx)
        also = LR.minibatch_stage_gather_torch(cols, 13, torch.tensor(idx, dtype=torch.int32))
        for c, st, st2 in zip(cols, got, also):
            want = SR.gather_ref(c.numpy(), 13, idx)
            assert st.dtype == c.dtype and tuple(st.shape) == want.shape and st.numpy().tobytes() == want.tobytes(), idx
            assert st2.numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        LR.minibatch_stage_gather_torch(cols, 2, [0, 1, 2])
    # the identity order is the contiguous stage
    staged, _ = LR.minibatch_stage_torch(cols, 13, (2, 9, 0, 0))
    for a, b in zip(staged, LR.minibatch_stage_gather_torch(cols, 13, range(2, 9))):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_the_restatement_clamps_as_the_contract_says():
    col = np.arange(1, 41, dtype=np.float32).reshape(10, 4)
    order = np.array([9, 8, 7, 6, 5, 4], dtype=np.int32)
    sched = [(4, 30, 5, 0), (0, 6, 9, 0), (-3, 2, 1, 0), (5, 3, 2, 0)]
    want = {0: [5, 4], 1: [9, 8, 7, 6], 2: [9, 8], 3: [], 4: [], -1: []}
    for cur, idx in want.items():
        got, nv = SR.stage_gather_ref(col, 4, order, sched, cur)
        assert np.array_equal(got, SR.gather_ref(col, 4, idx)) and nv == (sched[cur][2] if 0 <= cur < 4 else 0)
    assert not SR.stage_gather_ref(col, 4, order, sched, 1, src_chunks=7)[0][:2].any(), "chunks 9 and 8 lie beyond src_chunks = 7"


@pytest.mark.parametrize("learner,args", LEARNERS)
def test_the_flag_is_validated_after_the_other_modes_and_before_the_device(learner, args):
    for bad in ("yes", 1, None, 0, "True", np.bool_(True)):
        with pytest.raises(ValueError, match="shuffle_sequences"):
            learner(*args, shuffle_sequences=bad)
        with pytest.raises(ValueError, match="shuffle_sequences"):
            learner(*args, optimizer="fused", step="graph", grad_clip=0.5, shuffle_sequences=bad)
    with pytest.raises(ValueError, match="optimizer is one of"):
        learner(*args, optimizer="adam", shuffle_sequences="yes")
    with pytest.raises(ValueError, match='needs optimizer="fused"'):
        learner(*args, step="graph", shuffle_sequences="yes")
    with pytest.raises(ValueError, match="grad_clip"):
        learner(*args, grad_clip=-1, shuffle_sequences="yes")
    params = list(inspect.signature(learner.__init__).parameters.values())
    assert params[-1].name == "grad_clip" and params[-1].default is None
    assert params[-2].name == "shuffle_sequences" and params[-2].default is False
    assert LR._shuffle_flag(True) is True and LR._shuffle_flag(False) is False


def test_the_entry_point_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "hh_learner.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (HH_STAGE_[A-Z_]+)\s+(\d+)", txt)}
    assert defs["HH_STAGE_MAX_COLS"] == 8 == _lib.STAGE_MAX_COLS
    m = re.search(r"^int hh_minibatch_stage_gather\((.*?)\);", txt, re.M | re.S)
    assert m, "include/hh_learner.h declares hh_minibatch_stage_gather"
    got = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert got == ["int32_t n_cols", "const hh_stage_col *cols", "int32_t chunk_len", "int32_t cap", "int64_t src_chunks", "const int32_t *order",
                   "int64_t order_len", "const int32_t *schedule", "int32_t sched_rows", "const int32_t *cursor", "int32_t *n_valid", "void *stream"]
    assert "hh_minibatch_stage_gather" in _lib.LEARNER_EXPORTS and "hh_minibatch_stage" in _lib.LEARNER_EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "hh_minibatch_stage_gather"), "libhh_world.so does not export hh_minibatch_stage_gather"
    args = _lib.lib().hh_minibatch_stage_gather.argtypes
    assert len(args) == len(got) and args[6] is C.c_int64 and args[4] is C.c_int64 and args[8] is C.c_int32
    src = open(os.path.join(ROOT, "hhmarl_2d_amd", "csrc", "hh_train_step.h")).read()
    assert "hh_k_minibatch_stage_gather" in src and 'extern "C" int hh_minibatch_stage_gather(' in src
