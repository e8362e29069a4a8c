"""Plain-numpy restatements that the shuffle_sequences tests hold the code against (learner.sequence_order, learner.shuffled_schedule,
learner.minibatch_stage_gather: hh_minibatch_stage_gather), written from the contract in include/hh_learner.h and DESIGN.md section 22
and from nothing in the learner package."""
import numpy as np


def gather_ref(col, cap, idx, src_chunks=None):
    """one column [S, ...] (numpy, any dtype) gathered by the integers idx [n <= cap] -> [cap, ...]: chunk idx[i] at place i, zero bytes
    where idx[i] is outside [0, src_chunks) (default S), zero bytes behind"""
    col = np.asarray(col)
    src_chunks = col.shape[0] if src_chunks is None else int(src_chunks)
    out = np.zeros((int(cap),) + col.shape[1:], dtype=col.dtype)
    idx = [int(c) for c in np.asarray(idx).reshape(-1)]
    assert len(idx) <= cap
    for i, c in enumerate(idx):
        if 0 <= c < src_chunks:
            out[i] = col[c]
    return out


def clamp_row(row, cursor, sched_rows, order_len, cap):
    """what the kernel makes of schedule[cursor]: (o0, o1, n_valid) with 0 <= o0 <= o1 <= order_len and o1 - o0 <= cap; a cursor outside
    [0, sched_rows) gives the empty minibatch (0, 0, 0)"""
    if not 0 <= cursor < sched_rows:
        return 0, 0, 0
    o0, o1, nv = int(row[0]), int(row[1]), int(row[2])
    o0 = max(o0, 0)
    o1 = min(o1, int(order_len))
    o1 = max(o1, o0)
    o1 = min(o1, o0 + int(cap))
    return o0, o1, nv


def stage_gather_ref(col, cap, order, schedule, cursor, src_chunks=None, order_len=None):
    """one launch on one column -> (staged [cap, ...], n_valid)"""
    order = np.asarray(order).reshape(-1)
    order_len = len(order) if order_len is None else int(order_len)
    schedule = np.asarray(schedule).reshape(-1, 4)
    row = schedule[cursor] if 0 <= cursor < len(schedule) else (0, 0, 0, 0)
    o0, o1, nv = clamp_row(row, cursor, len(schedule), order_len, cap)
    return gather_ref(col, cap, order[o0:o1], src_chunks), nv


def sequence_order_ref(n, seed, update, policy, sgd_pass):
    return np.random.default_rng([seed, update, policy, sgd_pass, 1]).permutation(n)


def schedule_ref(seq_len, size, num_sgd_iter, seed, update, policy):
    """the contract, step by step: per pass the permutation, then runs in permuted order that end with the chunk that brings them to at
    least `size` unpadded rows (the last run takes the rest) -> (order, rows)"""
    seq_len = [int(x) for x in seq_len]
    S = len(seq_len)
    order, rows = [], []
    for p in range(num_sgd_iter):
        perm = [int(c) for c in sequence_order_ref(S, seed, update, policy, p)]
        order += perm
        start, acc = 0, 0
        for i, c in enumerate(perm):
            acc += seq_len[c]
            if acc >= size or i == S - 1:
                rows.append((p * S + start, p * S + i + 1, acc, 0))
                start, acc = i + 1, 0
    return np.asarray(order, dtype=np.int64), np.asarray(rows, dtype=np.int64).reshape(-1, 4)
