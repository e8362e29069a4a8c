"""Host restatement of the accumulated whole-episode batches (test infrastructure): what `EpisodeBatch(train_batch_size=B)` /
`CommanderEpisodeBatch(train_batch_size=B)` hold after every collect, from tests/episodes_ref.restate's per-collect batches and RLlib's
rule (training_step concatenates whole sample batches until at least train_batch_size environment steps are there, trims nothing, runs
one update and starts over):
  * the per-collect batches are concatenated in collect order;
  * ep_start and seq_start are shifted by the rows, seq_ep by the episodes, that the batch held before the collect;
  * a collect that follows one which reached B rows starts a new batch at 0.
`acc` restates the device accumulator of hh_episodes_emit_append (include/hh_abi.h, HH_EP_ACC): [0] rows, [1] episodes, [2] overflow,
[3] sequences, [4] rows >= B, [5] collects in this batch, [6] batches completed, [7] 0."""
import numpy as np

from episodes_ref import OUT_COLS, SEQ_TABLE, TABLE

SHIFT_ROWS, SHIFT_EPS = ("ep_start", "seq_start"), ("seq_ep",)


def with_tables(batch):
    """one restated batch with its episode table (restate gives it only with sequences): an episode starts on every row with t = 0, in
    row order, and its length is t + 1 of its done row"""
    if "ep_start" in batch:
        return batch
    b = dict(batch)
    first = np.nonzero(batch["t"] == 0)[0]
    b["ep_start"] = first.astype(np.int32)
    b["ep_len"] = (batch["t"][batch["done"] == 1] + 1).astype(np.int32)
    b["ep_arena"] = batch["arena"][first].astype(np.int32)
    assert len(b["ep_len"]) == len(first)
    return b


def accumulate(batches, train_rows, caps=None):
    """batches: restate()'s list, one per collect; train_rows: B >= 1; caps: None or (row_cap, ep_cap, seq_cap) of the accumulated batch
    -> one entry per collect: (the accumulated batch after it — dict of the columns, the tables, state_in —, acc i32 [8], counts (rows,
    episodes, sequences written by this collect)).  With caps the accumulator is clamped to them and acc[2] tells an overflow (sticky);
    the batch's contents are then the unclamped ones: what fits is for the caller to cut."""
    assert train_rows >= 1
    acc = np.zeros(8, dtype=np.int32)
    cur, out = None, []
    for b in batches:
        b = with_tables(b)
        if cur is None or acc[4]:
            if acc[4]:
                acc[5] = 0
                acc[6] += 1
            cur = {k: v[:0] for k, v in b.items()}
            acc[[0, 1, 3]] = 0
        base_rows, base_eps = int(acc[0]), int(acc[1])
        shifted = {k: (v + base_rows if k in SHIFT_ROWS else v + base_eps if k in SHIFT_EPS else v).astype(v.dtype) for k, v in b.items()}
        cur = {k: np.concatenate([cur[k], shifted[k]], axis=0) for k in cur}
        want = [base_rows + len(b["t"]), base_eps + len(b["ep_start"]), int(acc[3]) + len(b.get("seq_start", ()))]
        counts = []
        for slot, w, cap in zip((0, 1, 3), want, caps or (None,) * 3):
            end = w if cap is None else min(w, int(cap))
            if end < w:
                acc[2] = 1
            counts.append(end - int(acc[slot]))
            acc[slot] = end
        acc[4] = int(acc[0] >= train_rows)
        acc[5] += 1
        out.append((cur, acc.copy(), tuple(counts)))
    return out


def batch_keys(seq):
    """the parts of an accumulated batch: the columns, the episode table and (seq) the sequence table with state_in"""
    return OUT_COLS + TABLE + ((SEQ_TABLE + ("state_in",)) if seq else ())
