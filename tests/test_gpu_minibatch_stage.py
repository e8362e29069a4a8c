"""learner.minibatch_stage (hh_minibatch_stage) on the MI355X: bitwise equality with the restatement of tests/train_step_ref.py for a
fight batch (chunks of 20, staged large -> small, so stale chunks must be zeroed) and an escape batch (rows, one-byte mask chunks)."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_step_ref as TR

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


def _guarded_zeros(shape, dtype, fill=0):
    """a staging buffer inside a byte allocation filled with SENTINEL: 64 guard bytes on either side (alignment kept)"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    big = torch.full((n + 128,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = big[64:64 + n].view(dtype).reshape(shape)
    view.fill_(fill)
    return big, view


def _intact(big, view):
    n = view.numel() * view.element_size()
    return bool((big[:64] == SENTINEL).all() and (big[64 + n:] == SENTINEL).all())


def _fight_batch(S=37, Lc=20, seed=4):
    from hhmarl_2d_amd import learner as LR
    g = torch.Generator().manual_seed(seed)
    seq_len = torch.randint(1, Lc + 1, (S,), generator=g)
    seq_len[0], seq_len[1] = Lc, 1
    seq_start = torch.cumsum(seq_len, 0) - seq_len
    R = int(seq_len.sum())
    flat = {"obs": torch.randn((R, 30), generator=g), "critic": torch.randn((R, 57), generator=g),
            "actions": torch.randint(0, 9, (R, 4), generator=g).to(torch.int8), "old_logp": torch.randn((R,), generator=g),
            "adv": torch.randn((R,), generator=g), "target": torch.randn((R,), generator=g), "old_logits": torch.randn((R, 32), generator=g)}
    cols = {k: LR.pad_chunks(v, seq_start, seq_len, Lc) for k, v in flat.items()}
    cols["obs"][0, 3, 5] = float("nan")       # bytes are bytes: a NaN travels, and must be gone again when its chunk is not staged
    cols["mask"] = LR.chunk_mask(seq_len, Lc).to(torch.uint8)
    return {k: v.contiguous().cuda() for k, v in cols.items()}, seq_len.numpy()


def _run(cols, bounds, n_valid, cap, chunk_len, order, mask_counts=True):
    """stage the parts in `order` into guarded buffers that start full of ones; compare each with the restatement, byte for byte"""
    from hhmarl_2d_amd import learner as LR
    names = list(cols)
    sched = torch.tensor([(s0, s1, nv, 0) for (s0, s1), nv in zip(bounds, n_valid)], dtype=torch.int32, device="cuda")
    staged = {k: _guarded_zeros((cap,) + tuple(cols[k].shape[1:]), cols[k].dtype, fill=1) for k in names}
    cursor = torch.zeros((1,), dtype=torch.int32, device="cuda")
    nv_out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    host = {k: cols[k].cpu().numpy() for k in names}
    for i in order:
        cursor.fill_(i)
        LR.minibatch_stage([cols[k] for k in names], [staged[k][1] for k in names], chunk_len, sched, cursor, nv_out)
        assert int(nv_out.item()) == n_valid[i] and int(cursor.item()) == i          # n_valid written, the cursor untouched
        for k in names:
            want = TR.stage_ref(host[k], cap, sched[i].tolist())
            got = staged[k][1].cpu().numpy()
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (i, k)
            assert _intact(*staged[k])
        if mask_counts:
            assert int(staged["mask"][1].sum()) == n_valid[i]


def test_fight_batch_large_to_small():
    """37 chunks of 20 with ragged seq_len, parts of 1, 5, 16 and 15 chunks into cap = 16, the largest first"""
    cols, seq_len = _fight_batch()
    bounds = [(0, 1), (1, 6), (6, 22), (22, 37)]
    n_valid = [int(seq_len[s0:s1].sum()) for s0, s1 in bounds]
    _run(cols, bounds, n_valid, 16, 20, order=(2, 3, 1, 0, 2))


def test_escape_batch_of_rows():
    """1000 rows, L = 1: parts of 256, 256, 256 and 232 rows into cap = 256; the mask column moves one byte per chunk"""
    g = torch.Generator().manual_seed(6)
    R = 1000
    cols = {"obs": torch.randn((R, 30), generator=g), "critic": torch.randn((R, 66), generator=g),
            "actions": torch.randint(0, 9, (R, 4), generator=g).to(torch.int8), "old_logp": torch.randn((R,), generator=g),
            "adv": torch.randn((R,), generator=g), "target": torch.randn((R,), generator=g), "old_logits": torch.randn((R, 32), generator=g),
            "mask": torch.ones((R,), dtype=torch.uint8)}
    cols = {k: v.cuda() for k, v in cols.items()}
    bounds = [(0, 256), (256, 512), (512, 768), (768, 1000)]
    _run(cols, bounds, [s1 - s0 for s0, s1 in bounds], 256, 1, order=(0, 3, 1, 2, 3))


def test_odd_alignments_take_the_narrower_units():
    """a source that starts 2 and 1 bytes into its allocation, chunks of 6 and 3 bytes: the 2-byte and 1-byte copy units"""
    for shift, width in ((2, 6), (1, 3), (8, 24), (4, 20)):
        base = torch.randint(1, 255, (shift + 50 * width,), dtype=torch.uint8, device="cuda")
        col = base[shift:].reshape(50, width)
        _run({"mask": col}, [(0, 7), (7, 50), (10, 12)], [7, 43, 2], 43, 1, order=(1, 0, 2), mask_counts=False)


def test_a_bad_table_touches_nothing_outside():
    """rows that name chunks beyond the source, more chunks than cap, a negative start, and a cursor beyond the table: clamped, zeros staged"""
    from hhmarl_2d_amd import learner as LR
    col = torch.arange(1, 41, dtype=torch.float32, device="cuda").reshape(10, 4)
    sched = torch.tensor([(8, 30, 5, 0), (0, 10, 9, 0), (-3, 2, 1, 0)], dtype=torch.int32, device="cuda")
    big, st = _guarded_zeros((4, 4), torch.float32, fill=1)
    cursor = torch.zeros((1,), dtype=torch.int32, device="cuda")
    nv = torch.zeros((1,), dtype=torch.int32, device="cuda")
    want = {0: (8, 10), 1: (0, 4), 2: (0, 2), 3: (0, 0), -1: (0, 0)}
    for cur, (s0, s1) in want.items():
        cursor.fill_(cur)
        LR.minibatch_stage([col], [st], 1, sched, cursor, nv)
        ref = TR.stage_ref(col.cpu().numpy(), 4, (s0, s1, 0, 0))
        assert st.cpu().numpy().tobytes() == ref.tobytes() and _intact(big, st)
    assert int(nv.item()) == 0


def test_refused_arguments_enqueue_nothing():
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    lib = L.lib()
    col = torch.ones((10, 4), dtype=torch.float32, device="cuda")
    st = torch.full((4, 4), 3.0, dtype=torch.float32, device="cuda")
    sched = torch.tensor([(0, 4, 4, 0)], dtype=torch.int32, device="cuda")
    cursor = torch.zeros((1,), dtype=torch.int32, device="cuda")
    nv = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def desc(**kw):
        d = (L.HHStageCol * 1)()
        d[0].src, d[0].dst, d[0].chunk_bytes = col.data_ptr(), st.data_ptr(), 16
        for k, val in kw.items():
            setattr(d[0], k, val)
        return d
    good = dict(n_cols=1, cols=desc(), L=1, cap=4, src=10, sched=ptr(sched), rows=1, cursor=ptr(cursor), nv=ptr(nv))
    call = lambda **kw: lib.hh_minibatch_stage(*{**good, **kw}.values(), stream)
    E = -1      # HH_E_ARG
    for bad in (dict(cols=None), dict(sched=None), dict(cursor=None), dict(nv=None), dict(n_cols=-1), dict(n_cols=9), dict(cap=0), dict(L=0),
                dict(src=-1), dict(rows=-1), dict(cols=desc(src=None)), dict(cols=desc(dst=None)), dict(cols=desc(chunk_bytes=0)),
                dict(cols=desc(chunk_bytes=16), L=3)):
        assert call(**bad) == E, bad
    assert call(n_cols=0, cols=None) == 0            # no column: success, no launch
    torch.cuda.synchronize()
    assert bool((st == 3.0).all()) and int(nv.item()) == -5 and int(cursor.item()) == 0
    with pytest.raises(ValueError):
        LR.minibatch_stage([col], [st.double()], 1, sched, cursor, nv)
    with pytest.raises(ValueError):
        LR.minibatch_stage([col], [st], 1, sched.long(), cursor, nv)
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((st == 1.0).all()) and int(nv.item()) == 4
