"""learner.minibatch_stage_gather (hh_minibatch_stage_gather) on the MI355X: bitwise equality with the restatement of tests/shuffle_ref.py
for a fight batch (chunks of 20, staged large -> small, so stale chunks must vanish), an escape batch (rows, one- and four-byte chunks),
every copy unit, chunks of thousands of bytes, a staging buffer beyond one grid sweep, and tables that name what does not exist: those
are clamped or zeroed by contract, and the sentinel guards around every staging buffer stay intact."""
import ctypes as C

import numpy as np
import pytest
import torch

import shuffle_ref as SR

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def _guarded(shape, dtype, fill=1):
    """a staging buffer inside a byte allocation filled with SENTINEL: 64 guard bytes on either side (alignment kept)"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    big = torch.full((n + 128,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = big[64:64 + n].view(dtype).reshape(shape)
    view.fill_(fill)
    return big, view


def _intact(big, view):
    n = view.numel() * view.element_size()
    return bool((big[:64] == SENTINEL).all() and (big[64 + n:] == SENTINEL).all())


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def _run(cols, order, sched, cap, chunk_len, visits, src_chunks=None, order_len=None):
    """stage the schedule rows `visits` in turn into guarded buffers that start full of ones; after each launch every column equals the
    restatement byte for byte, n_valid is the row's, the cursor and both tables are untouched and the guards are intact"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import _lib as L
    names = list(cols)
    d_order = _i32(order)
    d_sched = _i32(sched).reshape(-1, 4)
    staged = {k: _guarded((cap,) + tuple(cols[k].shape[1:]), cols[k].dtype) for k in names}
    cursor, nv_out = _i32([0]), _i32([-1])
    host = {k: cols[k].cpu().numpy() for k in names}
    for cur in visits:
        cursor.fill_(cur)
        if order_len is None:
            LR.minibatch_stage_gather([cols[k] for k in names], [staged[k][1] for k in names], chunk_len, d_order, d_sched, cursor, nv_out,
                                      src_chunks=src_chunks)
        else:       # an order_len below the table's own length: the C entry point itself (the wrapper passes the tensor's length)
            desc = (L.HHStageCol * len(names))()
            for i, k in enumerate(names):
                desc[i].src, desc[i].dst, desc[i].chunk_bytes = cols[k].data_ptr(), staged[k][1].data_ptr(), cols[k][0].numel() * cols[k].element_size()
            ptr = lambda x: C.c_void_p(x.data_ptr())
            L.check(L.lib().hh_minibatch_stage_gather(len(names), desc, chunk_len, cap, cols[names[0]].shape[0] if src_chunks is None else src_chunks,
                                                      ptr(d_order), order_len, ptr(d_sched), d_sched.shape[0], ptr(cursor), ptr(nv_out),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        for k in names:
            want, nv = SR.stage_gather_ref(host[k], cap, order, sched, cur, src_chunks=src_chunks, order_len=order_len)
            got = staged[k][1].cpu().numpy()
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (cur, k)
            assert _intact(*staged[k]), (cur, k)
        assert int(nv_out.item()) == nv and int(cursor.item()) == cur
    assert d_order.cpu().tolist() == list(order) and d_sched.cpu().tolist() == [list(r) for r in sched]
    return {k: v[1] for k, v in staged.items()}


@pytest.fixture(scope="module")
def fight():
    """37 ragged chunks of 20 in the eight columns of a Fight1 policy batch; chunk 0 carries a NaN"""
    from hhmarl_2d_amd import learner as LR
    S, Lc = 37, 20
    g = torch.Generator().manual_seed(4)
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


def _fight_sched(order, seq_len):
    """minibatches of 16, 15, 5, 1 chunks over the 37 positions; visited 16, 15, 5, 1, 16"""
    bounds = [(0, 16), (16, 31), (31, 36), (36, 37)]
    return [(o0, o1, int(sum(seq_len[c] for c in order[o0:o1])), 0) for o0, o1 in bounds]


@pytest.mark.parametrize("how", ("permutation", "reversed", "repeated", "identity"))
def test_fight_batch_large_to_small(fight, how):
    from hhmarl_2d_amd import learner as LR
    cols, seq_len = fight
    assert len(cols) == 8
    S = 37
    order = {"permutation": np.random.default_rng(8).permutation(S).tolist(), "reversed": list(range(S - 1, -1, -1)),
             "repeated": [0, 5, 5, 0, 36, 5] * 6 + [0], "identity": list(range(S))}[how]
    sched = _fight_sched(order, seq_len)
    staged = _run(cols, order, sched, 16, 20, visits=(0, 1, 2, 3, 0))
    # every position is visited, so the NaN chunk is staged in some launch and must be gone in the next (the byte comparison sees both)
    assert int(staged["mask"].sum()) == sched[0][2] and bool(torch.isnan(staged["obs"]).any()) == (0 in order[:16])
    if how == "identity":      # the same bytes as the contiguous stage for the same ranges
        cursor, nv = _i32([0]), _i32([0])
        for i, row in enumerate(sched):
            st_a = {k: torch.ones((16,) + tuple(c.shape[1:]), dtype=c.dtype, device="cuda") for k, c in cols.items()}
            st_b = {k: torch.ones_like(v) for k, v in st_a.items()}
            cursor.fill_(i)
            LR.minibatch_stage(list(cols.values()), list(st_a.values()), 20, _i32(sched), cursor, nv)
            LR.minibatch_stage_gather(list(cols.values()), list(st_b.values()), 20, _i32(order), _i32(sched), cursor, nv)
            for k in cols:
                assert st_a[k].cpu().numpy().tobytes() == st_b[k].cpu().numpy().tobytes(), (i, k)


def test_escape_batch_of_rows():
    """1000 rows, chunk_len = 1, cap = 256: the mask moves one byte per chunk, old_logp / adv / target four"""
    g = torch.Generator().manual_seed(6)
    R = 1000
    cols = {"obs": torch.randn((R, 30), generator=g), "critic": torch.randn((R, 66), generator=g),
            "actions": torch.randint(0, 9, (R, 4), generator=g).to(torch.int8), "old_logp": torch.randn((R,), generator=g),
            "adv": torch.randn((R,), generator=g), "target": torch.randn((R,), generator=g), "old_logits": torch.randn((R, 32), generator=g),
            "mask": torch.randint(1, 255, (R,), generator=g).to(torch.uint8)}
    cols = {k: v.cuda() for k, v in cols.items()}
    order = np.random.default_rng(2).permutation(R).tolist()
    sched = [(0, 256, 256, 0), (256, 512, 256, 0), (512, 768, 256, 0), (768, 1000, 232, 0)]
    _run(cols, order, sched, 256, 1, visits=(0, 3, 1, 2, 3))


def test_every_copy_unit():
    """source bases 1, 2, 4, 8 bytes into their allocation and chunks of 3, 6, 20, 24 bytes: the 1-, 2-, 4- and 8-byte units (16 elsewhere)"""
    order = np.random.default_rng(3).permutation(50).tolist()
    for shift, width in ((1, 3), (2, 6), (4, 20), (8, 24), (1, 24), (2, 20), (4, 6)):
        base = torch.randint(1, 255, (shift + 50 * width,), dtype=torch.uint8, device="cuda")
        col = base[shift:].reshape(50, width)
        _run({"x": col}, order, [(0, 7, 7, 0), (7, 50, 43, 0), (10, 12, 2, 0)], 43, 1, visits=(1, 0, 2))


def test_edges():
    col = torch.arange(1, 13, dtype=torch.float32, device="cuda").reshape(1, 12)
    _run({"x": col}, [0], [(0, 1, 1, 0)], 1, 1, visits=(0,))                                   # S = 1, cap = 1
    _run({"x": col}, [0, 0, 0], [(0, 3, 3, 0), (1, 2, 1, 0)], 5, 1, visits=(0, 1))              # S = 1 staged three times
    col = torch.arange(1, 41, dtype=torch.float32, device="cuda").reshape(10, 4)
    _run({"x": col}, [3, 9, 0], [(0, 1, 1, 0), (1, 3, 2, 0)], 1, 1, visits=(0, 1, 0))           # cap = 1: the second row is cut to one chunk
    _run({"x": col}, [3, 9, 0], [(0, 3, 3, 0)], 4, 1, visits=(0,), order_len=0)                 # order_len = 0: nothing is read, zeros staged
    _run({"x": col}, [3, 9, 0, 6, 7], [(0, 5, 5, 0)], 6, 1, visits=(0,), src_chunks=7)          # chunks 9 and 7 lie beyond src_chunks


def test_a_chunk_of_5280_bytes():
    g = torch.Generator().manual_seed(12)
    col = torch.randn((23, 20, 66), generator=g).cuda()
    assert col[0].numel() * 4 == 5280
    _run({"critic": col}, np.random.default_rng(4).permutation(23).tolist(), [(0, 9, 9, 0), (9, 23, 14, 0)], 14, 20, visits=(1, 0))


def test_a_staging_buffer_beyond_one_grid_sweep():
    """cap = 4096 chunks of 2560 bytes: 4096 groups of 64 lanes are more than the grid's 512 workgroups hold, so slots stride"""
    g = torch.Generator().manual_seed(13)
    col = torch.randn((4200, 20, 32), generator=g).cuda()
    assert col[0].numel() * 4 == 2560
    order = np.random.default_rng(5).permutation(4200).tolist()
    _run({"old_logits": col}, order, [(0, 4096, 4096, 0), (4096, 4200, 104, 0)], 4096, 20, visits=(0, 1))


def test_bad_tables_touch_nothing_outside():
    """order entries that name no chunk give a zero chunk between intact neighbours; schedule rows beyond the order table, larger than cap
    or with a negative start are clamped; a cursor outside the table stages the empty minibatch"""
    col = torch.arange(1, 41, dtype=torch.float32, device="cuda").reshape(10, 4)
    wide = torch.arange(1, 10 * 330 * 4 + 1, dtype=torch.float32, device="cuda").reshape(10, 20, 66)
    order = [2, -1, 3, 10, 4, I32_MAX, 5, I32_MIN, 6]
    sched = [(0, 9, 5, 0), (4, 30, 5, 0), (0, 9, 9, 0), (-3, 2, 1, 0), (7, 3, 2, 0), (I32_MAX - 1, I32_MAX, 1, 0), (I32_MIN, I32_MAX, 1, 0)]
    for cols, chunk_len in (({"x": col}, 1), ({"x": wide}, 20)):
        st = _run(cols, order, sched, 9, chunk_len, visits=(0,))["x"]
        flat = st.reshape(9, -1)
        assert [bool(flat[i].any()) for i in range(9)] == [True, False] * 4 + [True], "zero chunks between intact neighbours"
        _run(cols, order, sched, 4, chunk_len, visits=(0, 1, 2, 3, 4, 5, 6, 7, -1, len(sched), I32_MAX, I32_MIN))


def test_refused_arguments_enqueue_nothing():
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    lib = L.lib()
    col = torch.ones((10, 4), dtype=torch.float32, device="cuda")
    st = torch.full((4, 4), 3.0, dtype=torch.float32, device="cuda")
    order, sched = _i32([1, 2, 3, 4]), _i32([(0, 4, 4, 0)])
    cursor, nv = _i32([0]), _i32([-5])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def desc(**kw):
        d = (L.HHStageCol * 1)()
        d[0].src, d[0].dst, d[0].chunk_bytes = col.data_ptr(), st.data_ptr(), 16
        for k, val in kw.items():
            setattr(d[0], k, val)
        return d
    good = dict(n_cols=1, cols=desc(), L=1, cap=4, src=10, order=ptr(order), order_len=4, sched=ptr(sched), rows=1, cursor=ptr(cursor), nv=ptr(nv))
    call = lambda **kw: lib.hh_minibatch_stage_gather(*{**good, **kw}.values(), stream)
    E = -1      # HH_E_ARG
    for bad in (dict(order=None), dict(order_len=-1), dict(cols=None), dict(sched=None), dict(cursor=None), dict(nv=None), dict(n_cols=-1),
                dict(n_cols=9), dict(cap=0), dict(L=0), dict(src=-1), dict(rows=-1), dict(cols=desc(src=None)), dict(cols=desc(dst=None)),
                dict(cols=desc(chunk_bytes=0)), dict(cols=desc(chunk_bytes=16), L=3)):
        assert call(**bad) == E, bad
        assert b"hh_minibatch_stage_gather" in lib.hh_last_error()
    assert call(n_cols=0, cols=None) == 0            # no column: success, no launch
    torch.cuda.synchronize()
    assert bool((st == 3.0).all()) and int(nv.item()) == -5 and int(cursor.item()) == 0
    for kw in (dict(staged=[st.double()]), dict(sched=sched.long()), dict(order=order.long()), dict(order=order.reshape(2, 2)), dict(order=order.cpu()),
               dict(order=order[:0]), dict(src_chunks=11)):
        a = {**dict(cols=[col], staged=[st], order=order, sched=sched, src_chunks=None), **kw}
        with pytest.raises(ValueError, match="minibatch_stage_gather"):
            LR.minibatch_stage_gather(a["cols"], a["staged"], 1, a["order"], a["sched"], cursor, nv, src_chunks=a["src_chunks"])
    torch.cuda.synchronize()
    assert bool((st == 3.0).all()) and int(nv.item()) == -5
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((st == 1.0).all()) and int(nv.item()) == 4
