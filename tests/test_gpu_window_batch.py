"""learner.window_cut / window_gather (hh_window_cut, hh_window_gather) on the MI355X against tests/window_batch_ref.py, byte for byte:
every shape at which the cut's walk, scan and write and the gather's groups and copy units take another path (one arena, a ragged last
wave, more than one workgroup; rows of 1 byte to 4800), done patterns at which a length cut and a done coincide, destinations with
guard bytes and 0xFF pre-fill, table entries that name no rows of the window, and the torch-op twins on the device."""
import numpy as np
import pytest
import torch

import window_batch_ref as WR

pytestmark = pytest.mark.gpu
TS, NS, LS = (1, 5, 20, 21, 64), (1, 63, 64, 65, 1000), (1, 4, 20, 32)
GUARD = 64


def _patterns(T, N, L, rng):
    t = np.arange(T)[:, None]
    z = np.zeros((T, N), dtype=np.uint8)
    return {"none": z, "every row": z + 1, "only T-1": z + (t == T - 1), "only 0": z + (t == 0), "every L rows": z + ((t + 1) % L == 0),
            "random 0.1": (rng.random((T, N)) < 0.1).astype(np.uint8), "random 0.5": (rng.random((T, N)) < 0.5).astype(np.uint8),
            "bytes of 255": (rng.random((T, N)) < 0.3).astype(np.uint8) * 255}


def _sources(T, N, dev, seed):
    """the columns of one launch: (name, source, tail, offset, per_seq) — widths 1, 4, 104, 228, 128, 4800 (per sequence), 408 and 4 bytes"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = lambda *shape: torch.randn(shape, generator=g).to(dev)
    return [("i8 at 1 of 2", torch.randint(-128, 128, (T, N, 2), generator=g, dtype=torch.int8).to(dev), (), 1, False),
            ("f32 of 4", f(T, N), (), 0, False),
            ("104 at 104 of 208", f(T + 1, N, 2, 26), (26,), 104, False),
            ("228", f(T, N, 57), (57,), 0, False),
            ("128 at 128 of 256", f(T, N, 2, 32), (32,), 128, False),
            ("4800 per sequence", f(T + 1, N, 3, 2, 200), (3, 2, 200), 0, True),
            ("a whole 408-byte step-row", f(T + 1, N, 3, 34), (3, 34), 0, False),
            ("4 at 4 of 8", f(T, N, 2), (), 4, False)]


def _dst(shape, dtype, dev, front):
    """a destination inside a buffer of 0xFF with guard bytes on both sides -> (buffer, view)"""
    n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((front + n + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    return buf, buf[front:front + n].view(dtype).reshape(shape)


def _gather_checked(LR, srcs, tabs_np, L, dev, T_src, fronts=None):
    """one launch of these columns into guarded 0xFF destinations, compared with the reference -> the destinations' bytes"""
    S = len(tabs_np[0])
    tabs = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in tabs_np]
    cols = [(src, tail, off, per_seq) for _, src, tail, off, per_seq in srcs]
    shapes = [((S,) if per_seq else (S, L)) + tuple(tail) for _, _, tail, _, per_seq in srcs]
    fronts = fronts or [GUARD + 4 * (i % 4) for i in range(len(srcs))]      # 16-, 4-, 8-, 4-byte aligned destinations: every copy unit
    bufs = [_dst(sh, src.dtype, dev, fr) for sh, (_, src, _, _, _), fr in zip(shapes, srcs, fronts)]
    got = LR.window_gather(cols, tabs, L, out=[v for _, v in bufs])
    torch.cuda.synchronize()
    out = []
    for (name, src, tail, off, per_seq), (buf, v), g, fr in zip(srcs, bufs, got, fronts):
        width = int(np.prod(tail, dtype=np.int64)) * src.element_size()
        want = WR.gather_ref(src.cpu().numpy(), *tabs_np, L, off, width, per_seq, T_src=T_src)
        b = buf.cpu().numpy()
        assert g.data_ptr() == v.data_ptr()
        assert (b[:fr] == 0xFF).all() and (b[len(b) - GUARD:] == 0xFF).all(), f"{name}: guard bytes"
        assert np.array_equal(b[fr:len(b) - GUARD], want.reshape(-1)), f"{name}: S {S} L {L}"
        out.append(b[fr:len(b) - GUARD])
    return out


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
def test_cut_and_gather_against_the_reference(T, N):
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng([T, N])
    srcs = _sources(T, N, dev, 7 * T + N)
    for L in LS:
        for name, done in _patterns(T, N, L, rng).items():
            want = WR.window_cut_ref(done, L)
            S = len(want[0])
            out = tuple(torch.full((T * N + 3,), -7, dtype=torch.int32, device=dev) for _ in range(3))
            d = torch.from_numpy(done).to(dev)
            got = LR.window_cut(d, L, out=out)
            twin = LR.window_cut_torch(d, L)
            for g, o, w, tw in zip(got, out, want, twin):
                assert g.dtype == torch.int32 and g.shape == (S,) and g.data_ptr() == o.data_ptr()
                assert np.array_equal(g.cpu().numpy(), w), f"{name}: T {T} N {N} L {L}"
                assert (o[S:] == -7).all().item(), f"{name}: entries at and beyond n_seq keep the sentinel"
                assert torch.equal(tw, g)
            if name in ("random 0.1", "every L rows"):
                first = _gather_checked(LR, srcs, want, L, dev, T)
                if name == "random 0.1":
                    again = _gather_checked(LR, srcs, want, L, dev, T)
                    assert all(np.array_equal(a, b) for a, b in zip(first, again)), "calling twice gives the same bytes"
                    _gather_checked(LR, srcs[2:3], want, L, dev, T + 1)                     # one column in one launch
                    tabs = [t.to(dev) for t in (torch.from_numpy(x) for x in want)]
                    cols = [(src, tail, off, per_seq) for _, src, tail, off, per_seq in srcs]
                    for a, b in zip(LR.window_gather(cols, tabs, L), LR.window_gather_torch(cols, tabs, L)):
                        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("T,N,L", [(21, 65, 4), (5, 1, 32), (64, 63, 20)])
def test_entries_that_name_no_rows_stage_zeros(T, N, L):
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng([T, N, L])
    done = (rng.random((T, N)) < 0.2).astype(np.uint8)
    good = WR.window_cut_ref(done, L)
    # the window's own entries, then entries that name no rows (or, the last two, the row behind the window, which a T+1-row source holds)
    extra = [(-1, 0, 1), (0, 0, L + 1), (0, N, 1), (0, -1, 1), (T, 0, 1), (T - 1, 0, 2), (0, 0, -1), (2 ** 31 - 1, N - 1, 1), (-2 ** 31, 0, L), (0, 0, 0)]
    tabs = [np.concatenate([g, np.asarray([e[i] for e in extra], dtype=np.int32)]) for i, g in enumerate(good)]
    srcs = _sources(T, N, dev, 5)
    _gather_checked(LR, srcs, tabs, L, dev, T)                                     # T_src = T: (T, 0, 1) and (T - 1, 0, 2) give zeros
    tall = [s for s in srcs if s[1].shape[0] == T + 1]
    out = _gather_checked(LR, tall, tabs, L, dev, T + 1)                           # T_src = T + 1: both read row T
    S, w = len(tabs[0]), 104
    rows = out[0].reshape(S, L, w)
    assert np.array_equal(rows[len(good[0]) + 4, 0], tall[0][1][T, 0].cpu().numpy().view(np.uint8).reshape(-1)[104:208]) and not rows[len(good[0]) + 4, 1:].any()
    if L >= 2:
        assert rows[len(good[0]) + 5, 1].any() and not rows[len(good[0]) + 5, 2:].any()
    assert not rows[len(good[0]):len(good[0]) + 4].any() and not rows[len(good[0]) + 6:].any()


def test_c_layer_refusals_enqueue_nothing():
    import ctypes as C
    from hhmarl_2d_amd import _lib as L
    dev = torch.device("cuda", 0)
    lib = L.lib()
    T, N = 4, 3
    done = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    tabs = [torch.full((T * N,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    small = torch.full((N + 1,), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    good = dict(T=T, N=N, done=p(done), L=4, t0=p(tabs[0]), ar=p(tabs[1]), ln=p(tabs[2]), n_seq=p(small[N:]), scratch=p(small))
    for bad in (dict(T=0), dict(N=0), dict(L=0), dict(L=33), dict(done=None), dict(t0=None), dict(ar=None), dict(ln=None), dict(n_seq=None),
                dict(scratch=None), dict(T=2 ** 16, N=2 ** 15)):
        assert lib.hh_window_cut(*{**good, **bad}.values(), st) == -1 and b"hh_window_cut" in lib.hh_last_error()
    src = torch.ones((T, N, 8), dtype=torch.float32, device=dev)
    dst = torch.full((T * N, 4, 8), -7.0, dtype=torch.float32, device=dev)

    def col(**kw):
        c = (L.HHWindowCol * 1)()
        c[0].src, c[0].dst, c[0].step_bytes, c[0].offset, c[0].width, c[0].per_seq = src.data_ptr(), dst.data_ptr(), 32, 0, 32, 0
        for k, v in kw.items():
            setattr(c[0], k, v)
        return c
    call = lambda c=None, n_cols=1, S=T * N, Lm=4, T_src=T, N_=N, t0=p(tabs[0]): lib.hh_window_gather(n_cols, c or col(), S, Lm, T_src, N_, t0, p(tabs[1]), p(tabs[2]), st)
    for rc in (call(n_cols=0), call(n_cols=9), call(Lm=0), call(Lm=33), call(S=-1), call(T_src=0), call(N_=0), call(t0=None),
               call(col(src=None)), call(col(dst=None)), call(col(width=0)), call(col(width=-4)), call(col(offset=-4)), call(col(offset=4)),
               call(col(step_bytes=-32)), call(col(per_seq=2)), call(col(reserved0=1))):
        assert rc == -1 and b"hh_window_gather" in lib.hh_last_error()
    torch.cuda.synchronize()
    assert all((t == -7).all().item() for t in tabs + [small]) and (dst == -7.0).all().item(), "a refused call writes nothing"
    assert call(S=0) == 0
    torch.cuda.synchronize()
    assert (dst == -7.0).all().item()
