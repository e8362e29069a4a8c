"""hh_episodes_emit_aux / hh_commander_episodes_emit_aux on the MI355X, on synthetic collects (no world): keyed random rows with random
done flags, episodes of at most carry_cap + 1 rows, K = 4 consecutive calls of T = 5 ticks with carry_cap = 11.
  * every existing column and table is byte-equal to what the entry point without the column writes from the same inputs and fresh
    carries;
  * the aux column is byte-equal to the host restatement (tests/episodes_ref.py) run with the aux rows in place of obs: its emitted
    "obs" is the expected column — the same episodes, the same row order;
  * x = NULL is the entry point without the column; argument errors; the overflow flag covers the column."""
import ctypes as C

import numpy as np
import pytest
import torch

from episodes_ref import restate

pytestmark = pytest.mark.gpu
T, K, CAP, L_SEQ = 5, 4, 11, 4
COLS = ("obs", "actions", "logp", "vf", "reward", "valid", "adv", "target", "done", "arena", "episode", "t")
TABLES = ("ep_start", "ep_len", "ep_arena")
SEQ = ("seq_start", "seq_len", "seq_ep", "state_in")


def _stream(N, nA, D, aux_dim, act_shape, seed, with_state=False, never_done=()):
    """K T ticks of rows (numpy, [K T, N, ...]); an episode ends with probability 0.15 per tick and at the latest on its (CAP + 1)-th row;
    arenas in never_done never end one"""
    rng = np.random.default_rng(seed)
    n = K * T
    s = {"obs": rng.standard_normal((n, N, nA, D), dtype=np.float32),
         "actions": rng.integers(0, 13, (n, N, nA) + act_shape).astype(np.int8),
         "logp": -rng.random((n, N, nA), dtype=np.float32), "vf": rng.standard_normal((n, N, nA), dtype=np.float32),
         "reward": rng.standard_normal((n, N, nA), dtype=np.float32), "valid": rng.integers(0, 2, (n, N, nA)).astype(np.uint8),
         "aux": rng.standard_normal((n, N, nA, aux_dim), dtype=np.float32)}
    done = (rng.random((n, N)) < 0.15).astype(np.uint8)
    run = np.zeros(N, dtype=np.int64)
    for t in range(n):
        run += 1
        done[t, run >= CAP + 1] = 1
        done[t, list(never_done)] = 0
        run[done[t] != 0] = 0
    s["done"] = done
    if with_state:
        s["state_in"] = rng.standard_normal((n, N, nA, 2, 200), dtype=np.float32)
    return s


class _Emitter:
    """device buffers of one emitter fed from a host stream, T ticks per call; aux: record the column (the _aux entry point)"""

    def __init__(self, stream, aux, commander=False, aux_offset=0):
        from hhmarl_2d_amd.commander import CommanderEpisodeBatch
        from hhmarl_2d_amd.rollout import EpisodeBatch
        self.s = stream
        self.names = [k for k in stream if k != "aux"] + (["aux"] if aux else [])
        self.dev = {k: torch.zeros(stream[k][:T].shape, dtype=torch.from_numpy(stream[k][:1]).dtype, device="cuda") for k in self.names}
        if aux and aux_offset:      # the collect's aux rows as a view aux_offset floats into a larger tensor: a base aligned to 4 bytes only
            shape = self.dev["aux"].shape
            self._aux_store = torch.zeros(self.dev["aux"].numel() + aux_offset, dtype=torch.float32, device="cuda")
            self.dev["aux"] = self._aux_store[aux_offset:].view(shape)
            assert self.dev["aux"].data_ptr() % 16 == 4 * aux_offset and self.dev["aux"].is_contiguous()
        collect = {k: v for k, v in self.dev.items() if k != "aux"}
        a = ("aux", self.dev["aux"]) if aux else None
        self.eb = (CommanderEpisodeBatch(collect, L_SEQ, CAP, 0.99, 0.95, aux=a) if commander else EpisodeBatch(collect, CAP, 0.99, 0.95, aux=a))

    def call(self, k, entry=None, null_aux=False):
        """upload collect k, emit through `entry` (default: the batch's own path) -> the emitted parts as numpy"""
        from hhmarl_2d_amd import _lib as L
        for name in self.names:
            self.dev[name].copy_(torch.from_numpy(self.s[name][k * T:(k + 1) * T]))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if entry is None:
            self.eb.emit(st)
        else:
            x = None if null_aux else C.byref(self.eb._aux)
            L.check(getattr(L.lib(), entry)(C.byref(self.eb._bufs), x, st))
        return {k2: v.cpu().numpy() for k2, v in self.eb.rows().items()}


def _expected_aux(stream, max_seq_len=None):
    """the restatement with the aux rows in place of obs: its emitted obs, per collect"""
    cols = ("obs", "actions", "logp", "vf", "reward", "valid", "done") + (("state_in",) if max_seq_len else ())
    collects = [{k: (stream["aux"] if k == "obs" else stream[k])[c * T:(c + 1) * T] for k in cols} for c in range(K)]
    want, carried = restate(collects, max_seq_len, gamma=0.99, lam=0.95)
    return [w["obs"] for w in want], carried


@pytest.mark.parametrize("N", [3, 300, 1100])
@pytest.mark.parametrize("nA,D,aux_dim", [(2, 26, 32), (3, 34, 4), (3, 34, 3), (2, 30, 1)])
def test_aux_column_and_unchanged_columns(N, nA, D, aux_dim):
    s = _stream(N, nA, D, aux_dim, (4,), seed=1000 * N + 10 * D + aux_dim)
    with_aux, plain, null = _Emitter(s, True), _Emitter(s, False), _Emitter(s, True)
    want_aux, want_carried = _expected_aux(s)
    rows = 0
    for k in range(K):
        g = with_aux.call(k)
        p = plain.call(k)
        z = null.call(k, "hh_episodes_emit_aux", null_aux=True)
        assert set(g) == set(COLS + TABLES + ("aux",)) and set(p) == set(COLS + TABLES)
        for name in COLS + TABLES:
            assert g[name].dtype == p[name].dtype and np.array_equal(g[name], p[name]), f"call {k}: {name} differs from hh_episodes_emit"
            assert np.array_equal(z[name], p[name]), f"call {k}: {name} of an x = NULL call differs from hh_episodes_emit"
        assert g["aux"].shape == want_aux[k].shape and g["aux"].dtype == np.float32
        assert np.array_equal(g["aux"].view(np.uint32), want_aux[k].view(np.uint32)), f"call {k}: the aux column differs from the restatement"
        assert not z["aux"].any(), "an x = NULL call writes no aux column"
        rows += len(g["t"])
    assert rows > 0 and np.array_equal(with_aux.eb.carried.cpu().numpy(), want_carried)
    assert np.array_equal(plain.eb.carried.cpu().numpy(), want_carried)
    if N >= 300:
        lens = with_aux.eb.t[: int(with_aux.eb.n_rows)][with_aux.eb.done[: int(with_aux.eb.n_rows)] == 1] + 1
        assert int(lens.max()) > T, "no episode spanning calls: the aux carry is not exercised"


@pytest.mark.parametrize("N", [3, 300])
@pytest.mark.parametrize("aux_dim", [4, 3])
def test_commander_aux_column_and_unchanged_columns(N, aux_dim):
    s = _stream(N, 3, 34, aux_dim, (), seed=77 * N + aux_dim, with_state=True)
    with_aux, plain, null = _Emitter(s, True, commander=True), _Emitter(s, False, commander=True), _Emitter(s, True, commander=True)
    want_aux, want_carried = _expected_aux(s, L_SEQ)
    for k in range(K):
        g = with_aux.call(k)
        p = plain.call(k)
        z = null.call(k, "hh_commander_episodes_emit_aux", null_aux=True)
        assert set(g) == set(COLS + TABLES + SEQ + ("aux",)) and set(p) == set(COLS + TABLES + SEQ)
        for name in COLS + TABLES + SEQ:
            assert np.array_equal(g[name], p[name]), f"call {k}: {name} differs from hh_commander_episodes_emit"
            assert np.array_equal(z[name], p[name]), f"call {k}: {name} of an x = NULL call differs from hh_commander_episodes_emit"
        assert g["aux"].shape == want_aux[k].shape
        assert np.array_equal(g["aux"].view(np.uint32), want_aux[k].view(np.uint32)), f"call {k}: the aux column differs from the restatement"
        # the padded form: zero past seq_len, the rows' values before
        q = with_aux.eb.sequences()["aux"].cpu().numpy()
        assert q.shape == (len(g["seq_start"]), L_SEQ, 3, aux_dim)
        for i, (s0, n) in enumerate(zip(g["seq_start"], g["seq_len"])):
            assert np.array_equal(q[i, :n], g["aux"][s0:s0 + n]) and not q[i, n:].any()
    assert np.array_equal(with_aux.eb.carried.cpu().numpy(), want_carried)


@pytest.mark.parametrize("N", [3, 300])
def test_rows_of_a_multiple_of_16_bytes_on_a_base_aligned_to_4(N):
    """aux_dim 4 with 3 agents is a 48 B row, but the collect's column starts 4 bytes into a larger tensor: the entry point must take
    the dword instance (a dwordx4 access there would be misaligned), with the same result"""
    s = _stream(N, 3, 34, 4, (4,), seed=31 * N)
    off, aligned = _Emitter(s, True, aux_offset=1), _Emitter(s, True)
    want_aux, want_carried = _expected_aux(s)
    for k in range(K):
        g, a = off.call(k), aligned.call(k)
        for name in COLS + TABLES:
            assert np.array_equal(g[name], a[name]), f"call {k}: {name}"
        assert np.array_equal(g["aux"].view(np.uint32), want_aux[k].view(np.uint32)), f"call {k}: the aux column differs from the restatement"
    assert np.array_equal(off.eb.carried.cpu().numpy(), want_carried)
    assert not off._aux_store[:1].any(), "the float in front of the view is untouched"


def test_argument_errors_on_real_buffers():
    from hhmarl_2d_amd import _lib as L
    e = _Emitter(_stream(3, 3, 34, 3, (4,), seed=5), True)
    b, x = e.eb._bufs, e.eb._aux
    f = L.lib().hh_episodes_emit_aux
    keep = (x.aux_dim, x.aux)
    for bad in (0, 33):
        x.aux_dim = bad
        assert f(C.byref(b), C.byref(x), None) == -1 and b"aux_dim" in L.lib().hh_last_error()
    x.aux_dim, x.reserved0 = keep[0], 7
    assert f(C.byref(b), C.byref(x), None) == -1 and b"reserved0" in L.lib().hh_last_error()
    x.reserved0, x.aux = 0, None
    assert f(C.byref(b), C.byref(x), None) == -1 and b"null aux buffer" in L.lib().hh_last_error()
    x.aux = keep[1]
    torch.cuda.synchronize()
    assert int(e.eb._counts.abs().sum()) == 0 and not e.eb.aux.any(), "a refused call launches nothing"


def test_an_episode_longer_than_the_carry_sets_the_flag():
    """arena 1 never ends an episode: after three calls it wants 15 carried rows where 11 fit.  The flag is set, rows() raises, the other
    arenas' carried rows are what they should be, and the carry holds no more than carry_cap rows (the buffers stay within capacity:
    the kernel's own bound is what is under test)"""
    s = _stream(300, 3, 34, 3, (4,), seed=9, never_done=(1,))
    e = _Emitter(s, True)
    for k in range(2):
        e.call(k)                                   # 10 rows carried: still fine
    assert int(e.eb._counts[2]) == 0
    for name in e.names:
        e.dev[name].copy_(torch.from_numpy(s[name][2 * T:3 * T]))
    e.eb.emit(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(e.eb._counts[2]) == 1
    with pytest.raises(RuntimeError, match="outgrew"):
        e.eb.rows()
    carried = e.eb.carried.cpu().numpy()
    assert carried[1] == CAP and carried.max() <= CAP
    # arena 1's carry: its first CAP rows, in order, in the aux column as in obs
    assert np.array_equal(e.eb._carry["aux"][1].cpu().numpy(), s["aux"][:CAP, 1])
    assert np.array_equal(e.eb._carry["obs"][1].cpu().numpy(), s["obs"][:CAP, 1])
