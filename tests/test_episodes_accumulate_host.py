"""train_batch_size (accumulated whole-episode batches) without a GPU: the host restatement of the accumulation
(tests/episodes_accumulate_ref.py) on hand-built done patterns, the keyword on both batches and both rollouts, the capacity formulas,
the exports and bindings of hh_episodes_emit_append / hh_commander_episodes_emit_append, and their argument checks through ctypes (they
fail before any launch, so no GPU is needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from episodes_accumulate_ref import accumulate, batch_keys, with_tables
from episodes_ref import restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from hhmarl_2d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _collect(T, N, done_rows, tick0, with_state=False):
    """one hand-built collect, one agent: done_rows = {arena: [ticks]}; obs encodes where a row came from (absolute tick + 100 arena),
    state_in (sequences) the same number"""
    done = np.zeros((T, N), dtype=np.uint8)
    for n, ts in done_rows.items():
        done[ts, n] = 1
    origin = (tick0 + np.arange(T, dtype=np.float32))[:, None] + 100 * np.arange(N, dtype=np.float32)[None, :]
    c = {"obs": np.broadcast_to(origin[:, :, None, None], (T, N, 1, 2)).copy(), "actions": np.zeros((T, N, 1), dtype=np.int8),
         "logp": -np.ones((T, N, 1), dtype=np.float32), "vf": np.zeros((T, N, 1), dtype=np.float32),
         "reward": np.ones((T, N, 1), dtype=np.float32), "valid": np.ones((T, N, 1), dtype=np.uint8), "done": done}
    if with_state:
        c["state_in"] = np.broadcast_to(origin[:, :, None, None, None], (T, N, 1, 2, 3)).copy()
    return c


# four collects of T = 3 ticks, two arenas: arena 0 ends episodes on ticks 0, 3 and 11 (1, 3 and 8 rows), arena 1 on ticks 5 and 11 (6 and
# 6 rows).  Rows emitted per collect: 1, then 3 + 6 = 9, then 0 (no done), then 8 + 6 = 14
DONES = [{0: [0]}, {0: [0], 1: [2]}, {}, {0: [2], 1: [2]}]


def _batches(max_seq_len=None):
    collects = [_collect(3, 2, d, 3 * i, with_state=max_seq_len is not None) for i, d in enumerate(DONES)]
    return restate(collects, max_seq_len, gamma=0.5, lam=0.5)[0]


def test_tables_derived_from_the_columns_are_the_restatements():
    """restate gives the episode table only with sequences: with_tables derives the same one from the t / done / arena columns"""
    for got, want in zip(_batches(), _batches(2)):
        assert "ep_start" not in got
        t = with_tables(got)
        for k in ("ep_start", "ep_len", "ep_arena"):
            assert t[k].dtype == np.int32 and np.array_equal(t[k], want[k]), k


def test_accumulation_without_a_restart_is_the_shifted_concatenation():
    """B = 100 is never reached.  Rows per collect 1, 9, 0, 14: arena 0 ends episodes of 1, 3 and 8 rows (ticks 0; 1..3; 4..11), arena 1 of
    6 and 6 (ticks 0..5; 6..11).  Collect 3 emits arena 0's 8 rows, then arena 1's 6."""
    out = accumulate(_batches(), 100)
    rows = [a[0] for _, a, _ in out]
    assert rows == [1, 10, 10, 24]
    assert [tuple(c) for _, _, c in out] == [(1, 1, 0), (9, 2, 0), (0, 0, 0), (14, 2, 0)]
    assert [a.tolist() for _, a, _ in out] == [[1, 1, 0, 0, 0, 1, 0, 0], [10, 3, 0, 0, 0, 2, 0, 0], [10, 3, 0, 0, 0, 3, 0, 0],
                                               [24, 5, 0, 0, 0, 4, 0, 0]]
    b = out[-1][0]
    assert set(b) == set(batch_keys(False))
    assert np.array_equal(b["ep_start"], [0, 1, 4, 10, 18]) and np.array_equal(b["ep_len"], [1, 3, 6, 8, 6])
    assert np.array_equal(b["ep_arena"], [0, 0, 1, 0, 1])
    assert np.array_equal(b["arena"], [0] * 4 + [1] * 6 + [0] * 8 + [1] * 6)
    assert np.array_equal(b["episode"], [0] + [1] * 3 + [0] * 6 + [2] * 8 + [1] * 6)
    assert np.array_equal(b["obs"][:, 0, 0], [0, 1, 2, 3] + [100 + t for t in range(6)] + list(range(4, 12)) + [100 + t for t in range(6, 12)])
    assert np.array_equal(np.nonzero(b["done"])[0] + 1, b["ep_start"] + b["ep_len"])
    # an emission that adds nothing leaves the batch as it was
    for k in b:
        assert out[2][0][k].tobytes() == out[1][0][k].tobytes(), k


def test_accumulation_starts_over_after_a_collect_that_reached_b():
    """B = 10: collects 0 + 1 make 10 rows (complete); collect 2 starts the next batch and emits nothing; collect 3 adds 14 rows to it.
    B = 1: every collect with a row completes its batch; the empty collect 2 opens one that collect 3 goes on filling."""
    out = accumulate(_batches(), 10)
    assert [a.tolist() for _, a, _ in out] == [[1, 1, 0, 0, 0, 1, 0, 0], [10, 3, 0, 0, 1, 2, 0, 0], [0, 0, 0, 0, 0, 1, 1, 0],
                                               [14, 2, 0, 0, 1, 2, 1, 0]]
    last = with_tables(_batches()[3])
    for k in out[3][0]:
        assert out[3][0][k].tobytes() == last[k].tobytes(), k
    assert len(out[2][0]["t"]) == 0 and out[2][0]["obs"].shape == (0, 1, 2)
    one = accumulate(_batches(), 1)
    assert [a.tolist() for _, a, _ in one] == [[1, 1, 0, 0, 1, 1, 0, 0], [9, 2, 0, 0, 1, 1, 1, 0], [0, 0, 0, 0, 0, 1, 2, 0],
                                               [14, 2, 0, 0, 1, 2, 2, 0]]
    for (b, _, _), per in zip(one, _batches()):
        per = with_tables(per)
        for k in b:
            assert b[k].tobytes() == per[k].tobytes(), k


def test_accumulated_sequence_table_points_into_the_accumulated_batch():
    """L = 2: episodes of 1, 3, 6, 8, 6 rows have 1, 2, 3, 4, 3 sequences; seq_start is shifted by the rows, seq_ep by the episodes"""
    out = accumulate(_batches(2), 100)
    b, acc, counts = out[-1]
    assert set(b) == set(batch_keys(True)) and acc.tolist() == [24, 5, 0, 13, 0, 4, 0, 0] and counts == (14, 2, 7)
    assert np.array_equal(b["seq_ep"], [0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4])
    assert np.array_equal(b["seq_start"], [0, 1, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22])
    assert np.array_equal(b["seq_len"], [1, 2, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2])
    # a sequence's state is that of its first row
    assert np.array_equal(b["state_in"][:, 0, 0, 0], b["obs"][b["seq_start"], 0, 0])
    assert np.array_equal(b["ep_start"][b["seq_ep"]] <= b["seq_start"], np.ones(13, dtype=bool))


def test_capacities_clamp_the_accumulator_and_set_the_flag():
    out = accumulate(_batches(2), 100, caps=(23, 5, 13))
    assert [a[2] for _, a, _ in out] == [0, 0, 0, 1] and out[-1][1].tolist() == [23, 5, 1, 13, 0, 4, 0, 0] and out[-1][2] == (13, 2, 7)
    out = accumulate(_batches(2), 100, caps=(24, 5, 12))
    assert out[-1][1].tolist() == [24, 5, 1, 12, 0, 4, 0, 0] and out[-1][2] == (14, 2, 6)
    assert accumulate(_batches(2), 100, caps=(24, 5, 13))[-1][1][2] == 0


def test_capacity_formulas():
    from hhmarl_2d_amd.commander import CommanderEpisodeBatch as CB
    from hhmarl_2d_amd.rollout import EpisodeBatch as EB
    N, T, cap, sl = 300, 5, 11, 4
    assert EB.capacities(N, T, cap) == (N * (cap + T), N * T)
    assert EB.capacities(N, T, cap, 1) == (N * (cap + T), N * T), "B = 1: the capacities of a batch that is overwritten"
    for B in (2, 777, 1 << 20):
        assert EB.capacities(N, T, cap, B) == (B - 1 + N * (cap + T), B - 1 + N * T)
        assert CB.capacities(N, T, cap, B, sl) == (B - 1 + N * (cap + T), B - 1 + N * T, B - 1 + N * (T + cap // sl))
        assert CB.capacities(N, T, cap, B, sl, seq_cap=N * (T + cap // sl) + 5)[2] == N * (T + cap // sl) + 5
    assert CB.capacities(N, T, cap, None, sl) == (N * (cap + T), N * T, N * (T + cap // sl))
    assert CB.capacities(N, T, cap, 9) == EB.capacities(N, T, cap, 9)
    # at or above 2^31
    big = (1 << 31) - N * (cap + T)
    assert EB.capacities(N, T, cap, big)[0] == (1 << 31) - 1
    for f in (lambda: EB.capacities(N, T, cap, big + 1), lambda: CB.capacities(N, T, cap, big + 1, sl),
              lambda: CB.capacities(N, T, cap, 10, sl, seq_cap=1 << 31)):
        with pytest.raises(ValueError, match="2\\^31"):
            f()
    # seq_cap: below the floor of one collect, not an int, or without train_batch_size
    for bad in (N * (T + cap // sl) - 1, 0, -1, 2.0e4, "9", True):
        with pytest.raises(ValueError, match="seq_cap"):
            CB.capacities(N, T, cap, 10, sl, seq_cap=bad)
    with pytest.raises(ValueError, match="seq_cap"):
        CB.capacities(N, T, cap, None, sl, seq_cap=N * (T + cap // sl))


def test_bad_values_are_refused_by_both_batches():
    import torch
    from hhmarl_2d_amd.commander import CommanderEpisodeBatch as CB
    from hhmarl_2d_amd.rollout import EpisodeBatch as EB
    assert EB.check_train_batch_size(None) is None and EB.check_train_batch_size(1) == 1 and EB.check_train_batch_size(4096) == 4096
    bad = (0, -1, 1.0, 2.5, "64", True, False, (64,), [64])
    for b in bad:
        with pytest.raises(ValueError, match="train_batch_size"):
            EB.check_train_batch_size(b)
    # the constructors refuse before they allocate or load anything: host tensors stand in for the collect
    T, N = 5, 3
    col = lambda *shape, dt=torch.float32: torch.zeros((T, N) + shape, dtype=dt)
    for cls, nA, D, act, extra in ((EB, 2, 26, (4,), ()), (CB, 3, 34, (), (4,))):
        collect = {"obs": col(nA, D), "actions": col(nA, *act, dt=torch.int8), "logp": col(nA), "vf": col(nA), "reward": col(nA),
                   "valid": col(nA, dt=torch.uint8), "done": col(dt=torch.uint8), "state_in": col(nA, 2, 200)}
        args = (collect,) + extra + (11, 0.99, 0.95)
        for b in bad:
            with pytest.raises(ValueError, match="train_batch_size"):
                cls(*args, train_batch_size=b)
        with pytest.raises(ValueError, match="2\\^31"):
            cls(*args, train_batch_size=1 << 31)
    for p in (inspect.signature(EB.__init__).parameters, inspect.signature(CB.__init__).parameters):
        assert p["train_batch_size"].default is None
    assert inspect.signature(CB.__init__).parameters["seq_cap"].default is None
    assert "seq_cap" not in inspect.signature(EB.__init__).parameters


def test_keyword_of_both_rollouts():
    from hhmarl_2d_amd.commander import CommanderRollout
    from hhmarl_2d_amd.rollout import PPORollout
    for cls in (PPORollout, CommanderRollout):
        p = inspect.signature(cls.__init__).parameters
        names = list(p)
        assert p["train_batch_size"].default is None
        assert names[-1] == "record_logits" and names[-2] == "train_batch_size", "in front of record_logits, which stays last"
        assert callable(getattr(cls, "collect_batch"))
        assert list(inspect.signature(cls.collect_batch).parameters) == ["self", "max_collects"]
    # refused without complete_episodes, and bad values, before the world is looked at
    with pytest.raises(ValueError, match="train_batch_size needs batch_mode='complete_episodes'"):
        PPORollout(None, None, 8, train_batch_size=64)
    with pytest.raises(ValueError, match="train_batch_size needs batch_mode='complete_episodes'"):
        PPORollout(None, None, 8, batch_mode="truncate_episodes", train_batch_size=64)
    with pytest.raises(ValueError, match="train_batch_size needs batch_mode='complete_episodes'"):
        CommanderRollout(None, None, None, 8, train_batch_size=64)
    for bad in (0, -3, 1.5, "64", True):
        with pytest.raises(ValueError, match="train_batch_size"):
            PPORollout(None, None, 8, batch_mode="complete_episodes", train_batch_size=bad)
        with pytest.raises(ValueError, match="train_batch_size"):
            CommanderRollout(None, None, None, 8, batch_mode="complete_episodes", train_batch_size=bad)
    with pytest.raises(ValueError, match="batch_mode"):           # the earlier checks still come first
        PPORollout(None, None, 8, batch_mode="whole", train_batch_size=64)


def test_entry_points_are_declared_exported_and_bound():
    _l = _lib()
    so = C.CDLL(_l.LIB_PATH)
    abi = open(os.path.join(ROOT, "include", "hh_abi.h")).read()
    cmd = open(os.path.join(ROOT, "include", "hh_commander.h")).read()
    ws = lambda s: re.sub(r"\s+", " ", s)
    assert ("int hh_episodes_emit_append(const hh_episode_bufs *b, const hh_episode_aux *x, int64_t train_rows, int32_t *acc, "
            "int64_t *totals, void *stream);") in ws(abi)
    assert ("int hh_commander_episodes_emit_append(const hh_commander_episode_bufs *b, const struct hh_episode_aux *x, int64_t train_rows, "
            "int32_t *acc, int64_t *totals, void *stream);") in ws(cmd)
    assert int(re.search(r"#define HH_EP_ACC (\d+)", abi).group(1)) == len(_l.EP_ACC) == 8
    assert _l.EP_ACC[:7] == ("rows", "episodes", "overflow", "sequences", "complete", "collects", "batches")
    assert hasattr(so, "hh_episodes_emit_append") and hasattr(so, "hh_commander_episodes_emit_append")
    assert "hh_episodes_emit_append" in _l.EXPORTS and "hh_commander_episodes_emit_append" in _l.COMMANDER_EXPORTS
    assert "hh_commander_episodes_emit_append" not in _l.EXPORTS
    lib = _l.lib()
    vp = C.c_void_p
    assert lib.hh_episodes_emit_append.argtypes == [C.POINTER(_l.HHEpisodeBufs), C.POINTER(_l.HHEpisodeAux), C.c_int64, vp, vp, vp]
    assert lib.hh_commander_episodes_emit_append.argtypes == [C.POINTER(_l.HHCommanderEpisodeBufs), C.POINTER(_l.HHEpisodeAux), C.c_int64,
                                                              vp, vp, vp]


def _fill_pointers(b, value=0x10000):
    """every pointer field a non-null, 16-byte aligned dummy: the checks under test all fail before any launch reads them"""
    for name, ct in b._fields_:
        if ct is C.c_void_p:
            setattr(b, name, value)


def _append_errors(_l, name, call):
    """the append checks of one entry point on a struct that passes its own; call(x, train_rows, acc, totals) -> rc"""
    err = lambda: _l.lib().hh_last_error()
    ok = 0x10000
    for B in (0, -1, -(1 << 40)):
        assert call(None, B, ok, None) == -1 and err().startswith(name + b": ") and b"train_rows" in err(), B
    assert call(None, 1, None, None) == -1 and b"null acc" in err()
    for off in (1, 2, 3):
        assert call(None, 1, ok + off, None) == -1 and b"acc must be 4-byte aligned" in err(), off
    for off in (1, 2, 4, 6):
        assert call(None, 1, ok, ok + off) == -1 and b"totals must be 8-byte aligned" in err(), off
    # with a valid accumulator the aux column's checks are those of the _aux entry points
    x = _l.HHEpisodeAux(aux_dim=0, reserved0=0, aux=ok, c_aux=ok, o_aux=ok)
    assert call(C.byref(x), 1, ok, ok) == -1 and b"aux_dim" in err()
    x.aux_dim, x.reserved0 = 4, 1
    assert call(C.byref(x), 1, ok, None) == -1 and b"reserved0" in err()
    x.reserved0, x.c_aux = 0, None
    assert call(C.byref(x), 1, ok, None) == -1 and b"null aux buffer" in err()


def test_append_argument_checks_fail_before_any_launch():
    _l = _lib()
    f = _l.lib().hh_episodes_emit_append
    b = _l.HHEpisodeBufs()
    assert f(None, None, 1, 0x10000, None, None) == -1
    assert f(C.byref(b), None, 1, 0x10000, None, None) == -1 and b"hh_episodes_emit_append: bad sizes" in _l.lib().hh_last_error()
    b.T, b.N, b.n_agents, b.obs_dim, b.carry_cap, b.row_cap, b.ep_cap = 5, 3, 3, 34, 11, 3 * 16 + 9, 3 * 5 + 9
    assert f(C.byref(b), None, 1, 0x10000, None, None) == -1 and b"null buffer" in _l.lib().hh_last_error()   # the struct's own checks first
    assert f(C.byref(b), None, 0, None, None, None) == -1 and b"null buffer" in _l.lib().hh_last_error()
    b.row_cap = 1 << 31
    assert f(C.byref(b), None, 1, 0x10000, None, None) == -1 and b"2^31" in _l.lib().hh_last_error()
    b.row_cap = 3 * 16 + 9
    _fill_pointers(b)
    _append_errors(_l, b"hh_episodes_emit_append", lambda x, B, acc, tot: f(C.byref(b), x, B, acc, tot, None))


def test_commander_append_argument_checks_fail_before_any_launch():
    _l = _lib()
    f = _l.lib().hh_commander_episodes_emit_append
    b = _l.HHCommanderEpisodeBufs()
    assert f(C.byref(b), None, 1, 0x10000, None, None) == -1
    assert b"hh_commander_episodes_emit_append: bad sizes" in _l.lib().hh_last_error()
    b.T, b.N, b.max_seq_len, b.carry_cap = 5, 3, 4, 11
    b.row_cap, b.ep_cap, b.seq_cap = 3 * 16 + 9, 3 * 5 + 9, 3 * (5 + 2) - 1
    assert f(C.byref(b), None, 1, 0x10000, None, None) == -1 and b"seq_cap >= N" in _l.lib().hh_last_error()
    b.seq_cap = 3 * (5 + 2) + 9
    assert f(C.byref(b), None, 1, 0x10000, None, None) == -1 and b"null buffer" in _l.lib().hh_last_error()
    _fill_pointers(b)
    _append_errors(_l, b"hh_commander_episodes_emit_append", lambda x, B, acc, tot: f(C.byref(b), x, B, acc, tot, None))
