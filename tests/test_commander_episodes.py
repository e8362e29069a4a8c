"""Whole-episode GRU-sequence batches of the commander (CommanderRollout batch_mode = "complete_episodes", train_hier.py:182) without a
GPU: argument validation, the C ABI of hh_commander_episodes_emit (export, binding, layout of hh_commander_episode_bufs, the capacity
checks), the default carry, and the host restatement that tests/test_gpu_commander_episodes.py compares the device's batches with,
pinned on hand-built streams of exactly representable numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from episodes_ref import pad_sequences, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from hhmarl_2d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_argument_validation_needs_no_world():
    from hhmarl_2d_amd.commander import CommanderRollout
    with pytest.raises(ValueError, match="batch_mode"):
        CommanderRollout(None, None, None, 8, batch_mode="complete")
    with pytest.raises(ValueError, match="max_seq_len"):
        CommanderRollout(None, None, None, 8, batch_mode="complete_episodes", max_seq_len=0)
    with pytest.raises(ValueError, match="carry_cap"):
        CommanderRollout(None, None, None, 8, batch_mode="complete_episodes", carry_cap=-1)


def test_emit_entry_point_is_exported_and_bound():
    _l = _lib()
    assert "hh_commander_episodes_emit" in _l.COMMANDER_EXPORTS and hasattr(C.CDLL(_l.LIB_PATH), "hh_commander_episodes_emit")
    assert _l.lib().hh_commander_episodes_emit.argtypes == [C.POINTER(_l.HHCommanderEpisodeBufs), C.c_void_p]


def test_episode_bufs_struct_layout_matches_header():
    from hhmarl_2d_amd import _lib
    txt = open(os.path.join(ROOT, "include", "hh_commander.h")).read()
    body = re.search(r"typedef struct hh_commander_episode_bufs \{(.*?)\} hh_commander_episode_bufs;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(int32_t|int64_t|double|float|int8_t|uint8_t)\s*(\*?)\s*([A-Za-z_0-9]+)\s*;", body)
    scalar = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    want = [(name, C.c_void_p if star else scalar[t]) for t, star, name in fields]
    assert len(want) == 47 and want == list(_lib.HHCommanderEpisodeBufs._fields_)
    assert C.sizeof(_lib.HHCommanderEpisodeBufs) == 4 * 4 + 3 * 8 + 2 * 8 + 38 * 8
    assert _lib.HHCommanderEpisodeBufs.gamma.offset == 40 and _lib.HHCommanderEpisodeBufs.obs.offset == 56


def test_entry_point_checks_sizes_and_capacities_before_any_launch():
    _l = _lib()
    f = _l.lib().hh_commander_episodes_emit
    b = _l.HHCommanderEpisodeBufs()
    assert f(C.byref(b), None) == -1 and b"bad sizes" in _l.lib().hh_last_error()
    b.T, b.N, b.max_seq_len, b.carry_cap = 16, 4, 20, 47
    b.row_cap, b.ep_cap, b.seq_cap = 4 * (47 + 16), 4 * 16, 4 * (16 + 2) - 1   # one sequence short of the bound
    assert f(C.byref(b), None) == -1 and b"seq_cap" in _l.lib().hh_last_error()
    b.seq_cap += 1
    assert f(C.byref(b), None) == -1 and b"null buffer" in _l.lib().hh_last_error()
    b.max_seq_len = 0
    assert f(C.byref(b), None) == -1


def test_default_carry_cap_bounds_every_unfinished_episode():
    from hhmarl_2d_amd.commander import default_carry_cap
    assert default_carry_cap(500) == 47 and default_carry_cap(500, 3, 3) == 47
    for H in range(1, 2000):
        # steps of an episode still running: kill-event steps (one death or more, both sides alive: <= 4) + others (>= 12 ticks, < H in all)
        strict = (H - 1) // 12 + 3 + 3 - 2
        assert default_carry_cap(H) >= strict + 1


def _collect(T, N, done_ticks, reward=None, vf=None, D=2, H=2):
    """one collect of hand-built values, done_ticks = {arena: [ticks]}; _stream fills in the tags of obs / actions / state_in"""
    done = np.zeros((T, N), dtype=np.uint8)
    for n, ts in done_ticks.items():
        done[ts, n] = 1
    z = np.zeros((T, N, 3), dtype=np.float32)
    return {"obs": np.zeros((T, N, 3, D), dtype=np.float32), "actions": np.zeros((T, N, 3), dtype=np.int8), "logp": -np.ones((T, N, 3), np.float32),
            "vf": z.copy() if vf is None else np.asarray(vf, np.float32), "reward": z.copy() if reward is None else np.asarray(reward, np.float32),
            "valid": np.ones((T, N, 3), dtype=np.uint8), "done": done, "state_in": np.zeros((T, N, 3, 2, H), dtype=np.float32)}


def _stream(collects):
    """the origin tags over the whole stream (global step g, arena n): obs = g + 100 n, state_in = (g + 1) + 1000 n, but zero at every
    episode's first step, as the sampler stores it"""
    T, N = collects[0]["done"].shape
    fresh = np.ones(N, dtype=bool)
    for ci, c in enumerate(collects):
        for t in range(T):
            g = ci * T + t
            for n in range(N):
                c["obs"][t, n] = g + 100 * n
                c["actions"][t, n] = (g + n) % 3
                c["state_in"][t, n] = 0.0 if fresh[n] else (g + 1) + 1000 * n
            fresh = c["done"][t].astype(bool)
    return collects


def test_restatement_on_hand_built_streams():
    """three collects of T = 2 steps, L = 3, three arenas, gamma = lambda = 0.5 (global steps g = 0..5).
    arena 0: done at g = 0 (a one-row episode), then one episode over g = 1..5 (E = 5, all three collects; T < L): its sequences
             start at g = 1 (collect 0, two collects before the episode ends) and g = 4; rewards 0 but 1 at g = 5, values 0 ->
             A = 0.25^(4 - t); the one-row episode: reward 4, value 1 -> A = 3, target 4.
    arena 1: done at g = 5 only: E = 6 = 2 L, sequences of 3 and 3 starting at g = 0 and g = 3.
    arena 2: no finished episode: all six rows stay carried."""
    T, N, L = 2, 3, 3
    r0, v0 = np.zeros((T, N, 3), np.float32), np.zeros((T, N, 3), np.float32)
    r0[0, 0], v0[0, 0] = 4.0, 1.0
    r2 = np.zeros((T, N, 3), np.float32)
    r2[1, 0] = 1.0
    c = _stream([_collect(T, N, {0: [0]}, r0, v0), _collect(T, N, {}), _collect(T, N, {0: [1], 1: [1]}, r2)])
    (b0, b1, b2), carried = restate(c, L, gamma=0.5, lam=0.5)
    assert np.array_equal(carried, [0, 0, 6])
    # collect 0: the one-row episode of arena 0, one sequence of one row, zero state
    assert np.array_equal(b0["t"], [0]) and np.array_equal(b0["done"], [1]) and np.array_equal(b0["arena"], [0])
    assert np.array_equal(b0["adv"][:, 0], [3.0]) and np.array_equal(b0["target"][:, 0], [4.0])
    assert np.array_equal(b0["ep_start"], [0]) and np.array_equal(b0["ep_len"], [1]) and np.array_equal(b0["ep_arena"], [0])
    assert np.array_equal(b0["seq_start"], [0]) and np.array_equal(b0["seq_len"], [1]) and np.array_equal(b0["seq_ep"], [0])
    assert b0["state_in"].shape == (1, 3, 2, 2) and not b0["state_in"].any()
    # collect 1: nothing ends
    assert all(len(v) == 0 for v in b1.values()) and b1["obs"].shape == (0, 3, 2) and b1["state_in"].shape == (0, 3, 2, 2)
    # collect 2: arena 0's five rows (g = 1..5), then arena 1's six (g = 0..5)
    assert np.array_equal(b2["obs"][:, 0, 0], [1, 2, 3, 4, 5, 100, 101, 102, 103, 104, 105])
    assert np.array_equal(b2["arena"], [0] * 5 + [1] * 6) and np.array_equal(b2["episode"], [1] * 5 + [0] * 6)
    assert np.array_equal(b2["t"], [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5])
    assert np.array_equal(b2["done"], [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1])
    assert np.array_equal(b2["adv"][:5, 0], [1 / 256, 1 / 64, 1 / 16, 1 / 4, 1.0]) and not b2["adv"][5:].any()
    assert np.array_equal(b2["ep_start"], [0, 5]) and np.array_equal(b2["ep_len"], [5, 6]) and np.array_equal(b2["ep_arena"], [0, 1])
    assert np.array_equal(b2["seq_start"], [0, 3, 5, 8]) and np.array_equal(b2["seq_len"], [3, 2, 3, 3])
    assert np.array_equal(b2["seq_ep"], [0, 0, 1, 1])
    # states: zero at every episode start, else the tag of the step the sequence starts on (g = 4 of arena 0: 5; g = 3 of arena 1: 1004)
    assert np.array_equal(b2["state_in"][:, 0, 0, 0], [0.0, 5.0, 0.0, 1004.0]) and (b2["state_in"] == b2["state_in"][:, :1, :1, :1]).all()
    # the padded form: arena 0's second sequence has two rows, then zeros
    p = pad_sequences(b2, L)
    assert p["obs"].shape == (4, 3, 3, 2) and np.array_equal(p["mask"][1], [True, True, False])
    assert np.array_equal(p["obs"][1, :, 0, 0], [4, 5, 0]) and np.array_equal(p["obs"][3, :, 0, 0], [103, 104, 105])


def test_restatement_of_a_stream_without_any_finished_episode_is_empty():
    c = _stream([_collect(4, 2, {})])
    (b,), carried = restate(c, 20)
    assert np.array_equal(carried, [4, 4]) and all(len(v) == 0 for v in b.values())
