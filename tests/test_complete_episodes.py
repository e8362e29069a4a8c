"""batch_mode = "complete_episodes" (train_hetero.py:212) without a GPU: argument validation of PPORollout, the C ABI of
hh_episodes_emit (export, binding, layout of hh_episode_bufs), and the host restatement of the whole-episode batch (tests/episodes_ref.py) that
tests/test_gpu_complete_episodes.py compares the device's batches with, pinned on hand-built streams of exactly representable numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from episodes_ref import restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_COLS = ("obs", "actions", "logp", "vf", "reward", "valid", "done")
OUT_COLS = ("obs", "actions", "logp", "vf", "reward", "valid", "adv", "target", "done", "arena", "episode", "t")


def _stream(T, N, nA, done_rows, reward, vf, D=2):
    """one collect of hand-built values: done_rows = {arena: [ticks]}, reward / vf [T, N, nA]; obs / logp / actions encode the tick and arena"""
    done = np.zeros((T, N), dtype=np.uint8)
    for n, ts in done_rows.items():
        done[ts, n] = 1
    tick = np.arange(T, dtype=np.float32)[:, None, None, None] + 100 * np.arange(N, dtype=np.float32)[None, :, None, None]
    return {"obs": np.broadcast_to(tick, (T, N, nA, D)).copy(), "actions": np.zeros((T, N, nA, 4), dtype=np.int8),
            "logp": -np.ones((T, N, nA), dtype=np.float32), "vf": np.asarray(vf, dtype=np.float32), "reward": np.asarray(reward, dtype=np.float32),
            "valid": np.ones((T, N, nA), dtype=np.uint8), "done": done}


def test_argument_validation_needs_no_world():
    from hhmarl_2d_amd.rollout import PPORollout
    with pytest.raises(ValueError, match="batch_mode"):
        PPORollout(None, None, 8, batch_mode="complete")
    with pytest.raises(ValueError, match="semantics='rllib'"):
        PPORollout(None, None, 8, semantics="masked", batch_mode="complete_episodes")


def test_emit_entry_point_is_exported_and_bound():
    from hhmarl_2d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert "hh_episodes_emit" in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), "hh_episodes_emit")
    f = _lib.lib().hh_episodes_emit
    assert f.argtypes == [C.POINTER(_lib.HHEpisodeBufs), C.c_void_p]


def test_episode_bufs_struct_layout_matches_header():
    from hhmarl_2d_amd import _lib
    txt = open(os.path.join(ROOT, "include", "hh_abi.h")).read()
    body = re.search(r"typedef struct hh_episode_bufs \{(.*?)\} hh_episode_bufs;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(int32_t|int64_t|double|float|int8_t|uint8_t)\s*(\*?)\s*([A-Za-z_0-9]+)\s*;", body)
    scalar = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    want = [(name, C.c_void_p if star else scalar[t]) for t, star, name in fields]
    assert len(want) == 42 and want == list(_lib.HHEpisodeBufs._fields_)
    assert C.sizeof(_lib.HHEpisodeBufs) == 6 * 4 + 4 * 8 + 32 * 8
    assert _lib.HHEpisodeBufs.gamma.offset == 40 and _lib.HHEpisodeBufs.obs.offset == 56


def test_restatement_on_hand_built_streams():
    """Two collects of T = 3 ticks, two arenas, one agent, gamma = lambda = 0.5.
    arena 0: done at tick 0 of collect 0 (a one-row episode), then an episode over ticks 1, 2 of collect 0 and tick 0 of collect 1
             (it spans the collects) with rewards [1, 0, 2] and values [0.5, 0.25, -1]; ticks 1, 2 of collect 1 stay carried.
             by hand (tests/test_rollout_post.py): delta = [0.625, -0.75, 3], A = [0.625, 0, 3], targets = [1.125, 0.25, 2];
             the one-row episode: reward 4, value 1 -> A = 4 + 0.5 * 0 - 1 = 3, target 4.
    arena 1: no done in collect 0, done at tick 2 of collect 1: one six-row episode, rewards [0, 0, 0, 0, 0, 1], values 0 ->
             delta = [0, 0, 0, 0, 0, 1], A = 0.25^(5 - t) = [1/1024, 1/256, 1/64, 1/16, 1/4, 1], targets = A."""
    r0 = np.array([[4, 0], [1, 0], [0, 0]], dtype=np.float32)[..., None]
    v0 = np.array([[1, 0], [0.5, 0], [0.25, 0]], dtype=np.float32)[..., None]
    r1 = np.array([[2, 0], [9, 0], [9, 1]], dtype=np.float32)[..., None]
    v1 = np.array([[-1, 0], [7, 0], [7, 0]], dtype=np.float32)[..., None]
    c0 = _stream(3, 2, 1, {0: [0]}, r0, v0)
    c1 = _stream(3, 2, 1, {0: [0], 1: [2]}, r1, v1)
    (b0, b1), carried = restate([c0, c1], gamma=0.5, lam=0.5)
    assert np.array_equal(carried, [2, 0])
    # collect 0: only the one-row episode of arena 0
    assert np.array_equal(b0["arena"], [0]) and np.array_equal(b0["episode"], [0]) and np.array_equal(b0["t"], [0])
    assert np.array_equal(b0["adv"][:, 0], [3.0]) and np.array_equal(b0["target"][:, 0], [4.0]) and np.array_equal(b0["done"], [1])
    # collect 1: arena 0's second episode (its first two rows from collect 0), then arena 1's six rows
    assert np.array_equal(b1["arena"], [0, 0, 0, 1, 1, 1, 1, 1, 1])
    assert np.array_equal(b1["episode"], [1, 1, 1, 0, 0, 0, 0, 0, 0])
    assert np.array_equal(b1["t"], [0, 1, 2, 0, 1, 2, 3, 4, 5])
    assert np.array_equal(b1["done"], [0, 0, 1, 0, 0, 0, 0, 0, 1])
    assert np.array_equal(b1["obs"][:, 0, 0], [1, 2, 0, 100, 101, 102, 100, 101, 102])    # tick + 100 arena: the rows' origins
    assert np.array_equal(b1["adv"][:, 0], [0.625, 0.0, 3.0, 1 / 1024, 1 / 256, 1 / 64, 1 / 16, 1 / 4, 1.0])
    assert np.array_equal(b1["target"][:, 0], [1.125, 0.25, 2.0, 1 / 1024, 1 / 256, 1 / 64, 1 / 16, 1 / 4, 1.0])
    assert b1["adv"].dtype == np.float32 and b1["obs"].shape == (9, 1, 2)


def test_restatement_without_any_finished_episode_is_empty():
    c = _stream(4, 3, 2, {}, np.zeros((4, 3, 2)), np.zeros((4, 3, 2)), D=5)
    (b,), carried = restate([c])
    assert np.array_equal(carried, [4, 4, 4])
    assert all(len(v) == 0 for v in b.values()) and b["obs"].shape == (0, 2, 5) and b["adv"].shape == (0, 2)
