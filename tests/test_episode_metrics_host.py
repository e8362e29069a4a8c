"""Episode metrics of whole-episode batches (hh_episodes_metrics, EpisodeBatch(metrics=True)) without a GPU: the float64 restatement of
tests/episode_metrics_ref.py pinned on a hand-computed table, the C ABI (exports, binding, layout of hh_episode_metrics_bufs, the summary's
slots) and the constructors' argument validation."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from episode_metrics_ref import bounds, explained_variance, restate_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "hh_abi.h")).read()


def test_restatement_on_a_hand_computed_table():
    """3 episodes x 2 agents of exactly representable numbers, lengths 2, 1, 3:
         episode 0 rows 0-1: agent returns 1 + 2 = 3, -0.5 + 0.25 = -0.25 -> reward 2.75
         episode 1 row  2:   4, -8                                         -> reward -4
         episode 2 rows 3-5: 0.5 + 0.5 - 2 = -1, 1 + 1 + 1 = 3             -> reward 2"""
    reward = np.array([[1, -0.5], [2, 0.25], [4, -8], [0.5, 1], [0.5, 1], [-2, 1]], dtype=np.float32)
    target = np.array([[0, 1], [2, 1], [4, 1], [6, 1], [8, 1], [10, 5]], dtype=np.float32)
    vf = np.array([[0, 0], [2, 0], [4, 0], [6, 0], [8, 0], [4, 0]], dtype=np.float32)
    m = restate_metrics(reward, vf, target, [0, 2, 3], [2, 1, 3])
    assert m["episodes"] == 3 and m["rows"] == 6
    assert np.array_equal(m["ep_return"], [[3, -0.25], [4, -8], [-1, 3]]) and m["ep_return"].dtype == np.float64
    assert np.array_equal(m["episode_reward"], [2.75, -4, 2])
    assert m["episode_reward_mean"] == 0.75 / 3 and m["episode_reward_min"] == -4 and m["episode_reward_max"] == 2.75
    assert m["episode_len_mean"] == 2.0 and m["episode_len_min"] == 1 and m["episode_len_max"] == 3
    assert np.array_equal(m["agent_return_mean"], [2.0, -5.25 / 3])
    assert np.array_equal(m["agent_return_min"], [-1, -8]) and np.array_equal(m["agent_return_max"], [4, 3])
    # agent 0: target 0, 2, .., 10: mean 5, M2 = 25 + 9 + 1 + 1 + 9 + 25 = 70; target - vf = 0, 0, 0, 0, 0, 6: mean 1, M2 = 5 + 25 = 30
    # agent 1: target 1 x 5, 5: mean 5/3 ...; target - vf = target: the ratio is 1 up to rounding -> explained variance ~ 0
    assert m["vf_explained_var"][0] == 1.0 - 30.0 / 70.0
    assert abs(m["vf_explained_var"][1]) < 1e-15
    # a prediction far worse than the mean clamps at -1; a constant target with an exact prediction has no variance at all: nan
    assert explained_variance(np.array([0.0, 1.0, 2.0]), np.array([50.0, -50.0, 50.0])) == -1.0
    assert math.isnan(explained_variance(np.ones(4), np.ones(4)))
    assert explained_variance(np.ones(4), np.arange(4.0)) == -1.0   # 1 - x / 0 = -inf
    b = bounds(reward, [0, 2, 3], [2, 1, 3], m)
    assert b["ep_return"].shape == (3, 2) and b["ep_return"][0, 0] == 2 * 2.0 ** -52 * 3.0 and b["ep_return"][1, 1] == 2.0 ** -52 * 8.0


def test_restatement_without_an_episode_is_nan():
    m = restate_metrics(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), [], [])
    assert m["episodes"] == 0 and m["rows"] == 0 and m["ep_return"].shape == (0, 3)
    for k in ("episode_reward_mean", "episode_reward_min", "episode_reward_max", "episode_len_mean", "episode_len_min", "episode_len_max"):
        assert math.isnan(m[k]), k
    for k in ("agent_return_mean", "agent_return_min", "agent_return_max", "vf_explained_var"):
        assert m[k].shape == (3,) and np.isnan(m[k]).all(), k


def test_sequential_sums_not_pairwise():
    """np.sum's pairwise tree gives another result on this input; the restatement adds one after the other"""
    x = np.array([1.0] + [2.0 ** -53] * 300, dtype=np.float64).astype(np.float32)[:, None]
    m = restate_metrics(x, np.zeros_like(x), np.zeros_like(x), [0], [301])
    assert m["ep_return"][0, 0] == 1.0   # every single addition of 2^-53 to 1.0 rounds back to 1.0


def test_entry_points_are_exported_and_bound():
    from hhmarl_2d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("hh_episodes_metrics", "hh_episodes_metrics_scratch_bytes"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    lib = _lib.lib()
    assert lib.hh_episodes_metrics.argtypes == [C.POINTER(_lib.HHEpisodeMetricsBufs), C.c_void_p]
    assert lib.hh_episodes_metrics_scratch_bytes.argtypes == [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]


def test_scratch_bytes_and_its_argument_checks_need_no_device():
    from hhmarl_2d_amd import _lib
    lib = _lib.lib()
    n = C.c_int64(-1)
    assert lib.hh_episodes_metrics_scratch_bytes(100, 1, 2, C.byref(n)) == 0 and n.value > 0 and n.value % 8 == 0
    small = n.value
    assert lib.hh_episodes_metrics_scratch_bytes(100, 1 << 22, 2, C.byref(n)) == 0 and n.value > small
    two = n.value
    assert lib.hh_episodes_metrics_scratch_bytes(100, 1 << 22, 3, C.byref(n)) == 0 and n.value > two
    for args in ((0, 10, 2), (10, 0, 2), (10, 10, 0), (10, 10, 6), (1 << 31, 10, 2), (10, 1 << 31, 2), (10, (1 << 31) - 1023, 2)):
        n.value = -7
        assert lib.hh_episodes_metrics_scratch_bytes(*args, C.byref(n)) == -1 and n.value == -7, args
        assert b"hh_episodes_metrics_scratch_bytes" in lib.hh_last_error()
    assert lib.hh_episodes_metrics_scratch_bytes(10, 10, 2, None) == -1
    # the argument checks of hh_episodes_metrics come before anything is enqueued: they need no device either
    assert lib.hh_episodes_metrics(None, None) == -1
    m = _lib.HHEpisodeMetricsBufs(n_agents=2, reserved0=0, row_cap=10, ep_cap=10)
    assert lib.hh_episodes_metrics(C.byref(m), None) == -1 and b"null buffer" in lib.hh_last_error()


def test_struct_layout_and_slots_match_the_header():
    from hhmarl_2d_amd import _lib
    txt = _header()
    body = re.search(r"typedef struct hh_episode_metrics_bufs \{(.*?)\} hh_episode_metrics_bufs;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(int32_t|int64_t|double|float|void)\s*(\*?)\s*([A-Za-z_0-9]+)\s*;", body)
    scalar = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    want = [(name, C.c_void_p if star else scalar[t]) for t, star, name in fields]
    assert len(want) == 15 and want == list(_lib.HHEpisodeMetricsBufs._fields_)
    S = _lib.HHEpisodeMetricsBufs
    assert C.sizeof(S) == 2 * 4 + 2 * 8 + 10 * 8 + 8 == 112
    offsets = {"n_agents": 0, "reserved0": 4, "row_cap": 8, "ep_cap": 16, "reward": 24, "vf": 32, "target": 40, "ep_start": 48, "ep_len": 56,
               "counts": 64, "ep_return": 72, "summary": 80, "totals": 88, "scratch": 96, "scratch_bytes": 104}
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == offsets
    # the summary: HH_EP_METRICS slots, the names in slot order, the per-agent blocks HH_EP_METRICS_MAX_AGENTS wide
    defs = {k: int(v) for k, v in re.findall(r"#define (HH_EPM_[A-Z_]+|HH_EP_METRICS(?:_MAX_AGENTS)?) (\d+)", txt)}
    assert defs["HH_EP_METRICS"] == len(_lib.EP_METRICS) and defs["HH_EP_METRICS_MAX_AGENTS"] == _lib.EP_METRICS_MAX_AGENTS == 5
    slot = _lib.EP_METRICS_SLOT
    assert len(slot) == len(_lib.EP_METRICS), "slot names are unique"
    pairs = {"HH_EPM_EPISODES": "episodes", "HH_EPM_ROWS": "rows", "HH_EPM_REWARD_MEAN": "episode_reward_mean",
             "HH_EPM_REWARD_MIN": "episode_reward_min", "HH_EPM_REWARD_MAX": "episode_reward_max", "HH_EPM_LEN_MEAN": "episode_len_mean",
             "HH_EPM_LEN_MIN": "episode_len_min", "HH_EPM_LEN_MAX": "episode_len_max", "HH_EPM_AGENT_MEAN": "agent_return_mean_0",
             "HH_EPM_AGENT_MIN": "agent_return_min_0", "HH_EPM_AGENT_MAX": "agent_return_max_0",
             "HH_EPM_AGENT_EXPLAINED_VAR": "vf_explained_var_0"}
    assert {k for k in defs if k.startswith("HH_EPM_")} == set(pairs)
    for macro, name in pairs.items():
        assert defs[macro] == slot[name], macro
    for base in ("agent_return_mean", "agent_return_min", "agent_return_max", "vf_explained_var"):
        assert [slot[f"{base}_{a}"] for a in range(5)] == list(range(slot[base + "_0"], slot[base + "_0"] + 5))
    assert "timesteps_total counts" in txt and "ENVIRONMENT steps" in txt, "the header states the timesteps_total convention"


def test_metrics_needs_whole_episode_batches():
    from hhmarl_2d_amd.commander import CommanderRollout
    from hhmarl_2d_amd.rollout import PPORollout
    with pytest.raises(ValueError, match="metrics=True needs batch_mode='complete_episodes'"):
        PPORollout(None, None, 8, metrics=True)
    with pytest.raises(ValueError, match="metrics=True needs batch_mode='complete_episodes'"):
        PPORollout(None, None, 8, batch_mode="truncate_episodes", metrics=True)
    with pytest.raises(ValueError, match="metrics=True needs batch_mode='complete_episodes'"):
        CommanderRollout(None, None, None, 8, batch_mode="truncate_episodes", metrics=True)
    with pytest.raises(ValueError, match="metrics=True needs batch_mode='complete_episodes'"):
        CommanderRollout(None, None, None, 8, metrics=True)
