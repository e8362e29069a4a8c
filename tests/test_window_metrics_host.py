"""Episode metrics of fixed-window rollouts (hh_window_metrics, rollout.WindowMetrics, window_metrics=True) without a GPU: the stateful
float64 restatement of tests/window_metrics_ref.py on hand-written windows, the C ABI (exports, binding, layout of
hh_window_metrics_bufs against the header, the argument checks that need no device), the constructors' validation, and the keys of a
rollout's state_dict without the option."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from window_metrics_ref import WindowMetricsRef, window_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _window(reward, done, target=None, vf=None):
    reward = np.asarray(reward, dtype=np.float32)
    T, N, nA = reward.shape
    target = np.arange(T * N * nA, dtype=np.float32).reshape(T, N, nA) if target is None else np.asarray(target, dtype=np.float32)
    vf = np.zeros((T + 1, N, nA), dtype=np.float32) if vf is None else np.asarray(vf, dtype=np.float32)
    return reward, vf, target, np.asarray(done, dtype=np.uint8)


def test_restatement_carries_episodes_across_hand_written_windows():
    """2 arenas x 1 agent, windows of 3 rows, exactly representable rewards:
         arena 0: rewards 1 2 4 | 8 16 32 | 64 ..., done at window 1 t = 0 -> an episode of 4 rows, return 15; then done at window 1
                  t = 1 -> length 1, return 16 (two consecutive done rows); 32 + 64 run on
         arena 1: rewards .5 .5 .5 | .5 .5 .5 | ..., never done: the carry only grows"""
    ref = WindowMetricsRef(2, 1)
    w0 = ref.window(*_window([[[1], [.5]], [[2], [.5]], [[4], [.5]]], [[0, 0], [0, 0], [0, 0]]))
    assert w0["episodes"] == 0 and w0["rows"] == 6 and w0["counts"].tolist() == [0, 6] and w0["ep_return"].shape == (0, 1)
    assert w0["run_return"].tolist() == [[7.0], [1.5]] and w0["run_len"].tolist() == [3, 3] and w0["totals"].tolist() == [0, 6]
    for k in ("episode_reward_mean", "episode_reward_min", "episode_reward_max", "episode_len_mean", "episode_len_min", "episode_len_max"):
        assert math.isnan(w0[k]), k
    assert np.isnan(w0["agent_return_mean"]).all() and np.isfinite(w0["vf_explained_var"]).all(), "the explained variance needs no episode"
    w1 = ref.window(*_window([[[8], [.5]], [[16], [.5]], [[32], [.5]]], [[1, 0], [1, 0], [0, 0]]))
    assert w1["episodes"] == 2 and w1["rows"] == 6 and w1["counts"].tolist() == [2, 6]
    assert w1["ep_return"].tolist() == [[15.0], [16.0]] and w1["ep_len"].tolist() == [4, 1]
    assert w1["ep_arena"].tolist() == [0, 0] and w1["ep_end"].tolist() == [0, 1]
    assert w1["run_return"].tolist() == [[32.0], [3.0]] and w1["run_len"].tolist() == [1, 6] and w1["totals"].tolist() == [2, 12]
    assert w1["episode_reward_mean"] == 15.5 and w1["episode_reward_min"] == 15 and w1["episode_reward_max"] == 16
    assert w1["episode_len_mean"] == 2.5 and w1["episode_len_min"] == 1 and w1["episode_len_max"] == 4
    assert w1["ep_return"].dtype == np.float64 and w1["ep_len"].dtype == np.int32
    b = window_bounds(w1, np.zeros((4, 2, 1), np.float32), np.arange(6, dtype=np.float32).reshape(3, 2, 1))
    assert b["episode_reward_mean"] > 0 and b["episode_len_mean"] == 2 * 2.0 ** -52 * 5 and b["vf_explained_var"].shape == (1,)
    ref.reset()
    assert not ref.run_return.any() and not ref.run_len.any() and ref.totals.tolist() == [0, 0]


def test_restatement_orders_the_table_arena_major_then_t_and_sums_agents_in_order():
    """3 arenas x 2 agents, one window of 2 rows: arena 2 is done at t = 0 and t = 1, arena 0 at t = 1, arena 1 never"""
    reward = [[[1, 10], [2, 20], [4, 40]], [[8, 80], [16, 160], [32, 320]]]
    ref = WindowMetricsRef(3, 2)
    w = ref.window(*_window(reward, [[0, 0, 1], [1, 0, 1]]))
    assert w["ep_arena"].tolist() == [0, 2, 2] and w["ep_end"].tolist() == [1, 0, 1] and w["ep_len"].tolist() == [2, 1, 1]
    assert w["ep_return"].tolist() == [[9, 90], [4, 40], [32, 320]] and w["episode_reward"].tolist() == [99, 44, 352]
    assert w["agent_return_min"].tolist() == [4, 40] and w["agent_return_max"].tolist() == [32, 320]
    assert w["agent_return_mean"].tolist() == [15.0, 150.0] and w["episode_reward_mean"] == 165.0
    assert w["run_return"].tolist() == [[0, 0], [18, 180], [0, 0]] and w["run_len"].tolist() == [0, 2, 0]


def test_the_carry_adds_sequentially_in_float64_across_the_cut():
    """1.0 followed by 300 rows of 2^-53 in windows of 7: every single float64 addition rounds back to 1.0 — a pairwise sum or a sum
    per window added to the carry afterwards gives more; a float32 carry could not hold 1 + 2^-24 either"""
    x = np.array([1.0] + [2.0 ** -53] * 300 + [2.0 ** -24], dtype=np.float32)
    done = np.zeros(len(x), dtype=np.uint8)
    done[-1] = 1
    pad = (-len(x)) % 7
    x, done = np.concatenate([x, np.zeros(pad, np.float32)]), np.concatenate([done, np.zeros(pad, np.uint8)])
    ref, got = WindowMetricsRef(1, 1), []
    for i in range(0, len(x), 7):
        w = ref.window(*_window(x[i:i + 7].reshape(7, 1, 1), done[i:i + 7].reshape(7, 1)))
        got += [(r[0], int(n)) for r, n in zip(w["ep_return"], w["ep_len"])]
    assert got == [(1.0 + 2.0 ** -24, 302)]


def test_entry_points_are_exported_and_bound():
    from hhmarl_2d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("hh_window_metrics", "hh_window_metrics_scratch_bytes"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    lib = _lib.lib()
    assert lib.hh_window_metrics.argtypes == [C.POINTER(_lib.HHWindowMetricsBufs), C.c_void_p]
    assert lib.hh_window_metrics_scratch_bytes.argtypes == [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]


def test_struct_layout_matches_the_header():
    from hhmarl_2d_amd import _lib
    txt = open(os.path.join(ROOT, "include", "hh_abi.h")).read()
    body = re.search(r"typedef struct hh_window_metrics_bufs \{(.*?)\} hh_window_metrics_bufs;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    scalar = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    want = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        t, names = re.fullmatch(r"(?:const\s+)?(int32_t|int64_t|uint8_t|double|float|void)\s+(.*)", decl, re.S).groups()
        for name in (x.strip() for x in names.split(",")):
            want.append((name.lstrip("* "), C.c_void_p if name.startswith("*") else scalar[t]))
    S = _lib.HHWindowMetricsBufs
    assert len(want) == 19 and want == list(S._fields_)
    assert C.sizeof(S) == 4 * 4 + 14 * 8 + 8 == 136
    names = [n for n, _ in S._fields_]
    assert names[:4] == ["T", "N", "n_agents", "reserved0"] and [getattr(S, n).offset for n in names[:4]] == [0, 4, 8, 12]
    assert [getattr(S, n).offset for n in names[4:]] == list(range(16, 136, 8)), "pointers and scratch_bytes: 8 bytes each from 16"
    assert "hh_window_metrics: " in txt and "ONE DIFFERENCE from hh_episodes_metrics" in txt, "the header states the refusals' prefix and the 0-episode rule"


def test_scratch_bytes_and_the_argument_checks_need_no_device():
    from hhmarl_2d_amd import _lib
    lib = _lib.lib()
    n = C.c_int64(-1)
    assert lib.hh_window_metrics_scratch_bytes(1, 1, 1, C.byref(n)) == 0 and n.value > 0 and n.value % 8 == 0
    assert lib.hh_window_metrics_scratch_bytes(64, 16384, 2, C.byref(n)) == 0 and n.value == 1024 * 4 * 2 * 8 + 16384 * 4
    assert lib.hh_window_metrics_scratch_bytes(3, 2050, 3, C.byref(n)) == 0 and n.value == 7 * 4 * 3 * 8 + 2050 * 4
    assert lib.hh_window_metrics_scratch_bytes(5, 65, 2, C.byref(n)) == 0 and n.value == 1 * 4 * 2 * 8 + 65 * 4 + 4, "rounded up to 8"
    assert lib.hh_window_metrics_scratch_bytes(1, (1 << 31) - 1024, 1, C.byref(n)) == 0
    for args in ((0, 10, 2), (10, 0, 2), (-1, 10, 2), (10, 10, 0), (10, 10, 6), (1, (1 << 31) - 1023, 1), (1 << 16, 1 << 16, 2)):
        n.value = -7
        assert lib.hh_window_metrics_scratch_bytes(*args, C.byref(n)) == -1 and n.value == -7, args
        assert lib.hh_last_error().startswith(b"hh_window_metrics_scratch_bytes: ")
    assert lib.hh_window_metrics_scratch_bytes(10, 10, 2, None) == -1
    assert lib.hh_window_metrics(None, None) == -1 and lib.hh_last_error().startswith(b"hh_window_metrics: ")
    m = _lib.HHWindowMetricsBufs(T=4, N=4, n_agents=2, reserved0=0)
    assert lib.hh_window_metrics(C.byref(m), None) == -1 and lib.hh_last_error() == b"hh_window_metrics: null buffer"
    m.reserved0 = 1
    assert lib.hh_window_metrics(C.byref(m), None) == -1 and b"reserved0" in lib.hh_last_error()


def test_window_metrics_needs_fixed_windows_and_rllib_semantics():
    """refused before the world is touched (None stands in for it), like the constructors' other checks"""
    from hhmarl_2d_amd.commander import CommanderRollout
    from hhmarl_2d_amd.rollout import PPORollout
    with pytest.raises(ValueError, match="window_metrics=True needs batch_mode='truncate_episodes'.*already has metrics=True"):
        PPORollout(None, None, 8, batch_mode="complete_episodes", window_metrics=True)
    with pytest.raises(ValueError, match="window_metrics=True needs batch_mode='truncate_episodes'.*already has metrics=True"):
        CommanderRollout(None, None, None, 8, batch_mode="complete_episodes", window_metrics=True)
    with pytest.raises(ValueError, match="window_metrics=True is defined for RLlib's trajectory view only"):
        PPORollout(None, None, 8, semantics="masked", window_metrics=True)
    with pytest.raises(ValueError, match="metrics=True needs batch_mode='complete_episodes'"):
        PPORollout(None, None, 8, metrics=True, window_metrics=True)          # metrics=True keeps its validation
    with pytest.raises(TypeError):
        PPORollout(None, None, 8, 0.99, 0.95, True, None, "rllib", "truncate_episodes", False, None, False, True)   # keyword-only
    with pytest.raises(TypeError):
        CommanderRollout(None, None, None, 8, 0.99, 1.0, True, "truncate_episodes", 20, None, False, None, False, True)


class _Stub:
    """what rollout_state_dict / rollout_load_plan read of a rollout, on CPU tensors"""

    def __init__(self, window_metrics=None):
        import torch
        self.w = type("W", (), {"device": torch.device("cpu")})()
        self.obs, self.done = torch.zeros(3, 2), torch.zeros(2, 2, dtype=torch.uint8)
        self.collects, self._started, self.episodes, self.window_metrics, self._graph = 2, True, None, window_metrics, object()


def test_a_state_dict_without_the_option_has_exactly_todays_keys(monkeypatch):
    import torch
    from hhmarl_2d_amd import rollout as R
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ro = _Stub()
    sd = R.rollout_state_dict(ro, ("obs", "done"), {"T": 2})
    assert list(sd) == ["options", "window", "collects", "started", "episodes"] and list(sd["window"]) == ["obs", "done"]
    R.rollout_load_plan(ro, sd, ("obs", "done"), {"T": 2})     # and loads back as always

    class _WM:
        def state_dict(self):
            return {"carry": torch.ones(1)}

        def _load_plan(self, sd):
            assert list(sd) == ["carry"]
            return lambda: None
    on = _Stub(_WM())
    sd_on = R.rollout_state_dict(on, ("obs", "done"), {"T": 2})
    assert list(sd_on) == list(sd) + ["window_metrics"] and sd_on["options"] == sd["options"]
    R.rollout_load_plan(on, sd_on, ("obs", "done"), {"T": 2})()
    # the option in the other position: refused by name, before anything is changed
    with pytest.raises(ValueError, match="window_metrics"):
        R.rollout_load_plan(ro, sd_on, ("obs", "done"), {"T": 2})
    with pytest.raises(ValueError, match="window_metrics"):
        R.rollout_load_plan(on, sd, ("obs", "done"), {"T": 2})
    assert on.collects == 2 and ro.collects == 2


def test_the_options_and_the_positional_signature_of_both_rollouts_stay():
    """_options() feeds check_options, which refuses unknown keys: a checkpoint of today's must keep loading.  The keyword is
    keyword-only, off by default, and the positional signature still ends with record_logits"""
    import inspect
    from hhmarl_2d_amd.commander import CommanderRollout
    from hhmarl_2d_amd.rollout import PPORollout
    for cls in (PPORollout, CommanderRollout):
        assert "window_metrics" not in inspect.getsource(cls._options)
        outer = inspect.signature(cls.__init__, follow_wrapped=False).parameters
        assert outer["window_metrics"].kind is inspect.Parameter.KEYWORD_ONLY and outer["window_metrics"].default is False
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[-1] == "record_logits" and p["record_logits"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert "window_metrics" in cls.__doc__ and "window_metrics" in cls.__init__.__doc__
