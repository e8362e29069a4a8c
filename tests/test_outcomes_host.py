"""Win / lose / draw of training episodes (hh_outcome_tap, hh_episode_outcomes, outcomes=True) without a GPU: the restatement of
tests/outcome_ref.py on two CPU-oracle runs (tests/outcome_fixtures.py) and on hand-written tables, the C ABI (exports, binding, the
struct's layout against the header, the argument checks that need no device), the constructors' validation and the key sets of a
rollout built without the option."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import outcome_ref as R
from outcome_fixtures import fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16


def _tapped(f):
    return np.stack([R.tap(f["done"][t], f["polled"][t]) for t in range(len(f["done"]))])


# ------------------------------------------------------------------------------------------------------------------ the fixtures' pins
def test_fixture_a_has_all_three_classes_and_fixture_b_two_episodes_per_window():
    a, b = fixture("A"), fixture("B")
    oc = a["polled"][a["done"] != 0]
    assert [(oc == c).sum() for c in (1, -1, 0)] == [4, 7, 56] and len(oc) == 67
    t, _ = np.nonzero(a["done"])
    assert t[oc == -1].min() == 30 and t[oc == 1].min() == 22
    ob = b["polled"][b["done"] != 0]
    assert len(ob) == 670 and (ob == 0).all()
    assert sum(int(((b["done"][i:i + T] != 0).sum(0) >= 2).sum()) for i in range(0, 64, T)) == 268


# ------------------------------------------------------------------------------------------------------------------ the tap
@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_tap_is_episode_stats_polled_after_every_tick(name):
    f = fixture(name)
    out = _tapped(f)
    assert out.dtype == np.int8 and out.shape == (64, 67)
    d = f["done"] != 0
    assert np.array_equal(out[d], f["polled"][d]) and np.isin(out[d], (-1, 0, 1)).all(), "a done row holds its episode's outcome"
    assert (out[~d] == 2).all(), "every other row holds 2, whatever episode_stats still remembers"
    assert (f["polled"][~d] != 2).any(), "the fixture has rows where episode_stats holds an older episode's outcome"


# ------------------------------------------------------------------------------------------------------------------ table and summary
def _plain_summary(code, ep_len, ep_return):
    """counts exactly; means by math.fsum (correctly rounded sums)"""
    rew = [math.fsum(r) for r in ep_return]
    out = {}
    for k, c in zip(R.CLASSES, (1, -1, 0)):
        sel = np.nonzero(code == c)[0]
        out[k] = (len(sel), math.fsum(rew[i] for i in sel) / len(sel) if len(sel) else math.nan,
                  math.fsum(int(ep_len[i]) for i in sel) / len(sel) if len(sel) else math.nan,
                  math.fsum(abs(rew[i]) for i in sel))
    return out


def _check_summary(s, tab):
    e1 = len(tab.ep_arena)
    assert s[0] == e1 and s[10] == 0 and s[11] == 0
    plain = _plain_summary(tab.ep_outcome, tab.ep_len, tab.ep_return)
    for k, name in enumerate(R.CLASSES):
        n, rew, ln, mag = plain[name]
        assert s[1 + k] == n
        if n == 0:
            assert math.isnan(s[4 + k]) and math.isnan(s[7 + k])
        else:
            assert s[7 + k] == ln, "lengths are integers: every order adds them exactly"
            # the tile order against correctly rounded sums: n roundings of at most 2^-53 sum|x| each, two more for the agents' sum
            assert abs(s[4 + k] - rew) <= (n + 2) * 2.0 ** -53 * mag / n + 2.0 ** -52 * abs(rew)


@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_table_overwriting_and_accumulating_four_windows(name):
    f = fixture(name)
    out = _tapped(f)
    over, acc = R.OutcomeTableRef(67, 2), R.OutcomeTableRef(67, 2, accumulate=True)
    pieces, flat = [], []
    for i in range(0, 64, T):
        w = (f["reward"][i:i + T], f["done"][i:i + T], out[i:i + T])
        flags, s = over.window(*w)
        m = int((w[1] != 0).sum())
        assert flags.tolist() == [0, m] and len(over.ep_outcome) == m
        _check_summary(s, over)
        # arena-major, then time
        n_idx, t_idx = np.nonzero(w[1].T != 0)
        assert np.array_equal(over.ep_arena, n_idx) and np.array_equal(over.ep_outcome, w[2][t_idx, n_idx])
        pieces.append((over.ep_arena.copy(), over.ep_len.copy(), over.ep_return.copy(), over.ep_outcome.copy()))
        before = acc.ep_outcome.copy()
        flags, s_acc = acc.window(*w)
        assert flags.tolist() == [0, m] and np.array_equal(acc.ep_outcome[:len(before)], before), "earlier segments keep their bytes"
        _check_summary(s_acc, acc)
        flat.append(s_acc)
    for k, name_ in enumerate(("ep_arena", "ep_len", "ep_return", "ep_outcome")):
        assert np.array_equal(getattr(acc, name_), np.concatenate([p[k] for p in pieces])), name_
    want = {"A": [4, 7, 56], "B": [0, 0, 670]}[name]
    assert flat[-1][1:4].tolist() == want and flat[-1][0] == sum(want)
    m = R.metrics(flat[-1])
    assert [m["agents_win"], m["opps_win"], m["draw"]] == want
    assert m["outcome_pct"]["draw"] == (want[2] / sum(want)) * 100


def test_fill_refuses_a_table_that_does_not_hold_the_window():
    done = np.array([[0, 1, 1], [1, 0, 1]], dtype=np.uint8)         # arena 0: t 1; arena 1: t 0; arena 2: t 0 and 1
    outcome = np.array([[2, -1, 0], [1, 2, 1]], dtype=np.int8)
    arena = np.array([9, 9, 0, 1, 2, 2], dtype=np.int32)
    old = np.array([5, 6, 7, 7, 7, 7], dtype=np.int8)
    got, flags = R.fill(done, outcome, 6, arena, old)
    assert got.tolist() == [5, 6, 1, -1, 0, 1] and flags.tolist() == [0, 4] and old.tolist() == [5, 6, 7, 7, 7, 7]
    bad = arena.copy()
    bad[4] = 1
    got, flags = R.fill(done, outcome, 6, bad, old)
    assert got.tolist() == old.tolist() and flags.tolist() == [1, 4], "an entry of another arena: nothing is written"
    got, flags = R.fill(done, outcome, 3, arena, old)
    assert got.tolist() == old.tolist() and flags.tolist() == [1, 4], "e1 < m: nothing is written"
    got, flags = R.fill(np.zeros_like(done), outcome, 6, arena, old)
    assert got.tolist() == old.tolist() and flags.tolist() == [0, 0], "no done row: an empty segment"


def test_summary_counts_other_codes_and_gives_nan_for_an_empty_class():
    code = np.array([1, 1, 2, 0, 3], dtype=np.int8)
    ret = np.array([[1, 2], [3, 4], [100, 100], [0.5, 0.25], [7, 7]], dtype=np.float64)
    s = R.summary(5, code, np.array([3, 5, 9, 2, 1], dtype=np.int32), ret)
    assert s.tolist()[:4] == [5, 2, 0, 1] and s[4] == 5.0 and math.isnan(s[5]) and s[6] == 0.75
    assert s[7] == 4.0 and math.isnan(s[8]) and s[9] == 2.0 and s[10] == 2 and s[11] == 0
    s0 = R.summary(0, code, np.zeros(5, np.int32), ret)
    assert s0[:4].tolist() == [0, 0, 0, 0] and np.isnan(s0[4:10]).all() and s0[10] == 0
    m = R.metrics(s0)
    assert all(math.isnan(v) for v in m["outcome_pct"].values()) and m["agents_win"] == 0


def test_summary_adds_in_tiles_of_1024_waves_of_64():
    """1.0 at entry 0 and 2^-53 everywhere else in 2 tiles + 5: a sequential sum stays at 1.0; the butterfly adds the small ones among
    themselves first, so they arrive — the restatement follows the kernel's order, not numpy's"""
    n = 2 * 1024 + 5
    x = np.full(n, 2.0 ** -53)
    x[0] = 1.0
    got = R._tile_sums(x)
    seq = np.float64(0.0)
    for v in x:
        seq = seq + v
    assert seq == 1.0 and got > 1.0 and got == 1.0 + round((n - 1) * 2.0 ** -53 / 2.0 ** -52) * 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_exported_and_bound():
    from hhmarl_2d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("hh_outcome_tap", "hh_episode_outcomes", "hh_episode_outcomes_scratch_bytes"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    lib = _lib.lib()
    assert lib.hh_outcome_tap.argtypes == [C.c_void_p] * 4
    assert lib.hh_episode_outcomes.argtypes == [C.POINTER(_lib.HHEpisodeOutcomeBufs), C.c_void_p]
    assert lib.hh_episode_outcomes_scratch_bytes.argtypes == [C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]
    assert (_lib.OUTCOME_WIN, _lib.OUTCOME_LOSE, _lib.OUTCOME_DRAW, _lib.OUTCOME_NONE) == (R.WIN, R.LOSE, R.DRAW, R.NONE)
    assert len(_lib.EO_SUMMARY) == R.N_SUMMARY


def test_struct_layout_matches_the_header():
    from hhmarl_2d_amd import _lib
    txt = open(os.path.join(ROOT, "include", "hh_abi.h")).read()
    body = re.search(r"typedef struct hh_episode_outcome_bufs \{(.*?)\} hh_episode_outcome_bufs;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    scalar = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    want = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        t, names = re.fullmatch(r"(?:const\s+)?(int32_t|int64_t|uint8_t|int8_t|double|float|void)\s+(.*)", decl, re.S).groups()
        for name in (x.strip() for x in names.split(",")):
            want.append((name.lstrip("* "), C.c_void_p if name.startswith("*") else scalar[t]))
    S = _lib.HHEpisodeOutcomeBufs
    assert len(want) == 16 and want == list(S._fields_)
    assert C.sizeof(S) == 4 * 4 + 8 + 10 * 8 + 8 == 112
    names = [n for n, _ in S._fields_]
    assert [getattr(S, n).offset for n in names] == [0, 4, 8, 12] + list(range(16, 112, 8))
    for macro, v in (("HH_OUTCOME_WIN", "1"), ("HH_OUTCOME_LOSE", "(-1)"), ("HH_OUTCOME_DRAW", "0"), ("HH_OUTCOME_NONE", "2"), ("HH_EO_SUMMARY", "12")):
        assert re.search(r"#define " + macro + r"\s+" + re.escape(v) + r"\s", txt), macro


def test_scratch_bytes_and_the_argument_checks_need_no_device():
    from hhmarl_2d_amd import _lib
    lib = _lib.lib()
    n = C.c_int64(-1)
    assert lib.hh_episode_outcomes_scratch_bytes(1, 1, 1, C.byref(n)) == 0 and n.value == 16, "8 + 1 rounded up to 8"
    assert lib.hh_episode_outcomes_scratch_bytes(64, 16384, 64 * 16384, C.byref(n)) == 0 and n.value == 8 * 16384 + 64 * 16384
    assert lib.hh_episode_outcomes_scratch_bytes(5, 67, 1000, C.byref(n)) == 0 and n.value == 8 * 67 + 5 * 67 + 1
    for args in ((0, 10, 10), (10, 0, 10), (-1, 10, 10), (10, 10, 0), (1, (1 << 31) - 1023, 5), (1 << 16, 1 << 16, 5), (4, 4, 1 << 31)):
        n.value = -7
        assert lib.hh_episode_outcomes_scratch_bytes(*args, C.byref(n)) == -1 and n.value == -7, args
        assert lib.hh_last_error().startswith(b"hh_episode_outcomes_scratch_bytes: ")
    assert lib.hh_episode_outcomes_scratch_bytes(10, 10, 10, None) == -1
    assert lib.hh_episode_outcomes(None, None) == -1 and lib.hh_last_error().startswith(b"hh_episode_outcomes: ")
    b = _lib.HHEpisodeOutcomeBufs(T=4, N=4, n_agents=2, reserved0=0, ep_cap=16)
    assert lib.hh_episode_outcomes(C.byref(b), None) == -1 and lib.hh_last_error() == b"hh_episode_outcomes: null buffer"
    b.reserved0 = 1
    assert lib.hh_episode_outcomes(C.byref(b), None) == -1 and b"reserved0" in lib.hh_last_error()
    b.reserved0, b.n_agents = 0, 6
    assert lib.hh_episode_outcomes(C.byref(b), None) == -1 and b"n_agents" in lib.hh_last_error()
    assert lib.hh_outcome_tap(None, None, None, None) == -1 and lib.hh_last_error().startswith(b"hh_outcome_tap: ")


# ------------------------------------------------------------------------------------------------------------------ the constructors
def test_outcomes_needs_a_consumer_and_a_bool_before_the_world_is_touched():
    """None stands in for the world: the refusal comes first"""
    from hhmarl_2d_amd.commander import CommanderRollout
    from hhmarl_2d_amd.rollout import PPORollout
    both = "metrics=True with batch_mode='complete_episodes'.*window_metrics=True"
    for make in (lambda **kw: PPORollout(None, None, 8, **kw), lambda **kw: CommanderRollout(None, None, None, 8, **kw)):
        with pytest.raises(ValueError, match=both):
            make(outcomes=True)
        with pytest.raises(ValueError, match=both):
            make(outcomes=True, batch_mode="complete_episodes")
        with pytest.raises(ValueError, match=both):
            make(outcomes=True, batch_mode="complete_episodes", train_batch_size=64)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="outcomes: False or True"):
                make(outcomes=bad, window_metrics=True)
    with pytest.raises(TypeError):
        PPORollout(None, None, 8, 0.99, 0.95, True, None, "rllib", "truncate_episodes", False, None, False, True)   # keyword-only
    with pytest.raises(TypeError):
        PPORollout(None, None, 8, outcome=True)


def test_the_positional_signatures_stay_and_the_keyword_is_keyword_only():
    from hhmarl_2d_amd.commander import CommanderRollout
    from hhmarl_2d_amd.rollout import PPORollout
    for cls in (PPORollout, CommanderRollout):
        outer = inspect.signature(cls.__init__, follow_wrapped=False).parameters
        assert outer["outcomes"].kind is inspect.Parameter.KEYWORD_ONLY and outer["outcomes"].default is False
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[-1] == "record_logits" and "outcomes" not in p and "window_metrics" not in p
        assert "outcomes" in cls.__doc__


def test_outcome_metrics_names_the_summary():
    from hhmarl_2d_amd import _lib
    from hhmarl_2d_amd.evaluation import LOWLEVEL_METRIC_KEYS, LOWLEVEL_STAT_KEYS
    from hhmarl_2d_amd.rollout import OUTCOME_CLASSES, outcome_metrics
    s = [8.0, 1.0, 2.0, 5.0, 10.5, -3.0, 0.25, 12.0, 30.0, 60.0, 0.0, 0.0]
    m = outcome_metrics(s)
    assert m == R.metrics(np.array(s))
    assert set(m) == {"agents_win", "opps_win", "draw", "outcome_pct", "episode_reward_mean_by_outcome", "episode_len_mean_by_outcome"}
    assert {"agents_win", "opps_win", "draw"} <= set(LOWLEVEL_STAT_KEYS) and tuple(m["outcome_pct"]) == LOWLEVEL_METRIC_KEYS == OUTCOME_CLASSES
    assert all(type(m[k]) is int for k in ("agents_win", "opps_win", "draw"))
    assert m["outcome_pct"] == {"win": (1 / 8) * 100, "lose": (2 / 8) * 100, "draw": (5 / 8) * 100}
    assert _lib.EO_SUMMARY[1:4] == ("agents_win", "opps_win", "draw") and _lib.EO_SUMMARY[10] == "other_codes"
    z = outcome_metrics([0.0] * 4 + [math.nan] * 6 + [0.0, 0.0])
    assert all(math.isnan(v) for v in z["outcome_pct"].values())


class _Stub:
    """what rollout_state_dict / rollout_load_plan / rollout_outcome_names read of a rollout, on CPU tensors"""

    def __init__(self, outcome=None):
        import torch
        self.w = type("W", (), {"device": torch.device("cpu")})()
        self.obs, self.done = torch.zeros(3, 2), torch.zeros(2, 2, dtype=torch.uint8)
        self.outcome = outcome
        self.collects, self._started, self.episodes, self.window_metrics, self._graph = 2, True, None, None, object()


def test_a_state_dict_without_the_option_has_todays_keys_and_the_other_setting_is_refused_by_name(monkeypatch):
    import torch
    from hhmarl_2d_amd import rollout as R_
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    off, on = _Stub(), _Stub(torch.full((2, 2), 2, dtype=torch.int8))
    assert R_.rollout_outcome_names(off) == ((), {}) and R_.rollout_outcome_names(on) == (("outcome",), {"outcomes": True})

    def sd_of(ro):
        names, opts = R_.rollout_outcome_names(ro)
        return R_.rollout_state_dict(ro, ("obs", "done") + names, dict({"T": 2}, **opts)), ("obs", "done") + names, dict({"T": 2}, **opts)
    sd_off, n_off, o_off = sd_of(off)
    sd_on, n_on, o_on = sd_of(on)
    assert list(sd_off["window"]) == ["obs", "done"] and sd_off["options"] == {"T": 2}
    assert list(sd_on["window"]) == ["obs", "done", "outcome"] and sd_on["options"] == {"T": 2, "outcomes": True}
    R_.rollout_load_plan(off, sd_off, n_off, o_off)()
    R_.rollout_load_plan(on, sd_on, n_on, o_on)()
    with pytest.raises(ValueError, match="outcomes"):
        R_.rollout_load_plan(off, sd_on, n_off, o_off)
    with pytest.raises(ValueError, match="outcomes"):
        R_.rollout_load_plan(on, sd_off, n_on, o_on)
