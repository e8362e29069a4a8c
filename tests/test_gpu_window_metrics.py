"""hh_window_metrics on the MI355X, the raw entry point through ctypes on synthetic windows against the stateful float64 restatement of
tests/window_metrics_ref.py.

Shapes (T, N, n_agents): (1, 1, 1) single elements, (5, 65, 2) a ragged wave, (3, 2050, 3) counts that cross the scan workgroup's 1024
and the walk's 256, (7, 130, 5) the agent maximum.  Four successive calls per shape on ONE carried state, seeded inputs; rewards are
float32 of mixed sign spanning 1e-3 .. 1e3, so a float32 carry or another order of additions shows in the bytes.

The done patterns are built, not drawn (`_done`), and each is asserted as a precondition (`_patterns`): a done at t = 0 of a later
window whose other rows all lie in earlier windows; a done at t = T-1, after which the next window starts from zero carry; two
consecutive done rows (an episode of length 1); an arena with no done in all four windows; a window in which no arena is done followed
by one in which every arena is.  The last two exclude each other on one state, so every shape runs two pattern families on a state
each — "mixed" holds the first four, "none-then-all" the fifth (and the first three again).  A single arena of single-row windows
(1, 1, 1) holds what it can: it cannot also be never done.

Exact, byte for byte against the restatement: ep_return, ep_len, ep_arena, ep_end, counts, run_return, run_len, totals, the
integer-valued slots (episodes, rows, episode_len_min / max) and every min / max.  Bounded by tests/episode_metrics_ref.py's derived
reordering bounds (window_metrics_ref.window_bounds): the means and vf_explained_var, on inputs whose Var(target) / mean(target^2) is
at least 1e-2, asserted first — one row (1, 1, 1) has no variance at all: there both sides must give nan."""
import ctypes as C

import numpy as np
import pytest
import torch

from window_metrics_ref import WindowMetricsRef, window_bounds

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (5, 65, 2), (3, 2050, 3), (7, 130, 5)]
FAMILIES = ("mixed", "none-then-all")
WINDOWS = 4
POISON = -777


def _done(T, N, family):
    """-> u8 [4, T, N], built from indices alone"""
    d = np.zeros((WINDOWS, T, N), dtype=np.uint8)
    w, t, n = np.meshgrid(np.arange(WINDOWS), np.arange(T), np.arange(N), indexing="ij")
    d[(w * T + t + 3 * n) % (2 + n % 7) == 0] = 1                 # every arena its own period 2 .. 8, its own phase
    if N == 1:                                                     # T = 1 as well: one flag per window
        # mixed: none | done (its other row lies in window 0) | done again (length 1) | none;  none-then-all: done | none | done | done
        d[:, 0, 0] = (0, 1, 1, 0) if family == "mixed" else (1, 0, 1, 1)
        return d
    else:
        d[:, :, :4] = 0
        d[1, 0, 1] = 1                                             # arena 1: t = 0 of window 1, T rows in window 0
        d[0, T - 1, 2] = d[2, T - 1, 2] = 1                        # arena 2: the last row of windows 0 and 2
        d[1, 0, 3] = d[1, 1, 3] = 1                                # arena 3: two consecutive rows inside window 1 ...
        d[2, T - 1, 3] = d[3, 0, 3] = 1                            # ... and across the cut between windows 2 and 3
    if family == "none-then-all":                                  # arena 0 included: nobody is never done here
        d[1] = 0
        d[2] = 0
        d[2, (np.arange(N) * 5) % T, np.arange(N)] = 1             # every arena once, at its own t
        d[2, T - 1, 2:4] = 1                                       # arenas 2 and 3 keep the last row of window 2
    return d


def _patterns(done, refs, family):
    """the preconditions of the module docstring, on the done flags and the restatement's tables"""
    W, T, N = done.shape
    per_window = done.reshape(W, T, N).sum(axis=1)
    late = any(((r["ep_end"] == 0) & (r["ep_len"] >= 2)).any() for r in refs[1:])
    assert late, "a done at t = 0 of a later window: all but one of its rows lie in earlier windows"
    zero_after = [w for w in range(W - 1) if ((done[w, T - 1] != 0) & (refs[w]["run_len"] == 0)).any()]
    assert zero_after, "a done at t = T-1: the next window starts from zero carry"
    assert any((r["ep_len"] == 1).any() for r in refs), "two consecutive done rows: an episode of length 1"
    flat = done.reshape(W * T, N)
    assert ((flat[1:] != 0) & (flat[:-1] != 0)).any()
    if family == "mixed":
        if N > 1:
            assert (per_window.sum(axis=0) == 0).any() and refs[-1]["run_len"].max() == W * T, "an arena with no done in all four windows"
    else:
        assert any(per_window[w].sum() == 0 and (per_window[w + 1] > 0).all() for w in range(W - 1)), "no arena done, then every arena"
        assert any(r["episodes"] == 0 for r in refs)


def _inputs(T, N, nA, family):
    rng = np.random.default_rng(1000 * T + N + 7 * nA + (family != "mixed"))
    shape = (WINDOWS, T, N, nA)
    reward = (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)
    target = (1.0 + 2.0 * rng.standard_normal(shape)).astype(np.float32)
    vf = (1.0 + 2.0 * rng.standard_normal((WINDOWS, T + 1, N, nA))).astype(np.float32)
    vf[:, :T] = (target + 0.5 * rng.standard_normal(shape)).astype(np.float32)    # row T is the bootstrap row: never read
    return reward, vf, target, _done(T, N, family)


class _Call:
    """device buffers of hh_window_metrics for one shape: the window's columns are rewritten per call, the state is carried"""

    def __init__(self, T, N, nA):
        from hhmarl_2d_amd import _lib as L
        self.L, self.T, self.N, self.nA = L, T, N, nA
        dev = torch.device("cuda", 0)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.reward, self.vf, self.target = z((T, N, nA), torch.float32), z((T + 1, N, nA), torch.float32), z((T, N, nA), torch.float32)
        self.done = z((T, N), torch.uint8)
        self.run_return, self.run_len = z((N, nA), torch.float64), z((N,), torch.int32)
        self.ep_return = z((T * N, nA), torch.float64)
        self.ep_len, self.ep_arena, self.ep_end = z((T * N,), torch.int32), z((T * N,), torch.int32), z((T * N,), torch.int32)
        self.counts, self.summary, self.totals = z((2,), torch.int32), z((len(L.EP_METRICS),), torch.float64), z((2,), torch.int64)
        n = C.c_int64(0)
        L.check(L.lib().hh_window_metrics_scratch_bytes(T, N, nA, C.byref(n)))
        self.scratch = torch.full((n.value // 8,), float("nan"), dtype=torch.float64, device=dev)
        self.m = L.HHWindowMetricsBufs(
            T=T, N=N, n_agents=nA, reserved0=0, reward=self.reward.data_ptr(), vf=self.vf.data_ptr(), target=self.target.data_ptr(),
            done=self.done.data_ptr(), run_return=self.run_return.data_ptr(), run_len=self.run_len.data_ptr(),
            ep_return=self.ep_return.data_ptr(), ep_len=self.ep_len.data_ptr(), ep_arena=self.ep_arena.data_ptr(),
            ep_end=self.ep_end.data_ptr(), counts=self.counts.data_ptr(), summary=self.summary.data_ptr(), totals=self.totals.data_ptr(),
            scratch=self.scratch.data_ptr(), scratch_bytes=n.value)

    OUT = ("ep_return", "ep_len", "ep_arena", "ep_end", "counts", "summary")
    STATE = ("run_return", "run_len", "totals")

    def load(self, reward, vf, target, done):
        for k, v in (("reward", reward), ("vf", vf), ("target", target), ("done", done)):
            getattr(self, k).copy_(torch.from_numpy(v))

    def poison(self):
        for k in self.OUT:
            getattr(self, k).fill_(POISON)

    def run(self):
        st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        rc = self.L.lib().hh_window_metrics(C.byref(self.m), st)
        torch.cuda.synchronize()
        return rc

    def read(self, names):
        return {k: getattr(self, k).cpu().numpy().copy() for k in names}

    def write(self, values):
        for k, v in values.items():
            getattr(self, k).copy_(torch.from_numpy(v))


_RUNS = {}


def _run(shape, family):
    """the four windows of one (shape, family), once: per window the inputs, the restatement and the device's outputs and state — from a
    first run and from a second one started at the restored carry and totals"""
    key = (shape, family)
    if key not in _RUNS:
        T, N, nA = shape
        reward, vf, target, done = _inputs(T, N, nA, family)
        ref, call, out = WindowMetricsRef(N, nA), _Call(T, N, nA), []
        call.write({"totals": np.array([5, 77], dtype=np.int64)})
        ref.totals[:] = (5, 77)
        for w in range(WINDOWS):
            call.load(reward[w], vf[w], target[w], done[w])
            before = call.read(call.STATE)
            call.poison()
            assert call.run() == 0
            got = call.read(call.OUT + call.STATE)
            call.write(before)
            call.poison()
            assert call.run() == 0
            again = call.read(call.OUT + call.STATE)
            out.append(((reward[w], vf[w], target[w], done[w]), ref.window(reward[w], vf[w], target[w], done[w]), got, again, before))
        _RUNS[key] = (done, out)
    return _RUNS[key]


def _slots(L, summary, base, nA):
    s = L.EP_METRICS_SLOT[base + "_0"]
    return summary[s:s + nA], summary[s + nA:s + 5]


CASES = [(s, f) for s in SHAPES for f in FAMILIES]
IDS = [f"T{s[0]}-N{s[1]}-A{s[2]}-{f}" for s, f in CASES]


@pytest.mark.parametrize("shape,family", CASES, ids=IDS)
def test_four_windows_on_one_carried_state(shape, family):
    from hhmarl_2d_amd import _lib as L
    T, N, nA = shape
    done, out = _run(shape, family)
    _patterns(done, [o[1] for o in out], family)
    slot = L.EP_METRICS_SLOT
    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    tot = np.array([5, 77], dtype=np.int64)
    for w, ((reward, vf, target, d), ref, got, again, before) in enumerate(out):
        E = int(ref["episodes"])
        tag = f"{shape} {family} window {w} ({E} episodes)"
        # ---- exact
        assert got["counts"].tolist() == [E, T * N], tag
        for k in ("ep_return", "ep_len", "ep_arena", "ep_end"):
            assert same(got[k][:E], ref[k]), f"{tag}: {k}"
            assert (got[k][E:] == POISON).all(), f"{tag}: {k} is not written beyond the count"
        assert same(got["run_return"], ref["run_return"]) and same(got["run_len"], ref["run_len"]), tag
        tot = tot + np.array([E, T * N])
        assert same(got["totals"], ref["totals"]) and got["totals"].tolist() == tot.tolist(), tag
        s = got["summary"]
        assert s[slot["episodes"]] == E and s[slot["rows"]] == T * N, tag
        exact = ["episode_reward_min", "episode_reward_max", "episode_len_min", "episode_len_max"]
        for k in exact:
            assert np.float64(s[slot[k]]).tobytes() == np.float64(ref[k]).tobytes(), f"{tag}: {k}"
        for base in ("agent_return_min", "agent_return_max"):
            g, rest = _slots(L, s, base, nA)
            assert g.tobytes() == ref[base].tobytes() and np.isnan(rest).all(), f"{tag}: {base}"
        # ---- bounded
        b = window_bounds(ref, vf, target)
        g_mean, rest = _slots(L, s, "agent_return_mean", nA)
        g_ev, rest_ev = _slots(L, s, "vf_explained_var", nA)
        assert np.isnan(rest).all() and np.isnan(rest_ev).all(), tag
        if E == 0:
            assert np.isnan(s[slot["episode_reward_mean"]]) and np.isnan(s[slot["episode_len_mean"]]) and np.isnan(g_mean).all(), tag
            assert all(np.isnan(s[slot[k]]) for k in exact), tag
            assert got["totals"][0] == before["totals"][0] and got["totals"][1] == before["totals"][1] + T * N, tag
        else:
            err = abs(s[slot["episode_reward_mean"]] - ref["episode_reward_mean"])
            print(f"{tag}: episode_reward_mean err {err:.3e} (bound {b['episode_reward_mean']:.3e})")
            assert err <= b["episode_reward_mean"], tag
            assert (np.abs(g_mean - ref["agent_return_mean"]) <= b["agent_return_mean"]).all(), tag
            assert abs(s[slot["episode_len_mean"]] - ref["episode_len_mean"]) <= b["episode_len_mean"], tag
        if T * N == 1:
            assert np.isnan(g_ev).all() and np.isnan(ref["vf_explained_var"]).all(), "one row has no variance"
        else:
            t64 = target.astype(np.float64).reshape(T * N, nA)
            ratio = t64.var(axis=0) / (t64 ** 2).mean(axis=0)
            assert (ratio >= 1e-2).all(), f"{tag}: the inputs' Var(target) / mean(target^2) = {ratio}"
            err = np.abs(g_ev - ref["vf_explained_var"])
            print(f"{tag}: vf_explained_var {g_ev}, error {err}, bound {b['vf_explained_var']}")
            assert np.isfinite(g_ev).all() and (err <= b["vf_explained_var"]).all(), tag
        # ---- the second run from the restored carry and totals
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), f"{tag}: {k} differs in the second run"


def test_rewards_do_round_in_float64():
    """the exact checks have something to catch: over the four windows of the 5-agent shape a float32 carry gives other bytes than the
    float64 chain (float32 values of 1e-3 .. 1e3 add up exactly in float64 over so few rows: per-window partial sums are printed, not
    asserted)"""
    shape = (7, 130, 5)
    done, out = _run(shape, "mixed")
    reward = np.stack([o[0][0] for o in out]).reshape(-1, 130, 5)                  # [4 T, N, nA]
    never = np.flatnonzero(done.reshape(-1, 130).sum(axis=0) == 0)[0]
    want = out[-1][2]["run_return"][never]
    f32 = np.add.accumulate(reward[:, never], axis=0, dtype=np.float32)[-1].astype(np.float64)
    per_window = sum(np.add.accumulate(o[0][0][:, never].astype(np.float64), axis=0)[-1] for o in out)
    assert (f32 != want).any() and want.tobytes() == out[-1][1]["run_return"][never].tobytes()
    print(f"run_return {want}\nfloat32 carry {f32}\nper-window partial sums {per_window}")


def test_argument_errors_enqueue_nothing():
    from hhmarl_2d_amd import _lib as L
    T, N, nA = 5, 65, 2
    reward, vf, target, done = _inputs(T, N, nA, "mixed")
    call = _Call(T, N, nA)
    call.load(reward[0], vf[0], target[0], done[0])
    call.write({"totals": np.array([5, 77], dtype=np.int64), "run_len": np.full(N, 3, dtype=np.int32)})
    call.poison()
    ptrs = ("reward", "vf", "target", "done", "run_return", "run_len", "ep_return", "ep_len", "ep_arena", "ep_end", "counts", "summary", "totals",
            "scratch")
    bad = [(k, None) for k in ptrs] + [("T", 0), ("N", 0), ("T", -1), ("N", -3), ("T", 1 << 30), ("N", (1 << 31) - 1), ("n_agents", 0),
                                       ("n_agents", 6), ("n_agents", -1), ("reserved0", 1), ("scratch_bytes", call.m.scratch_bytes - 8),
                                       ("scratch_bytes", 0)]
    bad += [(k, getattr(call, k).data_ptr() + 2) for k in ("reward", "vf", "target", "run_len", "ep_len", "ep_arena", "ep_end", "counts")]
    bad += [(k, getattr(call, k).data_ptr() + 4) for k in ("run_return", "ep_return", "summary", "totals", "scratch")]
    for field, value in bad:
        keep = getattr(call.m, field)
        setattr(call.m, field, value)
        assert call.run() == -1, (field, value)
        assert L.lib().hh_last_error().startswith(b"hh_window_metrics: "), (field, value)
        setattr(call.m, field, keep)
    st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    assert L.lib().hh_window_metrics(None, st) == -1 and L.lib().hh_last_error().startswith(b"hh_window_metrics: ")
    torch.cuda.synchronize()
    got = call.read(call.OUT + call.STATE)
    assert all((got[k] == POISON).all() for k in call.OUT), "nothing was written"
    assert got["totals"].tolist() == [5, 77] and (got["run_len"] == 3).all() and not got["run_return"].any()
    assert call.run() == 0 and call.read(("counts",))["counts"][1] == T * N, "the restored struct is accepted"
