"""hh_episodes_metrics on the MI355X, the raw entry point on synthetic whole-episode batches against the float64 restatement of
tests/episode_metrics_ref.py.

Cases: n_agents 2 and 3; episode lengths {1, 2, 63, 64, 65, 257, 300} three times over in one batch (2256 rows: the wave boundary of the
episode pass, three tiles of the row pass, the last one partial, and more episodes than one workgroup of the episode pass takes);
rewards of mixed sign with magnitudes 1e-3 .. 1e3 — and, because float32 values of that range in episodes of at most 300 rows add up
EXACTLY in float64 in any order (24 + 20 + 9 bits), a third case with magnitudes 1e-6 .. 1e6 whose sums do round, so that the
reordering bounds and the byte-for-byte checks have something to catch on the episode pass; row_cap and ep_cap larger than the counts, every row beyond them NaN and every
table entry beyond them a garbage index.

Bounds (derived, tests/episode_metrics_ref.bounds): ep_return within ep_len 2^-52 sum|reward| per episode and agent (two summation
orders of the same float64 terms); every summary mean within n 2^-52 sum|x| of the sequential float64 mean of the device's OWN
n values x (its ep_return, their per-episode sums over the agents, the lengths) — the mean's own summation, at exactly that bound —
and within that plus the mean of the values' own bounds of the restatement's mean, whose values may differ by those; episodes, rows and the lengths
exact; min / max EXACTLY the min / max of the device's own ep_return (and of its per-episode sums over the agents, added in agent
order), and within the largest per-episode bound of the restatement's; vf_explained_var within 1e-9 relative on inputs whose
Var(target) is at least 1e-2 of mean(target^2), which is asserted first.

At scale (test_at_scale_against_the_restatement): n_agents 1, 4 and 5 (the other kernel instances); 1100 episodes of lengths cycling
{1, 63, 64, 65, 257, 300, 1025} (278676 rows: more than 256 episodes and 256 row tiles, neither a multiple of 256 — the strided folds
of hh_k_epm_final), 9000 episodes of 1 .. 3 rows (hh_k_epm_episodes grid-strides beyond 8192) and 7400 episodes of 300 rows (2168
tiles: hh_k_epm_rows grid-strides beyond 2048).  The same bounds; vf_explained_var within the bound derived in
tests/episode_metrics_ref.explained_variance_bound from the two M2 sums' reordering bounds.  Measured on an MI355X: the sums and means
reach at most 0.33 of their bounds (the 9000 episodes of 1 .. 3 rows), vf_explained_var at most 1.4e-3 of its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from episode_metrics_ref import EPS, bounds, restate_metrics

pytestmark = pytest.mark.gpu
LENGTHS = (1, 2, 63, 64, 65, 257, 300)
POISON_START, POISON_LEN = 1 << 30, -5
CASES = [(2, False), (3, False), (3, True)]   # (n_agents, rewards of 1e-6 .. 1e6 instead of 1e-3 .. 1e3)
CASE_IDS = ["2-agents", "3-agents", "3-agents-wide-range"]


def _inputs(nA, seed, bad_vf=False, wide=False, lens=None):
    """-> numpy reward / vf / target [R, nA] f32 and the table of the 21 episodes (or of those of the lengths `lens`), laid out back to
    back as the emitter does"""
    rng = np.random.default_rng(seed)
    if lens is None:
        lens = rng.permutation(np.array(LENGTHS * 3, dtype=np.int32))
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    R = int(lens.sum())
    reward = (rng.choice([-1.0, 1.0], (R, nA)) * 10.0 ** rng.uniform(-6 if wide else -3, 6 if wide else 3, (R, nA))).astype(np.float32)
    target = (1.0 + 2.0 * rng.standard_normal((R, nA))).astype(np.float32)
    vf = (target + 0.5 * rng.standard_normal((R, nA))).astype(np.float32)
    if bad_vf:
        vf = (100.0 * rng.standard_normal((R, nA))).astype(np.float32)
    return reward, vf, target, start, lens


class _Call:
    """device buffers of one hh_episodes_metrics call: capacities beyond the counts, poisoned past them"""

    def __init__(self, reward, vf, target, start, lens, row_cap, ep_cap, n_eps=None):
        from hhmarl_2d_amd import _lib as L
        self.L = L
        R, nA = reward.shape
        E = len(lens) if n_eps is None else n_eps
        dev = torch.device("cuda", 0)

        def col(x):
            full = np.full((row_cap, nA), np.nan, dtype=np.float32)
            full[:R] = x
            return torch.from_numpy(full).to(dev)

        def table(x, poison):
            full = np.full(ep_cap, poison, dtype=np.int32)
            full[:len(x)] = x
            full[E:] = poison
            return torch.from_numpy(full).to(dev)
        self.reward, self.vf, self.target = col(reward), col(vf), col(target)
        self.ep_start, self.ep_len = table(start, POISON_START), table(lens, POISON_LEN)
        self.counts = torch.tensor([R if E else 0, E, 0], dtype=torch.int32, device=dev)
        self.ep_return = torch.full((ep_cap, nA), -777.0, dtype=torch.float64, device=dev)
        self.summary = torch.full((len(L.EP_METRICS),), -777.0, dtype=torch.float64, device=dev)
        self.totals = torch.tensor([5, 77], dtype=torch.int64, device=dev)
        n = C.c_int64(0)
        L.check(L.lib().hh_episodes_metrics_scratch_bytes(ep_cap, row_cap, nA, C.byref(n)))
        self.scratch = torch.full((n.value // 8,), float("nan"), dtype=torch.float64, device=dev)
        self.m = L.HHEpisodeMetricsBufs(
            n_agents=nA, reserved0=0, row_cap=row_cap, ep_cap=ep_cap, reward=self.reward.data_ptr(), vf=self.vf.data_ptr(),
            target=self.target.data_ptr(), ep_start=self.ep_start.data_ptr(), ep_len=self.ep_len.data_ptr(), counts=self.counts.data_ptr(),
            ep_return=self.ep_return.data_ptr(), summary=self.summary.data_ptr(), totals=self.totals.data_ptr(),
            scratch=self.scratch.data_ptr(), scratch_bytes=n.value)
        self.E, self.nA = E, nA

    def run(self):
        st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        rc = self.L.lib().hh_episodes_metrics(C.byref(self.m), st)
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return self.ep_return.cpu().numpy(), self.summary.cpu().numpy(), self.totals.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    """per (n_agents, wide range): the inputs, the restatement (computed once, never modified) and one device run"""
    out = {}
    for nA, wide in CASES:
        inp = _inputs(nA, seed=100 + nA + 10 * wide, wide=wide)
        ref = restate_metrics(*inp)
        call = _Call(*inp, row_cap=4000, ep_cap=40)
        assert call.run() == 0
        out[nA, wide] = (inp, ref, call, call.outputs())
    return out


def _slots(L, summary, base, nA):
    s = L.EP_METRICS_SLOT[base + "_0"]
    return summary[s:s + nA], summary[s + nA:s + 5]


def _check_episodes_and_means(inp, ref, outputs, wide):
    """everything but vf_explained_var and the totals, under the module's rules -> the largest error-to-bound ratio met"""
    from hhmarl_2d_amd import _lib as L
    (reward, vf, target, start, lens), (ep_return, summary, totals) = inp, outputs
    nA, E, slot = reward.shape[1], len(lens), L.EP_METRICS_SLOT
    t64 = target.astype(np.float64)
    ratio = t64.var(axis=0) / (t64 ** 2).mean(axis=0)
    assert (ratio >= 1e-2).all(), f"the inputs' Var(target) / mean(target^2) = {ratio}"
    b = bounds(reward, start, lens, ref)
    assert np.isfinite(ep_return[:E]).all() and np.isfinite(summary[:slot["agent_return_mean_0"]]).all()
    # per episode
    err = np.abs(ep_return[:E] - ref["ep_return"])
    print(f"nA={nA}: ep_return max err {err.max():.3e} (bound there {b['ep_return'].flat[err.argmax()]:.3e})")
    assert (err <= b["ep_return"]).all()
    if wide:
        assert err.max() > 0, "the wide-range sums round: the two summation orders must show"
    assert (ep_return[E:] == -777.0).all(), "entries beyond the counts are not written"
    # exact slots
    assert summary[slot["episodes"]] == E and summary[slot["rows"]] == lens.sum()
    assert summary[slot["episode_len_min"]] == lens.min() and summary[slot["episode_len_max"]] == lens.max()
    assert abs(summary[slot["episode_len_mean"]] - ref["episode_len_mean"]) <= b["episode_len_mean"]
    assert summary[slot["episode_len_mean"]] == lens.sum() / E, "integers below 2^53: exact in any order"
    # min / max: exactly those of the device's own values, and within the per-episode bounds of the restatement's
    own = ep_return[:E]
    own_reward = own[:, 0].copy()
    for a in range(1, nA):
        own_reward += own[:, a]
    assert summary[slot["episode_reward_min"]] == own_reward.min() and summary[slot["episode_reward_max"]] == own_reward.max()
    assert abs(summary[slot["episode_reward_min"]] - ref["episode_reward_min"]) <= b["episode_reward"].max()
    assert abs(summary[slot["episode_reward_max"]] - ref["episode_reward_max"]) <= b["episode_reward"].max()
    for base, want in (("agent_return_min", own.min(axis=0)), ("agent_return_max", own.max(axis=0))):
        got, rest = _slots(L, summary, base, nA)
        assert np.array_equal(got, want) and np.isnan(rest).all(), base
        assert (np.abs(got - ref[base]) <= b["ep_return"].max(axis=0)).all(), base
    # means: against the sequential mean of the device's own values at n 2^-52 sum|x|, then against the restatement's
    seq_mean = lambda x: np.add.accumulate(x, axis=0)[-1] / E
    own_tol = lambda x: E * EPS * np.abs(x).sum(axis=0)
    err = abs(summary[slot["episode_reward_mean"]] - seq_mean(own_reward))
    print(f"nA={nA}: episode_reward_mean against its own values: err {err:.3e} (bound {own_tol(own_reward):.3e})")
    assert err <= own_tol(own_reward)
    got, _ = _slots(L, summary, "agent_return_mean", nA)
    assert (np.abs(got - seq_mean(own)) <= own_tol(own)).all()
    err = abs(summary[slot["episode_reward_mean"]] - ref["episode_reward_mean"])
    print(f"nA={nA}: episode_reward_mean err {err:.3e} (bound {b['episode_reward_mean']:.3e})")
    assert err <= b["episode_reward_mean"]
    got, rest = _slots(L, summary, "agent_return_mean", nA)
    assert (np.abs(got - ref["agent_return_mean"]) <= b["agent_return_mean"]).all() and np.isnan(rest).all()
    worst = max(float((np.abs(ep_return[:E] - ref["ep_return"]) / np.maximum(b["ep_return"], 1e-300)).max()), err / b["episode_reward_mean"],
                float((np.abs(got - ref["agent_return_mean"]) / b["agent_return_mean"]).max()))
    return worst


@pytest.mark.parametrize("nA,wide", CASES, ids=CASE_IDS)
def test_against_the_restatement(cases, nA, wide):
    from hhmarl_2d_amd import _lib as L
    inp, ref, call, (ep_return, summary, totals) = cases[nA, wide]
    (reward, vf, target, start, lens), E = inp, len(inp[4])
    _check_episodes_and_means(inp, ref, (ep_return, summary, totals), wide)
    # explained variance
    got, rest = _slots(L, summary, "vf_explained_var", nA)
    rel = np.abs(got - ref["vf_explained_var"]) / np.abs(ref["vf_explained_var"])
    print(f"nA={nA}: vf_explained_var {got}, relative error {rel}")
    assert (rel <= 1e-9).all() and np.isnan(rest).all()
    assert (got > 0.5).all() and (got < 1.0).all(), "vf = target + noise of a quarter of its standard deviation"
    # totals accumulate: 5, 77 before the call
    assert totals.tolist() == [5 + E, 77 + int(lens.sum())]


@pytest.mark.parametrize("nA,wide", CASES, ids=CASE_IDS)
def test_deterministic_whatever_the_grid(cases, nA, wide):
    """the same bytes from a second run, from a second call on the same buffers (the totals accumulate), and from other capacities —
    ep_cap 40 / 10000 and row_cap 4000 / 3000000 are grids of 10 / 2048 and 4 / 2048 workgroups"""
    inp, ref, call, (ep_return, summary, totals) = cases[nA, wide]
    E, R = len(inp[4]), int(inp[4].sum())
    again = _Call(*inp, row_cap=4000, ep_cap=40)
    assert again.run() == 0
    for a, b in zip(again.outputs(), (ep_return, summary, totals)):
        assert a.tobytes() == b.tobytes()
    assert again.run() == 0
    e2, s2, t2 = again.outputs()
    assert e2.tobytes() == ep_return.tobytes() and s2.tobytes() == summary.tobytes() and t2.tolist() == [5 + 2 * E, 77 + 2 * R]
    for row_cap, ep_cap in ((4000, 10000), (3000000, 40), (2256, 21)):
        other = _Call(*inp, row_cap=row_cap, ep_cap=ep_cap)
        assert other.run() == 0
        e3, s3, t3 = other.outputs()
        assert e3[:E].tobytes() == ep_return[:E].tobytes() and s3.tobytes() == summary.tobytes() and t3.tobytes() == totals.tobytes(), (row_cap, ep_cap)


def _scale_lens(kind):
    if kind == "cycle":      # 278676 rows: 273 tiles and 1100 episodes, both above one trip of hh_k_epm_final's 256 lanes and no multiple of it
        return np.resize(np.array(SCALE_LENGTHS, dtype=np.int32), 1100)
    if kind == "many":       # above the 8192 waves of hh_k_epm_episodes' largest grid: its episode loop strides
        return np.random.default_rng(5).integers(1, 4, 9000).astype(np.int32)
    return np.full(7400, 300, dtype=np.int32)   # 2220000 rows = 2168 tiles, above hh_k_epm_rows' largest grid of 2048: its tile loop strides


SCALE_LENGTHS = (1, 63, 64, 65, 257, 300, 1025)
# (n_agents, lengths, do the per-episode sums round differently in the two orders?, other (row_cap, ep_cap) with other grids)
SCALE = {"1-agent-1100-episodes": (1, "cycle", True, ((278676, 1100), (3000000, 10000))),
         "5-agents-1100-episodes": (5, "cycle", True, ((278676, 1100), (3000000, 10000))),
         "4-agents-9000-episodes": (4, "many", False, ((27000, 9000), (100000, 40000))),
         "1-agent-7400x300-rows": (1, "long", True, ((2220000, 7400), (2220000, 7400 * 2)))}


@pytest.mark.parametrize("case", list(SCALE))
def test_at_scale_against_the_restatement(case):
    """the strided loops and the NA = 1, 4, 5 instances: more than 256 episodes and 256 row tiles (the folds of hh_k_epm_final), more
    than 8192 episodes (hh_k_epm_episodes grid-strides), more than 2048 tiles (hh_k_epm_rows grid-strides).  Rewards of 1e-6 .. 1e6.
    The same derived bounds as above; vf_explained_var within episode_metrics_ref.explained_variance_bound of the restatement's (the
    1e-9 above was set for 2256 rows); min / max exactly those of the device's own values; the same bytes from other capacities."""
    from episode_metrics_ref import explained_variance_bound
    from hhmarl_2d_amd import _lib as L
    nA, kind, rounds, others = SCALE[case]
    inp = _inputs(nA, seed=300 + nA, wide=True, lens=_scale_lens(kind))
    reward, vf, target, start, lens = inp
    E, R = len(lens), int(lens.sum())
    assert max(c[0] for c in others) >= R and all(c[0] >= R and c[1] >= E for c in others)
    if kind == "cycle":
        assert E > 256 and E % 256 and -(-R // 1024) > 256 and -(-R // 1024) % 256
    elif kind == "many":
        assert E > 8192
    else:
        assert -(-R // 1024) > 2048
    ref = restate_metrics(*inp)
    call = _Call(*inp, row_cap=R + 1000, ep_cap=E + 100)
    assert call.run() == 0
    ep_return, summary, totals = call.outputs()
    worst = _check_episodes_and_means(inp, ref, (ep_return, summary, totals), rounds)
    got, rest = _slots(L, summary, "vf_explained_var", nA)
    bound = np.array([explained_variance_bound(target[:, a], vf[:, a]) for a in range(nA)])
    err = np.abs(got - ref["vf_explained_var"])
    print(f"{case}: sums and means at most {worst:.3e} of their bounds; vf_explained_var {got}, error {err}, bound {bound}, "
          f"at most {(err / bound).max():.3e} of it")
    assert (bound > 0).all() and (bound < 1e-9).all(), "the derived bound is no wider than the fixed one it replaces"
    assert (err <= bound).all() and np.isnan(rest).all()
    assert (got > 0.5).all() and (got < 1.0).all(), "vf = target + noise of a quarter of its standard deviation"
    assert totals.tolist() == [5 + E, 77 + R]
    for row_cap, ep_cap in others:
        other = _Call(*inp, row_cap=row_cap, ep_cap=ep_cap)
        assert other.run() == 0
        e3, s3, t3 = other.outputs()
        assert e3[:E].tobytes() == ep_return[:E].tobytes() and s3.tobytes() == summary.tobytes() and t3.tobytes() == totals.tobytes(), (row_cap, ep_cap)


def test_a_value_function_far_worse_than_the_mean_clamps_at_minus_one():
    from hhmarl_2d_amd import _lib as L
    inp = _inputs(2, seed=7, bad_vf=True)
    ref = restate_metrics(*inp)
    assert (ref["vf_explained_var"] == -1.0).all()
    call = _Call(*inp, row_cap=2500, ep_cap=64)
    assert call.run() == 0
    got, rest = _slots(L, call.outputs()[1], "vf_explained_var", 2)
    assert (got == -1.0).all() and np.isnan(rest).all()


def test_zero_episodes_give_nan_and_leave_the_totals():
    from hhmarl_2d_amd import _lib as L
    inp = _inputs(3, seed=9)
    call = _Call(*inp, row_cap=2500, ep_cap=64, n_eps=0)
    assert call.counts.tolist() == [0, 0, 0]
    assert call.run() == 0
    ep_return, summary, totals = call.outputs()
    assert summary[0] == 0 and summary[1] == 0 and np.isnan(summary[2:]).all() and len(summary) == len(L.EP_METRICS)
    assert totals.tolist() == [5, 77] and (ep_return == -777.0).all()


def test_argument_errors_enqueue_nothing():
    from hhmarl_2d_amd import _lib as L
    inp = _inputs(2, seed=11)
    call = _Call(*inp, row_cap=2500, ep_cap=64)
    ptrs = ("reward", "vf", "target", "ep_start", "ep_len", "counts", "ep_return", "summary", "totals", "scratch")
    bad = [(k, None) for k in ptrs] + [("n_agents", 0), ("n_agents", 6), ("n_agents", -1), ("reserved0", 1), ("row_cap", 0), ("ep_cap", 0),
                                       ("row_cap", 1 << 31), ("scratch_bytes", call.m.scratch_bytes - 8), ("scratch_bytes", 0),
                                       ("summary", call.summary.data_ptr() + 4), ("scratch", call.scratch.data_ptr() + 4)]
    for field, value in bad:
        keep = getattr(call.m, field)
        setattr(call.m, field, value)
        assert call.run() == -1, (field, value)
        assert L.lib().hh_last_error().startswith(b"hh_episodes_metrics: "), (field, value)
        setattr(call.m, field, keep)
    st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    assert L.lib().hh_episodes_metrics(None, st) == -1
    torch.cuda.synchronize()
    ep_return, summary, totals = call.outputs()
    assert (ep_return == -777.0).all() and (summary == -777.0).all() and totals.tolist() == [5, 77]
    assert call.run() == 0 and call.outputs()[1][0] == 21, "the restored struct is accepted"
