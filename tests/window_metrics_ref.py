"""Host restatement of hh_window_metrics (test infrastructure; include/hh_abi.h states the semantics): the episode metrics of a rollout's
fixed [T, N] windows, STATEFUL — every arena's running return (float64) and length are carried from one window to the next, and the
episodes that finish inside a window are tabulated arena-major, then t, their rows of earlier windows included.

The carry is one sequential float64 addition per row in time order (`run + float64(reward[t])`, the way np.add.accumulate adds: one
after the other, no pairwise tree), so ep_return / run_return are what the device must give byte for byte, wherever the windows cut an
episode.  The summary comes from tests/episode_metrics_ref.py: `restate_metrics` is fed the tabulated returns as one float64 row per
episode (its own sequential sum of a single row is that row: the returns pass through unchanged) for the reward and per-agent
entries, the lengths are summarised the way it summarises them, and `explained_variance` runs per agent over the window's flat [T N]
columns — ALSO when no episode finished (the one difference from hh_episodes_metrics: rows = T N and the explained variances in every
call, only the episode entries nan).  The reordering bounds are that module's too (`window_bounds`): no tolerance is invented here."""
import numpy as np

from episode_metrics_ref import EPS, _seq_sum, bounds, explained_variance, explained_variance_bound, restate_metrics


class WindowMetricsRef:
    def __init__(self, N, n_agents):
        self.N, self.nA = int(N), int(n_agents)
        self.run_return = np.zeros((self.N, self.nA), dtype=np.float64)
        self.run_len = np.zeros(self.N, dtype=np.int32)
        self.totals = np.zeros(2, dtype=np.int64)

    def reset(self):
        self.run_return[:] = 0.0
        self.run_len[:] = 0
        self.totals[:] = 0

    def window(self, reward, vf, target, done):
        """reward / target [T, N, nA] f32, vf [T+1, N, nA] (or [T, N, nA]) f32, done [T, N] -> dict: ep_return f64 [E, nA], ep_len /
        ep_arena / ep_end i32 [E], counts i32 [2], run_return / run_len / totals (copies of the state after the window), and the summary
        entries under restate_metrics' names (episodes, rows, episode_reward[_mean/_min/_max], episode_len_mean/_min/_max,
        agent_return_mean/_min/_max, vf_explained_var)"""
        reward, target, vf, done = np.asarray(reward), np.asarray(target), np.asarray(vf), np.asarray(done)
        T, N, nA = reward.shape
        assert (N, nA) == (self.N, self.nA) and reward.dtype == np.float32 and done.shape == (T, N) and vf.shape[0] in (T, T + 1)
        ep_return, ep_len, ep_arena, ep_end = [], [], [], []
        for n in range(N):
            run, length = self.run_return[n].copy(), int(self.run_len[n])
            for t in range(T):
                run = run + reward[t, n].astype(np.float64)       # one float64 addition per row and agent, in time order
                length += 1
                if done[t, n] != 0:
                    ep_return.append(run)
                    ep_len.append(length)
                    ep_arena.append(n)
                    ep_end.append(t)
                    run, length = np.zeros(nA, dtype=np.float64), 0
            self.run_return[n], self.run_len[n] = run, length
        E = len(ep_len)
        self.totals += np.array([E, T * N], dtype=np.int64)
        ret = np.array(ep_return, dtype=np.float64).reshape(E, nA)
        lens = np.array(ep_len, dtype=np.int32)
        flat_t, flat_v = target.reshape(T * N, nA), vf[:T].reshape(T * N, nA)
        out = restate_metrics(ret, flat_v, flat_t, np.arange(E), np.ones(E, dtype=np.int32))   # one float64 "row" per episode
        assert np.array_equal(out["ep_return"], ret)
        nan = float("nan")
        l64 = lens.astype(np.float64)
        out.update(rows=T * N, episode_len_mean=float(_seq_sum(l64) / E) if E else nan, episode_len_min=float(l64.min()) if E else nan,
                   episode_len_max=float(l64.max()) if E else nan,
                   vf_explained_var=np.array([explained_variance(flat_t[:, a], flat_v[:, a]) for a in range(nA)]))
        out.update(ep_len=lens, ep_arena=np.array(ep_arena, dtype=np.int32), ep_end=np.array(ep_end, dtype=np.int32),
                   counts=np.array([E, T * N], dtype=np.int32), run_return=self.run_return.copy(), run_len=self.run_len.copy(),
                   totals=self.totals.copy())
        return out


def window_bounds(ref, vf, target):
    """the reordering bounds of episode_metrics_ref for `ref` = WindowMetricsRef.window(...): the tabulated returns and the lengths are
    exact (the same additions in the same order on both sides), so episode_metrics_ref.bounds is asked with no reward rows — every
    return's own bound vanishes and what it leaves is the means' own summation, E 2^-52 sum|x| (for episode_reward_mean plus its
    n_agents 2^-52 sum|ep_return| per episode for the sum over the agents, as it always allows); vf_explained_var:
    explained_variance_bound per agent over the window's rows"""
    E, nA = ref["ep_return"].shape
    T_N = int(ref["rows"])
    zero = bounds(np.zeros((E, nA)), np.arange(E), np.ones(E, dtype=np.int32), ref)    # no rewards: the values' own bounds vanish
    target, vf = np.asarray(target), np.asarray(vf)
    flat_t, flat_v = target.reshape(T_N, nA), vf[:target.shape[0]].reshape(T_N, nA)
    return {"episode_reward_mean": float(zero["episode_reward_mean"]), "agent_return_mean": zero["agent_return_mean"], "episode_len_mean": E * EPS * float(ref["ep_len"].sum()),
            "vf_explained_var": np.array([explained_variance_bound(flat_t[:, a], flat_v[:, a]) for a in range(nA)])}
