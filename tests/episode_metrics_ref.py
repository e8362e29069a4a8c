"""Host restatement of hh_episodes_metrics (test infrastructure): RLlib's per-iteration episode metrics of one whole-episode batch, in
float64 numpy with plain sequential sums (np.add.accumulate: one addition after the other, no pairwise tree), from the batch's reward / vf
/ target columns [R, n_agents] and its episode table.  An episode's reward is the sum of its agents' returns (RLlib's episode_reward:
the sum over agent ids); vf_explained_var is ray/rllib/utils/torch_utils.py explained_variance per agent over all rows,
max(-1, 1 - Var(target - vf) / Var(target)), from two-pass sums (the mean first, then the squared deviations from it) — the two
variances share their divisor, which cancels.  With no episode every mean / min / max / explained-variance entry is nan.

`bounds` gives the float64 reordering bounds the device results are held to: a sum of n terms added in another order differs by at most
(n - 1) u sum|x| (1 + O(n u)) from this one's, u = 2^-53 — each of the two orders is within that of the exact sum, twice that apart:
n 2^-52 sum|x| covers it for every n >= 1.  `explained_variance_bound` carries the same bound of the two M2 sums through their ratio."""
import numpy as np

EPS = 2.0 ** -52


def _seq_sum(x, axis=0):
    """sequential float64 sum along axis (0.0 for an empty axis)"""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), dtype=np.float64)
    return np.take(np.add.accumulate(x, axis=axis), -1, axis=axis)


def explained_variance(target, vf):
    """target, vf [R] -> max(-1, 1 - M2(target - vf) / M2(target)) in float64, two passes; nan where both M2 vanish (or R = 0)"""
    t = np.asarray(target, dtype=np.float64)
    d = t - np.asarray(vf, dtype=np.float64)
    if len(t) == 0:
        return float("nan")
    m2 = []
    for x in (d, t):
        mean = _seq_sum(x) / len(x)
        m2.append(_seq_sum((x - mean) ** 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        ev = 1.0 - np.float64(m2[0]) / np.float64(m2[1])
    return float(-1.0 if ev < -1.0 else ev)


def explained_variance_bound(target, vf):
    """the reordering bound for explained_variance(target, vf), derived as the bounds of the means are: each of the two M2 is a sum of n
    non-negative terms x = (value - mean)^2, so the same terms added in another order give a sum within n 2^-52 sum|x| = rho M2 of this
    one's, rho = n 2^-52 (module docstring).  Through the ratio: with both sums within a factor 1 +- rho of the restatement's, M2(d) /
    M2(t) lies within a factor (1 + rho) / (1 - rho) of the restatement's r, i.e. within r 2 rho / (1 - rho); the division and the
    subtraction from 1 round once each on either side: 2^-52 (r + |1 - r|) covers both.  The clamp at -1 moves two values no further
    apart.  0.0 where the restatement's value is nan (nothing to compare) — the caller checks nan against nan.
    The bound is NOT widened for the means the deviations are taken from, themselves sums in another order and off by at most eta =
    2^-52 sum|value| each: that moves one two-pass M2 by at most n eta^2, and per-tile M2 combined around the global mean (sum M2_i +
    n_i (mean_i - mean)^2, the device's way) by at most 4 eta sqrt(n M2) + n eta^2 with a tile's eta.  Both stay orders of magnitude
    inside rho M2 unless |mean| dwarfs the standard deviation; leaving them out makes this bound tighter, never wider."""
    t = np.asarray(target, dtype=np.float64)
    d = t - np.asarray(vf, dtype=np.float64)
    n = len(t)
    if n == 0:
        return 0.0
    m2 = [_seq_sum((x - _seq_sum(x) / n) ** 2) for x in (d, t)]
    if not m2[1] > 0.0:
        return 0.0
    rho, r = n * EPS, float(m2[0] / m2[1])
    return r * 2.0 * rho / (1.0 - rho) + EPS * (r + abs(1.0 - r))


def restate_metrics(reward, vf, target, ep_start, ep_len):
    """reward / vf / target [R, nA] (the emitted rows), ep_start / ep_len [E] -> dict: episodes, rows, ep_return f64 [E, nA],
    episode_reward f64 [E], episode_reward_mean / min / max, episode_len_mean / min / max, agent_return_mean / min / max f64 [nA],
    vf_explained_var f64 [nA]"""
    reward = np.asarray(reward)
    R, nA = reward.shape
    E = len(ep_start)
    ep_return = np.zeros((E, nA), dtype=np.float64)
    for e in range(E):
        s, n = int(ep_start[e]), int(ep_len[e])
        assert 0 <= s and n > 0 and s + n <= R
        ep_return[e] = _seq_sum(reward[s:s + n], axis=0)
    ep_reward = _seq_sum(ep_return, axis=1) if E else np.zeros(0)
    lens = np.asarray(ep_len, dtype=np.float64)
    nan = float("nan")
    out = {"episodes": E, "rows": R if E else 0, "ep_return": ep_return, "episode_reward": ep_reward}
    if E == 0:
        out.update(episode_reward_mean=nan, episode_reward_min=nan, episode_reward_max=nan, episode_len_mean=nan, episode_len_min=nan,
                   episode_len_max=nan, agent_return_mean=np.full(nA, nan), agent_return_min=np.full(nA, nan),
                   agent_return_max=np.full(nA, nan), vf_explained_var=np.full(nA, nan))
        return out
    out.update(episode_reward_mean=float(_seq_sum(ep_reward) / E), episode_reward_min=float(ep_reward.min()), episode_reward_max=float(ep_reward.max()),
               episode_len_mean=float(_seq_sum(lens) / E), episode_len_min=float(lens.min()), episode_len_max=float(lens.max()),
               agent_return_mean=_seq_sum(ep_return, axis=0) / E, agent_return_min=ep_return.min(axis=0), agent_return_max=ep_return.max(axis=0),
               vf_explained_var=np.array([explained_variance(np.asarray(target)[:, a], np.asarray(vf)[:, a]) for a in range(nA)]))
    return out


def bounds(reward, ep_start, ep_len, ref):
    """the reordering bounds (module docstring) for `ref` = restate_metrics(...): ep_return [E, nA] (ep_len 2^-52 sum|reward| per episode
    and agent), episode_reward [E] (the agents' bounds added, plus nA 2^-52 sum|ep_return| for the sum over agents), and for the
    means over E values x: E 2^-52 sum|x| for the mean's own summation, plus mean(b) where the values themselves are only within b of the
    restatement's (a mean of values each off by b is off by up to mean(b) however it is added)"""
    a = np.abs(np.asarray(reward, dtype=np.float64))
    E, nA = ref["ep_return"].shape
    b_ret = np.array([int(ep_len[e]) * EPS * a[int(ep_start[e]):int(ep_start[e]) + int(ep_len[e])].sum(axis=0) for e in range(E)]).reshape(E, nA)
    b_rew = b_ret.sum(axis=1) + nA * EPS * np.abs(ref["ep_return"]).sum(axis=1)
    mean_b = lambda x, b: E * EPS * np.abs(x).sum(axis=0) + b.sum(axis=0) / max(E, 1)
    return {"ep_return": b_ret, "episode_reward": b_rew, "episode_reward_mean": mean_b(ref["episode_reward"], b_rew),
            "agent_return_mean": mean_b(ref["ep_return"], b_ret), "episode_len_mean": E * EPS * float(np.sum(ep_len))}
