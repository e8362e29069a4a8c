"""Host restatement of hh_outcome_tap and hh_episode_outcomes (test infrastructure; include/hh_abi.h states the semantics): the tap
behind a tick, the fill of an episode table's outcomes with e0 = e1 - m, and the summary in the kernels' own summation order —
tiles of 1024 entries added in index order, inside a tile one entry per lane, a butterfly over each wave's 64 lanes (every step adds
the unordered pair (x, partner), so all lanes hold the same bits), then the tile's 16 waves in index order.  float64 addition is
commutative, so the same additions in the same order give the device's bytes: the tests compare bit for bit, no tolerance."""
import numpy as np

WIN, LOSE, DRAW, NONE = 1, -1, 0, 2      # hh_episode_stats' codes
CLASSES = ("win", "lose", "draw")        # the summary's class order: codes 1, -1, 0
TILE, WAVE = 1024, 64
N_SUMMARY = 12


def tap(done_row, last_outcome):
    """out_row[n] = done_row[n] ? last_outcome[n] : 2"""
    return np.where(np.asarray(done_row) != 0, np.asarray(last_outcome, dtype=np.int8), np.int8(NONE)).astype(np.int8)


def fill(done, outcome, e1, ep_arena, ep_outcome):
    """done u8 / outcome i8 [T, N]; e1: the table's count; ep_arena i32 [>= e1]; ep_outcome i8 [cap] as it stands
    -> (ep_outcome after the call (a copy), flags i32 [2]): the window's m done rows, arena-major then time, are the entries
    [e1 - m, e1); nothing is written when e1 < m or an entry names another arena"""
    done, outcome = np.asarray(done), np.asarray(outcome)
    out = np.array(ep_outcome, dtype=np.int8, copy=True)
    n_idx, t_idx = np.nonzero(done.T != 0)           # sorted by arena, then by t
    m, e1 = len(n_idx), int(e1)
    e0 = e1 - m
    flags = np.array([0, m], dtype=np.int32)
    if e0 < 0 or not np.array_equal(np.asarray(ep_arena)[e0:e1], n_idx):
        flags[0] = 1
        return out, flags
    out[e0:e1] = outcome[t_idx, n_idx]
    return out, flags


def _tile_sums(x):
    """x f64 [e1] -> the kernel's total: per tile of 1024 (absent entries hold 0.0) the butterfly per wave, the 16 waves in index order;
    the tiles in index order, from 0.0"""
    total = np.float64(0.0)
    lanes = np.arange(WAVE)
    for t0 in range(0, len(x), TILE):
        v = np.zeros(TILE, dtype=np.float64)
        part = x[t0:t0 + TILE]
        v[:len(part)] = part
        v = v.reshape(TILE // WAVE, WAVE)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lanes ^ off]
        r = v[0, 0]
        for w in range(1, TILE // WAVE):
            r = r + v[w, 0]
        total = total + r
    return total


def summary(e1, ep_outcome, ep_len, ep_return):
    """-> f64 [12] over the entries [0, e1): episodes | counts win, lose, draw | mean episode reward per class (the agents' returns
    added in agent order, from 0.0) | mean length per class | entries with another code | 0"""
    e1 = int(e1)
    code = np.asarray(ep_outcome)[:e1].astype(np.int64)
    ret = np.asarray(ep_return, dtype=np.float64)[:e1]
    rew = np.zeros(e1, dtype=np.float64)
    for a in range(ret.shape[1]):
        rew = rew + ret[:, a]
    ln = np.asarray(ep_len)[:e1].astype(np.float64)
    out = np.zeros(N_SUMMARY, dtype=np.float64)
    out[0] = e1
    with np.errstate(invalid="ignore"):
        for k, c in enumerate((WIN, LOSE, DRAW)):
            mask = code == c
            n = _tile_sums(mask.astype(np.float64))
            out[1 + k] = n
            out[4 + k] = _tile_sums(np.where(mask, rew, 0.0)) / n if n > 0 else np.nan
            out[7 + k] = _tile_sums(np.where(mask, ln, 0.0)) / n if n > 0 else np.nan
    out[10] = _tile_sums((~np.isin(code, (WIN, LOSE, DRAW))).astype(np.float64))
    return out


def metrics(s):
    """the summary under the names `metrics()` gains (rollout.outcome_metrics restated)"""
    n, counts = int(s[0]), [int(c) for c in s[1:4]]
    return {"agents_win": counts[0], "opps_win": counts[1], "draw": counts[2],
            "outcome_pct": {k: (c / n) * 100 if n else float("nan") for k, c in zip(CLASSES, counts)},
            "episode_reward_mean_by_outcome": {k: float(v) for k, v in zip(CLASSES, s[4:7])},
            "episode_len_mean_by_outcome": {k: float(v) for k, v in zip(CLASSES, s[7:10])}}


class OutcomeTableRef:
    """an episode table that grows by windows, as the emitter's (arena, length, return per finished episode: arena-major, then time) —
    the host stand-in for the table hh_episode_outcomes reads.  `accumulate` False: every window overwrites the table from 0."""

    def __init__(self, N, n_agents, accumulate=False):
        self.N, self.nA, self.accumulate = int(N), int(n_agents), bool(accumulate)
        self.run_return, self.run_len = np.zeros((self.N, self.nA), dtype=np.float64), np.zeros(self.N, dtype=np.int32)
        self.clear()

    def clear(self):
        self.ep_arena, self.ep_len = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
        self.ep_return, self.ep_outcome = np.zeros((0, self.nA), dtype=np.float64), np.zeros(0, dtype=np.int8)

    def window(self, reward, done, outcome):
        """reward f32 [T, N, nA], done u8 / outcome i8 [T, N] -> (flags, summary) after appending (or overwriting with) the window"""
        T, N = done.shape
        arena, length, ret = [], [], []
        for n in range(N):
            for t in range(T):
                self.run_return[n] = self.run_return[n] + reward[t, n].astype(np.float64)
                self.run_len[n] += 1
                if done[t, n]:
                    arena.append(n), length.append(int(self.run_len[n])), ret.append(self.run_return[n].copy())
                    self.run_return[n], self.run_len[n] = 0.0, 0
        if not self.accumulate:
            self.clear()
        self.ep_arena = np.concatenate([self.ep_arena, np.array(arena, dtype=np.int32)])
        self.ep_len = np.concatenate([self.ep_len, np.array(length, dtype=np.int32)])
        self.ep_return = np.concatenate([self.ep_return, np.array(ret, dtype=np.float64).reshape(len(ret), self.nA)])
        e1 = len(self.ep_arena)
        grown = np.concatenate([self.ep_outcome, np.full(e1 - len(self.ep_outcome), NONE, dtype=np.int8)])
        self.ep_outcome, flags = fill(done, outcome, e1, self.ep_arena, grown)
        return flags, summary(e1, self.ep_outcome, self.ep_len, self.ep_return)
