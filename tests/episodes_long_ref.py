"""Scripted whole-episode streams at production episode lengths (test infrastructure): the done flags come from a per-arena list of
episode lengths instead of a coin, so that the paths of csrc/hh_episodes.h which only long episodes and dense windows reach are met
on purpose.  With c = 512 // n_agents (the rows hh_k_ep_gae stages per chunk: HH_EP_GAE_LDS / n_agents), carry_cap = 3 c - 1 and
n = K T the smallest multiple of T that is at least 3 c + 2, eight arenas:

  0  [c - 1, c, c + 1]               one short of, exactly, and one past a chunk
  1  [2 c - 1, 1, c]
  2  [2 c, c]
  3  [2 c + 1, c - 1]
  4  [3 c]                           three whole chunks, exactly carry_cap + 1 rows
  5  [1] * 3 c                       a done on every tick: T episodes per window (more than one 64-episode trip for T = 96)
  6  [T] * (n // T)                  a done on the last tick of every window: keep = 0, the carry returns to 0
  7  [T + 1] + [T] * ((n - T - 1) // T)   a done on tick 0 of every later window behind T carried rows

and, with sequences (max_seq_len = L), a ninth whose lengths cycle max(L - 1, 1), L, L + 1, 2 L while they fit into n.  After its
script an arena ends no episode: the rest of the stream extends its carry (fewer than T + 2 rows, below carry_cap).  The rows are
random values keyed by the geometry, as in tests/test_gpu_episodes_accumulate.py; gamma 0.99, lam 0.95.

GEOMETRIES (n_agents, D, T): T = 96 is more than one ballot round of hh_ep_tick_tables and no multiple of 64; n_agents 1, 5 and 64
are instances of hh_k_ep_emit / hh_k_ep_gae that no rollout launches (the ABI admits 1 .. 64)."""
import functools

import numpy as np

from episodes_accumulate_ref import with_tables
from episodes_ref import restate

GEOMETRIES = [(2, 26, 96), (3, 34, 96), (1, 26, 96), (5, 7, 96), (64, 1, 7)]
COMMANDER = (3, 34, 96)
SEQ_LENS = (1, 4, 20)
GAMMA, LAM = 0.99, 0.95
GAE_LDS = 512   # HH_EP_GAE_LDS of csrc/hh_episodes.h


def script(n_agents, T, L=None):
    """-> (per-arena lists of episode lengths, c, n, K, carry_cap)"""
    c = GAE_LDS // n_agents
    K = -(-(3 * c + 2) // T)
    n = K * T
    arenas = [[c - 1, c, c + 1], [2 * c - 1, 1, c], [2 * c, c], [2 * c + 1, c - 1], [3 * c], [1] * (3 * c), [T] * (n // T),
              [T + 1] + [T] * ((n - T - 1) // T)]
    if L is not None:
        cycle, lens, k = (max(L - 1, 1), L, L + 1, 2 * L), [], 0
        while sum(lens) + cycle[k % 4] <= n:
            lens.append(cycle[k % 4])
            k += 1
        arenas.append(lens)
    assert all(sum(a) <= n and min(a) >= 1 for a in arenas)
    return arenas, c, n, K, 3 * c - 1


def stream(n_agents, D, T, L=None, aux_dim=0):
    """n = K T ticks of rows (numpy, [n, N, ...]) with the scripted done flags; with L the commander's columns (one action byte per
    agent, state_in [n, N, n_agents, 2, 200]), without it four action bytes per agent; aux_dim > 0: an "aux" column [n, N, n_agents, aux_dim]"""
    arenas, c, n, K, cap = script(n_agents, T, L)
    N, nA = len(arenas), n_agents
    rng = np.random.default_rng(100000 * nA + 1000 * D + 10 * T + (L or 0))
    s = {"obs": rng.standard_normal((n, N, nA, D), dtype=np.float32),
         "actions": rng.integers(0, 13, (n, N, nA) + (() if L is not None else (4,))).astype(np.int8),
         "logp": -rng.random((n, N, nA), dtype=np.float32), "vf": rng.standard_normal((n, N, nA), dtype=np.float32),
         "reward": rng.standard_normal((n, N, nA), dtype=np.float32), "valid": rng.integers(0, 2, (n, N, nA)).astype(np.uint8)}
    done = np.zeros((n, N), dtype=np.uint8)
    for a, lens in enumerate(arenas):
        done[np.cumsum(lens) - 1, a] = 1
    s["done"] = done
    if aux_dim:
        s["aux"] = rng.standard_normal((n, N, nA, aux_dim), dtype=np.float32)
    if L is not None:
        s["state_in"] = rng.standard_normal((n, N, nA, 2, 200), dtype=np.float32)
    return s


@functools.lru_cache(maxsize=None)
def reference(n_agents, D, T, L=None, aux_dim=0):
    """-> dict: stream, per (the per-collect restatement with its episode table; the aux column as "aux"), carried [K, N] after every
    collect, arenas (the scripted lengths), c, n, K, carry_cap.  Computed once per case, shared by the tests and never modified."""
    arenas, c, n, K, cap = script(n_agents, T, L)
    s = stream(n_agents, D, T, L, aux_dim)
    cols = ("obs", "actions", "logp", "vf", "reward", "valid", "done") + (("state_in",) if L is not None else ())
    cut = lambda src: [{k: src(k)[i * T:(i + 1) * T] for k in cols} for i in range(K)]
    per = [with_tables(p) for p in restate(cut(lambda k: s[k]), L, gamma=GAMMA, lam=LAM)[0]]
    if aux_dim:
        # the restatement with the aux rows in place of obs: its emitted obs is the expected aux column (tests/test_gpu_episodes_aux.py)
        cut_aux = [{k: v for k, v in col.items() if k != "state_in"} for col in cut(lambda k: s["aux"] if k == "obs" else s[k])]
        aux = restate(cut_aux, None, gamma=GAMMA, lam=LAM)[0]
        per = [dict(p, aux=a["obs"]) for p, a in zip(per, aux)]
    carried = np.zeros((K, len(arenas)), dtype=np.int32)
    for k in range(K):
        d = s["done"][:(k + 1) * T]
        last = np.where(d.any(axis=0), d.shape[0] - 1 - np.argmax(d[::-1], axis=0), -1)
        carried[k] = (k + 1) * T - 1 - last
    for v in s.values():
        v.setflags(write=False)
    for p in per:
        for v in p.values():
            v.setflags(write=False)
    carried.setflags(write=False)
    return dict(stream=s, per=per, carried=carried, arenas=arenas, c=c, n=n, K=K, carry_cap=cap, T=T, L=L)


def most_per_window(per, N):
    """the most episodes one arena ends in one collect"""
    return max(int(np.bincount(p["ep_arena"], minlength=N).max()) for p in per if len(p["ep_arena"]))
