"""The two CPU-oracle runs the outcome tests share (test infrastructure): 64 ticks of an auto-resetting level-3 2-vs-2 world, seed 5.
  A: horizon 60, helpers.pursuit_actions drawn from np.random.default_rng(5) on the oracle's own state — kills happen, so wins, losses
     and draws all occur (at 67 arenas: 4 / 7 / 56, the first win at tick 22, the first loss at tick 30);
  B: horizon 6, the keyed uniform tape action_tape_uniform(5, 0, 0, 64, N, n_ctrl) — every arena finishes an episode every 6 ticks, all
     draws (at 67 arenas: 670 episodes; every arena finishes at least two in every window of 16).
Computed once per (name, N) and shared; nobody writes into the arrays."""
import functools

import numpy as np

from helpers import pursuit_actions

TICKS = 64
LEVEL, SEED, HORIZON = 3, 5, {"A": 60, "B": 6}


def world_kwargs(name, n_arenas):
    return dict(n_arenas=int(n_arenas), level=LEVEL, horizon=HORIZON[name], seed=SEED, auto_reset=True)


@functools.lru_cache(maxsize=None)
def fixture(name, n_arenas=67):
    """-> dict: actions i8 [64, N, n_ctrl, 4], reward f32 [64, N, 2], done u8 [64, N], polled i8 [64, N] (OracleWorld.episode_stats()'
    outcome of every arena read after every tick, whether or not it was done), n_ctrl"""
    import oracle_lib
    oracle_lib.build()
    o = oracle_lib.OracleWorld(oracle_lib.make_config(**world_kwargs(name, n_arenas)))
    o.reset()
    N = o.N
    rng = np.random.default_rng(SEED)
    tape = oracle_lib.action_tape_uniform(SEED, 0, 0, TICKS, N, o.n_ctrl) if name == "B" else None
    actions = np.zeros((TICKS, N, o.n_ctrl, 4), dtype=np.int8)
    reward, done = np.zeros((TICKS, N, o.n_agents), dtype=np.float32), np.zeros((TICKS, N), dtype=np.uint8)
    polled = np.zeros((TICKS, N), dtype=np.int8)
    for t in range(TICKS):
        actions[t] = tape[t] if tape is not None else pursuit_actions(rng, o.get_state(), o.n_agents, o.n_ctrl)
        _, reward[t], _, done[t] = o.step(actions[t])
        polled[t] = o.episode_stats()[2]
    out = {"actions": actions, "reward": reward, "done": done, "polled": polled, "n_ctrl": o.n_ctrl}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
