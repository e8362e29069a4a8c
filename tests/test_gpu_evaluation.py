"""evaluation.py on the device (hhmarl_2d_amd.evaluation.Evaluator) on the MI355X: every episode's counters, outcome and total_n_actions
equal the reference's loop (evaluation.py:33-59) restated over single-arena HighLevelEnv(eval_info) facades that take their commander
actions from act_chain on that arena; with and without the commander, 3-vs-3, 2-vs-3 and a ten-slot 5-vs-4 world; and the result does
not depend on how the episodes are batched.  Synthetic commander and pilot weights; the pilot policy kernel form is pinned, as in
test_gpu_composition, because the batched world and the single-arena facades issue policy calls of different sizes."""
import os

import numpy as np
import pytest
import torch

from helpers import stub_reference_module

pytestmark = pytest.mark.gpu

CMD_SEED, SEED = 17, 3


def _policy_dir(tmp_path):
    """the files _get_policies("HighLevel") loads: L5 fights and escapes (eval_hl), plus the L4 opponent fights of eval_hl = False"""
    from hhmarl_2d_amd import policy_nets as PN
    files = {"L5_AC1_fight.pt": (PN.FIGHT1, 51), "L5_AC2_fight.pt": (PN.FIGHT2, 52), "L5_AC1_escape.pt": (PN.ESC1, 53),
             "L5_AC2_escape.pt": (PN.ESC2, 54), "L4_AC1_fight.pt": (PN.FIGHT1, 41), "L4_AC2_fight.pt": (PN.FIGHT2, 42)}
    for name, (kind, seed) in files.items():
        torch.save(stub_reference_module(kind, seed)[0], os.path.join(str(tmp_path), name))
    return str(tmp_path)


def _evaluator(tmp_path, n, m, eval_hl, **kw):
    from hhmarl_2d_amd.commander import random_weights
    from hhmarl_2d_amd.config import make_args
    from hhmarl_2d_amd.evaluation import Evaluator
    args = make_args(2, num_agents=n, num_opps=m, eval_hl=eval_hl)
    return Evaluator(args, commander=random_weights(CMD_SEED) if eval_hl else None, policy_dir=_policy_dir(tmp_path), **kw)


def _reference_loop(ev, arenas, seed, status=None):
    """evaluation.py:33-59 per episode on a one-arena HighLevelEnv (global arena `arenas[i]`, the same seed): the commander's actions from
    act_chain on that arena's observations in agent id order, or 1 for every agent without eval_hl -> int64 [len(arenas), 13]; status: a
    list that receives each arena's final (steps, alive_agents, alive_opps, done)"""
    from hhmarl_2d_amd.env_hier import HighLevelEnv
    from hhmarl_2d_amd.evaluation import STAT_KEYS
    args = ev.args
    net = ev._commander() if ev.eval_hl else None
    out = np.zeros((len(arenas), len(STAT_KEYS)), dtype=np.int64)
    for i, arena in enumerate(arenas):
        env = HighLevelEnv({"args": args, "seed": seed, "arena_offset": arena, "policy_dir": ev.policy_dir})
        eval_stats = dict.fromkeys(STAT_KEYS, 0)
        state, _ = env.reset()
        done = False
        while not done:
            actions = {}
            if args.eval_hl:
                obs = torch.from_numpy(np.stack([state[k] for k in sorted(state)])).to(device="cuda", dtype=torch.float32)[None].contiguous()
                a = net.act_chain(obs).cpu().numpy()[0]
                for j, ag_id in enumerate(sorted(state)):
                    actions[ag_id] = int(a[j])
            else:
                for n in range(1, args.num_agents + 1):
                    actions[n] = 1
            state, rew, hist, trunc, info = env.step(actions)
            done = hist["__all__"] or trunc["__all__"]
            for k, v in info.items():
                eval_stats[k] += v
            eval_stats["total_n_actions"] += 1
            assert eval_stats["total_n_actions"] <= args.horizon
        out[i] = [eval_stats[k] for k in STAT_KEYS]
        if status is not None:
            status.append(tuple(int(x) for x in env.world.arena_status().cpu().numpy()[0]))
        env.close()
    return out


@pytest.mark.parametrize("n,m,eval_hl", [(3, 3, True), (3, 3, False), (2, 3, True), (5, 4, True)],
                         ids=["3v3-commander", "3v3-low-level", "2v3-commander", "5v4-commander"])
def test_every_episode_equals_the_reference_loop(tmp_path, monkeypatch, n, m, eval_hl):
    monkeypatch.setenv("HH_POLICY_W", "0")     # read at hh_policy_create: one forward form for every call size
    from hhmarl_2d_amd.evaluation import STAT_KEYS, postprocess_eval
    n_eps = 24
    ev = _evaluator(tmp_path, n, m, eval_hl)
    stats = ev.run(n_episodes=n_eps, seed=SEED)
    want = _reference_loop(ev, range(n_eps), SEED)
    for i in range(n_eps):
        assert np.array_equal(ev.per_episode[i], want[i]), f"episode {i}: {dict(zip(STAT_KEYS, ev.per_episode[i]))} != {dict(zip(STAT_KEYS, want[i]))}"
    assert stats == {k: int(want[:, j].sum()) for j, k in enumerate(STAT_KEYS)}
    _check_outcomes(ev, range(n_eps), SEED)
    assert stats["agent_fight"] + stats["agent_escape"] == stats["agent_steps"] > 0
    if not eval_hl:
        assert stats["agent_escape"] == 0 and stats["opp1"] == stats["agent_fight"]  # action 1 for every agent
    assert ev.metrics == postprocess_eval(stats, n_eps)
    ev.close()


def _check_outcomes(ev, arenas, seed):
    """agents_win + opps_win + draw == n_episodes, except where the reference's own flags (env_base.py:104) give an episode no outcome
    (a side's last aircraft falls on the horizon tick: neither win counts, nor draw) or two (both sides' last aircraft fall in one step
    before the horizon): those episodes are replayed on a facade and their final arena status must be that case"""
    per = ev.per_episode
    n_out = per[:, :3].sum(axis=1)
    odd = [i for i in range(len(per)) if n_out[i] != 1]
    assert int(per[:, :3].sum()) == len(per) + sum(int(n_out[i]) - 1 for i in odd)
    if odd:
        status = []
        got = _reference_loop(ev, [list(arenas)[i] for i in odd], seed, status)
        H = ev.args.horizon
        for i, row, (steps, ag, op, done) in zip(odd, got, status):
            assert np.array_equal(per[i], row) and done == 1
            if n_out[i] == 0:
                assert steps >= H and (ag == 0 or op == 0), (i, steps, ag, op)
            else:
                assert n_out[i] == 2 and steps < H and ag == 0 and op == 0, (i, steps, ag, op)
        print(f"episodes with the reference's no-outcome / two-outcome flags: {[(i, int(n_out[i])) for i in odd]}")


def test_batching_does_not_change_the_result(tmp_path, monkeypatch):
    monkeypatch.setenv("HH_POLICY_W", "0")
    ev_small = _evaluator(tmp_path, 3, 3, True, max_arenas=32)
    ev_all = _evaluator(tmp_path, 3, 3, True, max_arenas=100)
    s_small = ev_small.run(n_episodes=100, seed=SEED, arena_offset=5)
    s_all = ev_all.run(n_episodes=100, seed=SEED, arena_offset=5)
    assert np.array_equal(ev_small.per_episode, ev_all.per_episode)
    assert s_small == s_all
    _check_outcomes(ev_all, range(5, 105), SEED)
    assert s_all["total_n_actions"] >= 100
    ev_small.close()
    ev_all.close()
