"""The reference's third entry point, evaluation.py (Config(2), "Mode 2 = Evaluation"), on the device: N episodes on N arenas of an
`auto_reset = 0` HighLevelEnv world, one episode each, stepped until all are done; the world's eval_info counters (env_base.py:91-107,
counted per arena inside hh_hl_end) summed over the episodes, and postprocess_eval's percentages (evaluation.py:66-82).

    ev = Evaluator(args, commander=state_dict, policy_dir="policies")    # args = config.make_args(mode=2)
    stats = ev.run(n_episodes=1000, seed=0)                              # evaluation.py:100-102's 13 counters
    metrics = postprocess_eval(stats, 1000)                              # win, lose, draw, fight, esc, fight_opp, esc_opp, opp1..3
    ev.write_json("results/EVAL_Commander_3-vs-3")                       # Metrics_Commander_3-vs-3.json

With args.eval_hl the commander decides as evaluation.py:40-48 runs it (CommanderNet.act_chain: every step from zero GRU state, the
actor's state threaded through the agents in id order, greedy); without it every agent's action is 1 and the opponents fly the
L{eval_level_opp} fight policies (env_base.py:343-346).  Out of scope: the per-100-episode PNGs of evaluation.py:61-62, and loading
an RLlib checkpoint (that needs ray) — the commander comes as CommanderGru's state dict or a module holding those parameters."""
import copy
import json
import os

import numpy as np
import torch

from . import _lib as L

# evaluation.py:100-102, in its order
STAT_KEYS = L.EVAL_KEYS[:9] + ("total_n_actions",) + L.EVAL_KEYS[9:]
METRIC_KEYS = ("win", "lose", "draw", "fight", "esc", "fight_opp", "esc_opp", "opp1", "opp2", "opp3")
MAX_SIDE = 5   # agents / opponents per side of a HighLevelEnv world


def _ratio(num, den):
    """num / den * 100; float("nan") where the reference's division raises ZeroDivisionError (den == 0)"""
    return (num / den) * 100 if den != 0 else float("nan")


def postprocess_eval(stats, n_episodes):
    """evaluation.py:66-82 (without its printing and file writing): the counters -> percentages.  Where a denominator is 0 — no agent or
    no opponent step counted, or no agent ever chose to fight — the reference raises ZeroDivisionError; this returns float("nan") for
    that entry instead.  n_episodes takes the place of the reference's N_EVALS."""
    n = int(n_episodes)
    if n < 1:
        raise ValueError("postprocess_eval: n_episodes must be at least 1")
    ev = stats
    return {"win": (ev["agents_win"] / n) * 100, "lose": (ev["opps_win"] / n) * 100, "draw": (ev["draw"] / n) * 100,
            "fight": _ratio(ev["agent_fight"], ev["agent_steps"]), "esc": _ratio(ev["agent_escape"], ev["agent_steps"]),
            "fight_opp": _ratio(ev["opp_fight"], ev["opp_steps"]), "esc_opp": _ratio(ev["opp_escape"], ev["opp_steps"]),
            "opp1": _ratio(ev["opp1"], ev["agent_fight"]), "opp2": _ratio(ev["opp2"], ev["agent_fight"]),
            "opp3": _ratio(ev["opp3"], ev["agent_fight"])}


def eval_args(args):
    """a copy of `args` with what Config(2).set_metrics adds and config.make_args does not: with eval_hl both teams fly level 5
    (config.py:100-102).  `args` itself is left as it is."""
    a = copy.copy(args)
    if getattr(a, "eval_hl", True):
        a.eval_level_ag = a.eval_level_opp = 5
    a.env_config = {"args": a}
    return a


def metrics_file_name(args):
    """evaluation.py:90-94: Metrics_Commander_{n}-vs-{m}.json, or Metrics_Low-Level_{n}-vs-{m}.json without eval_hl"""
    cfg = ("Commander_" if getattr(args, "eval_hl", True) else "Low-Level_") + f"{args.num_agents}-vs-{args.num_opps}"
    return f"Metrics_{cfg}.json"


def write_metrics(metrics, path):
    """json.dump(metrics, indent=3) as evaluation.py:80-81 writes it (a nan entry is written as NaN)"""
    with open(path, "w") as f:
        json.dump({k: metrics[k] for k in METRIC_KEYS}, f, indent=3)
    return path


def _commander_weights(commander):
    """a CommanderGru state dict (numpy or torch) or a module holding its parameters -> the state dict CommanderNet.set_weights takes"""
    from .commander import from_torch_module, state_keys
    if isinstance(commander, torch.nn.Module):
        return from_torch_module(commander)
    missing = [k for k in state_keys() if k not in commander]
    if missing:
        raise ValueError(f"Evaluator: the commander's state dict lacks {missing[:3]}{' ...' if len(missing) > 3 else ''}")
    return commander


class Evaluator:
    """evaluation.py's loop for many episodes at once.  Episode i of `run(n_episodes, seed, arena_offset)` is the first episode of global
    arena arena_offset + i of a HighLevelEnv world with that seed (the world's draws are keyed by global arena, so the result does not
    depend on max_arenas); more than max_arenas episodes run in consecutive batches, each on a world of its own.

    Per commander step: CommanderNet.act_chain (eval_hl) or the constant action 1, then env_hier.macro_step with the pilot the HighLevelEnv
    facade flies for policy_dir (pilots.own_pilot: the variant-row form up to three aircraft per side, the two-call form in ten-slot
    worlds).  Blocks of `block` commander steps are captured as one HIP graph and replayed; done.all() is polled once per block, and a
    batch whose arenas are not all done after `horizon` commander steps raises.  A finished arena neither steps nor counts: hh_hl_end
    gates its counters on the arena taking part in the step, and `total_n_actions` counts per arena the steps taken while it was running
    (the step that ends the episode included), as evaluation.py's eval_stats["total_n_actions"] += 1 does.

    After run(): `stats` (the 13 summed counters), `metrics` (postprocess_eval of them) and `per_episode`, int64 [n_episodes, 13] in
    STAT_KEYS order (agents_win / opps_win / draw are the episode's outcome)."""

    def __init__(self, args, commander=None, policy_dir=None, max_arenas=65536, device=0, block=16):
        eval_hl = bool(getattr(args, "eval_hl", True))
        for side in ("num_agents", "num_opps"):
            n = int(getattr(args, side))
            if not 1 <= n <= MAX_SIDE:
                raise ValueError(f"Evaluator: {side} must be 1..{MAX_SIDE}, got {n}")
        if eval_hl and commander is None:
            raise ValueError("Evaluator: args.eval_hl evaluates a commander: pass its CommanderGru state dict or module")
        if not eval_hl and commander is not None:
            raise ValueError("Evaluator: without args.eval_hl every agent's action is 1 (evaluation.py:49-52): no commander is used")
        if policy_dir is None:
            raise ValueError("Evaluator: policy_dir = the directory of the exported L*_AC*_{fight,escape}.pt pilot policies")
        if int(max_arenas) < 1 or int(block) < 1:
            raise ValueError("Evaluator: max_arenas and block must be at least 1")
        self.args = eval_args(args)
        self.eval_hl = eval_hl
        self.policy_dir = policy_dir
        self.max_arenas, self.block, self.device = int(max_arenas), int(block), device
        self._weights = _commander_weights(commander) if eval_hl else None
        self._net = None
        self.stats = self.metrics = self.per_episode = None

    def _commander(self):
        if self._net is None:
            from .commander import CommanderNet
            self._net = CommanderNet(self.device, self.max_arenas * self.args.num_agents).set_weights(self._weights)
        return self._net

    def _batch(self, n, seed, arena_offset):
        """one world of n arenas, one episode each -> int64 [n, 13] counters per arena (STAT_KEYS order)"""
        from .env_hetero import config_from_args
        from .env_hier import macro_step
        from .pilots import own_pilot
        from .world import World
        a = self.args
        w = World(config_from_args(a, L.ENV_HIGHLEVEL, n, seed, auto_reset=False, arena_offset=arena_offset), device=self.device)
        pilot = None
        try:
            pilot = own_pilot(w, self.policy_dir, a)
            dev = w.device
            obs, rew, val, done = w.alloc_outputs()
            cmd = torch.ones((n, a.num_agents), dtype=torch.int8, device=dev)   # evaluation.py:49-52 when no commander decides
            n_act = torch.zeros((n,), dtype=torch.int32, device=dev)
            pbuf = w.alloc_pilot_variants() if getattr(pilot, "variants", False) else w.alloc_pilot()
            net = self._commander() if self.eval_hl else None
            w.reset(obs=obs)
            w.eval_info(clear_total=True)

            def steps(k):
                for _ in range(k):
                    if net is not None:
                        net.act_chain(obs, actions=cmd)
                    n_act.add_(done == 0)        # running before this step: it counts (done is zero after the reset)
                    macro_step(w, cmd, pilot, out=(obs, rew, val, done), pilot_buf=pbuf, early_exit=False)

            # the first launch of every kernel outside the capture: the pilot's forward on rows without a network, the chain on the
            # reset observations (its actions are recomputed by the first captured step)
            nw = min(64, pilot.bank.max_rows)
            pilot.bank.act(torch.zeros((nw, 30), device=dev), torch.zeros((nw,), dtype=torch.uint8, device=dev))
            if net is not None:
                net.act_chain(obs, actions=cmd)
            torch.cuda.synchronize(dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    steps(self.block)
            torch.cuda.current_stream(dev).wait_stream(side)
            taken = 0
            while True:
                graph.replay()
                taken += self.block
                if bool(done.all()):
                    break
                if taken >= a.horizon:
                    raise RuntimeError(f"Evaluator: arenas still running after {taken} commander steps (horizon {a.horizon}): every "
                                       "commander step lasts at least one tick, so an episode must have ended by now")
            tot = w.eval_info(clear_total=True)[1].to(torch.int64)
            out = torch.cat([tot[:, :9], n_act.to(torch.int64)[:, None], tot[:, 9:]], dim=1)
            return out.cpu().numpy()
        finally:
            if pilot is not None and hasattr(pilot, "close"):
                pilot.close()
            w.close()

    def run(self, n_episodes=1000, seed=0, arena_offset=0):
        """evaluation.py's N_EVALS episodes -> the 13 summed counters {STAT_KEYS: int}; also sets stats, metrics, per_episode"""
        n_episodes, arena_offset = int(n_episodes), int(arena_offset)
        if n_episodes < 1:
            raise ValueError("Evaluator.run: n_episodes must be at least 1")
        if arena_offset < 0:
            raise ValueError("Evaluator.run: arena_offset must not be negative")
        per = []
        for b0 in range(0, n_episodes, self.max_arenas):
            per.append(self._batch(min(self.max_arenas, n_episodes - b0), int(seed), arena_offset + b0))
        self.per_episode = np.concatenate(per, axis=0)
        tot = self.per_episode.sum(axis=0, dtype=np.int64)
        self.stats = {k: int(tot[i]) for i, k in enumerate(STAT_KEYS)}
        self.metrics = postprocess_eval(self.stats, n_episodes)
        return dict(self.stats)

    def write_json(self, path=None):
        """the last run's metrics as evaluation.py writes them; path = a file, a directory (the reference's file name inside it) or None
        (that name in the working directory) -> the path written"""
        if self.metrics is None:
            raise RuntimeError("Evaluator.write_json: run() first")
        if path is None:
            path = metrics_file_name(self.args)
        elif os.path.isdir(path):
            path = os.path.join(path, metrics_file_name(self.args))
        return write_metrics(self.metrics, path)

    def close(self):
        if self._net is not None:
            self._net.close()
            self._net = None
