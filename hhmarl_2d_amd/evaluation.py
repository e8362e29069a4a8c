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
an RLlib checkpoint (that needs ray) — the commander comes as CommanderGru's state dict, a module holding those parameters, or the
path of a file CommanderLearner.export_commander wrote.  The pilot policies in policy_dir are this project's plain exports
(PPOLearner.export_policies; nothing but torch needed to read them) or the reference's pickled modules (those need the reference's
model classes importable), also mixed.

`LowLevelEvaluator` is the greedy evaluation train_hetero.py:55-96 runs on the 2-vs-2 policies while they train (explore=False episodes,
reward and outcome per episode): what decides that a level of the curriculum is done.

    ev = LowLevelEvaluator(make_args(0, level=4), learner, policy_dir="policies")
    stats = ev.run(n_episodes=1000, seed=0)            # episodes, agents_win, opps_win, draw, episode_reward_mean / min / max, episode_len_mean"""
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
    """a CommanderGru state dict (numpy or torch), a module holding its parameters, or the path of a file CommanderLearner.export_commander
    wrote -> the state dict CommanderNet.set_weights takes"""
    from .commander import from_torch_module, state_keys
    if isinstance(commander, (str, os.PathLike)):
        from .policy_files import load_commander
        return load_commander(commander)
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


# ------------------------------------------------------------------------------------------------ the 2-vs-2 policies, greedy
LOWLEVEL_STAT_KEYS = ("episodes", "agents_win", "opps_win", "draw", "episode_reward_mean", "episode_reward_min", "episode_reward_max",
                      "episode_len_mean")
LOWLEVEL_METRIC_KEYS = ("win", "lose", "draw")


def _mean64(x):
    """the float64 mean of a 1-D array, summed on the host in index order"""
    return float(np.cumsum(np.asarray(x, dtype=np.float64))[-1] / len(x))


def lowlevel_stats(per_episode):
    """per_episode (ret f32 [n], len i32 [n], outcome i8 [n]) -> LowLevelEvaluator's stats: counts as ints, means / min / max as floats"""
    ret, ln, oc = per_episode["ret"], per_episode["len"], per_episode["outcome"]
    return {"episodes": int(len(ret)), "agents_win": int((oc == 1).sum()), "opps_win": int((oc == -1).sum()), "draw": int((oc == 0).sum()),
            "episode_reward_mean": _mean64(ret), "episode_reward_min": float(ret.min()), "episode_reward_max": float(ret.max()),
            "episode_len_mean": _mean64(ln)}


class LowLevelEvaluator:
    """train_hetero.py:55-96's loop — one episode of LowLevelEnv with both agents acting greedily (explore=False), the summed reward and
    the length noted — for many episodes at once, in Evaluator's shape.  Episode i of `run(n_episodes, seed, arena_offset)` is the first
    episode of global arena arena_offset + i of an `auto_reset = 0` LowLevelEnv world of args' level and mode with that seed; more than
    max_arenas episodes run in consecutive batches, each on a world of its own.

    policies: a PPOLearner (its modules' weights as they stand when run() is called), a pair of state dicts (numpy or torch, keyed like
    the reference's state_dict(); the actor's keys are read) or a pair of policy-file paths (policy_files), for aircraft types 1 and 2;
    their kinds must be args.agent_mode's.  They go into slots 0 and 1 of a PolicyBank of 2 * max_arenas rows under the selectors
    SEL_FIGHT1 / SEL_FIGHT2 or SEL_ESC1 / SEL_ESC2, and the agents act through PolicyBank.act: greedy, the actor only (the reference's
    compute_single_action(explore=False) runs the value branch on zero action inputs and throws the value away).

    Opponents: levels 1-3 fly the world's scripted ones.  Levels 4-5 fly the exported policies of policy_dir by file name, as
    LowLevelEnv and PPORollout do: PolicyBank.from_reference_dir(..., "LowLevel", args) through OpponentNets(world, bank, bind=True,
    skip_first=False) between hh_step_begin and hh_step_finish, level 5 in fight mode with every arena observing in the mode of its own
    episode's draw (OPP_MODE_EPISODE).  policy_dir is required exactly then; escape mode at level 4 is refused as LowLevelEnv refuses it.

    Blocks of `block` ticks are captured as one HIP graph and replayed; done.all() is polled once per block, and a batch whose arenas
    are not all done after `horizon` ticks raises RuntimeError.  The world freezes a finished arena by itself (auto_reset = 0): it no
    longer steps, its rows may hold anything, and nothing of them is read.

    After run(): `per_episode` = {"ret": f32 [n], "len": i32 [n], "outcome": i8 [n]} from World.episode_stats() (the summed rewards of
    both agents, the ticks, 1 agents win / -1 opponents win / 0 draw), `stats` (LOWLEVEL_STAT_KEYS; the means in float64 on the host,
    summed in index order) and `metrics` (win, lose, draw in percent).

    Not promised: equal results for different max_arenas.  The world's draws are keyed by global arena, but the policy kernel's form
    depends on the row count of a call, two forms may differ in the last bit of a logit, and an arg-max near a tie may then fall the
    other way; one such action changes the rest of its episode.  Runs with the same batch shapes are reproducible bit for bit."""

    def __init__(self, args, policies, policy_dir=None, max_arenas=65536, device=0, block=16):
        from . import policy_files as PF
        mode, level = args.agent_mode, int(args.level)
        if mode not in PF.AGENT_MODES or not 1 <= level <= 5:
            raise ValueError(f"LowLevelEvaluator: args.level is 1..5 and args.agent_mode 'fight' or 'escape', got {level} / {mode!r}")
        if int(args.num_agents) != 2 or int(args.num_opps) != 2:
            raise ValueError("LowLevelEvaluator: LowLevelEnv is 2-vs-2 (args = config.make_args(0, level=..., agent_mode=...))")
        self.frozen = level >= 4
        if self.frozen and mode == "escape" and level < 5:
            raise ValueError("LowLevelEnv in escape mode flies frozen opponents at level 5 only (the reference loads no policy for "
                             f"escape mode at level {level}: envs/env_base.py:328-330)")
        if self.frozen and policy_dir is None:
            raise ValueError("LowLevelEvaluator: levels 4-5 fly frozen opponent policies: policy_dir = the directory of the exported "
                             "L*_AC*_{fight,escape}.pt files")
        if not self.frozen and policy_dir is not None:
            raise ValueError(f"LowLevelEvaluator: level {level} flies the world's scripted opponents: no policy_dir is read")
        if int(max_arenas) < 1 or int(block) < 1:
            raise ValueError("LowLevelEvaluator: max_arenas and block must be at least 1")
        self.args = copy.copy(args)
        self.args.env_config = {"args": self.args}
        self.horizon = int(args.horizon)           # the cap of a batch, in ticks
        self.policy_dir = policy_dir
        self.max_arenas, self.block, self.device = int(max_arenas), int(block), device
        self.kinds = PF.MODE_KINDS[mode]
        self._learner, self._weights = self._resolve(policies)
        self._bank = None
        self.stats = self.metrics = self.per_episode = None

    def _resolve(self, policies):
        """-> (the learner or None, [actor state dict per aircraft type] or None); the kinds checked against args.agent_mode"""
        from . import policy_files as PF
        from . import policy_nets as PN
        who, mode = "LowLevelEvaluator", self.args.agent_mode
        names = [PN.KIND_NAMES[k] for k in self.kinds]
        if hasattr(policies, "modules") and hasattr(policies, "kinds"):
            if tuple(policies.kinds) != tuple(self.kinds):
                raise ValueError(f"{who}: the learner trains kinds {tuple(policies.kinds)}, agent_mode={mode!r} flies {names}")
            return policies, None
        if not isinstance(policies, (list, tuple)) or len(policies) != 2:
            raise ValueError(f"{who}: policies is a PPOLearner, a pair of state dicts or a pair of policy-file paths (aircraft types 1, 2)")
        out = []
        for ac, (p, kind) in enumerate(zip(policies, self.kinds), 1):
            if isinstance(p, (str, os.PathLike)):
                got, sd = PF.load_policy(p)
                if got != kind:
                    raise ValueError(f"{who}: {os.fspath(p)} holds a {PN.KIND_NAMES[got]} network, the {mode} policy of aircraft type {ac} is {PN.KIND_NAMES[kind]}")
            elif isinstance(p, dict):
                sd = p
            else:
                raise ValueError(f"{who}: policies[{ac - 1}] is a state dict or a path, got {type(p).__name__}")
            out.append(self._actor(sd, kind, f"{who}: policies[{ac - 1}]"))
        return None, out

    @staticmethod
    def _actor(sd, kind, who):
        """the actor tensors of one state dict as numpy float32, keys and shapes checked against the kind's"""
        from . import policy_nets as PN
        a = {}
        for k, shp in PN.actor_keys(kind).items():
            if k not in sd:
                raise ValueError(f"{who} has no `{k}`: not a {PN.KIND_NAMES[kind]} network")
            v = sd[k]
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if tuple(v.shape) != tuple(shp):
                raise ValueError(f"{who}: `{k}` has shape {tuple(v.shape)}, a {PN.KIND_NAMES[kind]} network has {tuple(shp)}")
            a[k] = np.ascontiguousarray(v, dtype=np.float32)
        return a

    def _agents(self):
        """the agents' bank with the weights to evaluate, once per run: a learner's are read here, as they stand at the call of run()"""
        from . import pilots as P
        esc = self.args.agent_mode == "escape"
        fresh = self._bank is None
        if fresh:
            self._bank = P.PolicyBank(torch.device("cuda", self.device), 2 * self.max_arenas)
        if fresh or self._learner is not None:
            weights = self._weights
            if self._learner is not None:
                weights = [self._actor(m.state_dict(), k, "LowLevelEvaluator: the learner's module") for m, k in zip(self._learner.modules, self.kinds)]
            for slot, (kind, sd) in enumerate(zip(self.kinds, weights)):
                self._bank.set_net(slot, kind, sd)
        if fresh:   # the selector table names loaded slots
            self._bank.set_lut({(P.SEL_ESC1 if esc else P.SEL_FIGHT1): 0, (P.SEL_ESC2 if esc else P.SEL_FIGHT2): 1})
        return self._bank

    def _batch(self, n, seed, arena_offset):
        """one world of n arenas, one episode each -> (ret f32 [n], len i32 [n], outcome i8 [n]) as numpy arrays"""
        from . import pilots as P
        from .env_hetero import config_from_args
        from .world import World
        a = self.args
        esc = a.agent_mode == "escape"
        bank = self._bank
        w = World(config_from_args(a, L.ENV_LOWLEVEL, n, seed, auto_reset=False, arena_offset=arena_offset), device=self.device)
        obank = None
        try:
            dev = w.device
            opp = None
            if self.frozen:   # _get_policies("LowLevel"), env_base.py:312-332; bound before any step_begin
                obank = P.PolicyBank.from_reference_dir(dev, self.policy_dir, "LowLevel", a, max_rows=2 * n)
                opp = P.OpponentNets(w, bank=obank, bind=True, skip_first=False)
            opp_mode = L.OPP_MODE_EPISODE if (a.level == 5 and not esc) else 0
            obs, rew, val, done = out = w.alloc_outputs()
            act = torch.zeros((n, 2, 4), dtype=torch.int8, device=dev)
            sel = torch.tensor([P.SEL_ESC1, P.SEL_ESC2] if esc else [P.SEL_FIGHT1, P.SEL_FIGHT2], dtype=torch.uint8, device=dev).repeat(n, 1).contiguous()
            opp_obs = torch.zeros((n, 2, 30), dtype=torch.float32, device=dev) if self.frozen else None
            w.reset(obs=obs)

            def ticks(k):
                for _ in range(k):
                    bank.act(obs, sel, actions=act)
                    if self.frozen:   # agents act -> the frozen opponents observe and act -> tick (env_hetero.py:160-172)
                        w.step_begin(act, opp_mode, opp_obs=opp_obs)
                        w.step_finish(opp(opp_obs, None).contiguous(), out=out)
                    else:
                        w.step(act, out=out)

            # the first launch of the policy kernels outside the capture: the agents' forward on the reset observations (the first
            # captured tick recomputes its actions), the opponents' on rows without a network (nothing is listed)
            bank.act(obs, sel, actions=act)
            if obank is not None:
                nw = min(64, obank.max_rows)
                obank.act(torch.zeros((nw, 30), device=dev), torch.zeros((nw,), dtype=torch.uint8, device=dev))
            torch.cuda.synchronize(dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    ticks(self.block)
            torch.cuda.current_stream(dev).wait_stream(side)
            taken = 0
            while True:
                graph.replay()
                taken += self.block
                if bool(done.all()):
                    break
                if taken >= self.horizon:
                    raise RuntimeError(f"LowLevelEvaluator: arenas still running after {taken} ticks (horizon {self.horizon}): an episode "
                                       "ends at its horizon at the latest")
            ret, ln, oc = w.episode_stats()
            return ret.cpu().numpy(), ln.cpu().numpy(), oc.cpu().numpy()
        finally:
            if obank is not None:
                w.bind_policy(None)
                obank.close()
            w.close()

    def run(self, n_episodes=1000, seed=0, arena_offset=0):
        """n_episodes greedy episodes -> `stats` (a copy); also sets per_episode and metrics"""
        n_episodes, arena_offset = int(n_episodes), int(arena_offset)
        if n_episodes < 1:
            raise ValueError("LowLevelEvaluator.run: n_episodes must be at least 1")
        if arena_offset < 0:
            raise ValueError("LowLevelEvaluator.run: arena_offset must not be negative")
        try:
            self._agents()
        except BaseException:
            self.close()      # no half-loaded bank is kept
            raise
        per = [self._batch(min(self.max_arenas, n_episodes - b0), int(seed), arena_offset + b0) for b0 in range(0, n_episodes, self.max_arenas)]
        self.per_episode = {k: np.concatenate([p[i] for p in per]) for i, k in enumerate(("ret", "len", "outcome"))}
        self.stats = lowlevel_stats(self.per_episode)
        n = self.stats["episodes"]
        self.metrics = {"win": (self.stats["agents_win"] / n) * 100, "lose": (self.stats["opps_win"] / n) * 100, "draw": (self.stats["draw"] / n) * 100}
        return dict(self.stats)

    def metrics_file_name(self):
        return f"Metrics_Low-Level_L{int(self.args.level)}_{self.args.agent_mode}.json"

    def write_json(self, path=None):
        """the last run's metrics (win, lose, draw in percent) as Evaluator.write_json writes its own: json.dump(indent=3); path = a file,
        a directory (metrics_file_name() inside it) or None (that name in the working directory) -> the path written"""
        if self.metrics is None:
            raise RuntimeError("LowLevelEvaluator.write_json: run() first")
        if path is None:
            path = self.metrics_file_name()
        elif os.path.isdir(path):
            path = os.path.join(path, self.metrics_file_name())
        with open(path, "w") as f:
            json.dump({k: self.metrics[k] for k in LOWLEVEL_METRIC_KEYS}, f, indent=3)
        return path

    def close(self):
        if self._bank is not None:
            self._bank.close()
            self._bank = None
