"""What tests/test_gpu_lowlevel_evaluator.py compares evaluation.LowLevelEvaluator with (test infrastructure): the same greedy episodes as
a plain eager loop — per batch ONE `auto_reset = 0` world of the same size, one tick at a time, no graph and no blocks, `done` polled
after every tick — making the same PolicyBank.act and step calls.  The evaluator's blocks run past the end of an episode and past the
horizon; this loop stops at the tick every arena is done, so equality also shows that a finished arena stays as it finished."""
import numpy as np
import torch


def actor_weights(learner):
    """the learner's modules as the host arrays PolicyBank.set_net takes: [(kind, {actor key: numpy float32})]"""
    from hhmarl_2d_amd import policy_nets as PN
    out = []
    for kind, m in zip(learner.kinds, learner.modules):
        sd = m.state_dict()
        out.append((kind, {k: sd[k].detach().cpu().numpy().astype(np.float32) for k in PN.actor_keys(kind)}))
    return out


def plain_loop(args, weights, n_episodes, seed, arena_offset=0, max_arenas=65536, policy_dir=None, device=0):
    """weights: [(kind, actor state dict)] for aircraft types 1 and 2 -> {"ret": f32 [n], "len": i32 [n], "outcome": i8 [n]} and the
    number of ticks each batch took"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import pilots as P
    from hhmarl_2d_amd.env_hetero import config_from_args
    from hhmarl_2d_amd.world import World
    dev = torch.device("cuda", device)
    esc = args.agent_mode == "escape"
    frozen = args.level >= 4
    bank = P.PolicyBank(dev, 2 * max_arenas)
    for slot, (kind, sd) in enumerate(weights):
        bank.set_net(slot, kind, sd)
    bank.set_lut({(P.SEL_ESC1 if esc else P.SEL_FIGHT1): 0, (P.SEL_ESC2 if esc else P.SEL_FIGHT2): 1})
    per, ticks = [], []
    for b0 in range(0, n_episodes, max_arenas):
        n = min(max_arenas, n_episodes - b0)
        w = World(config_from_args(args, L.ENV_LOWLEVEL, n, seed, auto_reset=False, arena_offset=arena_offset + b0), device=device)
        obank = opp = None
        if frozen:
            obank = P.PolicyBank.from_reference_dir(dev, policy_dir, "LowLevel", args, max_rows=2 * n)
            opp = P.OpponentNets(w, bank=obank, bind=True, skip_first=False)
        opp_mode = L.OPP_MODE_EPISODE if (args.level == 5 and not esc) else 0
        out = w.alloc_outputs()
        obs, done = out[0], out[3]
        act = torch.zeros((n, 2, 4), dtype=torch.int8, device=dev)
        sel = torch.tensor([P.SEL_ESC1, P.SEL_ESC2] if esc else [P.SEL_FIGHT1, P.SEL_FIGHT2], dtype=torch.uint8, device=dev).repeat(n, 1).contiguous()
        opp_obs = torch.zeros((n, 2, 30), dtype=torch.float32, device=dev)
        w.reset(obs=obs)
        t = 0
        while not bool(done.all()):
            assert t < args.horizon, "an episode ends at its horizon at the latest"
            bank.act(obs, sel, actions=act)
            if frozen:
                w.step_begin(act, opp_mode, opp_obs=opp_obs)
                w.step_finish(opp(opp_obs, None).contiguous(), out=out)
            else:
                w.step(act, out=out)
            t += 1
        per.append([x.cpu().numpy() for x in w.episode_stats()])
        ticks.append(t)
        if obank is not None:
            w.bind_policy(None)
            obank.close()
        w.close()
    bank.close()
    return {k: np.concatenate([p[i] for p in per]) for i, k in enumerate(("ret", "len", "outcome"))}, ticks
