"""What tests/test_gpu_resume.py runs, in the parent and in its child process: the configurations of the training loop, one iteration of
each (collect -> update -> publish), what an iteration records, and the comparison.  Run as a script it is the child:
    python tests/resume_harness.py <configuration> <checkpoint> <iterations> <result file>
builds fresh objects from the configuration's constructor arguments, loads the checkpoint, runs the iterations and writes the records."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, T, HORIZON, HORIZON_HL = 64, 8, 27, 64
# kl_target = 0.5: two passes at lr 1e-4 leave the KL far below half of it, so update_kl halves kl_coeff at every update that takes a step
LEARN = dict(num_sgd_iter=2, sgd_minibatch_size=64, kl_target=0.5)
# Episodes of the 2-vs-2 worlds end together at the horizon (ticks 27, 54, 81, 108: collects 4, 7, 11, 14), so the whole-episode batches
# arrive in bursts of N x 27 rows.  PROLOGUE collects (with their updates) run before the K1 + K2 iterations in BOTH runs: they put the
# save point (after collect 13, tick 104) 23 ticks into every arena's running episode, behind several updates, and for the accumulating
# configuration (2592 rows = 1.5 bursts: complete at collects 7 and 14) behind a burst that left its batch partly filled.
PROLOGUE, K1, K2 = {"fight_torch": 11, "escape_graph": 11, "level5_fused": 11, "commander_graph": 0}, 2, 2
TRAIN_BATCH = (3 * N * HORIZON) // 2
PILOT_SEED = 2          # the frozen pilots' synthetic networks of the commander configuration


def build(name):
    """fresh objects of configuration `name` from its constructor arguments -> dict (the objects a checkpoint holds under these names,
    and `_keep`: what must stay alive with them)"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import commander as CM
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.pilots import OpponentNets, PolicyBank, VariantNetPilot
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    dev = torch.device("cuda", 0)
    if name == "commander_graph":
        w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True, horizon=HORIZON_HL), device=0)
        net = CM.CommanderNet(0, 3 * N).set_weights(CM.random_weights(6))
        pilot = VariantNetPilot(w, seed=PILOT_SEED)
        ro = CM.CommanderRollout(w, net, pilot, T, batch_mode="complete_episodes", max_seq_len=5)
        learner = LR.CommanderLearner.trainable_init(dev, seed=6, max_seq_len=5, optimizer="fused", step="graph", **LEARN)
        return dict(world=w, commander=net, pilots=pilot.bank, rollout=ro, learner=learner, _keep=pilot)
    mode = "escape" if name == "escape_graph" else "fight"
    level = 5 if name == "level5_fused" else 3
    w = World(make_config(n_arenas=N, level=level, seed=23, auto_reset=True, horizon=HORIZON, agent_mode=1 if mode == "escape" else 0,
                          ext_opp_actions=level == 5), device=0)
    bank = PolicyBank.trainable_init(dev, mode=mode, seed=5, max_rows=2 * N)
    objs = dict(world=w, bank=bank)
    if name == "fight_torch":
        ro = PPORollout(w, bank, T, batch_mode="complete_episodes", metrics=True, train_batch_size=TRAIN_BATCH, record_logits=True)
        learner = LR.PPOLearner.trainable_init(dev, mode=mode, seed=5, max_seq_len=5, optimizer="torch", **LEARN)
    elif name == "escape_graph":
        ro = PPORollout(w, bank, T)
        learner = LR.PPOLearner.trainable_init(dev, mode=mode, seed=5, optimizer="fused", step="graph", shuffle_sequences=True, grad_clip=0.5, **LEARN)
    elif name == "level5_fused":
        opp = OpponentNets(w, seed=9, skip_first=False)
        objs.update(opponents=opp.bank, _keep=opp)
        ro = PPORollout(w, bank, T, batch_mode="complete_episodes", opponents=opp)
        learner = LR.PPOLearner.trainable_init(dev, mode=mode, seed=5, max_seq_len=5, optimizer="fused", **LEARN)
    else:
        raise ValueError(name)
    objs.update(rollout=ro, learner=learner)
    return objs


def saved(objs):
    return {k: v for k, v in objs.items() if not k.startswith("_")}


def _host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().clone()
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x).copy())
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_host(v) for v in x]
    return x


def window(ro):
    names = ["obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target"] + (["logits"] if ro.record_logits else []) \
        + (["state_in"] if hasattr(ro, "state_in") else [])
    torch.cuda.synchronize()
    return {k: _host(getattr(ro, k)) for k in names}


def sampler_of(name, objs):
    return objs["commander"] if name == "commander_graph" else objs["bank"]


def collect(name, objs):
    """the first half of an iteration -> its record so far"""
    ro = objs["rollout"]
    ro.collect()
    rec = {"window": window(ro)}
    if ro.episodes is not None:
        rec["batch"] = _host(ro.episodes.rows())
        if ro.episodes._metrics is not None:
            rec["metrics"] = ro.episodes.metrics()
        if ro.episodes.train_batch_size is not None:
            rec["batch_info"], rec["ready"] = ro.episodes.batch_info(), ro.episodes.ready()
    return rec


def update(name, objs, rec):
    """the update of an iteration (none while an accumulating batch is not complete) -> its statistics into the record"""
    ro, learner, smp = objs["rollout"], objs["learner"], sampler_of(name, objs)
    if name == "escape_graph":
        rec["stats"] = learner.update_window(ro, smp)
    elif name == "fight_torch":
        rec["stats"] = learner.update(ro.episodes, smp) if rec["ready"] else None
    else:
        rec["stats"] = learner.update(ro.episodes, smp)
    return rec


def publish(name, objs):
    objs["learner"].publish(sampler_of(name, objs))


def iterate(name, objs, n):
    out = []
    for _ in range(n):
        rec = update(name, objs, collect(name, objs))
        publish(name, objs)
        out.append(rec)
    return out


def final(name, objs):
    """what the loop holds when it stops: the modules' weights, the Adam state, kl_coeff, and the sampler's outputs on a fixed block"""
    learner, smp = objs["learner"], sampler_of(name, objs)
    g = torch.Generator().manual_seed(3)
    if name == "commander_graph":
        obs = torch.randn((N, 3, 34), generator=g).cuda()
        h_in = (0.1 * torch.randn((N, 3, 2, 200), generator=g)).cuda()
        u = torch.rand((N, 3), generator=g, dtype=torch.float64).cuda()
        h_out, lg = torch.zeros_like(h_in), torch.zeros((N, 3, 4), device="cuda")
        sampled = list(smp.sample(obs, h_in, h_out, uniforms=u, logits=lg)) + [lg, h_out]
    else:
        ro = objs["rollout"]
        obs = torch.randn((N, 2, ro.obs.shape[3]), generator=g).cuda()
        u = torch.rand((N, 2, 4), generator=g, dtype=torch.float64).cuda()
        lg = torch.zeros((N, 2, 32), device="cuda")
        sampled = list(smp.sample(obs, ro.sel, uniforms=u, logits=lg)) + [lg]
    torch.cuda.synchronize()
    # the sampler's packed weights part by part and the world through its readers: the blobs also hold the banks' row lists, whose
    # order within a network's list is that of the binning kernels' atomics and may differ from run to run (a row's result does not)
    packed = [smp.packed(p) for p in (0, 1)] if name == "commander_graph" else [smp.packed(s, p) for s in (0, 1) for p in range(5)]
    w = objs["world"]
    world = [w.get_state(), list(w.episode_stats()), w.arena_status(), w.action_faults(), list(w.eval_info())]
    return {"learner": learner.state_dict(), "sampled": _host(sampled), "packed": _host(packed), "world": _host(world)}


def same(a, b, path="record"):
    """None when a and b are the same bit for bit (tensors by torch.equal, floats with nan == nan), else where they first differ"""
    if type(a) is not type(b) and not (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple))):
        return f"{path}: {type(a).__name__} / {type(b).__name__}"
    if isinstance(a, torch.Tensor):
        if a.dtype != b.dtype or a.shape != b.shape:
            return f"{path}: {a.dtype} {tuple(a.shape)} / {b.dtype} {tuple(b.shape)}"
        x, y = a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)
        return None if torch.equal(x, y) else f"{path}: {int((x != y).sum())} bytes differ"
    if isinstance(a, dict):
        if list(a) != list(b):
            return f"{path}: keys {list(a)} / {list(b)}"
        for k in a:
            d = same(a[k], b[k], f"{path}.{k}")
            if d:
                return d
        return None
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return f"{path}: lengths {len(a)} / {len(b)}"
        for i, (x, y) in enumerate(zip(a, b)):
            d = same(x, y, f"{path}[{i}]")
            if d:
                return d
        return None
    if isinstance(a, float) and math.isnan(a) and math.isnan(b):
        return None
    return None if a == b else f"{path}: {a!r} / {b!r}"


def main(argv):
    from hhmarl_2d_amd import checkpoint
    name, path, n, out = argv[0], argv[1], int(argv[2]), argv[3]
    objs = build(name)
    checkpoint.load(path, **saved(objs))
    recs = iterate(name, objs, n)
    torch.save({"records": recs, "final": final(name, objs)}, out)


if __name__ == "__main__":
    main(sys.argv[1:])
