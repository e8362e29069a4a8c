"""What a checkpoint costs (hhmarl_2d_amd/checkpoint.py): wall time of `checkpoint.save` and of `checkpoint.load`, separately, median of 5
after 1 warm-up, and the file's size, for the whole loop of both trainers at their benchmark sizes:

    python tools/checkpoint_bench.py [--dir DIR] [--collects 3]

  * train_hetero.py's loop at 16384 arenas, T = 64 (level 3, fight, batch_mode="complete_episodes"), without and with record_logits:
    World, PolicyBank, PPORollout with its EpisodeBatch, PPOLearner(optimizer="fused");
  * train_hier.py's loop at 8192 commander arenas, T = 16: World, CommanderNet, the pilots' PolicyBank, CommanderRollout with its
    CommanderEpisodeBatch, CommanderLearner(optimizer="fused").
The objects have run `--collects` collects (no update: the Adam state is saved at its full size whatever it holds), so the carry holds
running episodes and the batch what the last collect emitted.  A save is device-to-host copies, torch.save and an fsync; a load is
torch.load, validation and host-to-device copies into the live objects.  The file goes to --dir (default: a temporary directory), so
the figures include that file system.  Reported, not gated: profiles/checkpoint.log keeps the lines."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def hetero(n_arenas, T, record_logits):
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    dev = torch.device("cuda", 0)
    w = World(make_config(n_arenas=n_arenas, level=3, seed=1, auto_reset=True), device=0)
    bank = PolicyBank.trainable_init(dev, mode="fight", seed=5, max_rows=2 * n_arenas)
    ro = PPORollout(w, bank, T, batch_mode="complete_episodes", record_logits=record_logits)
    return dict(world=w, bank=bank, rollout=ro, learner=LR.PPOLearner.trainable_init(dev, mode="fight", seed=5, optimizer="fused")), None


def hier(n_arenas, T):
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import commander as CM
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=n_arenas, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=1, auto_reset=True), device=0)
    net = CM.CommanderNet(0, 3 * n_arenas).set_weights(CM.random_weights(6))
    pilot = VariantNetPilot(w, seed=8)
    ro = CM.CommanderRollout(w, net, pilot, T, batch_mode="complete_episodes")
    learner = LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, optimizer="fused")
    return dict(world=w, commander=net, pilots=pilot.bank, rollout=ro, learner=learner), pilot


def measure(what, build, folder, collects, repeats=5, warmup=1):
    from hhmarl_2d_amd import checkpoint
    objs, keep = build()
    for _ in range(collects):
        objs["rollout"].collect()
    torch.cuda.synchronize()
    path = os.path.join(folder, "bench.ckpt")
    save_s, load_s, size = [], [], 0
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        size = checkpoint.save(path, **objs)
        t1 = time.perf_counter()
        checkpoint.load(path, **objs)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warmup:
            save_s.append(t1 - t0)
            load_s.append(t2 - t1)
    os.unlink(path)
    ep = objs["rollout"].episodes
    line = (f"{what}: checkpoint {size} bytes ({size / 2 ** 20:.1f} MiB) | save median {1e3 * statistics.median(save_s):.1f} ms (min {1e3 * min(save_s):.1f}) | "
            f"load median {1e3 * statistics.median(load_s):.1f} ms (min {1e3 * min(load_s):.1f}) | median of {repeats} after {warmup} warm-up, after {collects} collects "
            f"(carry: longest running episode {int(ep.carried.max())} rows, last batch {int(ep.n_rows)} rows)")
    print(line, flush=True)
    del objs, keep
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", default=None, help="where the checkpoint file is written (default: a temporary directory)")
    ap.add_argument("--collects", type=int, default=3)
    ap.add_argument("--arenas", type=int, default=16384)
    ap.add_argument("--commander-arenas", type=int, default=8192)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as folder:
        print(f"device {torch.cuda.get_device_name(0)} | torch {torch.__version__} | file system of {a.dir or 'the system temporary directory'}", flush=True)
        measure(f"train_hetero loop, {a.arenas} arenas, T = 64", lambda: hetero(a.arenas, 64, False), folder, a.collects)
        measure(f"train_hetero loop, {a.arenas} arenas, T = 64, record_logits", lambda: hetero(a.arenas, 64, True), folder, a.collects)
        measure(f"train_hier loop, {a.commander_arenas} commander arenas, T = 16", lambda: hier(a.commander_arenas, 16), folder, a.collects)


if __name__ == "__main__":
    main()
