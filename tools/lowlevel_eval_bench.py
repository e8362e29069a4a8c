"""Timing of the greedy evaluation of the 2-vs-2 policies on the device (hhmarl_2d_amd.evaluation.LowLevelEvaluator) -> profiles/lowlevel_eval.log.

LowLevelEvaluator.run at level 3 in fight mode (scripted opponents, the default horizon of 300 ticks and the default map), one batch of
16384 arenas, the synthetic weights of PPOLearner.trainable_init: wall clock of run() — every run creates its world and captures its
block graph anew, and reads the learner's weights; those are in the time — 5 runs after 1 warm-up run, each with another seed; the
median, with the fastest and the slowest, as episodes/s and arena-ticks/s.  Reported only: nothing gates on it.

Run:  python tools/lowlevel_eval_bench.py [--out profiles/lowlevel_eval.log] [--arenas 16384] [--level 3]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.config import make_args
    from hhmarl_2d_amd.evaluation import LowLevelEvaluator
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowlevel_eval.log"))
    ap.add_argument("--arenas", type=int, default=16384)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    learner = LR.PPOLearner.trainable_init(dev, mode="fight", seed=0)
    args = make_args(0, level=a.level)
    lines = [f"# tools/lowlevel_eval_bench.py on {torch.cuda.get_device_name(0)}; wall clock of LowLevelEvaluator.run (world, graph capture and the "
             f"read of the learner's weights included), median of {a.runs} runs after 1 warm-up run, another seed each"]
    with tempfile.TemporaryDirectory() as pdir:
        if a.level >= 4:   # the opponents' files, from synthetic learners
            for level, mode in ((3, "fight"), (4, "fight"), (3, "escape")):
                LR.PPOLearner.trainable_init(dev, mode=mode, seed=10 * level).export_policies(pdir, level)
        ev = LowLevelEvaluator(args, learner, policy_dir=pdir if a.level >= 4 else None, max_arenas=a.arenas)
        ev.run(n_episodes=a.arenas, seed=100)     # warm-up: the first launches, the agents' bank
        times, ticks = [], []
        for r in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = ev.run(n_episodes=a.arenas, seed=r)
            times.append(time.perf_counter() - t0)
            ticks.append(st["episode_len_mean"] * a.arenas)
        ev.close()
    med = statistics.median(times)
    i = times.index(med)
    lines.append(f"level {a.level} fight  arenas {a.arenas}  horizon {args.horizon}  block 16   {med:7.3f} s per run (min {min(times):.3f}, max {max(times):.3f})   "
                 f"{a.arenas / med:10.1f} episodes/s (fastest {a.arenas / min(times):.1f}, slowest {a.arenas / max(times):.1f})   "
                 f"{ticks[i] / med:10.3e} arena-ticks/s   mean episode length {ticks[i] / a.arenas:.1f} ticks   "
                 f"win {st['agents_win']} lose {st['opps_win']} draw {st['draw']} (last run)")
    print("\n".join(lines), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
