"""Timing of evaluation.py on the device (hhmarl_2d_amd.evaluation, hh_commander_act_chain) -> profiles/evaluation.log.

  1. Evaluator.run, 3-vs-3 with the commander (eval_hl), synthetic commander and pilot weights (the pilot networks fly: a policy dir of
     stub modules as the tests write it): episodes/s for 1000 and 65536 episodes, wall clock of run() after a warm-up run that builds
     the graph's kernels once (each run creates its world, pilot bank and graph anew: those are in the time);
  2. the chain kernel against n_agents greedy hh_commander_sample calls on the same arenas (what a slot-by-slot replay with the sampler
     costs), n_agents 1..5 at 1000 and 65536 arenas, device events, the two alternated after a warm-up.  For the kernel time alone run
     it under the profiler (--kernels: part 2 only):
       rocprofv3 --kernel-trace --stats -d <dir> -o ev -- python tools/evaluation_bench.py --kernels

Run:  python tools/evaluation_bench.py [--out profiles/evaluation.log] [--kernels]
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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _time(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)   # ms


def kernels(lines):
    from hhmarl_2d_amd.commander import CommanderNet, random_weights
    net = CommanderNet(0, 5 * 65536 + 3).set_weights(random_weights(1))
    for N in (1000, 65536):
        M = -(-N // 3)
        for nA in range(1, 6):
            g = torch.Generator(device="cuda").manual_seed(N + nA)
            obs = torch.rand((N, nA, 34), device="cuda", generator=g)
            act = torch.empty((N, nA), dtype=torch.int8, device="cuda")
            slots = [torch.zeros((3 * M, 34), device="cuda") for _ in range(nA)]
            for k in range(nA):
                slots[k][:N] = obs[:, k]
            hs = [torch.zeros((3 * M, 2, 200), device="cuda") for _ in range(nA + 1)]
            fresh = torch.ones((M,), dtype=torch.uint8, device="cuda")
            a3, lp3 = torch.empty((M, 3), dtype=torch.int8, device="cuda"), torch.empty((M, 3), device="cuda")
            chain = lambda: net.act_chain(obs, actions=act)

            def replay():
                for k in range(nA):
                    net.sample(slots[k].view(M, 3, 34), hs[k], hs[k + 1], fresh=fresh if k == 0 else None, greedy=True, actions=a3,
                               logp=lp3, want_vf=False)
            for f in (chain, replay, chain, replay):
                f()
            torch.cuda.synchronize()
            t_c, t_r = [], []
            reps = 30 if N < 65536 else 10
            for _ in range(3):
                t_c.append(_time(chain, reps))
                t_r.append(_time(replay, reps))
            tc, tr = statistics.median(t_c), statistics.median(t_r)
            lines.append(f"kernels  arenas {N:6d}  n_agents {nA}  hh_k_commander_chain {1e3 * tc:9.1f} us   {nA} x greedy hh_commander_sample "
                         f"{1e3 * tr:9.1f} us   ratio {tr / tc:5.2f}x")
            print(lines[-1], flush=True)


def episodes(lines):
    from helpers import stub_reference_module
    from hhmarl_2d_amd import policy_nets as PN
    from hhmarl_2d_amd.commander import random_weights
    from hhmarl_2d_amd.config import make_args
    from hhmarl_2d_amd.evaluation import Evaluator
    with tempfile.TemporaryDirectory() as pdir:
        for name, (kind, seed) in {"L5_AC1_fight.pt": (PN.FIGHT1, 51), "L5_AC2_fight.pt": (PN.FIGHT2, 52), "L5_AC1_escape.pt": (PN.ESC1, 53),
                                   "L5_AC2_escape.pt": (PN.ESC2, 54)}.items():
            torch.save(stub_reference_module(kind, seed)[0], os.path.join(pdir, name))
        ev = Evaluator(make_args(2), commander=random_weights(1), policy_dir=pdir, max_arenas=65536)
        ev.run(n_episodes=64, seed=1)     # warm-up: first launches, pilot and commander setup
        for n in (1000, 65536):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = ev.run(n_episodes=n, seed=0)
            dt = time.perf_counter() - t0
            m = ev.metrics
            lines.append(f"episodes {n:6d}  3-vs-3 eval_hl  {dt:8.3f} s  {n / dt:10.1f} episodes/s  {st['total_n_actions'] / dt:10.3e} commander steps/s  "
                         f"({st['total_n_actions'] / n:.1f} commander steps per episode; win {m['win']:.1f} lose {m['lose']:.1f} draw {m['draw']:.1f} %)")
            print(lines[-1], flush=True)
        ev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluation.log"))
    ap.add_argument("--kernels", action="store_true", help="part 2 only (for rocprofv3), nothing written")
    a = ap.parse_args()
    lines = [f"# tools/evaluation_bench.py on {torch.cuda.get_device_name(0)}; episodes: wall clock of Evaluator.run after a warm-up; "
             "kernels: medians of device-event timings, the two alternated after a warm-up"]
    kernels(lines)
    if a.kernels:
        return
    episodes(lines)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
