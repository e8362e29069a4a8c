"""Cost and yield of whole-episode batches (PPORollout batch_mode = "complete_episodes", train_hetero.py:212) against today's fixed
windows (batch_mode = "truncate_episodes"): two rollouts of the same world configuration, timed alternately with device events over
`--collects` collects each round after a warm-up, and the share of the collected rows that leave as whole episodes over the steady-state
collects.  Level 3 fight (horizon 300), random-init Fight1/Fight2 policies, one HIP graph per collect.
    python tools/episode_emit_bench.py [--arenas 16384] [--ticks 64] [--warmup 20] [--collects 30] [--rounds 3]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hhmarl_2d_amd import pilots  # noqa: E402
from hhmarl_2d_amd.rollout import PPORollout  # noqa: E402
from hhmarl_2d_amd.world import World, make_config  # noqa: E402


def make(N, T, batch_mode):
    w = World(make_config(n_arenas=N, level=3, seed=1, auto_reset=True), device=0)
    bank = pilots.PolicyBank.trainable_init(w.device, seed=0, max_rows=2 * N)
    return PPORollout(w, bank, T, batch_mode=batch_mode)


def ms_per_collect(ro, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        ro.collect()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=16384)
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--collects", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    N, T = a.arenas, a.ticks
    runs = {m: make(N, T, m) for m in ("truncate_episodes", "complete_episodes")}
    ep = runs["complete_episodes"].episodes
    print(f"{N} arenas x {T} ticks per collect, level 3 fight, horizon {runs['complete_episodes'].w.cfg.horizon}; "
          f"EpisodeBatch capacity {ep.obs.shape[0]} rows, carry {ep.carry_cap} rows per arena")
    for ro in runs.values():
        for _ in range(a.warmup):
            ro.collect()
    torch.cuda.synchronize()
    times = {m: [] for m in runs}
    for r in range(a.rounds):                       # alternate the modes: drift of the box hits both
        for m, ro in runs.items():
            times[m].append(ms_per_collect(ro, a.collects))
        print(f"round {r}: " + " | ".join(f"{m} {times[m][-1]:.3f} ms/collect" for m in runs))
    tr, ce = statistics.median(times["truncate_episodes"]), statistics.median(times["complete_episodes"])
    print(f"median ms per collect: truncate_episodes {tr:.3f} | complete_episodes {ce:.3f} | emission overhead {ce - tr:.3f} ms = "
          f"{100 * (ce - tr) / tr:.2f} % of a collect")
    # yield: rows that leave as whole episodes over the next steady-state collects (one device count per collect, read once at the end)
    ro = runs["complete_episodes"]
    counts = torch.zeros((a.collects, 2), dtype=torch.int64, device=ro.w.device)
    for i in range(a.collects):
        ro.collect()
        counts[i, 0].copy_(ep.n_rows)
        counts[i, 1].copy_(ep.n_episodes)
    b = ep.rows()                                   # synchronises; raises on an overflow
    c = counts.cpu()
    rows, eps = int(c[:, 0].sum()), int(c[:, 1].sum())
    print(f"steady state ({a.collects} collects after {a.warmup + a.rounds * a.collects}): rows_emitted / rows_collected = {rows} / {a.collects * N * T} = "
          f"{rows / (a.collects * N * T):.4f}; {eps} episodes, mean length {rows / max(eps, 1):.1f}; per collect rows min {int(c[:, 0].min())} "
          f"max {int(c[:, 0].max())}; carried after the last: mean {ep.carried.float().mean().item():.1f} max {int(ep.carried.max())}; "
          f"last batch {len(b['t'])} rows")


if __name__ == "__main__":
    main()
