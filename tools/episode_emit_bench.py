"""Cost and yield of whole-episode batches (PPORollout batch_mode = "complete_episodes", train_hetero.py:212) against today's fixed
windows (batch_mode = "truncate_episodes"): two rollouts of the same world configuration, timed alternately with device events over
`--collects` collects each round after a warm-up, and the share of the collected rows that leave as whole episodes over the steady-state
collects.  Level 3 fight (horizon 300), random-init Fight1/Fight2 policies, one HIP graph per collect.
--logits adds both modes with record_logits=True (the sampler's logits as a batch column: 256 B more per row): the truncate pair
gives what writing the logits costs the sampler, the complete pair what the emission costs with the column.  The bytes the emission moves
per collect are counted from the batch and carry counts, so that a time (this tool's difference, or hh_k_ep_emit's in a separate
rocprofv3 --kernel-trace run) becomes bytes/s.
--metrics adds complete_episodes with metrics=True (the episode metrics behind the emitter, hh_episodes_metrics): what the flag costs a
collect (against complete_episodes without it, whose launches are the ones from before the flag existed), next to the emission's own
overhead, and the time of the three metrics launches alone on the last batch; those lines are appended to --out.
--accumulate measures only what train_batch_size costs a collect: complete_episodes overwriting its batch against complete_episodes
appending to it with B = 4 collects' worth of rows (tools/episode_accumulate_timing.py: medians of 20 after 3 warm-up, the spread
rule); its lines are appended to --out.
--window measures only what window_metrics=True costs a truncate_episodes collect (tools/episode_metrics_timing.py: the same rule, and
hh_window_metrics's five launches alone); its lines are appended to --out.
--outcomes measures only what outcomes=True costs a collect (T taps and hh_episode_outcomes' two launches), in the same run against its
own twin without the option, for both consumers: complete_episodes with metrics=True, and truncate_episodes with window_metrics=True
(tools/episode_metrics_timing.py: the same rule); its lines are appended to --out.
    python tools/episode_emit_bench.py [--arenas 16384] [--ticks 64] [--warmup 20] [--collects 30] [--rounds 3] [--logits]
        [--metrics [--out profiles/episode_emit.log]] | --accumulate | --window | --outcomes [--arenas 16384] [--ticks 64] [--out ...]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hhmarl_2d_amd import pilots  # noqa: E402
from hhmarl_2d_amd.rollout import PPORollout  # noqa: E402
from hhmarl_2d_amd.world import World, make_config  # noqa: E402
from episode_accumulate_timing import accumulate_lines  # noqa: E402  (tools/, next to this file)
from episode_metrics_timing import metrics_lines, outcome_lines, window_lines  # noqa: E402  (tools/, next to this file)


def make(N, T, mode, train_batch_size=None, outcomes=False):
    w = World(make_config(n_arenas=N, level=3, seed=1, auto_reset=True), device=0)
    bank = pilots.PolicyBank.trainable_init(w.device, seed=0, max_rows=2 * N)
    if outcomes:
        kw = dict(window_metrics=True) if mode.endswith("+window_metrics") else dict(metrics=True)
        return PPORollout(w, bank, T, batch_mode=mode.split("+")[0], outcomes=True, **kw)
    if mode.endswith("+window_metrics"):
        return PPORollout(w, bank, T, batch_mode=mode[:-len("+window_metrics")], window_metrics=True)
    if train_batch_size is not None:
        return PPORollout(w, bank, T, batch_mode=mode, train_batch_size=train_batch_size)
    if mode.endswith("+metrics"):
        return PPORollout(w, bank, T, batch_mode=mode[:-len("+metrics")], metrics=True)
    if mode.endswith("+logits"):
        return PPORollout(w, bank, T, batch_mode=mode[:-len("+logits")], record_logits=True)
    return PPORollout(w, bank, T, batch_mode=mode)


def emission_bytes(ep, done, carried_before, carried_after, rows):
    """bytes hh_k_ep_emit reads and writes in one collect: every emitted row once in (carry or window) and once out with its metadata,
    every row that enters the carry once in and once out; the count / scan / GAE traffic is left out"""
    D, nA = ep.D, ep.n_agents
    aux = 4 * nA * getattr(ep, ep.aux_name).shape[-1] if ep.aux_name else 0
    row_in = nA * (4 * D + 4 + 3 * 4 + 1) + aux            # obs, actions, logp / vf / reward, valid (, aux)
    row_out = row_in + 1 + 3 * 4                          # + done, arena / episode / t (adv / target are the GAE kernel's)
    fin = done.bool().any(dim=0)
    new_rows = torch.where(fin, carried_after, carried_after - carried_before).sum().item()
    return rows * (row_in + row_out) + new_rows * 2 * row_in


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
    ap.add_argument("--logits", action="store_true", help="also time both modes with record_logits=True")
    ap.add_argument("--metrics", action="store_true", help="also time complete_episodes with metrics=True; appends its lines to --out")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "episode_emit.log"))
    ap.add_argument("--accumulate", action="store_true", help="only: what train_batch_size = 4 N T costs a collect; appends its lines to --out")
    ap.add_argument("--window", action="store_true", help="only: what window_metrics=True costs a truncate_episodes collect; appends its lines to --out")
    ap.add_argument("--outcomes", action="store_true", help="only: what outcomes=True costs a collect, for both consumers; appends its lines to --out")
    a = ap.parse_args()
    N, T = a.arenas, a.ticks
    if a.outcomes:
        lines = [f"# tools/episode_emit_bench.py --outcomes on {torch.cuda.get_device_name(0)}: {N} arenas x {T} ticks per collect, level 3 fight"]
        for mode in ("complete_episodes+metrics", "truncate_episodes+window_metrics"):
            lines += outcome_lines(make(N, T, mode), make(N, T, mode, outcomes=True), mode)
        print("\n".join(lines))
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.window:
        lines = [f"# tools/episode_emit_bench.py --window on {torch.cuda.get_device_name(0)}: {N} arenas x {T} ticks per collect, level 3 fight"]
        lines += window_lines(make(N, T, "truncate_episodes"), make(N, T, "truncate_episodes+window_metrics"))
        print("\n".join(lines))
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.accumulate:
        lines = [f"# tools/episode_emit_bench.py --accumulate on {torch.cuda.get_device_name(0)}: {N} arenas x {T} ticks per collect, level 3 fight"]
        lines += accumulate_lines(make(N, T, "complete_episodes"), make(N, T, "complete_episodes", train_batch_size=4 * N * T))
        print("\n".join(lines))
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    modes = ("truncate_episodes", "complete_episodes") + (("truncate_episodes+logits", "complete_episodes+logits") if a.logits else ()) + \
        (("complete_episodes+metrics",) if a.metrics else ())
    runs = {m: make(N, T, m) for m in modes}
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
    over = {"complete_episodes": ce - tr}
    if a.logits:
        trl, cel = statistics.median(times["truncate_episodes+logits"]), statistics.median(times["complete_episodes+logits"])
        over["complete_episodes+logits"] = cel - trl
        print(f"with the logits column: truncate_episodes+logits {trl:.3f} (the sampler's logits stores: {trl - tr:+.3f} ms) | complete_episodes+logits "
              f"{cel:.3f} | emission overhead {cel - trl:.3f} ms = {100 * (cel - trl) / trl:.2f} % of a collect; {(cel - trl) / max(ce - tr, 1e-9):.2f} x the "
              f"emission without the column")
    if a.metrics:
        lines = [f"# tools/episode_emit_bench.py --metrics on {torch.cuda.get_device_name(0)}: {N} arenas x {T} ticks per collect, "
                 f"{a.collects} collects x {a.rounds} rounds after {a.warmup}"]
        lines += metrics_lines(runs["complete_episodes+metrics"].episodes, tr, ce, statistics.median(times["complete_episodes+metrics"]))
        print("\n".join(lines))
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    for m, dt in over.items():      # the bytes the emission moves, over a few steady-state collects of that rollout
        r, e = runs[m], runs[m].episodes
        nb = []
        for _ in range(5):
            cb = e.carried.clone()
            r.collect()
            nb.append(emission_bytes(e, r.done, cb, e.carried, int(e.n_rows)))
        mb = statistics.mean(nb) / 1e6
        print(f"{m}: hh_k_ep_emit moves {mb:.1f} MB per collect (row gather, carry rewrite): at 6.3 TB/s that is {mb / 6.3e3 * 1e3:.1f} us; over the "
              f"measured emission overhead (four kernels) {mb / max(dt, 1e-9):.0f} GB/s")
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
