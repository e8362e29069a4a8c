"""Cost and yield of the commander's whole-episode GRU-sequence batches (CommanderRollout batch_mode = "complete_episodes", train_hier.py:182)
against today's fixed windows: two rollouts of the same world configuration (N arenas, T commander steps, VariantNetPilot, horizon H),
timed alternately with device events after a warm-up; the emission's share of a collect; the share of the collected rows that leave as
whole episodes in steady state; and the bytes the emission moves per collect (for the bandwidth of a separate rocprofv3 --kernel-trace run).
--logits adds both modes with record_logits=True (the sampler's logits as a batch column, 48 B more per row).
--metrics adds complete_episodes with metrics=True (the episode metrics behind the emitter, hh_episodes_metrics): what the flag costs a
collect against complete_episodes without it, next to the emission's own overhead, and the three metrics launches alone on the last
batch; with it only those lines are written, APPENDED to --out.
--accumulate measures only what train_batch_size costs a collect: complete_episodes overwriting its batch against complete_episodes
appending to it with B = 4 collects' worth of rows (tools/episode_accumulate_timing.py: medians of 20 after 3 warm-up, the spread
rule); its lines are APPENDED to --out.
--window measures only what window_metrics=True costs a truncate_episodes collect (tools/episode_metrics_timing.py: the same rule, and
hh_window_metrics's five launches alone); its lines are APPENDED to --out.
--outcomes measures only what outcomes=True costs a collect (T taps and hh_episode_outcomes' two launches), in the same run against its
own twin without the option (complete_episodes with metrics=True; tools/episode_metrics_timing.py: the same rule); its lines are
APPENDED to --out.
    python tools/commander_episodes_bench.py [--arenas 8192] [--steps 16] [--horizon 500] [--warmup 8] [--collects 10] [--rounds 3]
        [--logits] [--metrics] [--accumulate] [--window] [--outcomes] [--out profiles/commander_episodes.log]"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hhmarl_2d_amd import _lib as L  # noqa: E402
from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights  # noqa: E402
from hhmarl_2d_amd.pilots import VariantNetPilot  # noqa: E402
from hhmarl_2d_amd.world import World, make_config  # noqa: E402
from episode_accumulate_timing import accumulate_lines  # noqa: E402  (tools/, next to this file)
from episode_metrics_timing import metrics_lines, outcome_lines, window_lines  # noqa: E402  (tools/, next to this file)

ROW_IN = 3 * 34 * 4 + 3 + 3 * 4 * 3 + 3          # obs, actions, logp / vf / reward, valid of one arena row
ROW_OUT = ROW_IN + 3 * 4 * 2 + 1 + 3 * 4          # + adv / target, done, arena / episode / t
STATE = 3 * 2 * 200 * 4                          # the GRU states of one arena row


def make(N, T, H, mode, train_batch_size=None, outcomes=False):
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=1, auto_reset=True, horizon=H), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    rec, met = mode.endswith("+logits"), mode.endswith("+metrics")
    return CommanderRollout(w, net, VariantNetPilot(w, seed=8), T, batch_mode=mode.split("+")[0], metrics=met, train_batch_size=train_batch_size,
                            record_logits=rec, window_metrics=mode.endswith("+window_metrics"), outcomes=outcomes)


def ms_per_collect(ro, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        ro.collect()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def emission_bytes(ep, done, carried_before, carried_after, rows, seqs):
    """bytes the commander's hh_k_ep_emit instance reads and writes in one collect (row gather, sequence-start states, carry rewrite);
    the small count / scan / GAE traffic is left out"""
    Lq = ep.L
    fin = done.bool().any(dim=0).cpu()                                      # arenas with an episode ending in the window
    cb, ca = carried_before.cpu().long(), carried_after.cpu().long()
    new_rows = torch.where(fin, ca, ca - cb).sum().item()
    slots = lambda c: (c + Lq - 1) // Lq
    new_states = torch.where(fin, slots(ca), slots(ca) - slots(cb)).sum().item()
    aux = 3 * 4 * getattr(ep, ep.aux_name).shape[-1] if ep.aux_name else 0
    return rows * (ROW_IN + ROW_OUT + 2 * aux) + seqs * 2 * STATE + new_rows * 2 * (ROW_IN + aux) + new_states * 2 * STATE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--collects", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--logits", action="store_true", help="also time both modes with record_logits=True")
    ap.add_argument("--metrics", action="store_true", help="also time complete_episodes with metrics=True; appends only its lines to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commander_episodes.log"))
    ap.add_argument("--accumulate", action="store_true", help="only: what train_batch_size = 4 N T costs a collect; appends its lines to --out")
    ap.add_argument("--window", action="store_true", help="only: what window_metrics=True costs a truncate_episodes collect; appends its lines to --out")
    ap.add_argument("--outcomes", action="store_true", help="only: what outcomes=True costs a collect; appends its lines to --out")
    a = ap.parse_args()
    N, T, H = a.arenas, a.steps, a.horizon
    if a.outcomes:
        olines = [f"# tools/commander_episodes_bench.py --outcomes on {torch.cuda.get_device_name(0)}: {N} arenas x {T} commander steps per "
                  f"collect, VariantNetPilot, horizon {H}"]
        mode = "complete_episodes+metrics"
        olines += outcome_lines(make(N, T, H, mode), make(N, T, H, mode, outcomes=True), mode)
        print("\n".join(olines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(olines) + "\n")
        return
    if a.window:
        wlines = [f"# tools/commander_episodes_bench.py --window on {torch.cuda.get_device_name(0)}: {N} arenas x {T} commander steps per "
                  f"collect, VariantNetPilot, horizon {H}"]
        wlines += window_lines(make(N, T, H, "truncate_episodes"), make(N, T, H, "truncate_episodes+window_metrics"))
        print("\n".join(wlines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(wlines) + "\n")
        return
    if a.accumulate:
        alines = [f"# tools/commander_episodes_bench.py --accumulate on {torch.cuda.get_device_name(0)}: {N} arenas x {T} commander steps per "
                  f"collect, VariantNetPilot, horizon {H}"]
        alines += accumulate_lines(make(N, T, H, "complete_episodes"), make(N, T, H, "complete_episodes", train_batch_size=4 * N * T))
        print("\n".join(alines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(alines) + "\n")
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    modes = ("truncate_episodes", "complete_episodes") + (("truncate_episodes+logits", "complete_episodes+logits") if a.logits else ()) + \
        (("complete_episodes+metrics",) if a.metrics else ())
    runs = {m: make(N, T, H, m) for m in modes}
    ro = runs["complete_episodes"]
    ep = ro.episodes
    say(f"# tools/commander_episodes_bench.py on {torch.cuda.get_device_name(0)}: {N} arenas x {T} commander steps per collect, VariantNetPilot, "
        f"horizon {H}; max_seq_len {ep.L}, carry_cap {ep.carry_cap} rows ({math.ceil(ep.carry_cap / ep.L)} states) per arena; capacity "
        f"{ep.obs.shape[0]} rows, {ep.seq_start.shape[0]} sequences")
    for r in runs.values():
        for _ in range(a.warmup):
            r.collect()
    torch.cuda.synchronize()
    times = {m: [] for m in runs}
    for i in range(a.rounds):                       # alternate the modes: drift of the box hits both
        for m, r in runs.items():
            times[m].append(ms_per_collect(r, a.collects))
        say(f"round {i}: " + " | ".join(f"{m} {times[m][-1]:.3f} ms/collect" for m in runs))
    tr, ce = statistics.median(times["truncate_episodes"]), statistics.median(times["complete_episodes"])
    say(f"median ms per collect: truncate_episodes {tr:.3f} | complete_episodes {ce:.3f} | emission {ce - tr:.3f} ms = "
        f"{100 * (ce - tr) / ce:.2f} % of a complete_episodes collect (target: 0.5 ms)")
    if a.metrics:
        mlines = [f"# tools/commander_episodes_bench.py --metrics on {torch.cuda.get_device_name(0)}: {N} arenas x {T} commander steps per collect, "
                  f"horizon {H}, {a.collects} collects x {a.rounds} rounds after {a.warmup}"]
        mlines += metrics_lines(runs["complete_episodes+metrics"].episodes, tr, ce, statistics.median(times["complete_episodes+metrics"]))
        print("\n".join(mlines), flush=True)
    if a.logits:
        trl, cel = statistics.median(times["truncate_episodes+logits"]), statistics.median(times["complete_episodes+logits"])
        say(f"with the logits column: truncate_episodes+logits {trl:.3f} (the sampler's logits stores: {trl - tr:+.3f} ms) | complete_episodes+logits "
            f"{cel:.3f} | emission {cel - trl:.3f} ms; {(cel - trl) / max(ce - tr, 1e-9):.2f} x the emission without the column")
        rl = runs["complete_episodes+logits"]
        nb = []
        for _ in range(a.collects):
            cb = rl.episodes.carried.clone()
            rl.collect()
            b = rl.episodes.rows()
            nb.append(emission_bytes(rl.episodes, rl.done, cb, rl.episodes.carried, len(b["t"]), len(b["seq_start"])))
        rate = f"over the measured emission {statistics.mean(nb) / 1e6 / (cel - trl):.0f} GB/s" if cel - trl > 0.02 else \
            "the measured emission is below what the difference of two collects resolves"
        say(f"with the logits column hh_k_ep_emit moves {statistics.mean(nb) / 1e6:.1f} MB per collect: {rate}")
    # yield and bytes over the next steady-state collects
    rows = seqs = eps = 0
    nbytes = []
    longest = 0
    for _ in range(a.collects):
        cb = ep.carried.clone()
        ro.collect()
        b = ep.rows()                               # synchronises; raises on an overflow
        r, s = len(b["t"]), len(b["seq_start"])
        rows, seqs, eps = rows + r, seqs + s, eps + len(b["ep_start"])
        if len(b["ep_len"]):
            longest = max(longest, int(b["ep_len"].max()))
        nbytes.append(emission_bytes(ep, ro.done, cb, ep.carried, r, s))
    say(f"steady state ({a.collects} collects after {a.warmup + a.rounds * a.collects}): rows_emitted / rows_collected = {rows} / "
        f"{a.collects * N * T} = {rows / (a.collects * N * T):.4f}; {eps} episodes (mean length {rows / max(eps, 1):.1f} steps, longest "
        f"{longest}), {seqs} sequences; carried after the last: mean {ep.carried.float().mean().item():.1f} max {int(ep.carried.max())}")
    mb = statistics.mean(nbytes) / 1e6
    say(f"hh_k_ep_emit (the commander's instance) moves {mb:.1f} MB per collect (row gather, sequence-start states, carry rewrite): at "
        f"6.3 TB/s that is {mb / 6.3e3 * 1e3:.1f} us; at the measured emission above {mb / max(ce - tr, 1e-9):.0f} GB/s over the whole emission")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.metrics else "w") as f:       # --metrics: its own lines only, after what the log holds
        f.write("\n".join(mlines if a.metrics else lines) + "\n")


if __name__ == "__main__":
    main()
