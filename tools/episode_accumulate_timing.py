"""What train_batch_size costs a collect (shared by tools/episode_emit_bench.py --accumulate and tools/commander_episodes_bench.py
--accumulate): two rollouts of the same world configuration and seed, one overwriting its whole-episode batch at every collect, one
appending to it (hh_episodes_emit_append / hh_commander_episodes_emit_append), timed alternately collect by collect with device
events — the same collects of the same episodes, so the two emit the same rows at every index.  The project's convention: medians of 20
timed collects after 3 warm-up collects, and a difference counts only where the medians differ by more than the larger of the two runs'
(max - min) spreads.  The expectation is no difference: the launches and the bytes moved are the same."""
import statistics

import torch

WARMUP, TIMED = 3, 20


def _ms(ro):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ro.collect()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def accumulate_lines(plain, acc):
    """plain / acc: the two rollouts (batch_mode="complete_episodes"; acc with train_batch_size) -> the lines for the log"""
    for _ in range(WARMUP):
        plain.collect()
        acc.collect()
    torch.cuda.synchronize()
    t_plain, t_acc, rows = [], [], []
    for _ in range(TIMED):                          # alternate: drift of the box hits both
        t_plain.append(_ms(plain))
        t_acc.append(_ms(acc))
        rows.append(int(plain.episodes.n_rows))
    info = acc.episodes.batch_info()
    acc.episodes.rows()                             # raises on an overflow
    med = statistics.median
    d = med(t_acc) - med(t_plain)
    spread = max(max(t_plain) - min(t_plain), max(t_acc) - min(t_acc))
    word = "no difference beyond the spread" if abs(d) <= spread else ("cost" if d > 0 else "gain")
    paired = med([a - p for a, p in zip(t_acc, t_plain)])
    B = acc.episodes.train_batch_size
    return [f"train_batch_size = {B} rows: batch capacity {acc.episodes.obs.shape[0]} rows against {plain.episodes.obs.shape[0]}; rows emitted per "
            f"timed collect min {min(rows)} max {max(rows)}; after the last: {info['rows']} rows in {info['collects']} collects, "
            f"{info['batches']} batches completed",
            f"ms per collect, medians of {TIMED} after {WARMUP}: overwrite {med(t_plain):.3f} (min {min(t_plain):.3f}, max {max(t_plain):.3f}) | "
            f"accumulate {med(t_acc):.3f} (min {min(t_acc):.3f}, max {max(t_acc):.3f})",
            f"overwrite -> accumulate: medians {d * 1e3:+.1f} us apart, larger spread {spread * 1e3:.1f} us: {word} "
            f"(median of the {TIMED} paired differences {paired * 1e3:+.1f} us)"]
