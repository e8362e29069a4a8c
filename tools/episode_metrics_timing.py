"""Shared by tools/episode_emit_bench.py and tools/commander_episodes_bench.py (--metrics): the time of hh_episodes_metrics's three
launches alone, and the lines both tools report about an `EpisodeBatch(metrics=True)`.
--window (both tools): what window_metrics=True costs a collect in batch_mode = "truncate_episodes" — two rollouts of the same world
configuration and seed in one process, one with the option and one without, timed alternately collect by collect with device events:
medians of 20 timed collects after 3 warm-up, and a difference counts only where the medians differ by more than the larger of the two
runs' (max - min) spreads; then hh_window_metrics's five launches alone.  Reported as a cost against the collect without the option,
not gated.
--outcomes (both tools): what outcomes=True costs a collect — T taps (hh_outcome_tap) and hh_episode_outcomes' two launches — by the
same rule, the rollout with the option against its own twin without it; then the two table launches and one tap alone."""
import ctypes as C
import statistics

import torch

WARMUP, TIMED = 3, 20


def metrics_launches_us(ep, n=200):
    """the three launches of hh_episodes_metrics alone, eagerly, back to back on the idle stream over the last emitted batch -> us per call
    (launch gaps included; the totals are put back afterwards)"""
    dev = ep.metrics_device()["totals"].device
    keep = ep.metrics_device()["totals"].clone()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(10):
        ep.enqueue_metrics(st)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        ep.enqueue_metrics(st)
    e1.record()
    torch.cuda.synchronize()
    ep.metrics_device()["totals"].copy_(keep)
    return 1e3 * e0.elapsed_time(e1) / n


def metrics_lines(ep, tr, ce, cm):
    """tr / ce / cm: median ms per collect of truncate_episodes, complete_episodes and complete_episodes with metrics=True"""
    us = metrics_launches_us(ep)
    m = ep.metrics()
    return [f"median ms per collect: truncate_episodes {tr:.3f} | complete_episodes {ce:.3f} | complete_episodes+metrics {cm:.3f}",
            f"emission overhead (four launches) {ce - tr:.3f} ms | metrics overhead (three launches) {cm - ce:+.3f} ms = "
            f"{100 * (cm - ce) / ce:+.2f} % of a complete_episodes collect = {(cm - ce) / max(ce - tr, 1e-9):.2f} x the emission",
            f"hh_episodes_metrics alone (eager, back to back, launch gaps included) on the last batch of {m['timesteps_this_iter']} rows / "
            f"{m['episodes_this_iter']} episodes: {us:.1f} us per call",
            f"last collect: episode_reward_mean {m['episode_reward_mean']:.4f} min {m['episode_reward_min']:.4f} max {m['episode_reward_max']:.4f} "
            f"episode_len_mean {m['episode_len_mean']:.2f} vf_explained_var {m['vf_explained_var']} episodes_total {m['episodes_total']} "
            f"timesteps_total {m['timesteps_total']}"]


def window_launches_us(wm, n=200):
    """the five launches of hh_window_metrics alone, eagerly, back to back on the idle stream over the last window -> us per call (launch
    gaps included; every call advances the carry and the totals: both are put back afterwards)"""
    keep = {k: getattr(wm, k).clone() for k in ("run_return", "run_len", "_totals")}
    st = C.c_void_p(torch.cuda.current_stream(wm.run_len.device).cuda_stream)
    for _ in range(10):
        wm.enqueue(st)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        wm.enqueue(st)
    e1.record()
    torch.cuda.synchronize()
    for k, v in keep.items():
        getattr(wm, k).copy_(v)
    return 1e3 * e0.elapsed_time(e1) / n


def _ms(ro):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ro.collect()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def window_lines(plain, on):
    """plain / on: the two rollouts (batch_mode="truncate_episodes"; on with window_metrics=True) -> the lines for the log"""
    for _ in range(WARMUP):
        plain.collect()
        on.collect()
    torch.cuda.synchronize()
    t_plain, t_on, eps = [], [], []
    for _ in range(TIMED):                          # alternate: drift of the box hits both
        t_plain.append(_ms(plain))
        t_on.append(_ms(on))
        eps.append(int(on.window_metrics.n_episodes))
    m = on.window_metrics.metrics()
    us = window_launches_us(on.window_metrics)
    med = statistics.median
    d = med(t_on) - med(t_plain)
    spread = max(max(t_plain) - min(t_plain), max(t_on) - min(t_on))
    word = "no difference beyond the spread" if abs(d) <= spread else ("cost" if d > 0 else "gain")
    paired = med([a - p for a, p in zip(t_on, t_plain)])
    return [f"ms per collect, medians of {TIMED} after {WARMUP}: truncate_episodes {med(t_plain):.3f} (min {min(t_plain):.3f}, max {max(t_plain):.3f}) | "
            f"truncate_episodes+window_metrics {med(t_on):.3f} (min {min(t_on):.3f}, max {max(t_on):.3f})",
            f"window_metrics overhead (five launches): medians {d * 1e3:+.1f} us apart = {100 * d / med(t_plain):+.3f} % of a collect, larger spread "
            f"{spread * 1e3:.1f} us: {word} (median of the {TIMED} paired differences {paired * 1e3:+.1f} us)",
            f"hh_window_metrics alone (eager, back to back, launch gaps included) on the last window of {m['timesteps_this_iter']} rows / "
            f"{m['episodes_this_iter']} episodes: {us:.1f} us per call; episodes per timed window min {min(eps)} max {max(eps)}",
            f"last collect: episode_reward_mean {m['episode_reward_mean']:.4f} min {m['episode_reward_min']:.4f} max {m['episode_reward_max']:.4f} "
            f"episode_len_mean {m['episode_len_mean']:.2f} vf_explained_var {m['vf_explained_var']} episodes_total {m['episodes_total']} "
            f"timesteps_total {m['timesteps_total']}"]


def _consumer(ro):
    return ro.episodes if ro.episodes is not None else ro.window_metrics


def _alone_us(call, n=200):
    """an idempotent enqueue, eagerly, back to back on the idle stream -> us per call (launch gaps included)"""
    for _ in range(10):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def outcome_lines(plain, on, what):
    """plain / on: two rollouts of one configuration and seed, on with outcomes=True; what: the configuration's name -> the lines for the
    log.  hh_episode_outcomes rewrites the same segment from the same window and a tap the same row: both are timed alone as they stand."""
    for _ in range(WARMUP):
        plain.collect()
        on.collect()
    torch.cuda.synchronize()
    t_plain, t_on, eps = [], [], []
    c = _consumer(on)
    for _ in range(TIMED):                          # alternate: drift of the box hits both
        t_plain.append(_ms(plain))
        t_on.append(_ms(on))
        eps.append(int(c.metrics_device()["outcome_flags"][1]))
    m = c.metrics()
    st = C.c_void_p(torch.cuda.current_stream(on.done.device).cuda_stream)
    table_us = _alone_us(lambda: c._outcomes.enqueue(st))
    tap_us = _alone_us(lambda: on.w.outcome_tap(on.done[0], on.outcome[0]))
    med = statistics.median
    d = med(t_on) - med(t_plain)
    spread = max(max(t_plain) - min(t_plain), max(t_on) - min(t_on))
    word = "no difference beyond the spread" if abs(d) <= spread else ("cost" if d > 0 else "gain")
    paired = med([a - p for a, p in zip(t_on, t_plain)])
    T = on.done.shape[0]
    return [f"{what}: ms per collect, medians of {TIMED} after {WARMUP}: without {med(t_plain):.3f} (min {min(t_plain):.3f}, max {max(t_plain):.3f}) | "
            f"outcomes=True {med(t_on):.3f} (min {min(t_on):.3f}, max {max(t_on):.3f})",
            f"{what}: outcomes overhead ({T} taps + two table launches): medians {d * 1e3:+.1f} us apart = {100 * d / med(t_plain):+.3f} % of a collect, "
            f"larger spread {spread * 1e3:.1f} us: {word} (median of the {TIMED} paired differences {paired * 1e3:+.1f} us)",
            f"{what}: alone (eager, back to back, launch gaps included): hh_episode_outcomes {table_us:.1f} us per call on a table of "
            f"{m['episodes_this_iter']} episodes, hh_outcome_tap {tap_us:.1f} us per call; episodes ended per timed window min {min(eps)} max {max(eps)}",
            f"{what}: last collect: agents_win {m['agents_win']} opps_win {m['opps_win']} draw {m['draw']} outcome_pct {m['outcome_pct']} "
            f"episode_reward_mean_by_outcome {m['episode_reward_mean_by_outcome']} episode_len_mean_by_outcome {m['episode_len_mean_by_outcome']}"]
