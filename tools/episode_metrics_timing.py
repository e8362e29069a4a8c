"""Shared by tools/episode_emit_bench.py and tools/commander_episodes_bench.py (--metrics): the time of hh_episodes_metrics's three
launches alone, and the lines both tools report about an `EpisodeBatch(metrics=True)`."""
import ctypes as C

import torch


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
