"""Timing of the trainable commander (hh_commander_sample, CommanderRollout) -> profiles/commander_rollout.log.

  1. the sampler kernel alone at 3 x {1024, 8192, 65536} rows, against the plain-PyTorch fp32 forward of the same weights on the GPU
     (tests/commander_ref.py), the variants alternated in one process after a warm-up, timed with device events;
  2. CommanderRollout (N = 8192, T = 16, VariantNetPilot, one HIP graph per collect) against the same macro steps replaying the actions it
     sampled (same world, same snapshot, same trajectories), and the sampling + bootstrap + GAE part alone: ms per commander step.
Useful FLOP: 2.06 MFLOP per agent row (both branches, the 500 x 500 shared layer twice); dense fp16 peak ~2.5 PFLOP/s.

Run:  python tools/commander_bench.py [--out profiles/commander_rollout.log] [--sampler-only]
"""
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FLOP_PER_ROW = 2.06e6
PEAK_F16 = 2.5e15


def _time(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)   # ms


def sampler(lines):
    import commander_ref as CR
    from hhmarl_2d_amd.commander import CommanderNet, random_weights
    sd = random_weights(1)
    net = CommanderNet(0, 3 * 65536).set_weights(sd)
    sdt = CR.to_torch(sd, torch.float32, "cuda")
    for N in (1024, 8192, 65536):
        g = torch.Generator(device="cuda").manual_seed(N)
        obs = torch.rand((N, 3, 34), device="cuda", generator=g)
        h = torch.rand((N, 3, 2, 200), device="cuda", generator=g) - 0.5
        h2 = torch.empty_like(h)
        u = torch.rand((N, 3), device="cuda", generator=g, dtype=torch.float64)
        a = torch.empty((N, 3), dtype=torch.int8, device="cuda")
        lp, vf = torch.empty((N, 3), device="cuda"), torch.empty((N, 3), device="cuda")
        hip = lambda: net.sample(obs, h, h2, uniforms=u, actions=a, logp=lp, vf=vf)

        def ref():
            with torch.no_grad():
                CR.arena_forward(sdt, obs, h)
        reps = 50 if N < 65536 else 20
        for f in (hip, ref, hip, ref):      # warm-up
            f()
        torch.cuda.synchronize()
        t_hip, t_ref = [], []
        for _ in range(3):                  # alternated
            t_hip.append(_time(hip, reps))
            t_ref.append(_time(ref, reps))
        th, tr = min(t_hip), min(t_ref)
        rows = 3 * N
        lines.append(f"sampler  rows {rows:7d}  hh_k_commander {th * 1e3:9.1f} us  ({rows * FLOP_PER_ROW / th / 1e9:6.1f} TFLOP/s useful, "
                     f"{100 * rows * FLOP_PER_ROW / th / 1e-3 / PEAK_F16:4.1f} % of dense fp16 peak)   PyTorch fp32 forward {tr * 1e3:9.1f} us   "
                     f"speed-up {tr / th:5.2f}x")
        print(lines[-1], flush=True)


def _time_setup(setup, fn, reps):
    """median of device-event timings of fn, with an untimed (host-synchronous) setup before every repetition"""
    ts = []
    for _ in range(reps):
        setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def rollout(lines):
    """Three graphs on ONE world, each replayed from the same snapshot (World.get_state / set_state + the rollout's carried buffers), so the
    first two run the same trajectories:
      collect   CommanderRollout.collect: T x (sample + macro step) + bootstrap + GAE
      fixed     T macro steps whose commander actions are the ones `collect` sampled from that snapshot (a static tensor)
      sampling  the collect's T samples + bootstrap + GAE without the world
    """
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.env_hier import macro_step
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    import ctypes as C
    N, T, ISSUE_STEP_MS = 8192, 16, 1.3
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=3, auto_reset=True), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(1))
    pilot = VariantNetPilot(w, seed=2)
    r = CommanderRollout(w, net, pilot, T)
    r.start()
    torch.cuda.synchronize()
    snap = w.get_state()
    carried = [x.clone() for x in (r.obs[T], r.state_in[T], r._fresh)]

    def restore():
        w.set_state(snap)
        for dst, src in zip((r.obs[T], r.state_in[T], r._fresh), carried):
            dst.copy_(src)
    restore()
    r.collect()                                                        # captures the collect's graph
    torch.cuda.synchronize()
    acts = r.actions.clone()
    end_obs = r.obs[T].clone()
    out, pbuf = w.alloc_outputs(), r._pbuf
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g_fixed = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_fixed, stream=side):
            for t in range(T):
                macro_step(w, acts[t], pilot, out=out, pilot_buf=pbuf, early_exit=False)
        g_samp = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_samp, stream=side):
            for t in range(T):
                net.sample(r.obs[t], r.state_in[t], r.state_in[t + 1], fresh=r._fresh if t == 0 else r.done[t - 1], world=w,
                           actions=r._tmp_act, logp=r.logp[t], vf=r.vf[t])
            net.sample(r.obs[T], r.state_in[T], r._h_scratch, fresh=r.done[T - 1], greedy=True, actions=r._tmp_act, logp=r._tmp_logp, vf=r.vf[T])
            L.check(L.lib().hh_gae_rllib(T, N, 3, C.c_void_p(r.reward.data_ptr()), C.c_void_p(r.vf.data_ptr()), C.c_void_p(r.done.data_ptr()),
                                         0.99, 1.0, C.c_void_p(r.adv.data_ptr()), C.c_void_p(r.target.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.current_stream().wait_stream(side)
    restore()
    g_fixed.replay()
    torch.cuda.synchronize()
    same = torch.equal(out[0], end_obs)
    coll, fixed, samp = (lambda: r.collect()), (lambda: g_fixed.replay()), (lambda: g_samp.replay())
    tc, tf, ts = [], [], []
    for _ in range(3):                                                 # alternated
        tc.append(_time_setup(restore, coll, 3))
        tf.append(_time_setup(restore, fixed, 3))
        ts.append(_time_setup(restore, samp, 3))
    c, f, sm = (statistics.median(x) / T for x in (tc, tf, ts))
    lines.append(f"rollout  N {N}  T {T}  VariantNetPilot, one world from one snapshot (same trajectories: {same}):")
    lines.append(f"  CommanderRollout.collect                        {c:6.3f} ms / commander step ({N / c / 1e3:5.2f}e6 commander-steps/s)")
    lines.append(f"  the same macro steps, sampled actions replayed  {f:6.3f} ms / commander step ({N / f / 1e3:5.2f}e6 commander-steps/s)")
    lines.append(f"  sampling + bootstrap + GAE alone                {sm:6.3f} ms / commander step")
    lines.append(f"  overhead: collect - replay = {c - f:5.3f} ms = {100 * (c - f) / f:5.1f} % of this box's step; sampling alone = "
                 f"{100 * sm / f:5.1f} % of it, {100 * sm / ISSUE_STEP_MS:5.1f} % of the {ISSUE_STEP_MS} ms step the 25 % target is stated against")
    for x in lines[-5:]:
        print(x, flush=True)


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "commander_rollout.log")
    lines = [f"# tools/commander_bench.py on {torch.cuda.get_device_name(0)}; medians of device-event timings, variants alternated after a warm-up"]
    sampler(lines)
    if "--sampler-only" in sys.argv:   # the profiler run (rocprofv3 --kernel-trace --stats)
        return
    rollout(lines)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
