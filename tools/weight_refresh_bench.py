"""Per-iteration cost of getting a learner's new weights into the samplers (train_hetero.py's two trainable policies + train_hier.py's
commander), measured three ways on the same fp32 CUDA tensors:
  host    PolicyBank.load_trainable x 2 from `.cpu()` copies of every tensor + CommanderNet.set_weights (which copies to the host itself):
          host clock around the calls, ended by a device synchronise
  device  PolicyBank.refresh x 2 + CommanderNet.refresh_weights, eager: device events around the enqueued work
  graph   the same three calls captured into one CUDA graph and replayed: device events
The packed bytes of both paths are compared once (they must be equal).  For kernel times run it under
`rocprofv3 --kernel-trace --stats -- python tools/weight_refresh_bench.py ...` (hh_k_refresh_actor / _critic / _commander).
    python tools/weight_refresh_bench.py [--iters 20] [--warmup 3] [--out profiles/weight_refresh.log]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hhmarl_2d_amd import commander as CM  # noqa: E402
from hhmarl_2d_amd import policy_nets as PN  # noqa: E402
from hhmarl_2d_amd.pilots import PolicyBank, tie_shared_layer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_refresh.log"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    kinds = (PN.FIGHT1, PN.FIGHT2)
    bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=1 << 15)
    net = CM.CommanderNet(0, 3 * 8192).set_weights(CM.random_weights(1))
    # the learner's parameters: fp32 CUDA tensors (one shared layer for both policies, as the reference's module-level SHARED_LAYER)
    sds = tie_shared_layer([PN.random_weights(k, 2) for k in kinds])
    cache = {}
    learner = []
    for k, sd in zip(kinds, sds):
        d = {n: cache.setdefault(id(v), torch.from_numpy(v).to(dev)) for n, v in sd.items()}
        d.update({n: torch.from_numpy(v).to(dev) for n, v in PN.random_critic_weights(k, 2).items()})
        learner.append(d)
    cmd = {n: torch.from_numpy(v).to(dev) for n, v in CM.random_weights(2).items()}
    n_bytes = sum(t.numel() * 4 for t in {id(t): t for d in learner for t in d.values()}.values()) + sum(t.numel() * 4 for t in cmd.values())
    say(f"# tools/weight_refresh_bench.py on {torch.cuda.get_device_name(0)}: Fight1 + Fight2 (actor + value branch, tied shared layer) "
        f"+ CommanderGru per iteration, {n_bytes / 1e6:.2f} MB of fp32 source tensors; {a.iters} iterations after {a.warmup} warm-up")

    def host_path():
        for slot, kind in enumerate(kinds):
            h = {n: t.cpu().numpy() for n, t in learner[slot].items()}
            bank.load_trainable(slot, kind, h, h)
        net.set_weights(cmd)

    def device_path():
        bank.refresh_trainable(learner)
        net.refresh_weights(cmd)

    for _ in range(a.warmup):
        host_path()
        device_path()
    torch.cuda.synchronize()
    # the two paths write the same bytes
    ref = [bank.packed(s, p) for s in (0, 1) for p in range(5)] + [net.packed(p) for p in (0, 1)]
    host_path()
    hst = [bank.packed(s, p) for s in (0, 1) for p in range(5)] + [net.packed(p) for p in (0, 1)]
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(ref, hst))
    say(f"packed bytes of the device path == host path: {same} ({sum(x.numel() for x in ref) / 1e6:.2f} MB compared)")

    host_ms = []
    for _ in range(a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_path()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)

    def events(fn):
        out = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.iters):
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    eager_ms = events(device_path)
    eager_wall = []
    for _ in range(a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device_path()
        torch.cuda.synchronize()
        eager_wall.append((time.perf_counter() - t0) * 1e3)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        device_path()
    g.replay()
    torch.cuda.synchronize()
    graph_ms = events(g.replay)
    q = lambda v: f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"
    say(f"host path   (load_trainable x 2 from .cpu() + CommanderNet.set_weights), host clock to a synchronise: {q(host_ms)}")
    say(f"device path eager (refresh x 2 + refresh_weights), device events:                             {q(eager_ms)}")
    say(f"device path eager, host clock from enqueue to a synchronise:                                   {q(eager_wall)}")
    say(f"device path in one CUDA graph, device events around the replay:                                {q(graph_ms)}")
    say(f"host / device(graph) = {statistics.median(host_ms) / statistics.median(graph_ms):.0f}x")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
