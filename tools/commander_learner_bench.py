"""Where the time of the commander's PPO update goes on the MI355X, per minibatch step, at 256 and at 16384 unpadded rows:
  gru     forward + backward of both GRUs over sequences of 20 steps, input projection x W_ih^T + b_ih and its gradients included in all
          three: gru_sequence_pair (hh_gru_seq_forward / hh_gru_seq_backward) against the torch-op cell (gru_sequence_torch) and against
          torch.nn.GRU (MIOpen) with the same weights, device events
  step    one minibatch step of CommanderLearner (forward, loss, backward, Adam), fused against unfused
  update  one whole update, fused against unfused, at N arenas and T commander steps per collect
  inputs  --inputs: only the minibatch step with CommanderLearner(inputs="fused") (hh_input_stage_*) against the default inputs="torch",
          both in one process, at 256 and 16384 rows; its lines are appended to --out.  A difference is called a gain (or a loss) only
          where the medians differ by more than the larger of the two (max - min) spreads
  trunk   --trunk: shared_layer, bias and tanh over the actor's and the critic's rows through CommanderLearner(trunk="fused")
          (hh_dense_tanh_*, split-fp16 MFMA) against the default two float32 GEMMs + tanh, both in one process: the layer alone (forward
          + backward) and the two kernel calls alone (useful TFLOP/s, 2 R K N per product) at 2 x 262 and 2 x 16396 rows, and the
          minibatch step with inputs="fused" at 256 and 16384 rows; its lines are appended to --out.  The same rule for gain / loss
  graph   --graph: CommanderLearner(optimizer="fused", step="graph") with inputs="fused" against the eager step, all in one process: one
          minibatch step at 256 and 16384 rows as eager + torch Adam, eager + device Adam and graph replay, 50 steps back to back, one
          whole update at sgd_minibatch_size = 256 eager against graph (captures included) and the cost of one capture; its lines are
          appended to --out.  The same rule for gain / loss, with eager + torch Adam as the base.  `--step graph --launches eager|graph`
          runs nothing but --launch-count steps of that form after the set-up: the program of a kernel trace that counts launches
          (--heads-mode fused: of a heads="fused" learner)
  heads   --heads: CommanderLearner(heads="fused") (hh_heads_loss, n_comp = 1) against heads="torch", both in one process, inputs="fused":
          the kernel alone at 280 and 71200 rows against its algorithmic bytes, the minibatch step at 256 and 16384 rows eager + torch
          Adam and as graph replay, 50 replays back to back, and one whole graph update at sgd_minibatch_size = 256; appended to --out.
          The same rule for gain / loss
  tile    --tile: the compiled tiles of hh_k_gru_seq_fwd / _bwd, each forced through HH_GRU_TILE in a child process of its own: both GRUs'
          forward + backward kernels alone at --tile-seqs sequence counts (13 ... 854) and the graph step at 256 rows; then every narrow
          tile against tile 16 by the same rule; appended to --out
  shuffle --shuffle: CommanderLearner(shuffle_sequences=True) against shuffle_sequences=False as a COST, both in one process: the two stage
          launches alone (hh_minibatch_stage against hh_minibatch_stage_gather drawing from the whole batch), the graph step at 256 and
          16384 rows, one whole update at sgd_minibatch_size = 256 (medians of --iters updates), the host time of shuffled_schedule and
          the order table's bytes; appended to --out.  The same spread rule, worded cost / gain / no difference
  window  --window: CommanderLearner.update_window on a CommanderRollout's fixed [T, N] window (batch_mode = "truncate_episodes") next to
          update on whole episodes, both in one process: window_cut and hh_window_gather against their torch twins (the gather as bytes/s of
          what it reads and writes), window_sequences against CommanderEpisodeBatch.sequences(), policy_batch on both, one whole update each,
          and the graph captures over three windows with kl_coeff = 0; appended to --out.  The same spread rule
Every GPU step runs as a child process of its own under `timeout -k 10`, the steps chained with && in one shell command: the first one
that fails or runs out of time ends the run, nothing is retried.
    python tools/commander_learner_bench.py [--arenas 8192] [--T 16] [--iters 20] [--out profiles/commander_learner.log]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("gru", 240), ("step", 300), ("update", 480))     # step -> its time limit in seconds


def events(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    out = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(iters):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def q(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def sequences(rows, L, seed, device):
    """ragged sequence lengths like a batch of episodes cut into chunks of L: about 13 sequences per 256 rows"""
    import torch
    g = torch.Generator().manual_seed(seed)
    lens, total = [], 0
    while total < rows:
        n = min(L if torch.rand((), generator=g) < 0.9 else int(torch.randint(1, L + 1, (), generator=g)), rows - total)
        lens.append(n)
        total += n
    return torch.tensor(lens, dtype=torch.int32, device=device)


def step_gru(a, say):
    import torch
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    Lm, H = 20, 200
    for rows in (256, 16384):
        seq_len = sequences(rows, Lm, 1, dev)
        S = seq_len.numel()
        g = torch.Generator().manual_seed(2)
        mk = lambda *shape, s=1.0: (s * torch.randn(shape, generator=g)).to(dev).requires_grad_(True)
        tail = [(mk(S, H, s=0.5), mk(3 * H, H, s=H ** -0.5), mk(3 * H, s=0.1)) for _ in range(2)]      # h0, w_hh, b_hh
        w_ih, b_ih = [mk(3 * H, H, s=H ** -0.5) for _ in range(2)], [mk(3 * H, s=0.1) for _ in range(2)]
        wy = [torch.randn((S, Lm, H), generator=g).to(dev) for _ in range(2)]
        grus = [torch.nn.GRU(H, H, batch_first=True).to(dev) for _ in range(2)]
        xs = [torch.randn((S, Lm, H), generator=g).to(dev).requires_grad_(True) for _ in range(2)]
        with torch.no_grad():
            for gru, (h0, w_hh, b_hh), wi, bi in zip(grus, tail, w_ih, b_ih):
                gru.weight_hh_l0.copy_(w_hh)
                gru.bias_hh_l0.copy_(b_hh)
                gru.weight_ih_l0.copy_(wi)
                gru.bias_ih_l0.copy_(bi)

        def clear():
            for t in [t for p in tail for t in p] + w_ih + b_ih:
                t.grad = None
            for gru, x in zip(grus, xs):
                gru.zero_grad(set_to_none=True)
                x.grad = None

        def parts():      # the time-parallel input projection, one GEMM per GRU
            return [(x @ wi.T + bi,) + p for x, wi, bi, p in zip(xs, w_ih, b_ih, tail)]

        def fused():
            clear()
            ya, yv = LR.gru_sequence_pair(*parts(), seq_len)
            ((ya * wy[0]).sum() + (yv * wy[1]).sum()).backward()

        def cell():
            clear()
            ys = [LR.gru_sequence_torch(*p, seq_len) for p in parts()]
            ((ys[0] * wy[0]).sum() + (ys[1] * wy[1]).sum()).backward()

        def miopen():     # nn.GRU over the padded [S, L] batch, all L steps of every sequence
            clear()
            ys = [gru(x, p[0][None].detach())[0] for gru, x, p in zip(grus, xs, tail)]
            ((ys[0] * wy[0]).sum() + (ys[1] * wy[1]).sum()).backward()

        t_f, t_c, t_m = (events(fn, a.iters, a.warmup) for fn in (fused, cell, miopen))
        mf, mc, mm = (statistics.median(t) for t in (t_f, t_c, t_m))
        say(f"both GRUs forward + backward with their input projections, {rows} rows in {S} sequences of <= {Lm} steps: fused (hh_gru_seq_*) "
            f"{q(t_f)}; torch-op cell {q(t_c)} ({mc / mf:.2f}x the fused time); torch.nn.GRU (MIOpen) {q(t_m)} ({mm / mf:.2f}x the fused time)")
        if mm < mf:
            say(f"    the fused kernels are SLOWER than torch.nn.GRU at {rows} rows")


def _rollout(a):
    import torch
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=a.arenas, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, auto_reset=True, horizon=a.horizon), device=0)
    net = CommanderNet(0, 3 * a.arenas).set_weights(random_weights(6))
    ro = CommanderRollout(w, net, VariantNetPilot(w, seed=8), a.T, batch_mode="complete_episodes", max_seq_len=20)
    for _ in range(max(3, a.horizon // (12 * a.T) + 2)):
        ro.collect()
    torch.cuda.synchronize()
    return ro, net


def step_step(a, say):
    import torch
    from hhmarl_2d_amd import learner as LR
    ro, net = _rollout(a)
    dev = torch.device("cuda", 0)
    for fused in (True, False):
        learner = LR.CommanderLearner.trainable_init(dev, seed=6, fused=fused)
        with torch.no_grad():
            b = learner.policy_batch(ro.episodes.sequences())
            b["old_logits"] = learner.old_logits(b)
        seq_len = b["seq_len"].cpu().numpy()
        for size in (256, 16384):
            s0, s1 = LR.minibatch_partition(seq_len, size)[0]
            mb = {k: v[s0:s1] for k, v in b.items()}
            mb["n_valid"] = torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device=dev)
            t = events(lambda: learner.minibatch_step(mb), a.iters, a.warmup)
            say(f"minibatch step (forward + loss + backward + Adam), fused = {fused!s:5}, {int(seq_len[s0:s1].sum())} unpadded rows in {s1 - s0} "
                f"sequences: {q(t)}")


def step_inputs(a, say):
    import torch
    from hhmarl_2d_amd import learner as LR
    ro, net = _rollout(a)
    dev = torch.device("cuda", 0)
    med = statistics.median
    say(f"# tools/commander_learner_bench.py --inputs on {torch.cuda.get_device_name(0)}: CommanderLearner(inputs=\"fused\") against the default "
        f"inputs=\"torch\", both in this run; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")
    learners = {inp: LR.CommanderLearner.trainable_init(dev, seed=6, inputs=inp) for inp in ("torch", "fused")}
    with torch.no_grad():
        b = learners["torch"].policy_batch(ro.episodes.sequences())
        b["old_logits"] = learners["torch"].old_logits(b)
    seq_len = b["seq_len"].cpu().numpy()
    for size in (256, 16384):
        s0, s1 = LR.minibatch_partition(seq_len, size)[0]
        mb = {k: v[s0:s1] for k, v in b.items()}
        mb["n_valid"] = torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device=dev)
        t = {inp: events(lambda: lr.minibatch_step(mb), a.iters, a.warmup) for inp, lr in learners.items()}
        spread = max(max(v) - min(v) for v in t.values())
        d = med(t["torch"]) - med(t["fused"])
        word = "no difference beyond the spread" if abs(d) <= spread else ("gain" if d > 0 else "loss")
        say(f"minibatch step (forward + loss + backward + Adam, fused GRU and loss), {int(seq_len[s0:s1].sum())} unpadded rows in {s1 - s0} sequences: "
            f"inputs = torch {q(t['torch'])}; inputs = fused {q(t['fused'])}; torch / fused = {med(t['torch']) / med(t['fused']):.2f}x, medians "
            f"{d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}")


def step_trunk(a, say):
    import ctypes as C

    import torch
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    med = statistics.median

    def verdict(t_torch, t_fused):
        spread = max(max(t_torch) - min(t_torch), max(t_fused) - min(t_fused))
        d = med(t_torch) - med(t_fused)
        word = "no difference beyond the spread" if abs(d) <= spread else ("gain" if d > 0 else "loss")
        return f"torch / fused = {med(t_torch) / med(t_fused):.2f}x, medians {d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}"

    say(f"# tools/commander_learner_bench.py --trunk on {torch.cuda.get_device_name(0)}: CommanderLearner(trunk=\"fused\") against the default "
        f"trunk=\"torch\", both in this run; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")
    lin = torch.nn.Linear(500, 500).to(dev)
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    for R in (262, 16396):
        g = torch.Generator().manual_seed(R)
        xs = [torch.tanh(torch.randn((R, 500), generator=g)).to(dev).requires_grad_(True) for _ in range(2)]
        dys = [(torch.randn((R, 500), generator=g) / R).to(dev) for _ in range(2)]

        def layer(fn):
            lin.zero_grad(set_to_none=True)
            for x in xs:
                x.grad = None
            torch.autograd.backward(fn(xs, lin.weight, lin.bias), dys)
        t_t, t_f = events(lambda: layer(LR.dense_tanh_torch), a.iters, a.warmup), events(lambda: layer(LR.dense_tanh), a.iters, a.warmup)
        say(f"shared layer (tanh(x W^T + b), 500 -> 500, the actor's and the critic's rows; forward + backward), 2 x {R} rows: "
            f"torch {q(t_t)}; fused {q(t_f)}; {verdict(t_t, t_f)}")
        io = (L.HHDenseSrc * 2)()
        keep = []
        for i in range(2):
            y, dx = torch.empty((R, 500), device=dev), torch.empty((R, 500), device=dev)
            keep += [y, dx]
            io[i].n_rows, io[i].x, io[i].ld, io[i].y, io[i].d_y, io[i].d_x = R, xs[i].data_ptr(), 500, y.data_ptr(), dys[i].data_ptr(), dx.data_ptr()
        nb = C.c_int64()
        L.check(lib.hh_dense_tanh_scratch_bytes(500, 500, 2, io, C.byref(nb)))
        scratch, d_w, d_b = torch.empty((nb.value // 4,), device=dev), torch.empty((500, 500), device=dev), torch.empty((500,), device=dev)
        w_, b_ = lin.weight.detach(), lin.bias.detach()
        flop = 2.0 * (2 * R) * 500 * 500
        runs = (("hh_dense_tanh_forward", 1, lambda: L.check(lib.hh_dense_tanh_forward(500, 500, 2, io, p(w_), p(b_), p(scratch), nb.value, st))),
                ("hh_dense_tanh_backward", 2, lambda: L.check(lib.hh_dense_tanh_backward(500, 500, 2, io, p(w_), p(d_w), p(d_b), p(scratch), nb.value, st))))
        for name, products, fn in runs:
            t = events(fn, a.iters, a.warmup)
            tf = products * flop / med(t) / 1e9
            say(f"    {name} alone, 2 x {R} rows: {q(t)} = {tf:.1f} useful TFLOP/s ({products} product(s) of 2 R K N = {flop / 1e9:.2f} GFLOP): "
                f"{100 * tf / 155:.1f} % of the 155 TF float32 matrix rate, {100 * tf / (2500 / 3):.1f} % of 2.5 PF / 3")
    ro, net = _rollout(a)
    learners = {tr: LR.CommanderLearner.trainable_init(dev, seed=6, inputs="fused", trunk=tr) for tr in ("torch", "fused")}
    with torch.no_grad():
        b = learners["torch"].policy_batch(ro.episodes.sequences())
        b["old_logits"] = learners["torch"].old_logits(b)
    seq_len = b["seq_len"].cpu().numpy()
    for size in (256, 16384):
        s0, s1 = LR.minibatch_partition(seq_len, size)[0]
        mb = {k: v[s0:s1] for k, v in b.items()}
        mb["n_valid"] = torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device=dev)
        t = {tr: events(lambda: lr.minibatch_step(mb), a.iters, a.warmup) for tr, lr in learners.items()}
        say(f"minibatch step (forward + loss + backward + Adam, fused GRU and loss, inputs = fused), {int(seq_len[s0:s1].sum())} unpadded rows in {s1 - s0} "
            f"sequences: trunk = torch {q(t['torch'])}; trunk = fused {q(t['fused'])}; {verdict(t['torch'], t['fused'])}")


GRAPH = dict(optimizer="fused", step="graph")


def verdict(t_base, t_new, base="base"):
    """the spread rule: a difference counts only where the medians differ by more than the larger of the two (max - min) spreads"""
    med = statistics.median
    spread = max(max(t_base) - min(t_base), max(t_new) - min(t_new))
    d = med(t_base) - med(t_new)
    word = "no difference beyond the spread" if abs(d) <= spread else ("gain" if d > 0 else "loss")
    return f"{base} / this = {med(t_base) / med(t_new):.2f}x, medians {d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}"


def _policy_batch(a, **kw):
    """the rollout's batch as a learner's policy batch with old_logits -> (rollout, net, batch, host seq_len)"""
    import torch
    from hhmarl_2d_amd import learner as LR
    ro, net = _rollout(a)
    base = LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, **kw)
    with torch.no_grad():
        b = base.policy_batch(ro.episodes.sequences())
        b["old_logits"] = base.old_logits(b)
    return ro, net, b, b["seq_len"].cpu().numpy()


def _one_minibatch(b, seq_len, size):
    """the first minibatch of >= size rows -> (its slice of the batch, the same with n_valid, sequences, unpadded rows)"""
    import torch
    from hhmarl_2d_amd import learner as LR
    s0, s1 = LR.minibatch_partition(seq_len, size)[0]
    sub = {k: v[s0:s1].contiguous() for k, v in b.items()}
    mb = dict(sub, n_valid=torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device=b["obs"].device))
    return sub, mb, s1 - s0, int(seq_len[s0:s1].sum())


def _graph_learner(sub, n_steps, **kw):
    """a graph learner whose one update is n_steps visits of the single minibatch `sub` -> (learner, milliseconds graph_prepare took)"""
    import torch
    from hhmarl_2d_amd import learner as LR
    lr = LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, num_sgd_iter=n_steps, sgd_minibatch_size=1 << 30, **GRAPH, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lr.graph_prepare(sub)
    torch.cuda.synchronize()
    return lr, (time.perf_counter() - t0) * 1e3


def step_graph(a, say):
    import torch
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    FUSED = dict(inputs="fused", heads=a.heads_mode if a.launches else "torch")
    make = lambda **kw: LR.CommanderLearner.trainable_init(dev, seed=6, **FUSED, **kw)
    ro, net, b, seq_len = _policy_batch(a, **FUSED)
    if a.launches:       # for a kernel trace: nothing but launch_count steps of one form after the set-up
        sub, mb, _, _ = _one_minibatch(b, seq_len, 256)
        if a.launches == "graph":
            lr, _ = _graph_learner(sub, a.launch_count, **FUSED)
            lr.graph_replay(a.launch_count)
        else:
            lr = make()
            for _ in range(a.launch_count):
                lr.minibatch_step(mb)
        torch.cuda.synchronize()
        print(f"{a.launch_count} {a.launches} steps done", flush=True)
        return
    say(f"# tools/commander_learner_bench.py --graph on {torch.cuda.get_device_name(0)}: CommanderLearner(optimizer=\"fused\", step=\"graph\") against the "
        f"eager step with torch.optim.Adam, all in this run; inputs = fused, GRU tile {LR.gru_seq_tile(13)} at 13 sequences and {LR.gru_seq_tile(854)} at "
        f"854; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")
    K = 50

    def burst(fn):
        """K steps back to back, no host synchronisation between them -> milliseconds per step, three times"""
        out = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append((e0.elapsed_time(e1) / K, (time.perf_counter() - t0) * 1e3 / K))
        return "; ".join(f"{d:.3f} device / {h:.3f} host" for d, h in out)

    base, dev_adam = make(), make(optimizer="fused")
    for size in (256, 16384):
        sub, mb, n_seq, n_rows = _one_minibatch(b, seq_len, size)
        n_total = 4 * (a.iters + a.warmup) + 4 * K + 8
        dev_adam._book.begin(n_total)
        graph, t_cap = _graph_learner(sub, n_total, **FUSED)
        t_e = events(lambda: base.minibatch_step(mb), a.iters, a.warmup)
        t_f = events(lambda: dev_adam.minibatch_step(mb), a.iters, a.warmup)
        t_g = events(lambda: graph.graph_replay(1), a.iters, a.warmup)
        say(f"minibatch step (forward + loss + backward + Adam, fused GRU and loss), {n_rows} unpadded rows in {n_seq} sequences: eager + torch Adam "
            f"{q(t_e)}; eager + device Adam {q(t_f)} [{verdict(t_e, t_f, 'eager+torch')}]; graph {q(t_g)} [{verdict(t_e, t_g, 'eager+torch')}]")
        say(f"    {K} steps back to back, ms per step, three runs: eager + torch Adam {burst(lambda: [base.minibatch_step(mb) for _ in range(K)])} | "
            f"eager + device Adam {burst(lambda: [dev_adam.minibatch_step(mb) for _ in range(K)])} | graph {burst(lambda: graph.graph_replay(K))}")
        say(f"    graph_prepare (upload, warm-up, capture) of this step: {t_cap:.1f} ms on the host clock")
        del graph
    res = {}
    for label, kw in (("eager + torch Adam", {}), ("graph", GRAPH)):
        lr = make(num_sgd_iter=a.passes, sgd_minibatch_size=256, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = lr.update(ro.episodes, net)
        torch.cuda.synchronize()
        res[label] = ((time.perf_counter() - t0) * 1e3, st, lr)
    (t_e, st_e, _), (t_g, st_g, lr_g) = res["eager + torch Adam"], res["graph"]
    say(f"one update at {a.arenas} arenas, T = {a.T} ({a.passes} pass(es), minibatches of >= 256 rows: {st_e['steps']} steps over {st_e['rows']} rows), "
        f"host clock to a synchronise, first update of a new learner (the graph's includes its {lr_g._book.captures} capture(s)): eager + torch Adam "
        f"{t_e:.1f} ms; graph {t_g:.1f} ms; eager / graph = {t_e / t_g:.2f}x")
    say(f"    mean statistics, eager: { {k: round(v, 6) for k, v in st_e.items()} }")
    say(f"    mean statistics, graph: { {k: round(v, 6) for k, v in st_g.items()} }")


def step_heads(a, say):
    """CommanderLearner(heads="fused") (hh_heads_loss with n_comp = 1: tanh, act_out, val_out, the Categorical's loss and their backward as one
    row pass) against heads="torch", both in this run, inputs = fused: the kernel alone at 280 and 71200 rows, the minibatch step at 256 and
    16384 rows (eager + torch Adam, and the graph step: one replay per timing and 50 back to back), one whole graph update."""
    import ctypes as C
    import torch
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    med = statistics.median
    K = 50
    say(f"# tools/commander_learner_bench.py --heads on {torch.cuda.get_device_name(0)}: CommanderLearner(heads=\"fused\") against the default "
        f"heads=\"torch\", both in this run; inputs = fused; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    for R in (280, 71200):
        g = torch.Generator().manual_seed(R)
        r = lambda *shape: torch.randn(shape, generator=g).to(dev)
        za, zc, w_act, b_act, w_val, b_val = r(R, 500), r(R, 500), 0.04 * r(3, 500), 0.04 * r(3), 0.04 * r(500), 0.04 * r(1)
        old, act, old_logp, adv, target = r(R, 4), torch.zeros((R,), dtype=torch.int8, device=dev), -1.0 + 0.1 * r(R), r(R), r(R)
        n_valid = torch.full((1,), R, dtype=torch.int32, device=dev)
        outs = [torch.empty_like(t) for t in (za, zc, w_act, b_act, w_val, b_val)]
        stats = torch.empty((6,), dtype=torch.float64, device=dev)
        nb = C.c_int64()
        L.check(lib.hh_heads_loss_scratch_bytes(R, 1, C.byref(nb)))
        scratch = torch.empty((nb.value // 8,), dtype=torch.float64, device=dev)
        prm = L.HHPpoLossParams(n_comp=1, reserved0=0, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2, reserved1=0.0)
        fn = lambda: L.check(lib.hh_heads_loss(R, p(za), p(zc), p(w_act), p(b_act), p(w_val), p(b_val), p(old), p(act), p(old_logp), p(adv), p(target),
                                               None, p(n_valid), C.byref(prm), p(stats), *[p(o) for o in outs], None, None, p(scratch), nb.value, st))
        t = events(fn, a.iters, a.warmup)
        nbytes = R * (4 * 500 * 4 + 4 * 4 + 1 + 12) + 2 * 4 * 501 * 4
        say(f"    hh_heads_loss alone (two launches), n_comp = 1, {R} rows: {q(t)} = {nbytes / med(t) / 1e6:.1f} GB/s of {nbytes / 1e6:.2f} MB algorithmic "
            f"bytes ({100 * nbytes / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")
        del za, zc, outs, scratch

    def burst(fn):
        out = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / K)
        return " ".join(f"{d:.3f}" for d in out)

    make = lambda **kw: LR.CommanderLearner.trainable_init(dev, seed=6, inputs="fused", **kw)
    ro, net, b, seq_len = _policy_batch(a, inputs="fused")
    eager = {h: make(heads=h) for h in ("torch", "fused")}
    for size in (256, 16384):
        sub, mb, n_seq, n_rows = _one_minibatch(b, seq_len, size)
        n_total = 2 * (a.iters + a.warmup) + 4 * K + 8
        graphs = {h: _graph_learner(sub, n_total, inputs="fused", heads=h)[0] for h in ("torch", "fused")}
        t_e = {h: events(lambda lr=lr: lr.minibatch_step(mb), a.iters, a.warmup) for h, lr in eager.items()}
        t_g = {h: events(lambda lr=lr: lr.graph_replay(1), a.iters, a.warmup) for h, lr in graphs.items()}
        say(f"minibatch step (forward + loss + backward + Adam, fused GRU), {n_rows} unpadded rows in {n_seq} sequences: eager + torch Adam: heads = torch "
            f"{q(t_e['torch'])}; heads = fused {q(t_e['fused'])} [{verdict(t_e['torch'], t_e['fused'], 'torch')}]")
        say(f"    graph step: heads = torch {q(t_g['torch'])}; heads = fused {q(t_g['fused'])} [{verdict(t_g['torch'], t_g['fused'], 'torch')}]")
        say(f"    {K} graph replays back to back, ms per step, three runs: heads = torch {burst(lambda: graphs['torch'].graph_replay(K))} | heads = fused "
            f"{burst(lambda: graphs['fused'].graph_replay(K))}")
        del graphs
    res = {}
    for h in ("torch", "fused", "torch", "fused"):
        lr = make(heads=h, num_sgd_iter=a.passes, sgd_minibatch_size=256, kl_coeff=0.0, **GRAPH)
        lr.update(ro.episodes, net)                # the first update captures
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stu = lr.update(ro.episodes, net)
            torch.cuda.synchronize()
            res.setdefault(h, []).append((time.perf_counter() - t0) * 1e3)
    say(f"one whole graph update at {a.arenas} arenas, T = {a.T} ({a.passes} pass(es), minibatches of >= 256 rows: {stu['steps']} steps over {stu['rows']} "
        f"rows, kl_coeff = 0 so that no graph is captured again), host clock to a synchronise, 2 x 3 updates after the capturing one, learners alternating: "
        f"heads = torch {q(res['torch'])}; heads = fused {q(res['fused'])} [{verdict(res['torch'], res['fused'], 'torch')}]")


def step_clip(a, say):
    """CommanderLearner(grad_clip=...) against grad_clip = None (the step as it was), both in this run: hh_grad_norm on the module's
    tensors, then the graph step at 256 and 16384 rows, one replay per timing and 50 back to back.  Reported as a cost."""
    import torch
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    med = statistics.median
    FUSED = dict(inputs="fused")
    ro, net, b, seq_len = _policy_batch(a, **FUSED)
    say(f"# tools/commander_learner_bench.py --clip on {torch.cuda.get_device_name(0)}: CommanderLearner(grad_clip=...) against grad_clip = None, both in "
        f"this run; inputs = fused, graph step; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")

    def cost(t_base, t_new):
        spread = max(max(t_base) - min(t_base), max(t_new) - min(t_new))
        d = med(t_new) - med(t_base)
        word = "no difference beyond the spread" if abs(d) <= spread else ("cost" if d > 0 else "gain")
        return f"without -> with: medians {d * 1e3:+.1f} us apart, larger spread {spread * 1e3:.1f} us: {word}"

    module = LR.CommanderLearner.trainable_init(dev, seed=6, **FUSED).module
    gs = [torch.randn_like(p) for p in module.parameters()]
    n = sum(g.numel() for g in gs)
    clip, scratch = torch.zeros((2,), dtype=torch.float64, device=dev), LR.grad_norm_scratch(gs)
    t = events(lambda: LR.grad_norm(gs, 1.0, clip, scratch=scratch), a.iters, a.warmup)
    say(f"    hh_grad_norm alone ({(len(gs) + 63) // 64} partial launch(es) + the final one), the module's {len(gs)} tensors ({n} elements, {scratch.numel()} "
        f"tiles): {q(t)} = {4 * n / med(t) / 1e6:.1f} GB/s of {4 * n / 1e6:.2f} MB algorithmic bytes")
    K = 50
    for size in (256, 16384):
        sub, _, n_seq, n_rows = _one_minibatch(b, seq_len, size)
        n_total = 2 * (a.iters + a.warmup) + 4 * K + 8
        probe, _ = _graph_learner(sub, 1, grad_clip=1e30, **FUSED)
        probe.graph_replay(1)
        n0 = float(probe._book.gnorm[0].item())
        ts, bursts = {}, {}
        for label, gc in (("without", None), ("with", n0 / 2.0)):
            lr, _ = _graph_learner(sub, n_total, grad_clip=gc, **FUSED)
            ts[label] = events(lambda: lr.graph_replay(1), a.iters, a.warmup)
            out = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                lr.graph_replay(K)
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / K)
            bursts[label] = out
            if gc is not None:
                used = int(lr._book.cursor.item())
                say(f"    grad_clip = N0 / 2 = {gc:.4e}: mean norm before clipping over {used} steps {float(lr._book.gnorm[:used].mean()):.4e}, last "
                    f"coefficient {lr.optimizer.clip[1].item():.4f}")
            del lr
        say(f"graph step (2 stages + forward + loss + backward + [norm, 2 launches] + Adam + commit), {n_rows} unpadded rows in {n_seq} sequences: "
            f"grad_clip = None {q(ts['without'])}; grad_clip set {q(ts['with'])}; {cost(ts['without'], ts['with'])}")
        say(f"    {K} replays back to back, ms per step, three runs: grad_clip = None {', '.join(f'{x:.4f}' for x in bursts['without'])} | grad_clip set "
            f"{', '.join(f'{x:.4f}' for x in bursts['with'])}")


def step_shuffle(a, say):
    """CommanderLearner(shuffle_sequences=True) against shuffle_sequences=False (the step as it was), both in this run, as a cost: the two
    stage launches alone (contiguous against gathered from the whole batch), the graph step at 256 and 16384 rows, one whole update at
    sgd_minibatch_size = 256, the host time of shuffled_schedule and the order table's bytes."""
    import numpy as np
    import torch
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    med = statistics.median
    FUSED = dict(inputs="fused")
    ro, net, b, seq_len = _policy_batch(a, **FUSED)
    S = len(seq_len)
    say(f"# tools/commander_learner_bench.py --shuffle on {torch.cuda.get_device_name(0)}: CommanderLearner(shuffle_sequences=True) against "
        f"shuffle_sequences=False, both in this run; {a.arenas} arenas, T = {a.T}: {S} sequences, {int(seq_len.sum())} rows; inputs = fused, graph "
        f"step; {a.iters} timed runs after {a.warmup} warm-up (a later run, appended):")

    def cost(t_base, t_new):
        spread = max(max(t_base) - min(t_base), max(t_new) - min(t_new))
        d = med(t_new) - med(t_base)
        word = "no difference beyond the spread" if abs(d) <= spread else ("cost" if d > 0 else "gain")
        return f"off -> on: medians {d * 1e3:+.1f} us apart, larger spread {spread * 1e3:.1f} us: {word}"

    # (a) the two stage launches alone, on the same columns: the first n sequences against n sequences drawn from the whole batch
    groups = [(LR.COMMANDER_STAGE_COLS[:L.STAGE_MAX_COLS], 20), (LR.COMMANDER_STAGE_COLS[L.STAGE_MAX_COLS:], 1)]
    cols = {k: b[k].contiguous() for k in LR.COMMANDER_STAGE_COLS}
    cols["mask"], cols["seq_len"] = cols["mask"].to(torch.uint8), cols["seq_len"].to(torch.int32)
    order = torch.from_numpy(LR.sequence_order(S, 6, 0, 0, 0).astype(np.int32)).to(dev)
    cur, nv = torch.zeros((1,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    for size in (256, 16384):
        n = LR.minibatch_partition(seq_len, size)[0][1]
        staged = {k: torch.zeros((n,) + tuple(c.shape[1:]), dtype=c.dtype, device=dev) for k, c in cols.items()}
        sched = torch.tensor([(0, n, 0, 0)], dtype=torch.int32, device=dev)
        nbytes = 2 * sum(st.numel() * st.element_size() for st in staged.values())

        def plain():
            for ks, chunk_len in groups:
                LR.minibatch_stage([cols[k] for k in ks], [staged[k] for k in ks], chunk_len, sched, cur, nv)

        def gather():
            for ks, chunk_len in groups:
                LR.minibatch_stage_gather([cols[k] for k in ks], [staged[k] for k in ks], chunk_len, order, sched, cur, nv)
        t_p, t_g = events(plain, a.iters, a.warmup), events(gather, a.iters, a.warmup)
        say(f"    the two stage launches alone, ten columns, {n} sequences ({nbytes / 1e6:.2f} MB read + written): hh_minibatch_stage {q(t_p)} = "
            f"{nbytes / med(t_p) / 1e6:.1f} GB/s; hh_minibatch_stage_gather {q(t_g)} = {nbytes / med(t_g) / 1e6:.1f} GB/s; {cost(t_p, t_g)}")
    # (b) the graph step
    K = 50
    for size in (256, 16384):
        sub, _, n_seq, n_rows = _one_minibatch(b, seq_len, size)
        n_total = 2 * (a.iters + a.warmup) + 4 * K + 8
        ts, bursts = {}, {}
        for flag in (False, True):
            lr, _ = _graph_learner(sub, n_total, shuffle_sequences=flag, **FUSED)
            ts[flag] = events(lambda: lr.graph_replay(1), a.iters, a.warmup)
            out = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                lr.graph_replay(K)
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / K)
            bursts[flag] = out
            del lr
        say(f"graph step (2 stages + forward + loss + backward + Adam + commit), {n_rows} unpadded rows in {n_seq} sequences, every pass over this one "
            f"minibatch: shuffle off {q(ts[False])}; on {q(ts[True])}; {cost(ts[False], ts[True])}")
        say(f"    {K} replays back to back, ms per step, three runs: off {', '.join(f'{x:.4f}' for x in bursts[False])} | on "
            f"{', '.join(f'{x:.4f}' for x in bursts[True])}")
    # (c) one whole update, kl_coeff = 0 so that only a changed cap captures again
    res = {}
    for flag in (False, True):
        lr = LR.CommanderLearner.trainable_init(dev, seed=6, num_sgd_iter=a.passes, sgd_minibatch_size=256, kl_coeff=0.0, shuffle_sequences=flag, **GRAPH,
                                                **FUSED)
        times = []
        for _ in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = lr.update(ro.episodes, net)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        res[flag] = (times[a.warmup:], st, lr._book.captures)
    (t_off, st_off, c_off), (t_on, st_on, c_on) = res[False], res[True]
    say(f"one update ({a.passes} pass(es), minibatches of >= 256 rows: {st_off['steps']} steps over {st_off['rows']} rows; shuffled: {st_on['steps']} "
        f"steps in the last one), graph, host clock to a synchronise, {a.iters} updates after {a.warmup}: shuffle off {q(t_off)} ({c_off} capture(s) in all); "
        f"on {q(t_on)} ({c_on} capture(s) in all: a pass whose largest minibatch has another size captures again); {cost(t_off, t_on)}")
    # (d) the host's part and the table
    t_h = []
    for i in range(a.warmup + a.iters):
        t0 = time.perf_counter()
        order_h, sched_h = LR.shuffled_schedule(seq_len, 256, 30, 6, i, 0)
        t_h.append((time.perf_counter() - t0) * 1e3)
    t_s = []
    for i in range(a.warmup + a.iters):
        t0 = time.perf_counter()
        LR.sequence_schedule(seq_len, 256, 30, 6, i, 0)
        t_s.append((time.perf_counter() - t0) * 1e3)
    say(f"    host: shuffled_schedule of 30 passes over {S} sequences ({len(sched_h)} steps) {q(t_h[a.warmup:])}; sequence_schedule (shuffle off) "
        f"{q(t_s[a.warmup:])}; {cost(t_s[a.warmup:], t_h[a.warmup:])}")
    say(f"    order table: 4 x 30 x {S} = {order_h.nbytes} bytes ({order_h.nbytes / 1e6:.2f} MB) for {int(seq_len.sum())} rows")


def tile_lengths(n_seq, L, seed, device):
    """n_seq ragged lengths drawn as `sequences` draws them (nine in ten full), the first one full"""
    import torch
    g = torch.Generator().manual_seed(seed)
    full = torch.rand((n_seq,), generator=g) < 0.9
    n = torch.where(full, torch.full((n_seq,), L), torch.randint(1, L + 1, (n_seq,), generator=g))
    n[0] = L
    return n.to(torch.int32).to(device)


def step_tile(a, say):
    """one tile (HH_GRU_TILE, set by the parent): both GRUs' forward + backward kernels alone at each sequence count, then the graph step"""
    import torch
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    tile = LR.gru_seq_tile(13)
    assert str(tile) == os.environ.get("HH_GRU_TILE"), "the parent sets HH_GRU_TILE"
    if tile == 16:
        say(f"# tools/commander_learner_bench.py --tile on {torch.cuda.get_device_name(0)}: the compiled instances of hh_k_gru_seq_fwd / _bwd, each forced "
            f"through HH_GRU_TILE in a process of its own; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")
    Lm, H = 20, 200
    for S in a.tile_seqs:
        seq_len = tile_lengths(S, Lm, 1, dev)
        g = torch.Generator().manual_seed(2)
        mk = lambda *shape, s=1.0: (s * torch.randn(shape, generator=g)).to(dev)
        parts = [(mk(S, Lm, 3 * H), mk(S, H, s=0.5), mk(3 * H, H, s=H ** -0.5), mk(3 * H, s=0.1)) for _ in range(2)]
        dys = [mk(S, Lm, H) for _ in range(2)]

        def both():
            ys, scratch = LR.gru_seq_forward(parts, seq_len)
            LR.gru_seq_backward(parts, ys, dys, seq_len, scratch)
        t = events(both, a.iters, a.warmup)
        say(f"tile {tile:2d}: hh_gru_seq_forward + hh_gru_seq_backward alone, both GRUs, {S} sequences of <= {Lm} steps ({int(seq_len.sum())} rows, "
            f"{2 * ((S + tile - 1) // tile)} workgroups per launch): {q(t)}")
        print("@tile", tile, f"gru{S}", " ".join(f"{x:.6f}" for x in t), flush=True)
    ro, net, b, seq_len = _policy_batch(a, inputs="fused")
    sub, _, n_seq, n_rows = _one_minibatch(b, seq_len, 256)
    graph, _ = _graph_learner(sub, 2 * (a.iters + a.warmup) + 8, inputs="fused")
    t = events(lambda: graph.graph_replay(1), a.iters, a.warmup)
    say(f"tile {tile:2d}: graph minibatch step (inputs = fused), {n_rows} unpadded rows in {n_seq} sequences (cap {graph._book.cap}): {q(t)}")
    print("@tile", tile, "graph", " ".join(f"{x:.6f}" for x in t), flush=True)


def run_tiles(a, fwd):
    """--tile: one child per compiled tile, then every narrow tile against tile 16 by the spread rule"""
    sys.path.insert(0, ROOT)
    from hhmarl_2d_amd import _lib
    got = {}
    for tile in _lib.GRU_TILES:
        cmd = f"timeout -k 10 300 '{sys.executable}' '{os.path.abspath(__file__)}' --step tile {' '.join(fwd)}"
        p = subprocess.run(cmd, shell=True, env=dict(os.environ, HH_GRU_TILE=str(tile)), stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode:
            return p.returncode         # the first child that fails or runs out of time ends the run
        for line in p.stdout.splitlines():
            if line.startswith("@tile "):
                _, t, key, *xs = line.split()
                got[(int(t), key)] = [float(x) for x in xs]
    with open(a.out, "a") as f:
        for (tile, key), t in sorted(got.items()):
            if tile != 16:
                what = "graph step" if key == "graph" else f"GRUs alone at {key[3:]} sequences"
                s = f"tile {tile:2d} against tile 16, {what}: {verdict(got[(16, key)], t, 'tile 16')}"
                print(s)
                f.write(s + "\n")
    return 0


def step_update(a, say):
    import torch
    from hhmarl_2d_amd import learner as LR
    ro, net = _rollout(a)
    dev = torch.device("cuda", 0)
    for fused in (True, False):
        learner = LR.CommanderLearner.trainable_init(dev, seed=6, fused=fused, num_sgd_iter=a.passes, sgd_minibatch_size=a.minibatch)
        times = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = learner.update(ro.episodes, net)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        say(f"one update at {a.arenas} arenas, T = {a.T} ({a.passes} pass(es), minibatches of >= {a.minibatch} rows: {st['steps']} steps over "
            f"{st['rows']} rows), fused = {fused!s:5}, host clock to a synchronise: first {times[0]:.1f} ms, second {times[1]:.1f} ms")
        say(f"    statistics of the second update: {st}")


def step_window(a, say):
    """CommanderLearner.update_window on a CommanderRollout's [T, N] window (batch_mode = "truncate_episodes") next to update on whole
    episodes, both in this process: the batch build (kernels against torch twins), one whole update each, the graph captures over three windows"""
    import torch
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    med = statistics.median
    dev = torch.device("cuda", 0)

    def cost(t_base, t_new, words=("twin -> kernel", "loss", "gain")):
        spread = max(max(t_base) - min(t_base), max(t_new) - min(t_new))
        d = med(t_new) - med(t_base)
        word = "no difference beyond the spread" if abs(d) <= spread else (words[1] if d > 0 else words[2])
        return f"{words[0]}: medians {d * 1e3:+.1f} us apart, larger spread {spread * 1e3:.1f} us: {word}"

    def host(fn):
        out = []
        for _ in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out[a.warmup:]

    N, T, Lm = a.arenas, a.T, 20
    ro_e, net = _rollout(a)                                    # whole episodes, as every other section of this file
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, auto_reset=True, horizon=a.horizon), device=0)
    ro = CommanderRollout(w, net, VariantNetPilot(w, seed=8), T)
    for _ in range(max(3, a.horizon // (12 * T) + 2)):
        ro.collect()
    torch.cuda.synchronize()
    say(f"# tools/commander_learner_bench.py --window on {torch.cuda.get_device_name(0)}: CommanderLearner.update_window on a CommanderRollout's [T, N] "
        f"window (batch_mode = truncate_episodes) next to update on whole episodes, both in this run; {N} arenas, T = {T}, horizon {a.horizon}; {a.iters} "
        f"timed runs after {a.warmup} warm-up, medians, (max - min) spread rule (a later run, appended):")
    ln = LR.CommanderLearner.trainable_init(dev, seed=6, num_sgd_iter=a.passes, sgd_minibatch_size=a.minibatch)
    with torch.no_grad():
        t_cut, t_cut_t = host(lambda: LR.window_cut(ro.done, Lm)), host(lambda: LR.window_cut_torch(ro.done, Lm))
        tables = LR.window_cut(ro.done, Lm)
        S = tables[0].numel()
        names = ["obs", "actions", "logp", "vf", "adv", "target", "state_in"]
        cols = [(getattr(ro, k), tuple(getattr(ro, k).shape[2:]), 0, k == "state_in") for k in names]
        outs = LR.window_gather(cols, tables, Lm)
        t_g = events(lambda: LR.window_gather(cols, tables, Lm, out=outs), a.iters, a.warmup)
        t_g_t = events(lambda: LR.window_gather_torch(cols, tables, Lm), a.iters, a.warmup)
        wrote = sum(o.numel() * o.element_size() for o in outs)
        read = sum((S if per_seq else T * N) * (src[0, 0].numel() * src.element_size()) for src, _, _, per_seq in cols) + 12 * S
        t_ws = host(lambda: ln.window_sequences(ro))
        t_es = host(lambda: ro_e.episodes.sequences())
        seqs_w, seqs_e = ln.window_sequences(ro), ro_e.episodes.sequences()
        t_pb_w, t_pb_e = host(lambda: ln.policy_batch(seqs_w)), host(lambda: ln.policy_batch(seqs_e))
    say(f"the window has {T * N} arena rows in {S} sequences of <= {Lm}; the episode batch of the last collect {int(seqs_e['seq_lens'].sum())} arena rows in "
        f"{seqs_e['obs'].shape[0]} sequences")
    say(f"    the cut (three launches + the read of n_seq, host clock): window_cut {q(t_cut)}; window_cut_torch {q(t_cut_t)}; {cost(t_cut_t, t_cut)}")
    say(f"    the gather of seven columns, state_in per sequence (ONE launch, device events): hh_window_gather {q(t_g)} = {(read + wrote) / med(t_g) / 1e6:.1f} GB/s of "
        f"{read / 1e6:.1f} MB read + {wrote / 1e6:.1f} MB written = {100 * (read + wrote) / med(t_g) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches; "
        f"window_gather_torch {q(t_g_t)}; {cost(t_g_t, t_g)}")
    say(f"    the padded sequences (host clock to a synchronise): window_sequences {q(t_ws)}; CommanderEpisodeBatch.sequences() on the episode batch {q(t_es)}")
    say(f"    policy_batch (critic rows, agent-major concatenation, masked standardisation; torch ops in both paths): on the window's sequences {q(t_pb_w)}; on the "
        f"episode batch's {q(t_pb_e)}")
    del outs, seqs_w, seqs_e
    ln_e = LR.CommanderLearner.trainable_init(dev, seed=6, num_sgd_iter=a.passes, sgd_minibatch_size=a.minibatch)
    t_w, t_u = host(lambda: ln.update_window(ro)), host(lambda: ln_e.update(ro_e.episodes, net))
    st_w, st_u = ln.update_window(ro), ln_e.update(ro_e.episodes, net)
    say(f"    one update ({a.passes} pass(es), minibatches of >= {a.minibatch} rows, eager, old logits from the module, host clock to a synchronise): update_window "
        f"{q(t_w)} ({st_w['steps']} steps over {st_w['rows']} rows); update {q(t_u)} ({st_u['steps']} steps over {st_u['rows']} rows); "
        f"{cost(t_u, t_w, ('update -> update_window', 'slower', 'faster'))} (the row counts differ: per row {1e3 * med(t_w) / st_w['rows']:.3f} us against "
        f"{1e3 * med(t_u) / max(st_u['rows'], 1):.3f} us)")
    del ln, ln_e, ro_e
    lg = LR.CommanderLearner.trainable_init(dev, seed=6, num_sgd_iter=a.passes, sgd_minibatch_size=1024, kl_coeff=0.0, inputs="fused", optimizer="fused", step="graph")
    caps, steps, t3 = [], [], []
    for _ in range(3):
        ro.collect()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = lg.update_window(ro)
        lg.publish(net)
        torch.cuda.synchronize()
        t3.append((time.perf_counter() - t0) * 1e3)
        caps.append(lg._book.captures)
        steps.append(st["steps"])
    say(f"    step=\"graph\", kl_coeff = 0, inputs = fused, minibatches of >= 1024 rows, three windows (collect, update_window, publish; no start()): captures after each "
        f"window {caps}, steps {steps}, update_window + publish {', '.join(f'{x:.1f}' for x in t3)} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=8192)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commander_learner.log"))
    ap.add_argument("--inputs", action="store_true", help="only the inputs=\"fused\" against inputs=\"torch\" minibatch step; appended to --out")
    ap.add_argument("--trunk", action="store_true", help="only the trunk=\"fused\" against trunk=\"torch\" section; appended to --out")
    ap.add_argument("--graph", action="store_true", help="only the step=\"graph\" against the eager step section; appended to --out")
    ap.add_argument("--clip", action="store_true", help="only the grad_clip against grad_clip = None section; appended to --out")
    ap.add_argument("--shuffle", action="store_true", help="only the shuffle_sequences against shuffle_sequences = False section; appended to --out")
    ap.add_argument("--tile", action="store_true", help="only the GRU tile instances, each through HH_GRU_TILE in a child; appended to --out")
    ap.add_argument("--tile-seqs", default="13,26,52,104,208,416,854", help="the sequence counts of --tile's GRUs-alone timing")
    ap.add_argument("--heads", action="store_true", help="only the heads=\"fused\" against heads=\"torch\" section; appended to --out")
    ap.add_argument("--window", action="store_true", help="only the update_window against update section; appended to --out")
    ap.add_argument("--heads-mode", choices=["torch", "fused"], default="torch", help="with --launches: the learner's heads option")
    ap.add_argument("--launches", choices=["eager", "graph"], help="with --step graph: only --launch-count steps of this form (for a kernel trace)")
    ap.add_argument("--launch-count", type=int, default=20)
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["inputs", "trunk", "graph", "tile", "clip", "shuffle", "heads", "window"], help="run one step in this process (what the parent starts)")
    a = ap.parse_args()
    a.tile_seqs = [int(x) for x in a.tile_seqs.split(",")]
    if a.step:
        sys.path.insert(0, ROOT)
        import torch

        def say(s):
            print(s, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(s + "\n")
        if a.step == "gru":
            say(f"# tools/commander_learner_bench.py on {torch.cuda.get_device_name(0)}: {a.iters} timed iterations after {a.warmup} warm-up, device events")
        {"gru": step_gru, "step": step_step, "update": step_update, "inputs": step_inputs, "trunk": step_trunk, "graph": step_graph,
         "tile": step_tile, "clip": step_clip, "shuffle": step_shuffle, "heads": step_heads, "window": step_window}[a.step](a, say)
        return
    fwd = [f"--{k} {getattr(a, k)}" for k in ("arenas", "T", "horizon", "iters", "warmup", "passes", "minibatch")] + [f"--out '{a.out}'"]
    if a.window:
        sys.exit(subprocess.call(f"timeout -k 10 480 '{sys.executable}' '{os.path.abspath(__file__)}' --step window {' '.join(fwd)}", shell=True))
    if a.heads:
        sys.exit(subprocess.call(f"timeout -k 10 480 '{sys.executable}' '{os.path.abspath(__file__)}' --step heads {' '.join(fwd)}", shell=True))
    if a.graph:
        sys.exit(subprocess.call(f"timeout -k 10 480 '{sys.executable}' '{os.path.abspath(__file__)}' --step graph {' '.join(fwd)}", shell=True))
    if a.clip:
        sys.exit(subprocess.call(f"timeout -k 10 300 '{sys.executable}' '{os.path.abspath(__file__)}' --step clip {' '.join(fwd)}", shell=True))
    if a.shuffle:
        sys.exit(subprocess.call(f"timeout -k 10 480 '{sys.executable}' '{os.path.abspath(__file__)}' --step shuffle {' '.join(fwd)}", shell=True))
    if a.tile:
        fwd.append("--tile-seqs " + ",".join(str(s) for s in a.tile_seqs))
        sys.exit(run_tiles(a, fwd))
    if a.inputs:
        sys.exit(subprocess.call(f"timeout -k 10 300 '{sys.executable}' '{os.path.abspath(__file__)}' --step inputs {' '.join(fwd)}", shell=True))
    if a.trunk:
        sys.exit(subprocess.call(f"timeout -k 10 300 '{sys.executable}' '{os.path.abspath(__file__)}' --step trunk {' '.join(fwd)}", shell=True))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    cmd = " && ".join(f"timeout -k 10 {limit} '{sys.executable}' '{os.path.abspath(__file__)}' --step {s} {' '.join(fwd)}" for s, limit in STEPS)
    sys.exit(subprocess.call(cmd, shell=True))


if __name__ == "__main__":
    main()
