"""Where the time of a PPO update goes on the MI355X (16384 arenas, T = 64, level-3 fight by default), and how exact the loss kernel is:
  errors  hh_ppo_loss and the float32 torch restatement against the float64 one (tests/ppo_loss_ref.py), on the GPU test's inputs
  loss    hh_ppo_loss alone against the torch-op loss alone (forward + backward to logits / vf) on the same tensors, device events;
          the kernel's achieved GB/s against its algorithmic bytes (ld + 32 logits in, ld out, 25 B of row scalars in, 4 B out)
  step    one minibatch step (forward, loss, backward, Adam) with fused = True and fused = False at 256 and at 65536 rows
  update  one collect next to one whole update.  The update is timed with num_sgd_iter = 1 and sgd_minibatch_size = 65536 by default
          (--passes / --minibatch): RLlib's 30 passes of 256-row minibatches over a million rows are a quarter of a million optimizer
          steps, the per-step figure above times the number of steps
  old     the old_logits pass of an update (ceil(R / N) greedy bank calls over the whole batch), which a batch that carries the sampler's
          logits (PPORollout(record_logits=True)) saves: PPOLearner.batch_old_logits then returns the column.  --old-logits-only runs this
          section alone and appends its lines to --out.  The section builds two worlds and two complete_episodes rollouts of its own,
          one of them with the logits column: at the default N = 16384, T = 64, H = 300 about 2.8 GB (rows and carry without the
          column) + 5.8 GB (with it: 2.8 GB of that the column's carry and batch, 0.27 GB its collect buffer), on top of the full
          run's own rollout when it runs at its end
  attention  --attention runs this section alone and appends its lines to --out: the fight networks' chunk attention through
          TrainableNet(attention="fused") (hh_chunk_attn_*, hh_residual_normalize_*) against the default nn.MultiheadAttention +
          F.normalize path, both timed in the same run: (a) one attention block, forward + backward, E = 100 and 150 at 14 and 3560
          chunks of 20; (b) the Fight1 minibatch step at 256 and 65536 rows; (c) the four kernels alone as bytes/s of their algorithmic
          bytes (core: 16 E per row forward, 28 E backward; normalize: 12 E + 4 each way).  A difference is called a gain (or a loss)
          only where the medians differ by more than the larger of the two (max - min) spreads
  inputs  --inputs runs this section alone and appends its lines to --out: everything in front of shared_layer through
          TrainableNet(inputs="fused") (hh_input_stage_*) against the default slices + cat + nn.Linear + tanh + cat, both timed in the
          same run: (a) each Fight1 stage (actor, critic), forward + backward, at 14 and 3560 chunks of 20; (b) the stage kernels
          alone as bytes/s of their algorithmic bytes (forward: the source row in, the activations out; backward: the source row, y
          and d_y in); (c) the Fight1 minibatch step with attention="fused" at 256 and 65536 rows.  The same rule for gain / loss
  trunk   --trunk runs this section alone and appends its lines to --out: shared_layer, its bias and tanh over the actor's and the critic's
          rows through TrainableNet(trunk="fused") (hh_dense_tanh_*, split-fp16 MFMA) against the default two float32 GEMMs + tanh, both
          timed in the same run: (a) the layer alone on both sides' rows, forward + backward, at 14 and 3560 chunks of 20; (b) the two
          kernel calls alone as useful TFLOP/s (2 R K N per product: one forward, two backward), against the 155 TF float32 matrix
          rate and against 2.5 PF / 3 (three fp16 products per float32 one); (c) the Fight1 minibatch step with attention="fused",
          inputs="fused" at 256 and 65536 rows.  The same rule for gain / loss
  step    --step runs this section alone and appends its lines to --out: the minibatch step as PPOLearner(optimizer="fused",
          step="graph") replays it from one HIP graph (hh_minibatch_stage, hh_adam_step, hh_train_commit) against the eager step, all in
          the same run: (a) hh_adam_step on a Fight1 module's tensors and on one 64 Mi-element tensor, hh_minibatch_stage on a Fight1 batch
          at 14 and 3560 chunks, as bytes/s of their algorithmic bytes (Adam: 16 B in, 12 B out per element; stage: every staged byte
          read and written once); (b) the Fight1 minibatch step with attention="fused", inputs="fused", trunk="torch" at 256 and 65536
          rows in three configurations — eager + torch.optim.Adam, eager + the device Adam, graph — one step per timing and 50 steps
          back to back, and what a capture costs; (c) one whole update at --step-minibatch (default 256) rows and --passes passes, eager
          against graph.  The same rule for gain / loss.  --step-launches eager|graph (with --step-count K) only runs K steps of that
          kind at 256 rows, for a kernel count under rocprofv3 --kernel-trace --stats in a run of its own (two values of K: the
          difference is the steps' share)
  clip    --clip runs this section alone and appends its lines to --out: gradient clipping by global norm (PPOLearner(grad_clip=...):
          hh_grad_norm, hh_adam_step_clipped) as a COST next to the grad_clip = None path of the same run: (a) hh_grad_norm on a Fight1
          module's tensors and on one 64 Mi-element tensor as bytes/s of the 4 B per element it reads, hh_adam_step_clipped against
          hh_adam_step at 64 Mi elements (the same 28 B per element); (b) the Fight1 graph step with attention="fused", inputs="fused"
          at 256 and 65536 rows with and without grad_clip (a threshold that binds), one replay per timing and 50 back to back.  A step
          with grad_clip has two launches more: the norm's partials and its final.  The same rule for gain / loss
  shuffle --shuffle runs this section alone and appends its lines to --out: PPOLearner(shuffle_sequences=True) as a COST next to
          shuffle_sequences=False in the same run: (a) the stage launch alone, hh_minibatch_stage on the first n chunks against
          hh_minibatch_stage_gather on n chunks drawn from the whole batch, the 8 Fight1 columns at 14 and 3560 chunks of 20 and 8 Esc1
          columns at 271 and 65544 rows; (b) the Fight1 graph step at 256 and 65536 rows, one replay per timing and 50 back to back;
          (c) one whole graph update at --step-minibatch (medians of --iters updates, kl_coeff = 0); (d) the host time of
          shuffled_schedule against sequence_schedule for 30 passes, and the order table's bytes.  The same spread rule, worded cost /
          gain / no difference
  heads   --heads runs this section alone and appends its lines to --out: PPOLearner(heads="fused") (hh_heads_loss: tanh, act_out, val_out,
          the loss and their backward as one row pass) against heads="torch" in the same run, attention="fused", inputs="fused" where they
          apply: (a) hh_heads_loss alone at 280 and 71200 rows as bytes/s of its algorithmic bytes (8 KB per row: za, zc in, d_za, d_zc
          out; plus the head weights in and their gradients out); (b) the Fight1 and the Esc1 minibatch step at 256 and 65536 rows, eager
          + torch Adam and the graph step, one step per timing and 50 replays back to back; (c) one whole graph update at
          --step-minibatch.  The same rule for gain / loss.  --step-launches with --heads-mode fused counts the launches of that path
  block   --attention-block runs this section alone and appends its lines to --out: TrainableNet(attention="block") (hh_attn_block_*: a whole
          attention block, projections included, as one launch forward and two backward) against attention="fused" in the same run:
          (a) one block, forward + backward, E = 100 and 150 at 14 and 3560 chunks of 20; (b) the two calls alone as bytes/s of their
          algorithmic bytes (forward: x in, y, qkv, ctx and the norm out, 24 E + 4 per row; backward: x, y, d_y, qkv, ctx and the norm in,
          d_x out, 32 E + 4 per row; the weights once each way); (c) the Fight1 graph step with inputs="fused", heads="fused" at 256 and
          65536 rows, one replay per timing and 50 back to back at 256.  The same rule for gain / loss.  --step-launches graph with
          --attention-mode block (and --heads-mode fused) counts the launches of that step under rocprofv3
--window: PPOLearner.update_window on a PPORollout's fixed [T, N] window (batch_mode = "truncate_episodes") next to update on whole
          episodes, fight and escape, in the same run: (a) the batch build — window_cut and hh_window_gather against their torch twins (the
          gather as bytes/s of what it reads and writes), the torch parts (critic rows, standardisation), window_batch against policy_batch
          on the episode batch of the last collect; (b) one whole update each; (c) the graph captures over three windows with kl_coeff = 0
--shards: PPOLearner(group=LocalShards(1)) (learner/shards.py) as a COST next to group=None in the same run: (a) hh_grad_pack and
          hh_grad_combine alone on a Fight1 module's tensors and on one 64 Mi-element tensor, as bytes/s of their algorithmic bytes (pack:
          4 B in, 4 B out per element; combine: 4 W B in, 4 B out); (b) the Fight1 eager minibatch step through the driver at 256 and
          65536 rows, run against run_sharded.  The same spread rule.  What W ranks gain on real hardware is unmeasured
The network GEMMs are PyTorch / rocBLAS in both modes; only the loss differs.
    python tools/ppo_learner_bench.py [--arenas 16384] [--T 64] [--iters 20] [--out profiles/ppo_learner.log]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ppo_loss_ref as REF  # noqa: E402
from hhmarl_2d_amd import learner as LR  # noqa: E402
from hhmarl_2d_amd.pilots import PolicyBank  # noqa: E402
from hhmarl_2d_amd.rollout import PPORollout  # noqa: E402
from hhmarl_2d_amd.world import World, make_config  # noqa: E402

KW = dict(clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=16384)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=300)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--minibatch", type=int, default=65536)
    ap.add_argument("--old-logits-only", action="store_true", help="only the old_logits section; its lines are appended to --out")
    ap.add_argument("--attention", action="store_true", help="only the chunk-attention section; its lines are appended to --out")
    ap.add_argument("--inputs", action="store_true", help="only the input-stage section; its lines are appended to --out")
    ap.add_argument("--trunk", action="store_true", help="only the shared-layer section; its lines are appended to --out")
    ap.add_argument("--step", action="store_true", help="only the graph-step section; its lines are appended to --out")
    ap.add_argument("--clip", action="store_true", help="only the gradient-clipping section; its lines are appended to --out")
    ap.add_argument("--shuffle", action="store_true", help="only the shuffle_sequences section; its lines are appended to --out")
    ap.add_argument("--heads", action="store_true", help="only the fused-tail section; its lines are appended to --out")
    ap.add_argument("--window", action="store_true", help="only the window-batch section (update_window); its lines are appended to --out")
    ap.add_argument("--shards", action="store_true", help="only the sharded-update section (group=LocalShards(1)); its lines are appended to --out")
    ap.add_argument("--attention-block", action="store_true", help="only the attention-block section (attention=\"block\" against \"fused\"); its lines are appended to --out")
    ap.add_argument("--heads-mode", choices=("torch", "fused"), default="torch", help="--step-launches: the learner's heads option")
    ap.add_argument("--attention-mode", choices=("fused", "block"), default="fused", help="--step-launches: the learner's attention option")
    ap.add_argument("--step-minibatch", type=int, default=256, help="--step: sgd_minibatch_size of the whole update")
    ap.add_argument("--step-launches", choices=("eager", "graph"), help="only --step-count minibatch steps of this kind (for a kernel count under rocprofv3)")
    ap.add_argument("--step-count", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_learner.log"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def events(fn, iters=a.iters):
        for _ in range(a.warmup):
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

    q = lambda v: f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"
    say(f"# tools/ppo_learner_bench.py on {torch.cuda.get_device_name(0)}: {a.arenas} arenas, T = {a.T}, level 3 fight; {a.iters} timed "
        f"iterations after {a.warmup} warm-up, device events")

    def old_logits_section():
        """the per-update pass that a recorded logits column saves, and what recording costs a collect"""
        w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
        ros = {rec: PPORollout(w if not rec else World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0),
                               bank, a.T, batch_mode="complete_episodes", record_logits=rec) for rec in (False, True)}
        for ro in ros.values():
            for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
                ro.collect()
        t_c = {rec: events(ro.collect, iters=5) for rec, ro in ros.items()}
        learner = LR.PPOLearner.trainable_init(dev, mode="fight", seed=1)
        rows, rows_l = ros[False].episodes.rows(), ros[True].episodes.rows()
        R, N = rows["obs"].shape[0], a.arenas
        with torch.no_grad():
            t_old = events(lambda: learner.batch_old_logits(rows, bank, N), iters=5)
            t_col = events(lambda: learner.batch_old_logits(rows_l, None), iters=5)
        say(f"old_logits of one update's batch ({R} rows): recomputed from the bank in {(R + N - 1) // N} greedy calls of [{N}, 2] rows: {q(t_old)}; "
            f"taken from the batch's logits column (record_logits=True, {rows_l['obs'].shape[0]} rows): {q(t_col)}")
        say(f"    collect with record_logits=False: {q(t_c[False])}; with record_logits=True (sampler writes 256 B per row, emission moves them): {q(t_c[True])}")

    if a.old_logits_only:
        old_logits_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines[1:]) + "\n")
        return

    def attention_section():
        """attention="fused" against attention="torch": one block, the minibatch step, the kernels alone"""
        import ctypes as C
        from hhmarl_2d_amd import _lib as L
        from hhmarl_2d_amd import policy_nets as PN
        med = statistics.median

        def verdict(t_torch, t_fused):
            spread = max(max(t_torch) - min(t_torch), max(t_fused) - min(t_fused))
            d = med(t_torch) - med(t_fused)
            word = "no difference beyond the spread" if abs(d) <= spread else ("gain" if d > 0 else "loss")
            return f"torch / fused = {med(t_torch) / med(t_fused):.2f}x, medians {d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}"

        say(f"# tools/ppo_learner_bench.py --attention on {torch.cuda.get_device_name(0)}: TrainableNet(attention=\"fused\") against the default "
            f"attention=\"torch\", both in this run; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")
        # (a) one block: in-projection, core, out-projection, residual + normalize; forward + backward
        for E in (100, 150):
            att = nn.MultiheadAttention(E, 2, batch_first=True).to(dev)
            for S in (14, 3560):
                g = torch.Generator().manual_seed(E + S)
                h = torch.tanh(torch.randn((S, 20, E), generator=g)).to(dev).requires_grad_(True)
                dy = torch.randn((S, 20, E), generator=g).to(dev)

                def block(fused):
                    h.grad = None
                    att.zero_grad(set_to_none=True)
                    if fused:
                        y = LR.TrainableNet._attend_fused(att, h)
                    else:
                        o, _ = att(h, h, h, need_weights=False)
                        y = F.normalize(h + o, dim=-1)
                    y.backward(dy)
                t_t, t_f = events(lambda: block(False)), events(lambda: block(True))
                say(f"attention block (in-projection, core, out-projection, normalize(x + att); forward + backward), E = {E}, {S} chunks of 20: "
                    f"torch {q(t_t)}; fused {q(t_f)}; {verdict(t_t, t_f)}")
        # (c) the kernels alone
        lib = L.lib()
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())
        for E in (100, 150):
            for S in (14, 3560):
                R = S * 20
                qkv, d_ctx = torch.randn((S, 20, 3 * E), device=dev), torch.randn((S, 20, E), device=dev)
                ctx, d_qkv = torch.empty_like(d_ctx), torch.empty_like(qkv)
                x, av = torch.randn((R, E), device=dev), torch.randn((R, E), device=dev)
                y, d_s, norm = torch.empty_like(x), torch.empty_like(x), torch.empty((R,), device=dev)
                runs = (("hh_chunk_attn_forward", 16 * E * R, lambda: L.check(lib.hh_chunk_attn_forward(S, 20, E, p(qkv), p(ctx), st))),
                        ("hh_chunk_attn_backward", 28 * E * R, lambda: L.check(lib.hh_chunk_attn_backward(S, 20, E, p(qkv), p(d_ctx), p(d_qkv), st))),
                        ("hh_residual_normalize_forward", (12 * E + 4) * R, lambda: L.check(lib.hh_residual_normalize_forward(R, E, p(x), p(av), p(y), p(norm), st))),
                        ("hh_residual_normalize_backward", (12 * E + 4) * R, lambda: L.check(lib.hh_residual_normalize_backward(R, E, p(y), p(norm), p(d_ctx), p(d_s), st))))
                for name, nbytes, fn in runs:
                    t = events(fn)
                    say(f"    {name} alone, E = {E}, {S} chunks of 20 ({R} rows): {q(t)} = {nbytes / med(t) / 1e6:.1f} GB/s of {nbytes / 1e6:.2f} MB "
                        f"algorithmic bytes ({100 * nbytes / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")
        # (b) the Fight1 minibatch step
        w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
        ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
        for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
            ro.collect()
        rows = ro.episodes.rows()
        learners = {att: LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, attention=att) for att in ("torch", "fused")}
        with torch.no_grad():
            old = learners["torch"].old_logits(rows["obs"], bank, ro.episodes.N)
            b = learners["torch"].policy_batch(rows, old, 0)
        seq_len = b["seq_len"].cpu().numpy()
        for size in (256, 65536):
            s0, s1 = LR.minibatch_partition(seq_len, size)[0]
            mb = {k: v[s0:s1] for k, v in b.items() if k != "seq_len"}
            mb["n_valid"] = torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device=dev)
            t = {att: events(lambda: lr.minibatch_step(0, mb)) for att, lr in learners.items()}
            say(f"minibatch step ({PN.KIND_NAMES[learners['torch'].kinds[0]]}, forward + loss + backward + Adam, fused loss), {int(seq_len[s0:s1].sum())} unpadded rows in "
                f"{s1 - s0} chunks of 20: attention = torch {q(t['torch'])}; attention = fused {q(t['fused'])}; {verdict(t['torch'], t['fused'])}")

    if a.attention:
        lines.clear()
        attention_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    def inputs_section():
        """inputs="fused" against inputs="torch": each Fight1 stage, the stage kernels alone, the minibatch step"""
        import ctypes as C
        from hhmarl_2d_amd import _lib as L
        from hhmarl_2d_amd import policy_nets as PN
        med = statistics.median

        def verdict(t_torch, t_fused):
            spread = max(max(t_torch) - min(t_torch), max(t_fused) - min(t_fused))
            d = med(t_torch) - med(t_fused)
            word = "no difference beyond the spread" if abs(d) <= spread else ("gain" if d > 0 else "loss")
            return f"torch / fused = {med(t_torch) / med(t_fused):.2f}x, medians {d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}"

        say(f"# tools/ppo_learner_bench.py --inputs on {torch.cuda.get_device_name(0)}: TrainableNet(inputs=\"fused\") against the default "
            f"inputs=\"torch\", both in this run; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")
        kind = PN.FIGHT1
        net = LR.TrainableNet(kind).to(dev)
        tables, layers = LR.stage_tables(kind), LR.stage_layers(kind)
        lib = L.lib()
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for side, width in (("actor", PN.OBS_DIM[kind]), ("critic", sum(PN.CRITIC_DIMS[kind]))):
            groups, packs = LR.stage_groups(net, layers[side], tables[side])
            for S in (14, 3560):
                R = S * 20
                g = torch.Generator().manual_seed(S + width)
                src = torch.rand((S, 20, width), generator=g).to(dev)
                d_out = [torch.randn((S, 20, sum(groups[i][0].shape[0] for i in p)), generator=g).to(dev) for p in packs]

                def stage(fn):
                    net.zero_grad(set_to_none=True)
                    torch.autograd.backward(fn(src, groups, packs), d_out)
                t_t, t_f = events(lambda: stage(LR.input_stage_torch)), events(lambda: stage(LR.input_stage))
                say(f"input stage (Fight1 {side}: {' '.join(layers[side])} -> {[d.shape[-1] for d in d_out]}; forward + backward), {S} chunks of 20: "
                    f"torch {q(t_t)}; fused {q(t_f)}; {verdict(t_t, t_f)}")
                # the kernels alone, on buffers of their own
                n = len(groups)
                io = (L.HHInputGroup * n)()
                outs = [torch.empty_like(d) for d in d_out]
                d_ws, d_bs = [torch.empty_like(w) for w, _, _ in groups], [torch.empty_like(b) for _, b, _ in groups]
                for pi, pk in enumerate(packs):
                    col = 0
                    for i in pk:
                        w_, b_, segs = groups[i]
                        io[i].n_out, io[i].n_seg = w_.shape[0], len(segs)
                        for k, (c0, ln) in enumerate(segs):
                            io[i].seg_col[k], io[i].seg_len[k] = c0, ln
                        io[i].w, io[i].b = w_.data_ptr(), b_.data_ptr()
                        io[i].y, io[i].y_ld = outs[pi].data_ptr() + 4 * col, outs[pi].shape[-1]
                        io[i].d_y, io[i].d_y_ld = d_out[pi].data_ptr() + 4 * col, d_out[pi].shape[-1]
                        io[i].d_w, io[i].d_b = d_ws[i].data_ptr(), d_bs[i].data_ptr()
                        col += w_.shape[0]
                nb = C.c_int64()
                L.check(lib.hh_input_stage_scratch_bytes(n, io, R, C.byref(nb)))
                scratch = torch.empty((nb.value // 4,), device=dev)
                p = lambda t: C.c_void_p(t.data_ptr())
                n_out = sum(w_.shape[0] for w_, _, _ in groups)
                runs = (("hh_input_stage_forward", 4 * R * (width + n_out), lambda: L.check(lib.hh_input_stage_forward(R, p(src), width, width, n, io, st))),
                        ("hh_input_stage_backward", 4 * R * (width + 2 * n_out),
                         lambda: L.check(lib.hh_input_stage_backward(R, p(src), width, width, n, io, p(scratch), nb.value, st))))
                for name, nbytes, fn in runs:
                    t = events(fn)
                    say(f"    {name} alone, Fight1 {side}, {S} chunks of 20 ({R} rows): {q(t)} = {nbytes / med(t) / 1e6:.1f} GB/s of {nbytes / 1e6:.2f} MB "
                        f"algorithmic bytes ({100 * nbytes / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")
        # the Fight1 minibatch step, attention = "fused" in both
        w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
        ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
        for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
            ro.collect()
        rows = ro.episodes.rows()
        learners = {inp: LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, attention="fused", inputs=inp) for inp in ("torch", "fused")}
        with torch.no_grad():
            old = learners["torch"].old_logits(rows["obs"], bank, ro.episodes.N)
            b = learners["torch"].policy_batch(rows, old, 0)
        seq_len = b["seq_len"].cpu().numpy()
        for size in (256, 65536):
            s0, s1 = LR.minibatch_partition(seq_len, size)[0]
            mb = {k: v[s0:s1] for k, v in b.items() if k != "seq_len"}
            mb["n_valid"] = torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device=dev)
            t = {inp: events(lambda: lr.minibatch_step(0, mb)) for inp, lr in learners.items()}
            say(f"minibatch step ({PN.KIND_NAMES[learners['torch'].kinds[0]]}, forward + loss + backward + Adam, fused loss, attention = fused), "
                f"{int(seq_len[s0:s1].sum())} unpadded rows in {s1 - s0} chunks of 20: inputs = torch {q(t['torch'])}; inputs = fused {q(t['fused'])}; "
                f"{verdict(t['torch'], t['fused'])}")

    if a.inputs:
        lines.clear()
        inputs_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    def trunk_section():
        """trunk="fused" against trunk="torch": the layer alone, the two kernel calls alone, the minibatch step"""
        import ctypes as C
        from hhmarl_2d_amd import _lib as L
        from hhmarl_2d_amd import policy_nets as PN
        med = statistics.median

        def verdict(t_torch, t_fused):
            spread = max(max(t_torch) - min(t_torch), max(t_fused) - min(t_fused))
            d = med(t_torch) - med(t_fused)
            word = "no difference beyond the spread" if abs(d) <= spread else ("gain" if d > 0 else "loss")
            return f"torch / fused = {med(t_torch) / med(t_fused):.2f}x, medians {d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}"

        say(f"# tools/ppo_learner_bench.py --trunk on {torch.cuda.get_device_name(0)}: TrainableNet(trunk=\"fused\") against the default "
            f"trunk=\"torch\", both in this run; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")
        lin = nn.Linear(500, 500).to(dev)
        lib = L.lib()
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())
        for S in (14, 3560):
            R = S * 20
            g = torch.Generator().manual_seed(S)
            xs = [torch.tanh(torch.randn((S, 20, 500), generator=g)).to(dev).requires_grad_(True) for _ in range(2)]
            dys = [(torch.randn((S, 20, 500), generator=g) / R).to(dev) for _ in range(2)]

            def layer(fn):
                lin.zero_grad(set_to_none=True)
                for x in xs:
                    x.grad = None
                torch.autograd.backward(fn(xs, lin.weight, lin.bias), dys)
            t_t, t_f = events(lambda: layer(LR.dense_tanh_torch)), events(lambda: layer(LR.dense_tanh))
            say(f"shared layer (tanh(x W^T + b), 500 -> 500, the actor's and the critic's rows; forward + backward), 2 x {S} chunks of 20: "
                f"torch {q(t_t)}; fused {q(t_f)}; {verdict(t_t, t_f)}")
            # the kernel calls alone, on buffers of their own
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
                t = events(fn)
                tf = products * flop / med(t) / 1e9
                say(f"    {name} alone, 2 x {R} rows: {q(t)} = {tf:.1f} useful TFLOP/s ({products} product(s) of 2 R K N = {flop / 1e9:.2f} GFLOP): "
                    f"{100 * tf / 155:.1f} % of the 155 TF float32 matrix rate, {100 * tf / (2500 / 3):.1f} % of 2.5 PF / 3")
        # the Fight1 minibatch step, attention = "fused" and inputs = "fused" in both
        w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
        ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
        for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
            ro.collect()
        rows = ro.episodes.rows()
        learners = {tr: LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, attention="fused", inputs="fused", trunk=tr) for tr in ("torch", "fused")}
        with torch.no_grad():
            old = learners["torch"].old_logits(rows["obs"], bank, ro.episodes.N)
            b = learners["torch"].policy_batch(rows, old, 0)
        seq_len = b["seq_len"].cpu().numpy()
        for size in (256, 65536):
            s0, s1 = LR.minibatch_partition(seq_len, size)[0]
            mb = {k: v[s0:s1] for k, v in b.items() if k != "seq_len"}
            mb["n_valid"] = torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device=dev)
            t = {tr: events(lambda: lr.minibatch_step(0, mb)) for tr, lr in learners.items()}
            say(f"minibatch step ({PN.KIND_NAMES[learners['torch'].kinds[0]]}, forward + loss + backward + Adam, fused loss, attention = fused, inputs = fused), "
                f"{int(seq_len[s0:s1].sum())} unpadded rows in {s1 - s0} chunks of 20: trunk = torch {q(t['torch'])}; trunk = fused {q(t['fused'])}; "
                f"{verdict(t['torch'], t['fused'])}")

    if a.trunk:
        lines.clear()
        trunk_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    def step_section():
        """step="graph" and optimizer="fused" against the eager step with torch.optim.Adam: the two kernels alone, the minibatch step, one update"""
        from hhmarl_2d_amd import policy_nets as PN
        med = statistics.median

        def verdict(t_base, t_new):
            spread = max(max(t_base) - min(t_base), max(t_new) - min(t_new))
            d = med(t_base) - med(t_new)
            word = "no difference beyond the spread" if abs(d) <= spread else ("gain" if d > 0 else "loss")
            return f"eager+torch / this = {med(t_base) / med(t_new):.2f}x, medians {d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}"

        FUSED = dict(attention=a.attention_mode if a.step_launches else "fused", inputs="fused", trunk="torch", heads=a.heads_mode if a.step_launches else "torch")
        make = lambda **kw: LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, **FUSED, **kw)
        w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
        ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
        for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
            ro.collect()
        rows = ro.episodes.rows()
        base = make()
        with torch.no_grad():
            old = base.old_logits(rows["obs"], bank, ro.episodes.N)
            b = base.policy_batch(rows, old, 0)
        seq_len = b["seq_len"].cpu().numpy()

        def one_minibatch(size):
            s0, s1 = LR.minibatch_partition(seq_len, size)[0]
            sub = {k: v[s0:s1].contiguous() for k, v in b.items()}
            mb = {k: v for k, v in sub.items() if k != "seq_len"}
            mb["n_valid"] = torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device=dev)
            return sub, mb, s1 - s0, int(seq_len[s0:s1].sum())

        def graph_learner(sub, n_steps):
            """a graph learner whose one pass is n_steps visits of the single minibatch `sub` -> (learner, milliseconds graph_prepare took)"""
            lr = make(optimizer="fused", step="graph", num_sgd_iter=n_steps, sgd_minibatch_size=1 << 30)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lr.graph_prepare(0, sub)
            torch.cuda.synchronize()
            return lr, (time.perf_counter() - t0) * 1e3

        if a.step_launches:
            sub, mb, _, _ = one_minibatch(256)
            if a.step_launches == "graph":
                lr, _ = graph_learner(sub, a.step_count)
                lr.graph_replay(0, a.step_count)
            else:
                for _ in range(a.step_count):
                    base.minibatch_step(0, mb)
            torch.cuda.synchronize()
            print(f"{a.step_count} {a.step_launches} steps done")
            return

        say(f"# tools/ppo_learner_bench.py --step on {torch.cuda.get_device_name(0)}: PPOLearner(optimizer=\"fused\", step=\"graph\") against the eager step "
            f"with torch.optim.Adam, all in this run; attention = fused, inputs = fused, trunk = torch; {a.iters} timed iterations after {a.warmup} "
            f"warm-up, device events (a later run, appended):")
        # (a) the kernels alone
        mod = base.modules[0]
        params = [p.detach().clone() for p in mod.parameters()]
        for label, ps in ((f"a Fight1 module's {len(params)} tensors", params), ("one tensor of 64 Mi elements", [torch.zeros((1 << 26,), device=dev)])):
            gs, ms, vs = [torch.randn_like(p) for p in ps], [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
            t_dev = torch.zeros((1,), dtype=torch.int32, device=dev)
            n = sum(p.numel() for p in ps)
            t = events(lambda: LR.adam_step(ps, gs, ms, vs, t_dev, lr=1e-4))
            say(f"    hh_adam_step alone, {label} ({n} elements): {q(t)} = {28 * n / med(t) / 1e6:.1f} GB/s of {28 * n / 1e6:.2f} MB algorithmic bytes "
                f"({100 * 28 * n / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")
            del gs, ms, vs
        names = [k for k in b if k != "seq_len"]
        for S in (14, 3560):
            srcs = [b[k][:S].contiguous() for k in names]
            staged = [torch.zeros_like(c) for c in srcs]
            sched = torch.tensor([(0, S, 0, 0)], dtype=torch.int32, device=dev)
            cur, nv = torch.zeros((1,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
            nbytes = 2 * sum(c.numel() * c.element_size() for c in srcs)
            t = events(lambda: LR.minibatch_stage(srcs, staged, 20, sched, cur, nv))
            say(f"    hh_minibatch_stage alone, the {len(names)} columns of a Fight1 batch, {S} chunks of 20: {q(t)} = {nbytes / med(t) / 1e6:.1f} GB/s of "
                f"{nbytes / 1e6:.2f} MB algorithmic bytes ({100 * nbytes / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")
        # (b) the minibatch step
        K = 50
        dev_adam = make(optimizer="fused")

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

        for size in (256, 65536):
            sub, mb, n_chunks, n_rows = one_minibatch(size)
            n_total = 4 * (a.iters + a.warmup) + 4 * K + 8
            dev_adam._books[0].begin(n_total)
            graph, t_cap = graph_learner(sub, n_total)
            t_e = events(lambda: base.minibatch_step(0, mb))
            t_f = events(lambda: dev_adam.minibatch_step(0, mb))
            t_g = events(lambda: graph.graph_replay(0, 1))
            say(f"minibatch step (Fight1, forward + loss + backward + Adam, fused loss), {n_rows} unpadded rows in {n_chunks} chunks of 20: eager + torch Adam "
                f"{q(t_e)}; eager + device Adam {q(t_f)} [{verdict(t_e, t_f)}]; graph {q(t_g)} [{verdict(t_e, t_g)}]")
            say(f"    {K} steps back to back, ms per step, three runs: eager + torch Adam {burst(lambda: [base.minibatch_step(0, mb) for _ in range(K)])} | "
                f"eager + device Adam {burst(lambda: [dev_adam.minibatch_step(0, mb) for _ in range(K)])} | graph {burst(lambda: graph.graph_replay(0, K))}")
            say(f"    graph_prepare (upload, warm-up, capture) of this step: {t_cap:.1f} ms on the host clock")
            del graph
        # (c) one whole update
        res = {}
        for label, kw in (("eager + torch Adam", {}), ("graph", dict(optimizer="fused", step="graph"))):
            lr = make(num_sgd_iter=a.passes, sgd_minibatch_size=a.step_minibatch, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = lr.update(ro.episodes, bank)
            torch.cuda.synchronize()
            res[label] = ((time.perf_counter() - t0) * 1e3, st)
        (t_e, st_e), (t_g, st_g) = res["eager + torch Adam"], res["graph"]
        say(f"one update of both policies ({a.passes} pass(es), minibatches of >= {a.step_minibatch} rows: {st_e[0]['steps']} + {st_e[1]['steps']} steps over "
            f"{st_e[0]['rows']} rows each), host clock to a synchronise, first update of a new learner (the graph's includes its two captures): "
            f"eager + torch Adam {t_e:.1f} ms; graph {t_g:.1f} ms; eager / graph = {t_e / t_g:.2f}x")
        say(f"    mean statistics, eager: {[{k: round(v, 6) for k, v in s.items()} for s in st_e]}")
        say(f"    mean statistics, graph: {[{k: round(v, 6) for k, v in s.items()} for s in st_g]}")

    if a.step or a.step_launches:
        lines.clear()
        step_section()
        if a.out and a.step:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    def clip_section():
        """grad_clip against grad_clip = None: the two kernels alone, the graph step"""
        med = statistics.median

        def verdict(t_base, t_new, base="without"):
            spread = max(max(t_base) - min(t_base), max(t_new) - min(t_new))
            d = med(t_new) - med(t_base)
            word = "no difference beyond the spread" if abs(d) <= spread else ("cost" if d > 0 else "gain")
            return f"{base} -> with: medians {d * 1e3:+.1f} us apart, larger spread {spread * 1e3:.1f} us: {word}"

        say(f"# tools/ppo_learner_bench.py --clip on {torch.cuda.get_device_name(0)}: PPOLearner(grad_clip=...) against grad_clip = None (the step as it "
            f"was), both in this run; attention = fused, inputs = fused, trunk = torch; {a.iters} timed iterations after {a.warmup} warm-up, device "
            f"events (a later run, appended):")
        FUSED = dict(attention="fused", inputs="fused", trunk="torch")
        make = lambda **kw: LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, **FUSED, **kw)
        base = make()
        # (a) the kernels alone
        params = [p.detach().clone() for p in base.modules[0].parameters()]
        for label, ps in ((f"a Fight1 module's {len(params)} tensors", params), ("one tensor of 64 Mi elements", [torch.zeros((1 << 26,), device=dev)])):
            gs = [torch.randn_like(p) for p in ps]
            n = sum(p.numel() for p in ps)
            clip, scratch = torch.zeros((2,), dtype=torch.float64, device=dev), LR.grad_norm_scratch(gs)
            t = events(lambda: LR.grad_norm(gs, 1.0, clip, scratch=scratch))
            say(f"    hh_grad_norm alone ({(len(ps) + 63) // 64} partial launch(es) + the final one), {label} ({n} elements, {scratch.numel()} tiles): {q(t)} = "
                f"{4 * n / med(t) / 1e6:.1f} GB/s of {4 * n / 1e6:.2f} MB algorithmic bytes ({100 * 4 * n / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 "
                f"copy reaches)")
        ps = [torch.zeros((1 << 26,), device=dev)]
        ms, vs, t_dev = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], torch.zeros((1,), dtype=torch.int32, device=dev)
        n = ps[0].numel()
        t_p = events(lambda: LR.adam_step(ps, gs, ms, vs, t_dev, lr=1e-4))
        t_c = events(lambda: LR.adam_step(ps, gs, ms, vs, t_dev, lr=1e-4, clip=clip))
        say(f"    hh_adam_step alone, 64 Mi elements: {q(t_p)} = {28 * n / med(t_p) / 1e6:.1f} GB/s; hh_adam_step_clipped (coefficient {clip[1].item():.3e}): "
            f"{q(t_c)} = {28 * n / med(t_c) / 1e6:.1f} GB/s of the same {28 * n / 1e6:.0f} MB; {verdict(t_p, t_c, 'unclipped')}")
        del ps, gs, ms, vs
        # (b) the graph step
        w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
        ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
        for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
            ro.collect()
        rows = ro.episodes.rows()
        with torch.no_grad():
            old = base.old_logits(rows["obs"], bank, ro.episodes.N)
            b = base.policy_batch(rows, old, 0)
        seq_len = b["seq_len"].cpu().numpy()
        K = 50
        for size in (256, 65536):
            s0, s1 = LR.minibatch_partition(seq_len, size)[0]
            sub = {k: v[s0:s1].contiguous() for k, v in b.items()}
            n_total = 2 * (a.iters + a.warmup) + 4 * K + 8
            probe = make(optimizer="fused", step="graph", num_sgd_iter=1, sgd_minibatch_size=1 << 30, grad_clip=1e30)
            probe.graph_prepare(0, sub)
            probe.graph_replay(0, 1)
            n0 = float(probe._books[0].gnorm[0].item())
            ts, bursts = {}, {}
            for label, gc in (("without", None), ("with", n0 / 2.0)):
                lr = make(optimizer="fused", step="graph", num_sgd_iter=n_total, sgd_minibatch_size=1 << 30, grad_clip=gc)
                lr.graph_prepare(0, sub)
                ts[label] = events(lambda: lr.graph_replay(0, 1))
                out = []
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    lr.graph_replay(0, K)
                    e1.record()
                    torch.cuda.synchronize()
                    out.append(e0.elapsed_time(e1) / K)
                bursts[label] = out
                if gc is not None:
                    used = int(lr._books[0].cursor.item())
                    say(f"    grad_clip = N0 / 2 = {gc:.4e}: mean norm before clipping over {used} steps {float(lr._books[0].gnorm[:used].mean()):.4e}, last "
                        f"coefficient {lr.optimizers[0].clip[1].item():.4f}")
                del lr
            say(f"graph step (Fight1, stage + forward + loss + backward + [norm, 2 launches] + Adam + commit), {int(seq_len[s0:s1].sum())} unpadded rows in "
                f"{s1 - s0} chunks of 20: grad_clip = None {q(ts['without'])}; grad_clip set {q(ts['with'])}; {verdict(ts['without'], ts['with'])}")
            say(f"    {K} replays back to back, ms per step, three runs: grad_clip = None {', '.join(f'{x:.4f}' for x in bursts['without'])} | grad_clip set "
                f"{', '.join(f'{x:.4f}' for x in bursts['with'])}")

    if a.clip:
        lines.clear()
        clip_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    def shuffle_section():
        """shuffle_sequences=True against shuffle_sequences=False: the stage launch alone, the graph step, one update, the host's schedule"""
        from hhmarl_2d_amd import policy_nets as PN
        med = statistics.median

        def cost(t_base, t_new):
            spread = max(max(t_base) - min(t_base), max(t_new) - min(t_new))
            d = med(t_new) - med(t_base)
            word = "no difference beyond the spread" if abs(d) <= spread else ("cost" if d > 0 else "gain")
            return f"off -> on: medians {d * 1e3:+.1f} us apart, larger spread {spread * 1e3:.1f} us: {word}"

        FUSED = dict(attention="fused", inputs="fused", trunk="torch", heads=a.heads_mode if a.step_launches else "torch")
        make = lambda **kw: LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, **FUSED, **kw)
        w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
        ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
        for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
            ro.collect()
        rows = ro.episodes.rows()
        base = make()
        with torch.no_grad():
            old = base.old_logits(rows["obs"], bank, ro.episodes.N)
            b = base.policy_batch(rows, old, 0)
        seq_len = b["seq_len"].cpu().numpy()
        S, R = len(seq_len), int(seq_len.sum())
        say(f"# tools/ppo_learner_bench.py --shuffle on {torch.cuda.get_device_name(0)}: PPOLearner(shuffle_sequences=True) against shuffle_sequences=False "
            f"(the step as it was), both in this run; {a.arenas} arenas, T = {a.T}: {S} chunks of 20, {R} rows per policy; attention = fused, inputs = "
            f"fused, trunk = torch; {a.iters} timed runs after {a.warmup} warm-up (a later run, appended):")
        # (a) the stage launch alone, on the same columns: the first n chunks against n chunks drawn from the whole batch
        cur, nv = torch.zeros((1,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)

        def stage_pair(label, cols, chunk_len, n):
            total = cols[0].shape[0]
            staged = [torch.zeros((n,) + tuple(c.shape[1:]), dtype=c.dtype, device=dev) for c in cols]
            sched = torch.tensor([(0, n, 0, 0)], dtype=torch.int32, device=dev)
            order = torch.from_numpy(LR.sequence_order(total, 1, 0, 0, 0).astype(np.int32)).to(dev)
            nbytes = 2 * sum(st.numel() * st.element_size() for st in staged)
            t_p = events(lambda: LR.minibatch_stage(cols, staged, chunk_len, sched, cur, nv))
            t_g = events(lambda: LR.minibatch_stage_gather(cols, staged, chunk_len, order, sched, cur, nv))
            say(f"    the stage launch alone, {label}, {n} of {total} chunks of {chunk_len} ({nbytes / 1e6:.2f} MB read + written): hh_minibatch_stage {q(t_p)} = "
                f"{nbytes / med(t_p) / 1e6:.1f} GB/s; hh_minibatch_stage_gather {q(t_g)} = {nbytes / med(t_g) / 1e6:.1f} GB/s; {cost(t_p, t_g)}")

        names = [k for k in b if k != "seq_len"]
        fight_cols = [b[k].contiguous() for k in names]
        for n in (14, 3560):
            stage_pair(f"the {len(names)} columns of a Fight1 batch", fight_cols, 20, min(n, S))
        d1, a1, d2, a2 = PN.CRITIC_DIMS[PN.ESC1]
        g = torch.Generator(device=dev).manual_seed(3)
        esc_cols = [torch.rand((R, PN.OBS_DIM[PN.ESC1]), generator=g, device=dev), torch.rand((R, d1 + a1 + d2 + a2), generator=g, device=dev),
                    torch.zeros((R, 4), dtype=torch.int8, device=dev), torch.rand((R,), generator=g, device=dev), torch.rand((R,), generator=g, device=dev),
                    torch.rand((R,), generator=g, device=dev), torch.rand((R, 32), generator=g, device=dev), torch.ones((R,), dtype=torch.uint8, device=dev)]
        for n in (271, 65544):
            stage_pair("the 8 columns of an Esc1 batch of as many rows (synthetic content)", esc_cols, 1, min(n, R))
        del esc_cols
        # (b) the graph step: every pass over ONE minibatch, so the gather draws from that minibatch's chunks
        K = 50
        for size in (256, 65536):
            s0, s1 = LR.minibatch_partition(seq_len, size)[0]
            sub = {k: v[s0:s1].contiguous() for k, v in b.items()}
            n_total = 2 * (a.iters + a.warmup) + 4 * K + 8
            ts, bursts = {}, {}
            for flag in (False, True):
                lr = make(optimizer="fused", step="graph", num_sgd_iter=n_total, sgd_minibatch_size=1 << 30, shuffle_sequences=flag)
                lr.graph_prepare(0, sub)
                ts[flag] = events(lambda: lr.graph_replay(0, 1))
                out = []
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    lr.graph_replay(0, K)
                    e1.record()
                    torch.cuda.synchronize()
                    out.append(e0.elapsed_time(e1) / K)
                bursts[flag] = out
                del lr
            say(f"graph step (Fight1, stage + forward + loss + backward + Adam + commit), {int(seq_len[s0:s1].sum())} unpadded rows in {s1 - s0} chunks of 20: "
                f"shuffle off {q(ts[False])}; on {q(ts[True])}; {cost(ts[False], ts[True])}")
            say(f"    {K} replays back to back, ms per step, three runs: off {', '.join(f'{x:.4f}' for x in bursts[False])} | on "
                f"{', '.join(f'{x:.4f}' for x in bursts[True])}")
        # (c) one whole update of both policies, kl_coeff = 0 so that only a changed cap captures again
        res = {}
        for flag in (False, True):
            lr = make(optimizer="fused", step="graph", num_sgd_iter=a.passes, sgd_minibatch_size=a.step_minibatch, kl_coeff=0.0, shuffle_sequences=flag)
            times = []
            for _ in range(a.warmup + a.iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = lr.update(ro.episodes, bank)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            res[flag] = (times[a.warmup:], st, [bk.captures for bk in lr._books])
            del lr
        (t_off, st_off, c_off), (t_on, st_on, c_on) = res[False], res[True]
        say(f"one update of both policies ({a.passes} pass(es), minibatches of >= {a.step_minibatch} rows: {st_off[0]['steps']} + {st_off[1]['steps']} steps "
            f"over {st_off[0]['rows']} rows each; shuffled: {st_on[0]['steps']} + {st_on[1]['steps']} in the last one), graph, host clock to a synchronise, "
            f"{a.iters} updates after {a.warmup}: shuffle off {q(t_off)} (captures in all {c_off}); on {q(t_on)} (captures in all {c_on}: an update whose "
            f"largest minibatch has another size captures again); {cost(t_off, t_on)}")
        # (d) the host's part and the table
        for label, lens in ((f"{S} chunks of <= 20 rows", seq_len), (f"the same {R} rows as escape rows", np.ones(R, dtype=np.int64))):
            t_h, t_s = [], []
            for i in range(a.warmup + a.iters):
                t0 = time.perf_counter()
                order_h, sched_h = LR.shuffled_schedule(lens, 256, 30, 1, i, 0)
                t_h.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                LR.sequence_schedule(lens, 256, 30, 1, i, 0)
                t_s.append((time.perf_counter() - t0) * 1e3)
            say(f"    host, {label}, 30 passes of minibatches of >= 256 rows ({len(sched_h)} steps): shuffled_schedule {q(t_h[a.warmup:])}; sequence_schedule "
                f"(shuffle off) {q(t_s[a.warmup:])}; {cost(t_s[a.warmup:], t_h[a.warmup:])}")
            say(f"    order table, {label}: 4 x 30 x {len(lens)} = {order_h.nbytes} bytes ({order_h.nbytes / 1e6:.2f} MB)")

    if a.shuffle:
        lines.clear()
        shuffle_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    def heads_section():
        """heads="fused" against heads="torch": the kernel alone, the Fight1 and Esc1 minibatch step (eager and graph), one graph update"""
        import ctypes as C
        from hhmarl_2d_amd import _lib as L
        med = statistics.median
        K = 50

        def verdict(t_torch, t_fused):
            spread = max(max(t_torch) - min(t_torch), max(t_fused) - min(t_fused))
            d = med(t_torch) - med(t_fused)
            word = "no difference beyond the spread" if abs(d) <= spread else ("gain" if d > 0 else "loss")
            return f"torch / fused = {med(t_torch) / med(t_fused):.2f}x, medians {d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}"

        say(f"# tools/ppo_learner_bench.py --heads on {torch.cuda.get_device_name(0)}: PPOLearner(heads=\"fused\") against the default heads=\"torch\", both in "
            f"this run; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended):")
        # (a) the kernel alone
        lib = L.lib()
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())
        for n_comp, n_out in ((4, 26), (3, 24)):
            for R in (280, 71200):
                g = torch.Generator().manual_seed(R + n_comp)
                r = lambda *shape: torch.randn(shape, generator=g).to(dev)
                za, zc, w_act, b_act, w_val, b_val = r(R, 500), r(R, 500), 0.04 * r(n_out, 500), 0.04 * r(n_out), 0.04 * r(500), 0.04 * r(1)
                old, act = r(R, 32), torch.zeros((R, 4), dtype=torch.int8, device=dev)
                old_logp, adv, target = -6.0 + 0.1 * r(R), r(R), r(R)
                n_valid = torch.full((1,), R, dtype=torch.int32, device=dev)
                outs = [torch.empty_like(t) for t in (za, zc, w_act, b_act, w_val, b_val)]
                stats = torch.empty((6,), dtype=torch.float64, device=dev)
                nb, tile, wgs = C.c_int64(), C.c_int32(), C.c_int32()
                L.check(lib.hh_heads_loss_scratch_bytes(R, n_comp, C.byref(nb)))
                L.check(lib.hh_heads_loss_geometry(R, n_comp, C.byref(tile), C.byref(wgs)))
                scratch = torch.empty((nb.value // 8,), dtype=torch.float64, device=dev)
                prm = L.HHPpoLossParams(n_comp=n_comp, reserved0=0, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2, reserved1=0.0)
                fn = lambda: L.check(lib.hh_heads_loss(R, p(za), p(zc), p(w_act), p(b_act), p(w_val), p(b_val), p(old), p(act), p(old_logp), p(adv), p(target),
                                                       None, p(n_valid), C.byref(prm), p(stats), *[p(o) for o in outs], None, None, p(scratch), nb.value, st))
                t = events(fn)
                nbytes = R * (4 * 500 * 4 + 32 * 4 + 4 + 12) + 2 * (n_out + 1) * 501 * 4
                say(f"    hh_heads_loss alone (two launches), n_comp = {n_comp}, {R} rows ({wgs.value} workgroups, tiles of {tile.value} rows, {nb.value / 1e6:.2f} MB of "
                    f"scratch): {q(t)} = {nbytes / med(t) / 1e6:.1f} GB/s of {nbytes / 1e6:.2f} MB algorithmic bytes "
                    f"({100 * nbytes / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")
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

        # (b) the minibatch step, (c) the whole update
        for mode, name, opts in (("fight", "Fight1", dict(attention="fused", inputs="fused")), ("escape", "Esc1", dict(inputs="fused"))):
            make = lambda **kw: LR.PPOLearner.trainable_init(dev, mode=mode, seed=1, **opts, **kw)
            w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon, agent_mode=1 if mode == "escape" else 0), device=0)
            bank = PolicyBank.trainable_init(dev, mode=mode, seed=1, max_rows=2 * a.arenas)
            ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
            for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
                ro.collect()
            rows = ro.episodes.rows()
            eager = {h: make(heads=h) for h in ("torch", "fused")}
            with torch.no_grad():
                old = eager["torch"].old_logits(rows["obs"], bank, ro.episodes.N)
                b = eager["torch"].policy_batch(rows, old, 0)
            cols, seq_len = eager["torch"]._columns(b)
            for size in (256, 65536):
                s0, s1 = LR.minibatch_partition(seq_len, size)[0]
                sub = {k: v[s0:s1].contiguous() for k, v in b.items()}
                mb = {k: v for k, v in sub.items() if k != "seq_len"}
                n_rows = int(seq_len[s0:s1].sum())
                mb["n_valid"] = torch.tensor([n_rows], dtype=torch.int32, device=dev)
                n_total = 2 * (a.iters + a.warmup) + 4 * K + 8
                graphs = {h: make(heads=h, optimizer="fused", step="graph", num_sgd_iter=n_total, sgd_minibatch_size=1 << 30) for h in ("torch", "fused")}
                for lr in graphs.values():
                    lr.graph_prepare(0, sub)
                t_e = {h: events(lambda lr=lr: lr.minibatch_step(0, mb)) for h, lr in eager.items()}
                t_g = {h: events(lambda lr=lr: lr.graph_replay(0, 1)) for h, lr in graphs.items()}
                say(f"minibatch step ({name}, forward + loss + backward + Adam), {n_rows} unpadded rows in {s1 - s0} {'chunks of 20' if mode == 'fight' else 'rows'}: "
                    f"eager + torch Adam: heads = torch {q(t_e['torch'])}; heads = fused {q(t_e['fused'])} [{verdict(t_e['torch'], t_e['fused'])}]")
                say(f"    graph step: heads = torch {q(t_g['torch'])}; heads = fused {q(t_g['fused'])} [{verdict(t_g['torch'], t_g['fused'])}]")
                say(f"    {K} graph replays back to back, ms per step, three runs: heads = torch {burst(lambda: graphs['torch'].graph_replay(0, K))} | "
                    f"heads = fused {burst(lambda: graphs['fused'].graph_replay(0, K))}")
                del graphs
        # (c) one whole graph update at 1024 arenas (a world of its own: the steps above need the large batch, this does not)
        N_UPD = 1024
        make = lambda **kw: LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, attention="fused", inputs="fused", **kw)
        w = World(make_config(n_arenas=N_UPD, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * N_UPD)
        ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
        for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
            ro.collect()
        res = {}
        for h in ("torch", "fused", "torch", "fused"):
            lr = make(heads=h, optimizer="fused", step="graph", num_sgd_iter=a.passes, sgd_minibatch_size=a.step_minibatch, kl_coeff=0.0)
            lr.update(ro.episodes, bank)           # the first update captures
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stu = lr.update(ro.episodes, bank)
                torch.cuda.synchronize()
                res.setdefault(h, []).append((time.perf_counter() - t0) * 1e3)
        say(f"one whole graph update of both Fight policies at {N_UPD} arenas ({a.passes} pass(es), minibatches of >= {a.step_minibatch} rows, "
            f"{stu[0]['steps']} + {stu[1]['steps']} steps over {stu[0]['rows']} rows each, kl_coeff = 0 so that no graph is captured again), host clock to a "
            f"synchronise, 2 x 3 updates after the capturing one, learners alternating: heads = torch {q(res['torch'])}; heads = fused {q(res['fused'])} "
            f"[{verdict(res['torch'], res['fused'])}]")

    if a.heads:
        lines.clear()
        heads_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    def attention_block_section():
        """attention="block" against attention="fused": one block, the two kernel calls alone, the Fight1 graph step"""
        import ctypes as C
        from hhmarl_2d_amd import _lib as L
        med = statistics.median
        K = 50

        def verdict(t_fused, t_block):
            spread = max(max(t_fused) - min(t_fused), max(t_block) - min(t_block))
            d = med(t_fused) - med(t_block)
            word = "no difference beyond the spread" if abs(d) <= spread else ("gain" if d > 0 else "loss")
            return f"fused / block = {med(t_fused) / med(t_block):.2f}x, medians {d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}"

        say(f"# tools/ppo_learner_bench.py --attention-block on {torch.cuda.get_device_name(0)}: TrainableNet(attention=\"block\") (hh_attn_block_*: one launch "
            f"forward, two backward per block) against attention=\"fused\" (GEMMs + hh_chunk_attn_* + hh_residual_normalize_*), both in this run; {a.iters} timed "
            f"iterations after {a.warmup} warm-up, device events (a later run, appended):")
        # (a) one block, forward + backward
        for E in (100, 150):
            att = nn.MultiheadAttention(E, 2, batch_first=True).to(dev)
            for S in (14, 3560):
                g = torch.Generator().manual_seed(E + S)
                h = torch.tanh(torch.randn((S, 20, E), generator=g)).to(dev).requires_grad_(True)
                dy = torch.randn((S, 20, E), generator=g).to(dev)

                def block(attend):
                    h.grad = None
                    att.zero_grad(set_to_none=True)
                    attend(att, h).backward(dy)
                t_f, t_b = events(lambda: block(LR.TrainableNet._attend_fused)), events(lambda: block(LR.TrainableNet._attend_block))
                say(f"attention block (in-projection, core, out-projection, normalize(x + att); forward + backward, eager launches), E = {E}, {S} chunks of 20: "
                    f"fused {q(t_f)}; block {q(t_b)}; {verdict(t_f, t_b)}")
        # (b) the two calls alone
        lib = L.lib()
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())
        for E in (100, 150):
            for S in (14, 3560):
                R = S * 20
                r = lambda *shape: torch.randn(shape, device=dev)
                x, d_y, w_in, b_in, w_out, b_out = r(S, 20, E), r(S, 20, E), 0.1 * r(3 * E, E), 0.1 * r(3 * E), 0.1 * r(E, E), 0.1 * r(E)
                y, d_x = torch.empty_like(x), torch.empty_like(x)
                outs = [torch.empty_like(t) for t in (w_in, b_in, w_out, b_out)]
                nb_save, nb_scr = C.c_int64(), C.c_int64()
                L.check(lib.hh_attn_block_save_bytes(S, 20, E, C.byref(nb_save)))
                L.check(lib.hh_attn_block_scratch_bytes(S, 20, E, C.byref(nb_scr)))
                save, scratch = torch.empty((nb_save.value // 4,), device=dev), torch.empty((nb_scr.value // 4,), device=dev)
                spt, nwg = LR.attention_block_tile(S, 20, E)
                wbytes = (4 * E * E + 4 * E) * 4
                runs = (("hh_attn_block_forward (one launch)", R * (24 * E + 4) + wbytes,
                         lambda: L.check(lib.hh_attn_block_forward(S, 20, E, p(x), p(w_in), p(b_in), p(w_out), p(b_out), p(y), p(save), nb_save.value, st))),
                        ("hh_attn_block_backward (two launches)", R * (32 * E + 4) + 2 * wbytes,
                         lambda: L.check(lib.hh_attn_block_backward(S, 20, E, p(x), p(w_in), p(w_out), p(y), p(save), nb_save.value, p(d_y), p(d_x),
                                                                    *[p(o) for o in outs], p(scratch), nb_scr.value, st))))
                for name, nbytes, fn in runs:
                    t = events(fn)
                    say(f"    {name} alone, E = {E}, {S} chunks of 20 ({R} rows; {spt} sequence(s) per tile, {nwg} backward workgroups, {nb_scr.value / 1e6:.2f} MB of "
                        f"scratch): {q(t)} = {nbytes / med(t) / 1e6:.1f} GB/s of {nbytes / 1e6:.2f} MB algorithmic bytes "
                        f"({100 * nbytes / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")
                del save, scratch

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

        # (c) the Fight1 graph step with inputs = fused, heads = fused
        make = lambda **kw: LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, inputs="fused", heads="fused", **kw)
        w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
        ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
        for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
            ro.collect()
        rows = ro.episodes.rows()
        base = make(attention="fused")
        with torch.no_grad():
            old = base.old_logits(rows["obs"], bank, ro.episodes.N)
            b = base.policy_batch(rows, old, 0)
        cols, seq_len = base._columns(b)
        for size in (256, 65536):
            s0, s1 = LR.minibatch_partition(seq_len, size)[0]
            sub = {k: v[s0:s1].contiguous() for k, v in b.items()}
            n_rows = int(seq_len[s0:s1].sum())
            n_total = 2 * (a.iters + a.warmup) + 4 * K + 8
            graphs = {m: make(attention=m, optimizer="fused", step="graph", num_sgd_iter=n_total, sgd_minibatch_size=1 << 30) for m in ("fused", "block")}
            for lr in graphs.values():
                lr.graph_prepare(0, sub)
            t_g = {m: events(lambda lr=lr: lr.graph_replay(0, 1)) for m, lr in graphs.items()}
            say(f"graph step (Fight1, inputs = fused, heads = fused; stage + forward + loss + backward + Adam + commit), {n_rows} unpadded rows in {s1 - s0} chunks "
                f"of 20: attention = fused {q(t_g['fused'])}; attention = block {q(t_g['block'])} [{verdict(t_g['fused'], t_g['block'])}]")
            if size == 256:
                say(f"    {K} graph replays back to back, ms per step, three runs: attention = fused {burst(lambda: graphs['fused'].graph_replay(0, K))} | "
                    f"attention = block {burst(lambda: graphs['block'].graph_replay(0, K))}")
            del graphs

    if a.attention_block:
        lines.clear()
        attention_block_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    def window_section():
        """update_window (batch_mode = "truncate_episodes") next to update (complete_episodes): the batch build, kernels against torch twins,
        one whole update each, and the graph captures over three windows"""
        from hhmarl_2d_amd import policy_nets as PN
        from hhmarl_2d_amd.rollout import central_critic_rows
        med = statistics.median

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

        say(f"# tools/ppo_learner_bench.py --window on {torch.cuda.get_device_name(0)}: PPOLearner.update_window on a PPORollout's [T, N] window "
            f"(batch_mode = truncate_episodes) next to update on whole episodes, both in this run; {a.arenas} arenas, T = {a.T}, horizon {a.horizon}, "
            f"level 3; {a.iters} timed runs after {a.warmup} warm-up, medians, (max - min) spread rule (a later run, appended):")
        N, T = a.arenas, a.T
        for mode in ("fight", "escape"):
            cfg = dict(n_arenas=N, level=3, seed=7, auto_reset=True, horizon=a.horizon, agent_mode=1 if mode == "escape" else 0)
            bank = PolicyBank.trainable_init(dev, mode=mode, seed=1, max_rows=2 * N)
            ro = PPORollout(World(make_config(**cfg), device=0), bank, T, record_logits=True)
            ro_e = PPORollout(World(make_config(**cfg), device=0), bank, T, batch_mode="complete_episodes", record_logits=True)
            for _ in range(max(2, (a.horizon + T - 1) // T)):
                ro.collect()
                ro_e.collect()
            ln = LR.PPOLearner.trainable_init(dev, mode=mode, seed=1, num_sgd_iter=a.passes, sgd_minibatch_size=a.minibatch)
            Lm = ln.max_seq_len if ln.recurrent else 1
            with torch.no_grad():
                # (a) the pieces of the batch build
                t_cut, t_cut_t = host(lambda: LR.window_cut(ro.done, Lm)), host(lambda: LR.window_cut_torch(ro.done, Lm))
                shared = ln._window_shared(ro, bank)
                _, _, tables, logits, adv_rows = shared
                S = tables[0].numel()
                t_crit = events(lambda: central_critic_rows(ro.obs[:T], ro.actions, 1).contiguous())
                t_std = events(lambda: LR.standardize(ro.adv.transpose(0, 1).reshape(N * T, 2)[:, 0]).reshape(N, T).t().contiguous())
                critic = central_critic_rows(ro.obs[:T], ro.actions, 1).contiguous()
                adv = LR.standardize(adv_rows[:, 0]).reshape(N, T).t().contiguous()
                Dk = PN.OBS_DIM[ln.kinds[0]]
                cols = [(ro.obs, (Dk,), 0, False), (critic, (critic.shape[2],), 0, False), (ro.actions, (4,), 0, False), (ro.logp, (), 0, False),
                        (adv, (), 0, False), (ro.target, (), 0, False), (logits, (LR.OLD_LD,), 0, False)]
                outs = LR.window_gather(cols, tables, Lm)
                t_g, t_g_t = events(lambda: LR.window_gather(cols, tables, Lm, out=outs)), events(lambda: LR.window_gather_torch(cols, tables, Lm))
                wrote = sum(o.numel() * o.element_size() for o in outs)
                read = T * N * sum(int(np.prod(c[1], dtype=np.int64)) * c[0].element_size() for c in cols) + 12 * S
                t_b = host(lambda: ln.window_batch(ro, bank, 0, shared))
                t_b_all = host(lambda: ln.window_batch(ro, bank, 0))
                rows_e = ro_e.episodes.rows()
                old_e = ln.batch_old_logits(rows_e, bank, N)
                t_pb = host(lambda: ln.policy_batch(rows_e, old_e, 0))
            say(f"{mode}: the window has {T * N} rows in {S} sequences of <= {Lm}; the episode batch of the last collect {rows_e['obs'].shape[0]} rows in "
                f"{rows_e['ep_len'].shape[0]} episodes")
            say(f"    the cut (three launches + the read of n_seq, host clock): window_cut {q(t_cut)}; window_cut_torch {q(t_cut_t)}; {cost(t_cut_t, t_cut)}")
            say(f"    the gather of policy 0's seven columns (ONE launch, device events): hh_window_gather {q(t_g)} = {(read + wrote) / med(t_g) / 1e6:.1f} GB/s of "
                f"{read / 1e6:.1f} MB read + {wrote / 1e6:.1f} MB written = {100 * (read + wrote) / med(t_g) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy "
                f"reaches; window_gather_torch {q(t_g_t)}; {cost(t_g_t, t_g)}")
            say(f"    torch parts of the build (device events): central_critic_rows on [T, N] {q(t_crit)}; the advantages to arena-major rows, standardize, and back {q(t_std)}")
            say(f"    window_batch of policy 0 (host clock to a synchronise): from the shared cut and logits {q(t_b)}; with the cut and the shared parts {q(t_b_all)}; "
                f"policy_batch of policy 0 on the episode batch ({rows_e['obs'].shape[0]} rows) {q(t_pb)}")
            # (b) one whole update each
            t_w = host(lambda: ln.update_window(ro, bank))
            ln_e = LR.PPOLearner.trainable_init(dev, mode=mode, seed=1, num_sgd_iter=a.passes, sgd_minibatch_size=a.minibatch)
            t_u = host(lambda: ln_e.update(ro_e.episodes, bank))
            st_w, st_u = ln.update_window(ro, bank), ln_e.update(ro_e.episodes, bank)
            say(f"    one update of both policies ({a.passes} pass(es), minibatches of >= {a.minibatch} rows, eager, recorded logits, host clock to a synchronise): "
                f"update_window {q(t_w)} ({st_w[0]['steps']} + {st_w[1]['steps']} steps over {st_w[0]['rows']} rows each); update {q(t_u)} "
                f"({st_u[0]['steps']} + {st_u[1]['steps']} steps over {st_u[0]['rows']} rows each); {cost(t_u, t_w, ('update -> update_window', 'slower', 'faster'))} "
                f"(the row counts differ: per row {1e3 * med(t_w) / st_w[0]['rows']:.3f} us against {1e3 * med(t_u) / max(st_u[0]['rows'], 1):.3f} us)")
            del ln_e, ro_e, rows_e, old_e, outs, critic, adv, shared, logits, adv_rows
            # (c) the graph step over three windows: the row count is constant, so is the schedule's shape
            lg = LR.PPOLearner.trainable_init(dev, mode=mode, seed=1, num_sgd_iter=a.passes, sgd_minibatch_size=a.step_minibatch, kl_coeff=0.0,
                                              optimizer="fused", step="graph")
            caps, steps, t3 = [], [], []
            for _ in range(3):
                ro.collect()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = lg.update_window(ro, bank)
                lg.publish(bank)
                torch.cuda.synchronize()
                t3.append((time.perf_counter() - t0) * 1e3)
                caps.append([bk.captures for bk in lg._books])
                steps.append((st[0]["steps"], st[1]["steps"]))
            say(f"    step=\"graph\", kl_coeff = 0, minibatches of >= {a.step_minibatch} rows, three windows (collect, update_window, publish; no start()): captures "
                f"after each window {caps}, steps {steps}, update_window + publish {', '.join(f'{x:.1f}' for x in t3)} ms")
            del lg, ln, ro, bank

    if a.window:
        lines.clear()
        window_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    def shards_section():
        """PPOLearner(group=LocalShards(1)) as a COST next to group=None, and hh_grad_pack / hh_grad_combine alone"""
        med = statistics.median

        def verdict(t_base, t_new):
            spread = max(max(t_base) - min(t_base), max(t_new) - min(t_new))
            d = med(t_new) - med(t_base)
            word = "no difference beyond the spread" if abs(d) <= spread else ("cost" if d > 0 else "gain")
            return f"this / group=None = {med(t_new) / med(t_base):.2f}x, medians {d:+.3f} ms apart, larger spread {spread:.3f} ms: {word}"

        say(f"# tools/ppo_learner_bench.py --shards on {torch.cuda.get_device_name(0)}: PPOLearner(group=LocalShards(1)) against group=None, all in this "
            f"run; {a.iters} timed iterations after {a.warmup} warm-up, device events (a later run, appended).  What W ranks gain on real hardware "
            f"is unmeasured: this is the cost one rank pays")
        make = lambda **kw: LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, num_sgd_iter=1, sgd_minibatch_size=1 << 30, **kw)
        base, one = make(), make(group=LR.LocalShards(1))
        # (a) the two kernels alone
        params = [p.detach() for p in base.modules[0].parameters()]
        for label, ps in ((f"a Fight1 module's {len(params)} tensors", params), ("one tensor of 64 Mi elements", [torch.zeros((1 << 26,), device=dev)])):
            gs = [torch.randn_like(p) for p in ps]
            lay = LR.grad_layout(gs)
            n = sum(lay[0])
            bucket = torch.zeros((lay[2],), dtype=torch.float32, device=dev)
            t = events(lambda: LR.grad_pack(gs, bucket, lay))
            say(f"    hh_grad_pack alone, {label} ({n} elements): {q(t)} = {8 * n / med(t) / 1e6:.1f} GB/s of {8 * n / 1e6:.2f} MB algorithmic bytes "
                f"({100 * 8 * n / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")
            for W in (1, 2, 8) if n < (1 << 26) else (1, 2):
                buckets = bucket.repeat(W, 1).contiguous()
                wt = [1.0 / W] * W
                t = events(lambda: LR.grad_combine(gs, buckets, wt, lay))
                nb = 4 * n * (W + 1)
                say(f"    hh_grad_combine alone, {label}, W = {W}: {q(t)} = {nb / med(t) / 1e6:.1f} GB/s of {nb / 1e6:.2f} MB algorithmic bytes "
                    f"({100 * nb / med(t) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")
                del buckets
            del gs, bucket
        # (b) one eager minibatch step of the driver: run against run_sharded on one minibatch
        w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
        bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
        ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
        for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):
            ro.collect()
        rows = ro.episodes.rows()
        with torch.no_grad():
            b = base.policy_batch(rows, base.old_logits(rows["obs"], bank, ro.episodes.N), 0)
        seq_len = b["seq_len"].cpu().numpy()
        for size in (256, 65536):
            s0, s1 = LR.minibatch_partition(seq_len, size)[0]
            sub = {k: v[s0:s1].contiguous() for k, v in b.items()}
            t_n = events(lambda: base._sgd[0].run(*base._columns(sub)))
            t_s = events(lambda: one._sgd[0].run_sharded(one.group, [one._columns(sub)]))
            say(f"one eager minibatch step through the driver (Fight1, schedule + forward + loss + backward + Adam + the statistics read back), "
                f"{int(seq_len[s0:s1].sum())} unpadded rows in {s1 - s0} chunks of 20: group=None {q(t_n)}; LocalShards(1) (+ pack, combine, the "
                f"statistics through the host) {q(t_s)} [{verdict(t_n, t_s)}]")

    if a.shards:
        lines.clear()
        shards_section()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

    # ---- errors against float64 (the GPU test's generator and bound: kernel <= 4 x e32 per quantity)
    say("errors against the float64 restatement, largest absolute difference (statistics | d_logits | d_vf), entropy_coeff 0.01, kl_coeff 0.2:")
    for R, n_comp, masked in ((63, 4, True), (4096, 3, False), (100003, 4, True), (100003, 3, False)):
        ld = {4: 26, 3: 24}[n_comp] if R % 2 else 32
        kw = dict(KW, n_comp=n_comp, entropy_coeff=0.01)
        inp = REF.make_inputs(R, n_comp, ld, masked, 0)
        want = REF.reference(inp, torch.float64, **kw)
        s32, dl32, dv32, _ = REF.reference(inp, torch.float32, **kw)
        keep = ~REF.near_kink(want[3], kw["clip_param"], kw["vf_clip_param"])
        logits, vf = inp["logits"].to(dev).requires_grad_(True), inp["vf"].to(dev).requires_grad_(True)
        batch = {k: inp[k].to(dev) for k in ("old_logits", "actions", "old_logp", "adv", "target")}
        if masked:
            batch["mask"] = inp["mask"].to(dev)
        total, stats = LR.ppo_loss(logits, vf, batch, **kw)
        total.backward()

        def err(s, dl, dv):
            return (max(abs(float(x) - y) for x, y in zip(s[:5], want[0][:5])), (dl.double().cpu()[keep] - want[1][keep]).abs().max().item(),
                    (dv.double().cpu()[keep] - want[2][keep]).abs().max().item())
        e32, ek = err(s32, dl32, dv32), err(stats.cpu(), logits.grad, vf.grad)
        say(f"  R = {R:6d} n_comp = {n_comp} mask = {masked!s:5}: e32 = {e32[0]:.3e} | {e32[1]:.3e} | {e32[2]:.3e}   "
            f"hh_ppo_loss = {ek[0]:.3e} | {ek[1]:.3e} | {ek[2]:.3e}   ({int((~keep).sum())} rows at a kink left out)")

    # ---- the loss alone
    for R in (256, 65536, 1 << 20):
        for n_comp, ld in ((4, 26), (3, 24)):
            kw = dict(KW, n_comp=n_comp)
            inp = REF.make_inputs(R, n_comp, ld, True, 2)
            logits, vf = inp["logits"].to(dev).requires_grad_(True), inp["vf"].to(dev).requires_grad_(True)
            batch = {k: inp[k].to(dev) for k in ("old_logits", "actions", "old_logp", "adv", "target")}
            batch["mask"] = inp["mask"].to(dev).to(torch.uint8)
            batch["n_valid"] = batch["mask"].sum(dtype=torch.int32).reshape(1)

            def run(fn):
                logits.grad = vf.grad = None
                total, _ = fn(logits, vf, batch, **kw)
                total.backward()

            def fwd(fn):
                with torch.no_grad():
                    fn(logits, vf, batch, **kw)
            t_k, t_t = events(lambda: run(LR.ppo_loss)), events(lambda: run(LR.ppo_loss_torch))
            t_kf = events(lambda: fwd(LR.ppo_loss))
            nbytes = R * (ld * 4 * 2 + 128 + 4 + 16 + 1 + 4)
            say(f"loss alone, R = {R:7d}, ld = {ld}: hh_ppo_loss + backward scaling {q(t_k)}; torch-op loss + autograd {q(t_t)}; "
                f"ratio {statistics.median(t_t) / statistics.median(t_k):.1f}x")
            say(f"    the kernel call alone (two launches + torch's output allocations; gradients included): {q(t_kf)} = "
                f"{nbytes / statistics.median(t_kf) / 1e6:.1f} GB/s of {nbytes / 1e6:.2f} MB algorithmic bytes "
                f"({100 * nbytes / statistics.median(t_kf) / 1e6 / 6290:.1f} % of the 6.29 TB/s a float4 copy reaches)")

    # ---- a world, a collect, the batch
    w = World(make_config(n_arenas=a.arenas, level=3, seed=7, auto_reset=True, horizon=a.horizon), device=0)
    bank = PolicyBank.trainable_init(dev, mode="fight", seed=1, max_rows=2 * a.arenas)
    ro = PPORollout(w, bank, a.T, batch_mode="complete_episodes")
    for _ in range(max(2, (a.horizon + a.T - 1) // a.T)):     # until whole episodes arrive in every collect
        ro.collect()
    t_collect = events(ro.collect, iters=5)
    rows = ro.episodes.rows()
    say(f"collect ({a.T} ticks x {a.arenas} arenas, one graph replay): {q(t_collect)}; the batch of the last collect: {rows['obs'].shape[0]} rows, "
        f"{rows['ep_len'].shape[0]} episodes")

    # ---- one minibatch step
    for fused in (True, False):
        learner = LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, fused=fused)
        with torch.no_grad():
            old = learner.old_logits(rows["obs"], bank, ro.episodes.N)
            b = learner.policy_batch(rows, old, 0)
        seq_len = b["seq_len"].cpu().numpy()
        for size in (256, 65536):
            parts = LR.minibatch_partition(seq_len, size)
            s0, s1 = parts[0]
            mb = {k: v[s0:s1] for k, v in b.items() if k != "seq_len"}
            mb["n_valid"] = torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device=dev)
            t = events(lambda: learner.minibatch_step(0, mb))
            say(f"minibatch step (Fight1, forward + loss + backward + Adam), fused = {fused!s:5}, {int(seq_len[s0:s1].sum())} unpadded rows in "
                f"{s1 - s0} chunks of 20: {q(t)}")

    # ---- one whole update
    learner = LR.PPOLearner.trainable_init(dev, mode="fight", seed=1, num_sgd_iter=a.passes, sgd_minibatch_size=a.minibatch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = learner.update(ro.episodes, bank)
    torch.cuda.synchronize()
    t_up = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    st = learner.update(ro.episodes, bank)
    learner.publish(bank)
    torch.cuda.synchronize()
    t_up2 = (time.perf_counter() - t0) * 1e3
    say(f"one update + publish of both policies ({a.passes} pass(es), minibatches of >= {a.minibatch} rows: {st[0]['steps']} + {st[1]['steps']} steps over "
        f"{st[0]['rows']} rows each), host clock to a synchronise: first {t_up:.1f} ms, second {t_up2:.1f} ms; next to one collect of "
        f"{statistics.median(t_collect):.1f} ms")
    say(f"    statistics of the second update: {st}")
    del ro, learner, rows
    old_logits_section()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
