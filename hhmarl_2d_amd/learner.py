"""The learner half of train_hetero.py's and train_hier.py's PPO on the device (train_hetero.py:206-243 with RLlib 2.4's PPO): the fused loss kernel
`hh_ppo_loss` (include/hh_learner.h) behind a torch.autograd.Function, the four trainable networks as torch modules in TRAINING form, and
`PPOLearner`, which turns the `EpisodeBatch` of a `PPORollout(batch_mode="complete_episodes")` into one PPO update of ac1_policy and
ac2_policy and hands the new weights back to the sampler's `PolicyBank` — collect -> update -> publish -> collect on one GPU, the
batch never leaving it.  The network GEMMs stay in PyTorch / rocBLAS; the loss and its gradient are one HIP pass.  Opt-in
(`attention="fused"`): what the fight networks' two attention blocks do between and after their projections runs in HIP too
(`chunk_attention`: hh_chunk_attn_*, `residual_normalize`: hh_residual_normalize_*); the default path is nn.MultiheadAttention.
Opt-in as well (`inputs="fused"`, all five networks): the layers in front of shared_layer as one grouped launch per side
(`input_stage`: hh_input_stage_*); the default path slices, concatenates and runs them one by one.
And (`trunk="fused"`, all five networks): shared_layer with its bias and tanh over the actor's and the critic's rows as ONE call
on the matrix cores (`dense_tanh`: hh_dense_tanh_*, split-fp16 MFMA); the default path is two float32 GEMMs and two tanh.
And (`heads="fused"`, all five networks, not with trunk="fused"): what follows shared_layer's GEMM — tanh, act_out and val_out, the PPO
loss, and the backward of all of it down to shared_layer's pre-activations — as ONE row pass and a fixed-order final sum (`heads_loss`:
hh_heads_loss); the default path is tanh, two GEMMs, hh_ppo_loss and autograd's backward of each.
And (`PPOLearner(optimizer="fused", step="graph")`): Adam on the device (`adam_step`: hh_adam_step) and the whole minibatch step — the
minibatch staged by a device schedule (`minibatch_stage`: hh_minibatch_stage), forward, loss, backward, Adam and the step's bookkeeping
(`train_commit`: hh_train_commit) — replayed from ONE HIP graph per policy; the default is torch.optim.Adam and the eager step.
Both learners also train from the rollouts' default batch_mode="truncate_episodes" (`update_window`): the fixed [T, N] window is cut into
sequences (`window_cut`: hh_window_cut) and its columns gathered into the padded form (`window_gather`: hh_window_gather); from there on
it is `update`.

The reference's learner does not compute what its sampler computes, and this module keeps the difference:
  * Fight1 / Fight2 are RLlib `RecurrentNetwork`s with a dummy state.  The sampler sees sequences of length 1 (attention =
    out_proj(v_proj(x)), what hh_policy_sample folds).  The learner sees each agent trajectory cut into chunks of max_seq_len = 20 rows,
    the last one zero-padded (rnn_sequencing.pad_batch_to_sequences_of_same_size), and `add_time_dimension` makes att_act / att_val
    attend over the 20 steps of a chunk, padded rows included as keys (no key padding mask).  ModelV2.__call__ hands the dummy state_in
    back as the state, so PPOTorchPolicy.loss takes its RNN branch: the loss is averaged over the unpadded rows only.
    Esc1 / Esc2 are plain TorchModelV2s: no chunks, no mask.
  * The critic is trained on rows with the actions filled in (rollout.central_critic_rows), while the batch's `vf` was predicted with
    zero action inputs.
  * ac1_policy and ac2_policy hold the same 500 x 500 shared_layer tensor (models/ac_models_hetero.py:22) and each has its own optimizer.

The commander half (train_hier.py with models/ac_models_hier.py:CommanderGru) is the second part of this file: `gru_sequence`, both
200-wide GRUs over whole chunks of max_seq_len steps in one fused launch each way (hh_gru_seq_forward / hh_gru_seq_backward),
`ppo_loss_categorical` (hh_ppo_loss_categorical), `CommanderTrainable` and `CommanderLearner`, which does for
`commander.CommanderRollout(batch_mode="complete_episodes")` what `PPOLearner` does for `PPORollout`."""
import ctypes as C
import functools
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import pilots
from . import policy_nets as PN
from .rollout import central_critic_rows, central_critic_rows_hl

OLD_LD = 32   # HH_POLICY_LOGITS: row width of the sampler's logits


def n_comp_of(kind):
    """action components of the kind's MultiDiscrete: 4 ([13, 9, 2, 2], 26 logits) for type-1 aircraft, 3 ([13, 9, 2], 24) for type-2"""
    return 4 if PN.N_OUT[kind] == 26 else 3


# ------------------------------------------------------------------------------------------------------------------ the loss
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _PPOLoss(torch.autograd.Function):
    """forward: hh_ppo_loss (loss, stats and the gradients in one pass); backward: the kept gradients times the incoming one"""

    @staticmethod
    def forward(ctx, logits, vf, old_logits, actions, old_logp, adv, target, mask, n_valid, prm):
        R, ld = logits.shape
        dev = logits.device
        stats = torch.empty((len(L.PPO_STATS),), dtype=torch.float64, device=dev)
        d_logits, d_vf = torch.empty_like(logits), torch.empty_like(vf)
        nbytes = C.c_int64()
        lib = L.lib()
        L.check(lib.hh_ppo_loss_scratch_bytes(R, C.byref(nbytes)))
        scratch = torch.empty((nbytes.value // 8,), dtype=torch.float64, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(lib.hh_ppo_loss(R, ld, _p(logits), _p(old_logits), _p(actions), _p(old_logp), _p(adv), _p(vf), _p(target), _p(mask), _p(n_valid),
                                C.byref(prm), _p(stats), _p(d_logits), _p(d_vf), _p(scratch), nbytes.value, st))
        ctx.save_for_backward(d_logits, d_vf)
        ctx.mark_non_differentiable(stats)
        return stats[0].float(), stats

    @staticmethod
    def backward(ctx, g_total, g_stats):
        d_logits, d_vf = ctx.saved_tensors
        return (d_logits * g_total, d_vf * g_total) + (None,) * 8


def _flat_batch(logits, vf, batch):
    """the learner's outputs and the batch columns as contiguous [R, ...] rows; n_valid made on the device where the batch has none"""
    ld = logits.shape[-1]
    logits = logits.reshape(-1, ld)
    R = logits.shape[0]
    col = lambda k, dt, w=None: batch[k].reshape((R,) if w is None else (R, w)).to(dt).contiguous()
    mask = batch.get("mask")
    mask = None if mask is None else col("mask", torch.uint8)
    n_valid = batch.get("n_valid")
    if n_valid is None:
        n_valid = (torch.full((1,), R, dtype=torch.int32, device=logits.device) if mask is None
                   else mask.ne(0).sum(dtype=torch.int32).reshape(1))
    return (logits, vf.reshape(R), col("old_logits", torch.float32, OLD_LD), col("actions", torch.int8, 4), col("old_logp", torch.float32),
            col("adv", torch.float32), col("target", torch.float32), mask, n_valid.reshape(1))


def ppo_loss(logits, vf, batch, *, n_comp, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2):
    """RLlib 2.4's PPOTorchPolicy.loss for a TorchMultiCategorical, fused (hh_ppo_loss: include/hh_learner.h has the formulas).
    logits f32 [..., ld] (ld >= 26 | 24, at most 32) and vf f32 [...]: the learner's outputs, CUDA, with autograd history.
    batch: dict of CUDA tensors over the same leading shape — old_logits f32 [..., 32] (the sampler's logits rows), actions i8 [..., 4],
    old_logp / adv / target f32 [...]; optional mask (u8 | bool [...], rows that count; absent = all) and n_valid (i32 [1] on the
    device: the number of rows that count, computed here when absent).
    -> (total loss: float32 0-d tensor on the device, differentiable with respect to logits and vf;
        stats f64 [6] on the device: total_loss, mean_policy_loss, mean_vf_loss, mean_kl, mean_entropy, n_valid  (_lib.PPO_STATS))
    No host synchronisation.  A missing library or GPU is an error, there is no fallback."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and vf.dtype == torch.float32):
        raise ValueError("ppo_loss: logits and vf are float32 CUDA tensors (the torch-op form for other dtypes is ppo_loss_torch)")
    flat = _flat_batch(logits.contiguous(), vf.contiguous(), batch)
    prm = L.HHPpoLossParams(n_comp=int(n_comp), reserved0=0, clip_param=clip_param, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff,
                            entropy_coeff=entropy_coeff, kl_coeff=kl_coeff, reserved1=0.0)
    return _PPOLoss.apply(*flat, prm)


def ppo_loss_torch(logits, vf, batch, *, n_comp, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2):
    """the same loss with torch ops in the dtype of `logits` (PPOLearner(fused=False): the A/B and timing partner of ppo_loss; same
    arguments, same results up to rounding)"""
    logits, vf, old_logits, actions, old_logp, adv, target, mask, n_valid = _flat_batch(logits, vf, batch)
    dt = logits.dtype
    splits = PN.ACTION_SPLIT[:n_comp]
    n_out = sum(splits)
    logp, ent, kl = 0.0, 0.0, 0.0
    a = actions.long()
    for c, (new, old) in enumerate(zip(logits[:, :n_out].split(splits, dim=1), old_logits[:, :n_out].to(dt).split(splits, dim=1))):
        lp, lq = F.log_softmax(new, dim=1), F.log_softmax(old, dim=1)
        logp = logp + lp.gather(1, a[:, c:c + 1]).squeeze(1)
        ent = ent - (lp.exp() * lp).sum(dim=1)
        kl = kl + (lq.exp() * (lq - lp)).sum(dim=1)
    ratio = torch.exp(logp - old_logp.to(dt))
    A = adv.to(dt)
    surrogate = torch.min(A * ratio, A * torch.clamp(ratio, 1 - clip_param, 1 + clip_param))
    vf_loss = torch.clamp(torch.pow(vf - target.to(dt), 2.0), 0, vf_clip_param)
    w = torch.ones_like(ratio) if mask is None else mask.ne(0).to(dt)
    n = n_valid.to(dt)[0]
    mean = lambda t: (t * w).sum() / n
    total = mean(-surrogate + vf_loss_coeff * vf_loss - entropy_coeff * ent)
    mean_kl = mean(kl) if kl_coeff > 0.0 else torch.zeros((), dtype=dt, device=logits.device)
    if kl_coeff > 0.0:
        total = total + kl_coeff * mean_kl
    stats = torch.stack([total, mean(-surrogate), mean(vf_loss), mean_kl, mean(ent), n]).detach().double()
    return total, stats


# ------------------------------------------------------------------------------------------------------------------ the chunk attention
ATTENTION_MODES = ("torch", "fused")


def _need_gpu(who):
    if not torch.cuda.is_available():
        raise RuntimeError(f"hhmarl_2d_amd.{who} needs a ROCm GPU (no CPU fallback)")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _ChunkAttn(torch.autograd.Function):
    """forward: hh_chunk_attn_forward; backward: hh_chunk_attn_backward, the probabilities recomputed from the kept qkv"""

    @staticmethod
    def forward(ctx, qkv):
        S, Lm, E3 = qkv.shape
        out = torch.empty((S, Lm, E3 // 3), dtype=torch.float32, device=qkv.device)
        L.check(L.lib().hh_chunk_attn_forward(S, Lm, E3 // 3, _p(qkv), _p(out), _stream(qkv.device)))
        ctx.save_for_backward(qkv)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        qkv, = ctx.saved_tensors
        S, Lm, E3 = qkv.shape
        d_qkv = torch.empty_like(qkv)
        L.check(L.lib().hh_chunk_attn_backward(S, Lm, E3 // 3, _p(qkv), _p(d_out.contiguous()), _p(d_qkv), _stream(qkv.device)))
        return d_qkv


class _ResidualNormalize(torch.autograd.Function):
    """forward: hh_residual_normalize_forward; backward: hh_residual_normalize_backward from the kept y and norm, one gradient for both inputs"""

    @staticmethod
    def forward(ctx, x, a):
        E = x.shape[-1]
        R = x.numel() // E
        y = torch.empty_like(x)
        norm = torch.empty((R,), dtype=torch.float32, device=x.device)
        L.check(L.lib().hh_residual_normalize_forward(R, E, _p(x), _p(a), _p(y), _p(norm), _stream(x.device)))
        ctx.save_for_backward(y, norm)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_y):
        y, norm = ctx.saved_tensors
        d_s = torch.empty_like(y)
        L.check(L.lib().hh_residual_normalize_backward(norm.numel(), y.shape[-1], _p(y), _p(norm), _p(d_y.contiguous()), _p(d_s), _stream(y.device)))
        return d_s, d_s


def _fused_input(who, t, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{who}: {what} is a contiguous float32 CUDA tensor (the torch-op form for other dtypes and devices is {who}_torch)")


def chunk_attention(qkv):
    """The core of nn.MultiheadAttention(E, 2, batch_first=True) between its in- and its out-projection, fused (hh_chunk_attn_forward /
    hh_chunk_attn_backward, include/hh_learner.h): qkv f32 [S, L, 3E] = x W_in^T + b_in (columns q | k | v, two head slices of E / 2
    each), contiguous, CUDA, E = 100 | 150, 1 <= L <= 32 -> ctx f32 [S, L, E] = softmax(Q K^T / sqrt(E / 2)) V per sequence and head,
    heads concatenated; no mask.  Differentiable with respect to qkv (first order).  No host synchronisation; a missing library or
    GPU is an error."""
    _need_gpu("chunk_attention")
    _fused_input("chunk_attention", qkv, "qkv")
    if qkv.dim() != 3 or qkv.shape[2] % 3 or qkv.shape[2] // 3 not in L.ATTN_WIDTHS or not 1 <= qkv.shape[1] <= L.ATTN_MAX_LEN:
        raise ValueError(f"chunk_attention: qkv is [S, L, 3E] with E in {L.ATTN_WIDTHS} and 1 <= L <= {L.ATTN_MAX_LEN}, got {tuple(qkv.shape)}")
    return _ChunkAttn.apply(qkv)


def residual_normalize(x, a):
    """F.normalize(x + a, dim=-1), fused (hh_residual_normalize_forward / _backward): x, a f32 [..., E] of one shape, contiguous, CUDA,
    E = 100 | 150 -> f32 [..., E].  Differentiable with respect to both (first order).  No host synchronisation, no fallback."""
    _need_gpu("residual_normalize")
    _fused_input("residual_normalize", x, "x")
    _fused_input("residual_normalize", a, "a")
    if x.shape != a.shape or x.dim() < 1 or x.shape[-1] not in L.ATTN_WIDTHS or x.device != a.device:
        raise ValueError(f"residual_normalize: x and a are [..., E] of one shape on one device with E in {L.ATTN_WIDTHS}, got {tuple(x.shape)} and {tuple(a.shape)}")
    return _ResidualNormalize.apply(x, a)


def chunk_attention_torch(qkv):
    """chunk_attention with torch ops, any dtype and device (the A/B partner): [S, L, 3E] -> [S, L, E]"""
    S, Lm, E3 = qkv.shape
    d = E3 // (3 * L.ATTN_HEADS)
    q, k, v = (t.reshape(S, Lm, L.ATTN_HEADS, d).transpose(1, 2) for t in qkv.split(E3 // 3, dim=-1))       # [S, heads, L, d]
    p = torch.softmax((q @ k.transpose(-1, -2)) / d ** 0.5, dim=-1)
    return (p @ v).transpose(1, 2).reshape(S, Lm, E3 // 3)


def residual_normalize_torch(x, a):
    """residual_normalize with torch ops, any dtype and device"""
    return F.normalize(x + a, dim=-1)


# ------------------------------------------------------------------------------------------------------------------ the input stage
INPUT_MODES = ("torch", "fused")


def _stage_layout(src_width, groups, packs):
    """checks of input_stage / input_stage_torch that need no device -> (packs as a tuple of tuples, per group (pack, first column))"""
    n = len(groups)
    packs = (tuple(range(n)),) if packs is None else tuple(tuple(int(i) for i in p) for p in packs)
    if sorted(i for p in packs for i in p) != list(range(n)) or not all(packs):
        raise ValueError(f"input_stage: packs is a partition of the group indices 0..{n - 1}, got {packs}")
    place = {}
    for pi, p in enumerate(packs):
        c = 0
        for i in p:
            place[i] = (pi, c)
            c += groups[i][0].shape[0]
    for w, b, segs in groups:
        k = sum(ln for _, ln in segs)
        if w.dim() != 2 or w.shape[1] != k or tuple(b.shape) != (w.shape[0],):
            raise ValueError(f"input_stage: a group is (weight [n_out, K], bias [n_out], segments of K columns in all), got {tuple(w.shape)}, "
                             f"{tuple(b.shape)} and K = {k}")
        if any(c0 < 0 or ln < 1 or c0 + ln > src_width for c0, ln in segs):
            raise ValueError(f"input_stage: a segment of {tuple(segs)} reaches outside the source's {src_width} columns")
    return packs, place


class _InputStage(torch.autograd.Function):
    """forward: hh_input_stage_forward into the packs; backward: hh_input_stage_backward from the kept src and packs (d_w, d_b only)"""

    @staticmethod
    def forward(ctx, src, segments, packs, place, *wb):
        n = len(segments)
        ld = src.shape[-1]
        R = src.numel() // ld
        ws, bs = [t.detach().contiguous() for t in wb[:n]], [t.detach().contiguous() for t in wb[n:]]
        widths = [sum(ws[i].shape[0] for i in p) for p in packs]
        outs = [torch.empty(tuple(src.shape[:-1]) + (wd,), dtype=torch.float32, device=src.device) for wd in widths]
        io = (L.HHInputGroup * n)()
        for i, segs in enumerate(segments):
            g, (pi, c) = io[i], place[i]
            g.n_out, g.n_seg = ws[i].shape[0], len(segs)
            for s, (c0, ln) in enumerate(segs):
                g.seg_col[s], g.seg_len[s] = c0, ln
            g.w, g.b = ws[i].data_ptr(), bs[i].data_ptr()
            g.y, g.y_ld = outs[pi].data_ptr() + 4 * c, widths[pi]
        L.check(L.lib().hh_input_stage_forward(R, _p(src), ld, ld, n, io, _stream(src.device)))
        ctx.io, ctx.place, ctx.n_packs, ctx.shapes = io, place, len(packs), [(w.shape, w.device) for w in ws]
        ctx.save_for_backward(src, *outs)
        ctx.keep = (ws, bs)        # io holds their addresses
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *d_outs):
        src, *outs = ctx.saved_tensors
        n, io = len(ctx.shapes), ctx.io
        ld = src.shape[-1]
        R = src.numel() // ld
        dev = src.device
        d_outs = [torch.zeros_like(o) if d is None else d.contiguous() for d, o in zip(d_outs, outs)]
        d_ws = [torch.empty(tuple(shp), dtype=torch.float32, device=dev) for shp, _ in ctx.shapes]
        d_bs = [torch.empty((shp[0],), dtype=torch.float32, device=dev) for shp, _ in ctx.shapes]
        for i in range(n):
            pi, c = ctx.place[i]
            io[i].y, io[i].y_ld = outs[pi].data_ptr() + 4 * c, outs[pi].shape[-1]
            io[i].d_y, io[i].d_y_ld = d_outs[pi].data_ptr() + 4 * c, d_outs[pi].shape[-1]
            io[i].d_w, io[i].d_b = d_ws[i].data_ptr(), d_bs[i].data_ptr()
        nbytes = C.c_int64()
        lib = L.lib()
        L.check(lib.hh_input_stage_scratch_bytes(n, io, R, C.byref(nbytes)))
        scratch = torch.empty((nbytes.value // 4,), dtype=torch.float32, device=dev)
        L.check(lib.hh_input_stage_backward(R, _p(src), ld, ld, n, io, _p(scratch), nbytes.value, _stream(dev)))
        return (None, None, None, None) + tuple(d_ws) + tuple(d_bs)


def input_stage(src, groups, packs=None):
    """What a network does in front of shared_layer, fused (hh_input_stage_forward / hh_input_stage_backward, include/hh_learner.h):
    G <= 4 layers y_g = tanh(W_g gather_g(src) + b_g) from one source, one launch forward and two backward.
    src f32 [..., ld], CUDA, contiguous (an observation or a critic row; no gradient flows into it).  groups: a sequence of
    (weight [n_out, K], bias [n_out], segments), segments = ((first column, length), ...): the layer's input is these column runs of a
    source row side by side, K columns in all.  packs: a partition of the group indices, each pack one output tensor
    [..., sum of its groups' n_out] with its groups side by side in the order given; default one pack of all groups.
    -> a tuple of tensors, one per pack.  Differentiable with respect to every weight and bias (first order).  No host
    synchronisation; a missing library or GPU is an error."""
    _need_gpu("input_stage")
    _fused_input("input_stage", src, "src")
    for w, b, _ in groups:
        if not (w.is_cuda and b.is_cuda and w.dtype == torch.float32 and b.dtype == torch.float32 and w.device == src.device and b.device == src.device):
            raise ValueError("input_stage: weights and biases are float32 CUDA tensors on the source's device (the torch-op form is input_stage_torch)")
    if src.dim() < 1 or not 1 <= len(groups) <= L.INSTAGE_MAX_GROUPS:
        raise ValueError(f"input_stage: src is [..., ld] and there are 1 .. {L.INSTAGE_MAX_GROUPS} groups")
    segments = tuple(tuple((int(c0), int(ln)) for c0, ln in segs) for _, _, segs in groups)
    packs, place = _stage_layout(src.shape[-1], [(w, b, sg) for (w, b, _), sg in zip(groups, segments)], packs)
    if (any(not 1 <= len(sg) <= L.INSTAGE_MAX_SEGS or sum(ln for _, ln in sg) > L.INSTAGE_MAX_K for sg in segments)
            or sum(w.shape[0] for w, _, _ in groups) > L.INSTAGE_MAX_OUT):
        raise ValueError(f"input_stage: at most {L.INSTAGE_MAX_SEGS} segments and {L.INSTAGE_MAX_K} inputs per group, {L.INSTAGE_MAX_OUT} outputs in all")
    return _InputStage.apply(src, segments, packs, place, *[w for w, _, _ in groups], *[b for _, b, _ in groups])


def input_stage_torch(src, groups, packs=None):
    """input_stage with torch ops, any dtype and device (the A/B partner, and the modules' own front restated): per group the column runs
    sliced and concatenated, F.linear, tanh; per pack the results concatenated"""
    packs, _ = _stage_layout(src.shape[-1], groups, packs)
    ys = []
    for w, b, segs in groups:
        runs = [src[..., c0:c0 + ln] for c0, ln in segs]
        ys.append(torch.tanh(F.linear(runs[0] if len(runs) == 1 else torch.cat(runs, dim=-1), w, b)))
    return tuple(ys[p[0]] if len(p) == 1 else torch.cat([ys[i] for i in p], dim=-1) for p in packs)


def stage_layers(kind):
    """the modules of TrainableNet(kind) that hold the stages' parameters, in the order of stage_tables' groups"""
    names = tuple(f"inp{i + 1}" for i in range(len(PN.INPUTS[kind])))
    return {"actor": names, "critic": ("v1", "v2", "v3") if PN.HAS_ATT[kind] else ("inp1_val",)}


COMMANDER_STAGE_LAYERS = {"actor": ("inp1", "inp2", "inp3", "inp4"), "critic": ("v1", "v2", "v3", "v4")}


def stage_tables(kind):
    """the input stages of TrainableNet(kind), derived from PN.INPUTS and PN.CRITIC_DIMS -> {"actor" | "critic": (segments per layer,
    packs)}: the actor reads the own observation, the critic the [act_own | act_2 | o_own | o_2] row of central_critic_rows; the
    layers are stage_layers(kind)'s"""
    segs = tuple(((c0, c1 - c0),) for c0, c1, _ in PN.INPUTS[kind])
    d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
    own, other = ((a1 + a2, d1), (0, a1)), ((a1 + a2 + d1, d2), (a1, a2))      # [o_own | act_own], [o_2 | act_2]
    if PN.HAS_ATT[kind]:
        return {"actor": (segs, ((0, 1), (2,))), "critic": ((own, other, own + other), ((0, 1), (2,)))}
    return {"actor": (segs, ((0, 1, 2),)), "critic": ((own + other,), ((0,),))}


def commander_stage_tables():
    """stage_tables for CommanderTrainable (layers: COMMANDER_STAGE_LAYERS): the actor reads the 34-wide observation, the critic
    central_critic_rows_hl's [a_own, a_o1, a_o2 | obs_own | obs_o1 | obs_o2] row, v_k = [obs_k | a_k]"""
    v = tuple(((3 + 34 * k, 34), (k, 1)) for k in range(3))
    return {"actor": ((((0, 4),), ((4, 20),), ((24, 10),), ((0, 34),)), ((0, 1, 2), (3,))),
            "critic": (v + (v[0] + v[1] + v[2],), ((0, 1, 2), (3,)))}


def stage_groups(module, names, table):
    """(groups, packs) for input_stage / input_stage_torch from a module's layers `names` and one of stage_tables' (segments, packs)"""
    segs, packs = table
    lin = [getattr(module, nm)._model[0] for nm in names]
    return [(l.weight, l.bias, sg) for l, sg in zip(lin, segs)], packs


# ------------------------------------------------------------------------------------------------------------------ the shared layer
TRUNK_MODES = ("torch", "fused")


def _dense_rows(x):
    """x [..., K] -> (its rows as a 2-D tensor the kernels can read in place, the row stride in floats): a view where the last dimension is
    contiguous and the leading ones collapse to one stride >= K (a column slice of a wider row is read where it lies), else a copy"""
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    if (K > 1 and x2.stride(1) != 1) or (x2.shape[0] > 1 and x2.stride(0) < K):
        x2 = x2.contiguous()
    return x2, (x2.stride(0) if x2.shape[0] > 1 else K)


class _DenseTanh(torch.autograd.Function):
    """forward: hh_dense_tanh_forward over all row blocks; backward: hh_dense_tanh_backward from the kept inputs and outputs"""

    @staticmethod
    def forward(ctx, weight, bias, *xs):
        N, K = weight.shape
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        flat = [_dense_rows(x.detach())[0] for x in xs]
        ys = [torch.empty(tuple(x.shape[:-1]) + (N,), dtype=torch.float32, device=x.device) for x in xs]
        io = (L.HHDenseSrc * len(xs))()
        for i, (x2, y) in enumerate(zip(flat, ys)):
            io[i].n_rows, io[i].x, io[i].ld, io[i].y = x2.shape[0], x2.data_ptr(), _dense_rows(x2)[1], y.data_ptr()
        scratch = torch.empty((L.DENSE_FWD_SCRATCH_BYTES // 4,), dtype=torch.int32, device=w.device)
        L.check(L.lib().hh_dense_tanh_forward(K, N, len(xs), io, _p(w), _p(b), _p(scratch), L.DENSE_FWD_SCRATCH_BYTES, _stream(w.device)))
        ctx.save_for_backward(w, *flat, *ys)
        ctx.n, ctx.x_shapes = len(xs), [tuple(x.shape) for x in xs]
        return tuple(ys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *d_ys):
        w, *rest = ctx.saved_tensors
        n = ctx.n
        flat, ys = rest[:n], rest[n:]
        N, K = w.shape
        dev = w.device
        d_ys = [torch.zeros_like(y) if d is None else d.contiguous() for d, y in zip(d_ys, ys)]
        d_xs = [torch.empty(shp, dtype=torch.float32, device=dev) for shp in ctx.x_shapes]
        d_w, d_b = torch.empty_like(w), torch.empty((N,), dtype=torch.float32, device=dev)
        io = (L.HHDenseSrc * n)()
        for i in range(n):
            x2 = flat[i]
            io[i].n_rows, io[i].x, io[i].ld = x2.shape[0], x2.data_ptr(), _dense_rows(x2)[1]
            io[i].y, io[i].d_y, io[i].d_x = ys[i].data_ptr(), d_ys[i].data_ptr(), d_xs[i].data_ptr()
        if all(x2.shape[0] == 0 for x2 in flat):
            return (torch.zeros_like(w), torch.zeros_like(d_b)) + tuple(d_xs)
        nbytes = C.c_int64()
        lib = L.lib()
        L.check(lib.hh_dense_tanh_scratch_bytes(K, N, n, io, C.byref(nbytes)))
        scratch = torch.empty((nbytes.value // 4,), dtype=torch.float32, device=dev)
        L.check(lib.hh_dense_tanh_backward(K, N, n, io, _p(w), _p(d_w), _p(d_b), _p(scratch), nbytes.value, _stream(dev)))
        return (d_w, d_b) + tuple(d_xs)


def _dense_args(xs):
    """one tensor or a sequence of them -> (list, whether a single tensor came in)"""
    single = isinstance(xs, torch.Tensor)
    return ([xs] if single else list(xs)), single


def dense_tanh(xs, weight, bias):
    """tanh(F.linear(x, weight, bias)) for one or two tensors x [..., K] that go through the same layer, fused and on the matrix cores
    (hh_dense_tanh_forward / hh_dense_tanh_backward, include/hh_learner.h): split-fp16 MFMA with float32 accumulators, within
    (4 * 2^-22 + (n + 2) * 2^-24) |A| |B| of float64 per product.  xs: a float32 CUDA tensor or a sequence of one or two (the actor's
    and the critic's rows: one call serves both); the last dimension may be a column slice of a wider row.  weight f32 [N, K], bias f32
    [N], 1 <= K, N <= 512, on the same device.  -> a tensor [..., N] per input (a single tensor for a single tensor).  Differentiable
    with respect to every input, the weight and the bias (first order); the same inputs give the same bytes.  No host synchronisation;
    a missing library or GPU is an error."""
    _need_gpu("dense_tanh")
    xs, single = _dense_args(xs)
    if not 1 <= len(xs) <= L.DENSE_MAX_SRC:
        raise ValueError(f"dense_tanh: one .. {L.DENSE_MAX_SRC} inputs, got {len(xs)}")
    for what, t in [("x", x) for x in xs] + [("weight", weight), ("bias", bias)]:
        if not (t.is_cuda and t.dtype == torch.float32):
            raise ValueError(f"dense_tanh: {what} is a contiguous float32 CUDA tensor (the torch-op form for other dtypes and devices is dense_tanh_torch)")
    if (weight.dim() != 2 or tuple(bias.shape) != (weight.shape[0],) or not all(1 <= d <= L.DENSE_MAX_DIM for d in weight.shape)
            or any(x.dim() < 1 or x.shape[-1] != weight.shape[1] or x.device != weight.device for x in xs) or bias.device != weight.device):
        raise ValueError(f"dense_tanh: weight [N, K], bias [N], inputs [..., K] on one device with 1 <= K, N <= {L.DENSE_MAX_DIM}, got "
                         f"{tuple(weight.shape)}, {tuple(bias.shape)} and {[tuple(x.shape) for x in xs]}")
    ys = _DenseTanh.apply(weight, bias, *xs)
    return ys[0] if single else ys


def dense_tanh_torch(xs, weight, bias):
    """dense_tanh with torch ops, any dtype and device (the A/B partner): tanh(F.linear(x, weight, bias)) per input"""
    xs, single = _dense_args(xs)
    ys = tuple(torch.tanh(F.linear(x, weight, bias)) for x in xs)
    return ys[0] if single else ys


def _trunk_mode(trunk):
    if trunk not in TRUNK_MODES:
        raise ValueError(f"trunk is one of {TRUNK_MODES}, got {trunk!r}")
    return trunk


# ------------------------------------------------------------------------------------------------------------------ the heads and the loss
HEADS_MODES = ("torch", "fused")


def _heads_mode(heads, trunk="torch"):
    if heads not in HEADS_MODES:
        raise ValueError(f"heads is one of {HEADS_MODES}, got {heads!r}")
    if heads == "fused" and trunk == "fused":
        raise ValueError('heads="fused" needs trunk="torch": dense_tanh has the tanh inside, so there are no pre-activations to hand over')
    return heads


def _heads_keyword(init):
    """a learner's __init__ with one more argument, `heads`, that can only be given by keyword: it is taken off before `init` runs and
    kept as `self._heads_arg`, which `init` hands to _learner_options for validation in its place.  The constructors' own signatures stay
    as they are — grad_clip their last parameter, so no positional caller moves — and functools.wraps keeps them what introspection
    and help() show; the docstrings describe `heads`."""
    @functools.wraps(init)
    def __init__(self, *args, heads="torch", **kw):
        self._heads_arg = heads
        init(self, *args, **kw)
    return __init__


class _HeadsLoss(torch.autograd.Function):
    """forward: hh_heads_loss (tanh, both heads, the loss, and all six gradients in one pass); backward: the kept gradients, times the
    incoming one where the call asked for that"""

    @staticmethod
    def forward(ctx, za, zc, w_act, b_act, w_val, b_val, old_logits, actions, old_logp, adv, target, mask, n_valid, prm, scale_grad):
        dev = za.device
        R = za.numel() // L.HEADS_K
        e = lambda t: torch.empty_like(t, memory_format=torch.contiguous_format)
        stats = torch.empty((len(L.PPO_STATS),), dtype=torch.float64, device=dev)
        grads = (e(za), e(zc), e(w_act), e(b_act), e(w_val), e(b_val))
        nbytes = C.c_int64()
        lib = L.lib()
        L.check(lib.hh_heads_loss_scratch_bytes(R, prm.n_comp, C.byref(nbytes)))
        scratch = torch.empty((nbytes.value // 8,), dtype=torch.float64, device=dev)
        L.check(lib.hh_heads_loss(R, _p(za), _p(zc), _p(w_act), _p(b_act), _p(w_val), _p(b_val), _p(old_logits), _p(actions), _p(old_logp), _p(adv),
                                  _p(target), _p(mask), _p(n_valid), C.byref(prm), _p(stats), *[_p(g) for g in grads], None, None, _p(scratch),
                                  nbytes.value, _stream(dev)))
        ctx.save_for_backward(*grads)
        ctx.scale_grad = scale_grad
        ctx.mark_non_differentiable(stats)
        return stats[0].float(), stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total, g_stats):
        grads = list(ctx.saved_tensors)
        if ctx.scale_grad:
            torch._foreach_mul_(grads, g_total)
        return tuple(grads) + (None,) * 9


def _head_params(head):
    """(weight, bias) of an output head given as that pair, as an nn.Linear or as a module that keeps one in `_model.0` (_FC)"""
    if isinstance(head, (tuple, list)):
        return head[0], head[1]
    lin = head._model[0] if hasattr(head, "_model") else head
    return lin.weight, lin.bias


def _flat_heads_batch(R, batch, n_comp, device):
    """_flat_batch / _flat_batch_cat without the learner's outputs: the batch columns as contiguous rows for R rows of pre-activations"""
    old_ld, act_w = (CMD_LD, None) if n_comp == 1 else (OLD_LD, 4)
    col = lambda k, dt, w=None: batch[k].reshape((R,) if w is None else (R, w)).to(dt).contiguous()
    mask = batch.get("mask")
    mask = None if mask is None else col("mask", torch.uint8)
    n_valid = batch.get("n_valid")
    if n_valid is None:
        n_valid = (torch.full((1,), R, dtype=torch.int32, device=device) if mask is None else mask.ne(0).sum(dtype=torch.int32).reshape(1))
    return (col("old_logits", torch.float32, old_ld), col("actions", torch.int8, act_w), col("old_logp", torch.float32), col("adv", torch.float32),
            col("target", torch.float32), mask, n_valid.reshape(1))


def heads_loss(za, zc, act_out, val_out, batch, *, n_comp, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2,
               scale_grad=True):
    """Everything behind shared_layer's GEMM in one fused pass (hh_heads_loss, include/hh_learner.h): h = tanh(za), y = tanh(zc),
    logits = act_out(h), vf = val_out(y), then ppo_loss (n_comp 4 | 3) or ppo_loss_categorical (n_comp 1) — and, in the same pass, the
    gradient of the total with respect to za, zc and the four head parameters.
    za, zc f32 [..., 500]: shared_layer's outputs for the actor's and the critic's rows, bias added, before tanh (TrainableNet.pre_heads,
    CommanderTrainable.pre_heads); contiguous CUDA tensors of one shape.  act_out, val_out: the heads as (weight, bias) pairs, nn.Linear
    or _FC modules: [n_out, 500], [n_out] and [1, 500], [1], contiguous float32 on the same device.  batch: as ppo_loss /
    ppo_loss_categorical take it, over za's leading shape.
    -> (total loss: float32 0-d tensor, differentiable with respect to za, zc and the four head parameters (first order, ONE backward
        per call); stats f64 [6] as ppo_loss).
    The six gradients are computed by the forward call and kept.  scale_grad=True (the default) multiplies them by the gradient that
    arrives at `total`, in place, with one multi-tensor launch, so the function is correct under any upstream gradient;
    scale_grad=False hands them over as they are, which is right exactly when that gradient is 1 — `total.backward()`, what the learners
    call — and saves the pass over two [R, 500] tensors.  No host synchronisation; a missing library or GPU is an error."""
    _need_gpu("heads_loss")
    (w_act, b_act), (w_val, b_val) = _head_params(act_out), _head_params(val_out)
    n_out = L.HEADS_N_OUT.get(int(n_comp))
    if n_out is None:
        raise ValueError(f"heads_loss: n_comp is one of {sorted(L.HEADS_N_OUT)}, got {n_comp!r}")
    for what, t in (("za", za), ("zc", zc), ("act_out's weight", w_act), ("act_out's bias", b_act), ("val_out's weight", w_val), ("val_out's bias", b_val)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == za.device):
            raise ValueError(f"heads_loss: {what} is a contiguous float32 CUDA tensor on za's device (the torch-op form for other dtypes and devices is heads_loss_torch)")
    if (za.dim() < 1 or za.shape[-1] != L.HEADS_K or za.shape != zc.shape or za.numel() == 0 or tuple(w_act.shape) != (n_out, L.HEADS_K)
            or tuple(b_act.shape) != (n_out,) or w_val.numel() != L.HEADS_K or b_val.numel() != 1):
        raise ValueError(f"heads_loss: za and zc [..., {L.HEADS_K}] of one shape with at least one row, act_out [{n_out}, {L.HEADS_K}] + [{n_out}], val_out "
                         f"[1, {L.HEADS_K}] + [1]; got {tuple(za.shape)}, {tuple(zc.shape)}, {tuple(w_act.shape)}, {tuple(b_act.shape)}, "
                         f"{tuple(w_val.shape)}, {tuple(b_val.shape)}")
    flat = _flat_heads_batch(za.numel() // L.HEADS_K, batch, int(n_comp), za.device)
    prm = L.HHPpoLossParams(n_comp=int(n_comp), reserved0=0, clip_param=clip_param, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff,
                            entropy_coeff=entropy_coeff, kl_coeff=kl_coeff, reserved1=0.0)
    return _HeadsLoss.apply(za, zc, w_act, b_act, w_val, b_val, *flat, prm, bool(scale_grad))


def heads_loss_torch(za, zc, act_out, val_out, batch, *, n_comp, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0,
                     kl_coeff=0.2, scale_grad=True):
    """heads_loss with torch ops on any device, in za's dtype (the A/B partner): tanh, F.linear, then ppo_loss_torch (n_comp 4 | 3) or
    ppo_loss_categorical_torch (n_comp 1); autograd does the backward, so scale_grad has nothing to switch"""
    (w_act, b_act), (w_val, b_val) = _head_params(act_out), _head_params(val_out)
    logits = F.linear(torch.tanh(za), w_act, b_act)
    vf = F.linear(torch.tanh(zc), w_val.reshape(1, -1), b_val.reshape(1)).squeeze(-1)
    kw = dict(clip_param=clip_param, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff, entropy_coeff=entropy_coeff, kl_coeff=kl_coeff)
    if int(n_comp) == 1:
        return ppo_loss_categorical_torch(logits, vf, batch, **kw)
    return ppo_loss_torch(logits, vf, batch, n_comp=n_comp, **kw)


# ------------------------------------------------------------------------------------------------------------------ the networks
class _FC(nn.Module):
    """a linear layer under the reference's parameter names (RLlib's SlimFC keeps its nn.Linear in `_model.0`)"""

    def __init__(self, n_in, n_out):
        super().__init__()
        self._model = nn.Sequential(nn.Linear(n_in, n_out))

    def forward(self, x):
        return self._model(x)


class TrainableNet(nn.Module):
    """One of the four trainable architectures (policy_nets: Fight1 / Fight2 / Esc1 / Esc2) in training form, written from the architecture
    tables of policy_nets.py; parameters named and shaped exactly as actor_keys(kind) + critic_keys(kind), so `state_dict()` goes
    straight into `PolicyBank.refresh`.

    forward(obs_own, critic_row) -> (logits, value):
      fight kinds:  obs_own [S, L, >= OBS_DIM] and critic_row [S, L, 57] are chunks of L consecutive steps of one agent; att_act / att_val
                    attend over the L steps of a chunk with no padding mask (a zero-padded row is a key like any other), then
                    normalize(x + att) per row.  2-D inputs [R, ...] are R chunks of length 1 — the sampler's forward.
                    -> logits [S, L, 26 | 24], value [S, L]
      escape kinds: rows [..., >= OBS_DIM], [..., 66] -> logits [..., 26 | 24], value [...]
    critic_row is rollout.central_critic_rows' layout: [own act | friend's act | own obs | friend's obs].

    attention = "torch" (the default) runs att_act / att_val through nn.MultiheadAttention and F.normalize.  "fused" (fight kinds only,
    float32 on the GPU) keeps the two projections as GEMMs and runs what lies between and after them through chunk_attention and
    residual_normalize; the nn.MultiheadAttention objects stay the parameter holders, so state_dict() is the same either way.

    inputs = "torch" (the default) slices, concatenates and runs inp1..inp3 and v1..v3 / inp1_val one by one.  "fused" (any kind, float32
    on the GPU) runs each side's layers as ONE input_stage that reads obs_own / critic_row as they are and writes the concatenated
    activations (stage_tables(kind)); the _FC modules stay the parameter holders.  Independent of `attention`.

    trunk = "torch" (the default) applies shared_layer and tanh to the actor's and to the critic's rows one after the other.  "fused" (any
    kind, float32 on the GPU) runs both through ONE dense_tanh (split-fp16 MFMA, bias and tanh in its epilogue); the _FC module stays
    the parameter holder, so state_dict(), tie and publish are the same, and a tied layer receives gradients only from the module that
    ran.  Independent of `attention` and `inputs`.

    heads = "torch" (the default) changes nothing.  "fused" (any kind, trunk="torch") marks the module for the learners' fused tail:
    `pre_heads(obs_own, critic_row) -> (za, zc)` is everything up to shared_layer's pre-activations, and heads_loss takes it from there
    with this module's act_out and val_out.  `forward` is the same code and returns the same bytes in both modes (the sampler-form
    forward, old_logits and the golden-file tests use it); state_dict() is the same."""

    def __init__(self, kind, attention="torch", inputs="torch", trunk="torch", heads="torch"):
        super().__init__()
        self.kind = int(kind)
        self.trunk = _trunk_mode(trunk)
        self.heads = _heads_mode(heads, self.trunk)
        if inputs not in INPUT_MODES:
            raise ValueError(f"inputs is one of {INPUT_MODES}, got {inputs!r}")
        self.inputs = inputs
        if attention not in ATTENTION_MODES:
            raise ValueError(f"attention is one of {ATTENTION_MODES}, got {attention!r}")
        if attention == "fused" and not PN.HAS_ATT[self.kind]:
            raise ValueError(f'attention="fused": {PN.KIND_NAMES[self.kind]} has no attention')
        self.attention = attention
        for i, (c0, c1, w) in enumerate(PN.INPUTS[kind]):
            setattr(self, f"inp{i + 1}", _FC(c1 - c0, w))
        self.shared_layer = _FC(500, 500)
        self.act_out = _FC(500, PN.N_OUT[kind])
        d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
        if PN.HAS_ATT[kind]:
            self.att_act = nn.MultiheadAttention(100, 2, batch_first=True)
            self.v1, self.v2, self.v3 = _FC(d1 + a1, 175), _FC(d2 + a2, 175), _FC(d1 + a1 + d2 + a2, 150)
            self.att_val = nn.MultiheadAttention(150, 2, batch_first=True)
        else:
            self.inp1_val = _FC(d1 + a1 + d2 + a2, 500)
        self.val_out = _FC(500, 1)

    @staticmethod
    def _attend_fused(att, h):
        """normalize(h + att(h, h, h)) with the in- and out-projection as GEMMs and the rest in two fused launches each way"""
        qkv = F.linear(h, att.in_proj_weight, att.in_proj_bias)
        out = F.linear(chunk_attention(qkv), att.out_proj.weight, att.out_proj.bias)
        return residual_normalize(h, out)

    @staticmethod
    def _attend_torch(att, h):
        """normalize(h + att(h, h, h)) through nn.MultiheadAttention and F.normalize"""
        a, _ = att(h, h, h, need_weights=False)
        return F.normalize(h + a, dim=-1)

    def _front(self, obs_own, critic_row):
        """-> (h, y, flat): the actor's and the critic's rows as shared_layer sees them; flat: 2-D fight inputs, run as chunks of length 1"""
        kind = self.kind
        flat = PN.HAS_ATT[kind] and obs_own.dim() == 2
        if flat:
            obs_own, critic_row = obs_own[:, None], critic_row[:, None]
        # the front: h and y are the pieces that shared_layer sees side by side; a fight kind's last piece goes through its attention block first
        if self.inputs == "fused":
            tables, layers = stage_tables(kind), stage_layers(kind)
            h = list(input_stage(obs_own.contiguous(), *stage_groups(self, layers["actor"], tables["actor"])))
            y = list(input_stage(critic_row.contiguous(), *stage_groups(self, layers["critic"], tables["critic"])))
        else:
            d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
            x = obs_own[..., :PN.OBS_DIM[kind]]
            h = [torch.tanh(getattr(self, f"inp{i + 1}")(x[..., c0:c1])) for i, (c0, c1, _) in enumerate(PN.INPUTS[kind])]
            act_own, act_2 = critic_row[..., :a1], critic_row[..., a1:a1 + a2]
            o_own, o_2 = critic_row[..., a1 + a2:a1 + a2 + d1], critic_row[..., a1 + a2 + d1:]
            v1, v2 = torch.cat((o_own, act_own), dim=-1), torch.cat((o_2, act_2), dim=-1)
            v3 = torch.cat((v1, v2), dim=-1)
            if PN.HAS_ATT[kind]:
                y = [torch.cat((torch.tanh(self.v1(v1)), torch.tanh(self.v2(v2))), dim=-1), torch.tanh(self.v3(v3))]
            else:
                y = [torch.tanh(self.inp1_val(v3))]
        if PN.HAS_ATT[kind]:
            attend = self._attend_fused if self.attention == "fused" else self._attend_torch
            h[-1], y[-1] = attend(self.att_act, h[-1]), attend(self.att_val, y[-1])
        h, y = (t[0] if len(t) == 1 else torch.cat(t, dim=-1) for t in (h, y))
        return h, y, flat

    def pre_heads(self, obs_own, critic_row):
        """forward up to shared_layer's pre-activations -> (za, zc) [..., 500] (fight kinds: [S, L, 500], or [R, 500] for 2-D inputs):
        what heads_loss takes.  trunk="torch" only: dense_tanh keeps no pre-activation."""
        if self.trunk == "fused":
            raise ValueError('pre_heads needs trunk="torch": dense_tanh has the tanh inside')
        h, y, flat = self._front(obs_own, critic_row)
        za, zc = self.shared_layer(h), self.shared_layer(y)
        return (za.squeeze(1), zc.squeeze(1)) if flat else (za, zc)

    def forward(self, obs_own, critic_row):
        h, y, flat = self._front(obs_own, critic_row)
        if self.trunk == "fused":
            lin = self.shared_layer._model[0]
            h, y = dense_tanh((h, y), lin.weight, lin.bias)
            logits, value = self.act_out(h), self.val_out(y).squeeze(-1)
        else:
            logits = self.act_out(torch.tanh(self.shared_layer(h)))
            value = self.val_out(torch.tanh(self.shared_layer(y))).squeeze(-1)
        if flat:
            logits, value = logits[:, 0], value[:, 0]
        return logits, value

    def load_numpy(self, sd):
        """the weights of a dict of numpy arrays keyed like state_dict() (policy_nets.random_weights + random_critic_weights)"""
        own = self.state_dict()
        with torch.no_grad():
            for k, v in sd.items():
                own[k].copy_(torch.as_tensor(np.asarray(v)))
        return self


def tie(modules):
    """make every module hold the FIRST one's shared_layer: ONE parameter object for all (models/ac_models_hetero.py:22: one
    module-level SHARED_LAYER serves Fight1, Fight2, Esc1 and Esc2)"""
    for m in modules[1:]:
        m.shared_layer = modules[0].shared_layer
    return modules


# ------------------------------------------------------------------------------------------------------------------ batch geometry
def cut_chunks(ep_start, ep_len, max_seq_len):
    """chop_into_sequences (rllib/policy/rnn_sequencing.py) on an episode table: every episode's rows cut into chunks of max_seq_len
    (L, ..., L, remainder).  ep_start / ep_len integer tensors [E] (any device) -> (seq_start, seq_len) int64 [S], episodes in order"""
    Lm = int(max_seq_len)
    ep_start, ep_len = ep_start.long(), ep_len.long()
    n_ch = (ep_len + (Lm - 1)) // Lm
    seq_ep = torch.repeat_interleave(torch.arange(ep_len.numel(), device=ep_len.device), n_ch)
    first = torch.cumsum(n_ch, dim=0) - n_ch
    j = torch.arange(seq_ep.numel(), device=ep_len.device) - first[seq_ep]
    return ep_start[seq_ep] + j * Lm, torch.clamp(ep_len[seq_ep] - j * Lm, max=Lm)


def pad_chunks(col, seq_start, seq_len, max_seq_len):
    """pad_batch_to_sequences_of_same_size on one column [R, ...]: -> [S, L, ...], zero beyond each chunk's seq_len"""
    Lm = int(max_seq_len)
    t = torch.arange(Lm, device=col.device)
    mask = t[None, :] < seq_len[:, None]
    idx = torch.where(mask, seq_start[:, None] + t[None, :], torch.zeros_like(seq_start[:, None]))
    out = col[idx.reshape(-1)].reshape((idx.shape[0], Lm) + tuple(col.shape[1:]))
    return out * mask.reshape(mask.shape + (1,) * (col.dim() - 1)).to(col.dtype)


def chunk_mask(seq_len, max_seq_len):
    """sequence_mask: bool [S, L], the unpadded rows"""
    return torch.arange(int(max_seq_len), device=seq_len.device)[None, :] < seq_len[:, None]


def minibatch_partition(seq_len, sgd_minibatch_size):
    """the chunks (escape: rows, seq_len all 1) in order, split into consecutive minibatches of at least sgd_minibatch_size unpadded rows
    (the last one holds what is left).  seq_len: host integers [S] -> list of (first chunk, last chunk + 1)"""
    csum = np.cumsum(np.asarray(seq_len, dtype=np.int64))
    out, s0, base = [], 0, 0
    S = len(csum)
    while s0 < S:
        s1 = int(np.searchsorted(csum, base + int(sgd_minibatch_size), side="left")) + 1
        s1 = min(s1, S)
        out.append((s0, s1))
        base, s0 = int(csum[s1 - 1]), s1
    return out


def minibatch_order(n, seed, update, policy, sgd_pass):
    """the order in which one pass visits its n minibatches: keyed by (seed, update count, policy, pass), so two learners with the same
    seed visit the same order.  (RLlib shuffles with the unseeded global numpy generator: its order is not reproducible at all.)"""
    return np.random.default_rng([int(seed), int(update), int(policy), int(sgd_pass)]).permutation(int(n))


def sequence_order(n, seed, update, policy, sgd_pass):
    """shuffle_sequences: the order of one pass's n chunks (escape: rows), a permutation keyed by (seed, update count, policy, pass) and a
    fifth entry 1 that keeps it a different stream from minibatch_order's -> int64 [n]"""
    return np.random.default_rng([int(seed), int(update), int(policy), int(sgd_pass), 1]).permutation(int(n))


def shuffled_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy):
    """shuffle_sequences: the minibatch steps of one update over S chunks of these lengths (host integers [S]) as hh_minibatch_stage_gather's
    two tables -> (order int32 [num_sgd_iter * S], sched int32 [n_steps, 4]).  Pass p owns order[p S:(p + 1) S] = sequence_order(S, seed,
    update, policy, p); its minibatches are minibatch_partition's of the lengths in that order — consecutive runs of at least
    sgd_minibatch_size unpadded rows, the last one what is left — visited in position order.  A schedule row is (o0, o1, unpadded rows, 0)
    with o0, o1 absolute positions in order; the passes may differ in their number of steps."""
    seq_len = np.asarray(seq_len, dtype=np.int64).reshape(-1)
    S, passes = len(seq_len), int(num_sgd_iter)
    if passes * S > np.iinfo(np.int32).max:
        raise ValueError(f"shuffled_schedule: the order table of {passes} passes over {S} chunks does not fit int32 positions")
    order = np.empty((max(passes, 0) * S,), dtype=np.int32)
    rows = []
    for p in range(passes):
        perm = sequence_order(S, seed, update, policy, p)
        order[p * S:(p + 1) * S] = perm
        lens = seq_len[perm]
        csum = np.concatenate([[0], np.cumsum(lens)])
        rows += [(p * S + s0, p * S + s1, int(csum[s1] - csum[s0]), 0) for s0, s1 in minibatch_partition(lens, sgd_minibatch_size)]
    return order, np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def update_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy, shuffle):
    """The minibatch steps of one policy's update as the ONE table that every step mode walks row by row, the eager loop on the host and
    the graph's cursor on the device -> (order, sched int32 [n_steps, 4], need).  shuffle False: order is None and sched is
    sequence_schedule's — rows (first chunk, last chunk + 1, unpadded rows, 0), per pass in minibatch_order's order.  True:
    shuffled_schedule's (order, sched), the rows naming positions of order.  need: the chunks of the largest minibatch, the smallest
    staging capacity (1 where there is no minibatch)."""
    if shuffle:
        order, sched = shuffled_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy)
        return order, sched, int((sched[:, 1] - sched[:, 0]).max()) if len(sched) else 1
    parts, sched = sequence_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy)
    return None, sched, max((s1 - s0 for s0, s1 in parts), default=1)


def _shuffle_flag(shuffle_sequences):
    """RLlib's shuffle_sequences: a bool and nothing else (1, "yes" and None are refused)"""
    if not isinstance(shuffle_sequences, bool):
        raise ValueError(f"shuffle_sequences is True or False, got {shuffle_sequences!r}")
    return shuffle_sequences


def kl_coeff_update(kl_coeff, sampled_kl, kl_target):
    """KLCoeffMixin.update_kl (ray/rllib/policy/torch_mixins.py): above 2 x target the coefficient grows by 1.5, below 0.5 x target it halves"""
    if sampled_kl > 2.0 * kl_target:
        return kl_coeff * 1.5
    if sampled_kl < 0.5 * kl_target:
        return kl_coeff * 0.5
    return kl_coeff


def standardize(adv):
    """standardized (ray/rllib/utils/sgd.py) over a policy's whole batch: (x - mean) / max(1e-4, std), population std"""
    return (adv - adv.mean()) / torch.clamp(adv.std(unbiased=False), min=1e-4)


# ------------------------------------------------------------------------------------------------------------------ the replayable step
OPTIMIZER_MODES = ("torch", "fused")
STEP_MODES = ("eager", "graph")
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8      # torch.optim.Adam's defaults, which the learners use


def _optimizer_mode(optimizer):
    if optimizer not in OPTIMIZER_MODES:
        raise ValueError(f"optimizer is one of {OPTIMIZER_MODES}, got {optimizer!r}")
    return optimizer


def _step_mode(step, optimizer):
    if step not in STEP_MODES:
        raise ValueError(f"step is one of {STEP_MODES}, got {step!r}")
    if step == "graph" and optimizer != "fused":
        raise ValueError(f'step="graph" needs optimizer="fused" (torch.optim.Adam keeps its step count on the host), got optimizer={optimizer!r}')
    return step


def _grad_clip(grad_clip):
    """RLlib's grad_clip: None (no clipping) or a finite float > 0, the largest global L2 norm of one optimizer's gradients"""
    if grad_clip is None:
        return None
    if isinstance(grad_clip, bool) or not isinstance(grad_clip, (int, float)) or not (math.isfinite(grad_clip) and grad_clip > 0):
        raise ValueError(f"grad_clip is None or a finite float > 0, got {grad_clip!r}")
    return float(grad_clip)


def _adam_desc(who, params, grads, ms, vs, dev):
    desc = (L.HHAdamTensor * max(len(params), 1))()
    for i, (p, g, m, v) in enumerate(zip(params, grads, ms, vs)):
        for what, x in (("a parameter", p), ("a gradient", g), ("a first moment", m), ("a second moment", v)):
            if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape == p.shape and x.device == dev):
                raise ValueError(f"{who}: {what} is a contiguous float32 CUDA tensor of its parameter's shape on t's device (the torch-op form "
                                 f"is {who}_torch)")
        desc[i].p, desc[i].g, desc[i].m, desc[i].v, desc[i].n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    return desc


def _is_clip(clip, dev):
    return (isinstance(clip, torch.Tensor) and clip.is_cuda and clip.dtype == torch.float64 and clip.is_contiguous()
            and clip.numel() == L.CLIP_OUT and clip.device == dev)


def grad_norm_scratch(grads):
    """the scratch of grad_norm for these gradients (or tensors of their shapes): float64 [tiles], one slot per tensor and 4096 elements"""
    tiles = sum((g.numel() + 4095) // 4096 for g in grads)
    return torch.empty((max(tiles, 1),), dtype=torch.float64, device=grads[0].device if len(grads) else "cuda")


def grad_norm(grads, max_norm, clip=None, cursor=None, table=None, scratch=None):
    """The global L2 norm of a list of gradients and torch.nn.utils.clip_grad_norm_'s coefficient for it, on the device (hh_grad_norm,
    include/hh_learner.h): grads is a list of contiguous float32 CUDA tensors, max_norm a finite float > 0
    -> clip f64 [2] = (norm, min(1, max_norm / (norm + 1e-6))), the tensor given or a new one.  With cursor (int32 [1]) and table (f64 [n])
    the norm also goes to table[cursor] (skipped outside the table; the cursor is only read).  scratch: grad_norm_scratch's (allocated
    when not given).  Float64 sums in a fixed order: the same bytes on every run.  The gradients are not changed: adam_step(clip=...)
    scales them as it reads them.  ceil(n / 64) + 1 launches, no host synchronisation, HIP-graph capturable; a missing library or GPU
    is an error."""
    _need_gpu("grad_norm")
    grads = list(grads)
    if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)) or not (math.isfinite(max_norm) and max_norm > 0):
        raise ValueError(f"grad_norm: max_norm is a finite float > 0, got {max_norm!r}")
    dev = clip.device if clip is not None else (grads[0].device if grads else torch.device("cuda", torch.cuda.current_device()))
    if clip is None:
        clip = torch.empty((L.CLIP_OUT,), dtype=torch.float64, device=dev)
    if not _is_clip(clip, dev):
        raise ValueError("grad_norm: clip is a contiguous float64 [2] CUDA tensor")
    if (cursor is None) != (table is None):
        raise ValueError("grad_norm: cursor and table come together")
    if cursor is not None and not (cursor.is_cuda and cursor.dtype == torch.int32 and cursor.numel() == 1 and cursor.device == dev and table.is_cuda
                                   and table.dtype == torch.float64 and table.dim() == 1 and table.is_contiguous() and table.device == dev):
        raise ValueError("grad_norm: cursor is an int32 [1] and table a contiguous float64 [n] CUDA tensor on clip's device")
    desc = (L.HHAdamTensor * max(len(grads), 1))()
    for i, g in enumerate(grads):
        if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.device == dev):
            raise ValueError("grad_norm: a gradient is a contiguous float32 CUDA tensor on one device (the torch-op form is grad_norm_torch)")
        desc[i].g, desc[i].n = g.data_ptr(), g.numel()
    nbytes = C.c_int64()
    L.check(L.lib().hh_grad_norm_scratch_bytes(len(grads), desc, C.byref(nbytes)))
    if scratch is None:
        scratch = torch.empty((max(nbytes.value // 8, 1),), dtype=torch.float64, device=dev)
    if not (scratch.is_cuda and scratch.dtype == torch.float64 and scratch.is_contiguous() and scratch.device == dev and scratch.numel() * 8 >= nbytes.value):
        raise ValueError(f"grad_norm: scratch is a contiguous float64 CUDA tensor of at least {nbytes.value // 8} elements (grad_norm_scratch)")
    L.check(L.lib().hh_grad_norm(len(grads), desc, float(max_norm), _p(clip), None if cursor is None else _p(cursor), None if table is None else _p(table),
                                 0 if table is None else table.shape[0], _p(scratch), scratch.numel() * 8, _stream(dev)))
    return clip


def grad_norm_torch(grads, max_norm):
    """grad_norm with torch ops, any dtype and device (the A/B partner): float64 throughout -> (norm, coef), two 0-d float64 tensors"""
    grads = list(grads)
    dev = grads[0].device if grads else "cpu"
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for g in grads:
        total = total + g.detach().double().square().sum()
    norm = total.sqrt()
    return norm, torch.clamp(float(max_norm) / (norm + 1e-6), max=1.0)


def adam_step(params, grads, ms, vs, t, *, lr, betas=ADAM_BETAS, eps=ADAM_EPS, clip=None):
    """One step of torch.optim.Adam (amsgrad = False, weight_decay = 0) on a list of tensors, on the device (hh_adam_step, include/hh_learner.h):
    params, grads, ms, vs are lists of contiguous float32 CUDA tensors, shape by shape the same; t is an int32 [1] CUDA tensor holding the
    number of steps taken so far (the step uses t + 1; train_commit advances it).  In place on params, ms and vs.  ceil(n / 64) launches,
    no host synchronisation, HIP-graph capturable; a missing library or GPU is an error.
    clip: grad_norm's float64 [2] CUDA tensor; with it every gradient is read as float32(float64(g) * clip[1]) (hh_adam_step_clipped) — the
    step of clip_grad_norm_ followed by Adam, except that the gradient tensors keep their unscaled values."""
    _need_gpu("adam_step")
    n = len(params)
    if not (len(grads) == len(ms) == len(vs) == n):
        raise ValueError("adam_step: params, grads, ms and vs are lists of one length")
    if not (t.is_cuda and t.dtype == torch.int32 and t.numel() == 1):
        raise ValueError("adam_step: t is an int32 [1] CUDA tensor (the torch-op form is adam_step_torch)")
    desc = _adam_desc("adam_step", params, grads, ms, vs, t.device)
    if clip is None:
        L.check(L.lib().hh_adam_step(n, desc, _p(t), float(lr), float(betas[0]), float(betas[1]), float(eps), _stream(t.device)))
        return
    if not _is_clip(clip, t.device):
        raise ValueError("adam_step: clip is grad_norm's contiguous float64 [2] CUDA tensor on t's device")
    L.check(L.lib().hh_adam_step_clipped(n, desc, _p(t), _p(clip), float(lr), float(betas[0]), float(betas[1]), float(eps), _stream(t.device)))


def adam_step_torch(params, grads, ms, vs, t, *, lr, betas=ADAM_BETAS, eps=ADAM_EPS, clip=None):
    """adam_step with torch ops, any dtype and device (the A/B partner): t is the number of steps taken so far, a Python int or a
    one-element tensor (read on the host); in place on params, ms and vs.  clip: (norm, coef) as grad_norm_torch returns them or a
    two-element tensor; every gradient is read as (float64(g) * coef) rounded to its own dtype, and left as it is"""
    step = int(t) + 1
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    with torch.no_grad():
        if clip is not None:
            grads = [(g.double() * clip[1]).to(g.dtype) for g in grads]
        for p, g, m, v in zip(params, grads, ms, vs):
            m.mul_(b1).add_(g, alpha=1.0 - b1)
            v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
            p.addcdiv_(m, v.sqrt() / bc2 ** 0.5 + eps, value=-(lr / bc1))


def minibatch_schedule(parts, n_valid, num_sgd_iter, seed, update, policy):
    """the minibatch steps of one policy's update as hh_minibatch_stage's table: per pass the parts of minibatch_partition in
    minibatch_order's order -> int32 [num_sgd_iter * len(parts), 4] = (first chunk, last chunk + 1, unpadded rows, 0)"""
    rows = [(parts[i][0], parts[i][1], int(n_valid[i]), 0) for sgd_pass in range(int(num_sgd_iter))
            for i in minibatch_order(len(parts), seed, update, policy, sgd_pass)]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def sequence_schedule(seq_len, sgd_minibatch_size, num_sgd_iter, seed, update, policy):
    """the minibatch steps of one update over sequences of these lengths (host integers [S]): minibatch_partition's parts and their
    minibatch_schedule — per pass minibatch_order's order, what the eager path visits -> (parts, int32 [num_sgd_iter * len(parts), 4])"""
    seq_len = np.asarray(seq_len, dtype=np.int64)
    parts = minibatch_partition(seq_len, sgd_minibatch_size)
    csum = np.concatenate([[0], np.cumsum(seq_len)])
    return parts, minibatch_schedule(parts, [csum[s1] - csum[s0] for s0, s1 in parts], num_sgd_iter, seed, update, policy)


def minibatch_stage(cols, staged, chunk_len, schedule, cursor, n_valid, src_chunks=None):
    """The minibatch that schedule[cursor] names, copied into fixed-address staging buffers in ONE launch (hh_minibatch_stage,
    include/hh_learner.h).  cols: up to 8 contiguous CUDA tensors [S, ...] (chunks first; any dtype); staged: per column a contiguous
    tensor [cap, ...] of the same dtype and trailing shape; schedule int32 [n_steps, 4] and cursor int32 [1] on the device; n_valid
    int32 [1] receives the row's third entry.  Chunks beyond the minibatch's are zeroed in every staged tensor.  src_chunks: the chunks the
    kernel may read of every column (default S).  The cursor is not written.  No host synchronisation, HIP-graph capturable."""
    _need_gpu("minibatch_stage")
    dev, desc, cap, src_chunks = _stage_desc("minibatch_stage", cols, staged, (("schedule", schedule), ("cursor", cursor), ("n_valid", n_valid)), src_chunks)
    L.check(L.lib().hh_minibatch_stage(len(cols), desc, int(chunk_len), cap, src_chunks, _p(schedule), schedule.shape[0], _p(cursor), _p(n_valid), _stream(dev)))


def _stage_desc(who, cols, staged, tables, src_chunks):
    """the checks that minibatch_stage and minibatch_stage_gather share -> (device, hh_stage_col array, cap, src_chunks); tables: (name,
    tensor) pairs that end with schedule, cursor and n_valid"""
    if len(cols) != len(staged) or len(cols) > L.STAGE_MAX_COLS:
        raise ValueError(f"{who}: as many staging buffers as columns, at most {L.STAGE_MAX_COLS}")
    (_, schedule), (_, cursor), (_, n_valid) = tables[-3:]
    dev = cursor.device
    for what, x in tables:
        if not (x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and x.device == dev):
            raise ValueError(f"{who}: {what} is a contiguous int32 CUDA tensor (the torch-op form is {who}_torch)")
    if schedule.dim() != 2 or schedule.shape[1] != 4 or cursor.numel() != 1 or n_valid.numel() != 1:
        raise ValueError(f"{who}: schedule is [n_steps, 4], cursor and n_valid hold one element")
    S = cols[0].shape[0] if cols else 0
    cap = staged[0].shape[0] if staged else 1
    desc = (L.HHStageCol * max(len(cols), 1))()
    for i, (c, s) in enumerate(zip(cols, staged)):
        if not (c.is_cuda and s.is_cuda and c.device == dev and s.device == dev and c.is_contiguous() and s.is_contiguous() and c.dtype == s.dtype
                and c.shape[1:] == s.shape[1:] and c.shape[0] == S and s.shape[0] == cap and c.dim() >= 1):
            raise ValueError(f"{who}: a column is a contiguous CUDA tensor [S, ...] and its staging buffer [cap, ...] has its dtype and trailing shape")
        desc[i].src, desc[i].dst, desc[i].chunk_bytes = c.data_ptr(), s.data_ptr(), (c.numel() // S if S else s.numel() // cap) * c.element_size()
    src_chunks = S if src_chunks is None else int(src_chunks)
    if not 0 <= src_chunks <= S:
        raise ValueError(f"{who}: src_chunks is within the columns' {S} chunks")
    return dev, desc, cap, src_chunks


def minibatch_stage_gather(cols, staged, chunk_len, order, schedule, cursor, n_valid, src_chunks=None):
    """minibatch_stage through an order table (hh_minibatch_stage_gather, include/hh_learner.h): schedule[cursor] = (o0, o1, unpadded rows, 0)
    names positions of `order` (a contiguous int32 [n] CUDA tensor on the same device), and staged chunk i becomes chunk order[o0 + i] of
    every column — zero where that entry names no chunk of [0, src_chunks) and behind the minibatch.  Everything else is minibatch_stage's:
    ONE launch, the tables only read, no host synchronisation, HIP-graph capturable."""
    _need_gpu("minibatch_stage_gather")
    dev, desc, cap, src_chunks = _stage_desc("minibatch_stage_gather", cols, staged,
                                             (("order", order), ("schedule", schedule), ("cursor", cursor), ("n_valid", n_valid)), src_chunks)
    if order.dim() != 1 or order.numel() == 0:
        raise ValueError("minibatch_stage_gather: order is [n], n >= 1 (an empty tensor has no address to hand over)")
    L.check(L.lib().hh_minibatch_stage_gather(len(cols), desc, int(chunk_len), cap, src_chunks, C.c_void_p(order.data_ptr()), order.shape[0], _p(schedule),
                                              schedule.shape[0], _p(cursor), _p(n_valid), _stream(dev)))


def minibatch_stage_gather_torch(cols, cap, idx):
    """minibatch_stage_gather with torch ops, any device: idx = the minibatch's order entries (integers [n], n <= cap) -> per column a new
    tensor [cap, ...]: chunk idx[i] at place i (index_select), zero where idx[i] names no chunk of the column, zeros behind"""
    out = []
    for c in cols:
        ix = torch.as_tensor(np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64), device=c.device).reshape(-1)
        if ix.numel() > int(cap):
            raise ValueError(f"minibatch_stage_gather_torch: {ix.numel()} chunks do not fit cap = {int(cap)}")
        ok = (ix >= 0) & (ix < c.shape[0])
        z = torch.zeros((int(cap),) + tuple(c.shape[1:]), dtype=c.dtype, device=c.device)
        if c.shape[0] and ix.numel():
            got = c.index_select(0, torch.where(ok, ix, torch.zeros_like(ix)))
            got[~ok] = 0
            z[:ix.numel()] = got
        out.append(z)
    return out


def minibatch_stage_torch(cols, cap, row):
    """minibatch_stage with torch ops, any device: row = (first chunk, last chunk + 1, unpadded rows, 0) -> (per column a new tensor
    [cap, ...]: the chunks, then zeros; n_valid)"""
    s0, s1, nv = int(row[0]), int(row[1]), int(row[2])
    out = []
    for c in cols:
        z = torch.zeros((int(cap),) + tuple(c.shape[1:]), dtype=c.dtype, device=c.device)
        z[:s1 - s0] = c[s0:s1]
        out.append(z)
    return out, nv


def train_commit(stats, table, cursor, t):
    """the step's bookkeeping in one one-thread launch (hh_train_commit): table[cursor] = stats (f64 [6] -> f64 [n, 6]), cursor += 1,
    t += 1; cursor and t int32 [1], all CUDA.  The only writer of the two counters (include/hh_learner.h has the hazard)."""
    _need_gpu("train_commit")
    ok = (stats.is_cuda and table.is_cuda and stats.dtype == torch.float64 and table.dtype == torch.float64 and stats.is_contiguous()
          and table.is_contiguous() and stats.numel() == len(L.PPO_STATS) and table.dim() == 2 and table.shape[1] == len(L.PPO_STATS)
          and all(x.is_cuda and x.dtype == torch.int32 and x.numel() == 1 for x in (cursor, t)))
    if not ok:
        raise ValueError("train_commit: stats f64 [6], table f64 [n, 6], cursor and t int32 [1], all CUDA")
    L.check(L.lib().hh_train_commit(_p(stats), _p(table), table.shape[0], _p(cursor), _p(t), _stream(table.device)))


# ------------------------------------------------------------------------------------------------------------------ the window batch
def _cut_args(who, done, max_seq_len):
    """the checks that window_cut and window_cut_torch share -> (T, N, max_seq_len)"""
    if isinstance(max_seq_len, bool) or int(max_seq_len) != max_seq_len or not 1 <= int(max_seq_len) <= L.WINDOW_MAX_LEN:
        raise ValueError(f"{who}: max_seq_len is an integer in 1 .. {L.WINDOW_MAX_LEN}, got {max_seq_len!r}")
    if not isinstance(done, torch.Tensor) or done.dtype != torch.uint8 or done.dim() != 2 or done.shape[0] < 1 or done.shape[1] < 1:
        raise ValueError(f"{who}: done is a uint8 tensor [T, N] with T, N >= 1 (the rollouts' done buffer)")
    if done.shape[0] * done.shape[1] >= 2 ** 31:
        raise ValueError(f"{who}: T N = {done.shape[0] * done.shape[1]} rows do not fit int32 sequence tables")
    return done.shape[0], done.shape[1], int(max_seq_len)


def window_cut(done, max_seq_len, out=None):
    """The sequences of a rollout's [T, N] window (hh_window_cut, include/hh_learner.h): per arena, walking t, a sequence ends at a done
    row (any non-zero byte of done u8 [T, N]), at its max_seq_len-th row, or at t = T-1 — chop_into_sequences on the window's
    fragments.  -> (seq_t0, seq_arena, seq_len): int32 [S] device views, arena-major, then time; S <= T N.  Three launches, then ONE
    synchronising read of the count, as EpisodeBatch.rows() makes one.  out: the three tables to write into (contiguous int32 CUDA
    tensors of at least T N elements each; entries at and beyond S are left as they were); default: new ones."""
    T, N, Lm = _cut_args("window_cut", done, max_seq_len)
    _need_gpu("window_cut")
    if not (done.is_cuda and done.is_contiguous()):
        raise ValueError("window_cut: done is a contiguous CUDA tensor (the torch-op form is window_cut_torch)")
    dev = done.device
    if out is None:
        out = tuple(torch.empty((T * N,), dtype=torch.int32, device=dev) for _ in range(3))
    if len(out) != 3 or any(not (o.is_cuda and o.device == dev and o.dtype == torch.int32 and o.is_contiguous() and o.dim() == 1 and o.numel() >= T * N) for o in out):
        raise ValueError(f"window_cut: out is three contiguous int32 CUDA tensors of at least T N = {T * N} elements on done's device")
    small = torch.empty((N + 1,), dtype=torch.int32, device=dev)        # the scratch [N], then n_seq
    L.check(L.lib().hh_window_cut(T, N, _p(done), Lm, _p(out[0]), _p(out[1]), _p(out[2]), _p(small[N:]), _p(small), _stream(dev)))
    S = int(small[N])
    return out[0][:S], out[1][:S], out[2][:S]


def window_cut_torch(done, max_seq_len):
    """window_cut with torch ops, any device -> (seq_t0, seq_arena, seq_len) int32 [S], the same entries in the same order"""
    T, N, Lm = _cut_args("window_cut_torch", done, max_seq_len)
    dev = done.device
    end = (done != 0).t().contiguous()                                    # [N, T]: arena-major
    end[:, T - 1] = True
    t = torch.arange(T, device=dev)[None, :].expand(N, T)
    first = torch.ones((N, T), dtype=torch.bool, device=dev)
    first[:, 1:] = end[:, :-1]                                            # a fragment starts at t = 0 and behind every done row
    frag_t0 = torch.cummax(torch.where(first, t, torch.zeros_like(t)), dim=1).values
    r0 = torch.nonzero((first | ((t - frag_t0) % Lm == 0)).reshape(-1)).reshape(-1)   # every sequence's first row, r = n T + t
    nxt = torch.cat([r0[1:], torch.full((1,), N * T, dtype=r0.dtype, device=dev)])    # t = 0 starts one in every arena: none crosses arenas
    return (r0 % T).to(torch.int32), (r0 // T).to(torch.int32), (nxt - r0).to(torch.int32)


def _gather_args(who, cols, tables, max_seq_len):
    """the checks that window_gather and window_gather_torch share.  cols: per column (src, tail, offset, per_seq) — src a contiguous
    tensor [T_src, N, ...] (a step-row is src[t, n]), tail the trailing shape of one gathered row in src's dtype, offset the BYTES from the
    step-row's start to it, per_seq False | True -> (S, max_seq_len, T_src, N, [(src, tail, offset, width, step_bytes, per_seq)])"""
    if isinstance(max_seq_len, bool) or int(max_seq_len) != max_seq_len or not 1 <= int(max_seq_len) <= L.WINDOW_MAX_LEN:
        raise ValueError(f"{who}: max_seq_len is an integer in 1 .. {L.WINDOW_MAX_LEN}, got {max_seq_len!r}")
    if not 1 <= len(cols) <= L.STAGE_MAX_COLS:
        raise ValueError(f"{who}: 1 .. {L.STAGE_MAX_COLS} columns per call, got {len(cols)}")
    if len(tables) != 3 or any(not isinstance(x, torch.Tensor) or x.dtype != torch.int32 or x.dim() != 1 or x.numel() != tables[0].numel() for x in tables):
        raise ValueError(f"{who}: tables is (seq_t0, seq_arena, seq_len), int32 [S] each (window_cut's)")
    out, T_src, N = [], None, None
    for col in cols:
        src, tail, offset, per_seq = col
        tail = tuple(int(x) for x in tail)
        if not isinstance(src, torch.Tensor) or src.dim() < 2 or not src.is_contiguous() or src.shape[0] < 1 or src.shape[1] < 1:
            raise ValueError(f"{who}: a column's source is a contiguous tensor [T_src, N, ...]")
        if N is not None and src.shape[1] != N:
            raise ValueError(f"{who}: the columns of one call hold the same N arenas")
        N = src.shape[1]
        T_src = src.shape[0] if T_src is None else min(T_src, src.shape[0])     # the rows EVERY column of the call holds
        step_bytes = (src.numel() // (src.shape[0] * N)) * src.element_size()
        width = int(np.prod(tail, dtype=np.int64)) * src.element_size()
        if width < 1 or int(offset) < 0 or int(offset) % src.element_size() or int(offset) + width > step_bytes:
            raise ValueError(f"{who}: a slice of {width} bytes at offset {offset} does not lie, element-aligned, inside its {step_bytes}-byte step-row")
        out.append((src, tail, int(offset), width, step_bytes, bool(per_seq)))
    return tables[0].numel(), int(max_seq_len), T_src, N, out


def window_gather(cols, tables, max_seq_len, out=None):
    """The window's columns as padded sequences in ONE launch (hh_window_gather, include/hh_learner.h).  cols: up to 8 tuples
    (src, tail, offset, per_seq) — src a contiguous CUDA tensor [T_src, N, ...] (the rollout's buffer as it lies), tail the trailing shape
    of one gathered row in src's dtype, offset the bytes from the step-row src[t, n] to that slice (one agent's part), per_seq True for
    the first row of every sequence only; tables: window_cut's (seq_t0, seq_arena, seq_len).  -> per column a new tensor
    [S, max_seq_len, *tail], zero beyond every sequence's length, or [S, *tail] with per_seq.  The kernel may read the rows that every
    column of the call holds (T_src = the smallest of the sources' first dimensions).  A table entry that names no rows of the window
    stages zeros.  out: the destinations to write into instead (contiguous, the same shapes and dtypes; every byte of them is written).
    No host synchronisation, HIP-graph capturable."""
    S, Lm, T_src, N, cs = _gather_args("window_gather", cols, tables, max_seq_len)
    _need_gpu("window_gather")
    dev = tables[0].device
    if any(not (x.is_cuda and x.is_contiguous() and x.device == dev) for x in tables) or any(not (c[0].is_cuda and c[0].device == dev) for c in cs):
        raise ValueError("window_gather: the tables and the sources are contiguous CUDA tensors on one device (the torch-op form is window_gather_torch)")
    shapes = [((S,) if per_seq else (S, Lm)) + tail for _, tail, _, _, _, per_seq in cs]
    if out is None:
        out = [torch.empty(sh, dtype=c[0].dtype, device=dev) for sh, c in zip(shapes, cs)]
    if len(out) != len(cs) or any(not (o.is_cuda and o.device == dev and o.is_contiguous() and o.dtype == c[0].dtype and tuple(o.shape) == sh)
                                  for o, sh, c in zip(out, shapes, cs)):
        raise ValueError("window_gather: out holds per column a contiguous CUDA tensor [S, max_seq_len, *tail] ([S, *tail] with per_seq) of the source's dtype")
    if S == 0:
        return list(out)
    desc = (L.HHWindowCol * len(cs))()
    for d, o, (src, _, offset, width, step_bytes, per_seq) in zip(desc, out, cs):
        d.src, d.dst, d.step_bytes, d.offset, d.width, d.per_seq = src.data_ptr(), o.data_ptr(), step_bytes, offset, width, int(per_seq)
    L.check(L.lib().hh_window_gather(len(cs), desc, S, Lm, T_src, N, _p(tables[0]), _p(tables[1]), _p(tables[2]), _stream(dev)))
    return list(out)


def window_gather_torch(cols, tables, max_seq_len):
    """window_gather with torch ops, any device: the same arguments -> per column a new tensor with the same bytes (index_select through the
    tables; an entry that names no rows of the window gives zeros)"""
    S, Lm, T_src, N, cs = _gather_args("window_gather_torch", cols, tables, max_seq_len)
    t0, n, ln = (x.long() for x in tables)
    ok = (t0 >= 0) & (ln >= 0) & (ln <= Lm) & (n >= 0) & (n < N) & (t0 + ln <= T_src)
    t0, n, ln = (torch.where(ok, x, torch.zeros_like(x)) for x in (t0, n, ln))
    out = []
    for src, tail, offset, width, step_bytes, per_seq in cs:
        rows = 1 if per_seq else Lm
        j = torch.arange(rows, device=src.device)[None, :]
        keep = j < ln[:, None]                                                     # [S, rows]
        r = torch.where(keep, (t0[:, None] + j) * N + n[:, None], torch.zeros_like(keep, dtype=torch.int64))
        flat = src.reshape(src.shape[0] * N, -1).view(torch.uint8)[:, offset:offset + width]
        got = flat.index_select(0, r.reshape(-1)).reshape(S, rows, width) * keep[:, :, None].to(torch.uint8)
        got = got.contiguous().view(src.dtype).reshape((S, rows) + tail)
        out.append(got[:, 0] if per_seq else got)
    return out


class DeviceAdam:
    """torch.optim.Adam(params, lr) with its state on the device: m and v per parameter and the step count t (int32 [1]), stepped by
    adam_step (hh_adam_step).  t is advanced by train_commit, not by step().
    max_norm: clip the gradients by their global L2 norm over all of params (torch.nn.utils.clip_grad_norm_(params, max_norm)) inside
    step(): grad_norm (hh_grad_norm) into `clip` f64 [2] = (the norm before clipping, the coefficient), then the clipped adam_step
    (hh_adam_step_clipped).  Unlike torch's in-place scaling, .grad KEEPS THE UNSCALED GRADIENT: the step scales what it reads.
    record(cursor, table) makes every step also write its norm to table[cursor] (the learners' per-step record)."""

    def __init__(self, params, lr, betas=ADAM_BETAS, eps=ADAM_EPS, max_norm=None):
        self.params = list(params)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_norm = _grad_clip(max_norm)
        self.cursor = self.table = self.clip = self.scratch = None
        if self.max_norm is not None:
            self.clip = torch.zeros((L.CLIP_OUT,), dtype=torch.float64, device=self.params[0].device)
            self.scratch = grad_norm_scratch(self.params)       # room for every parameter: a step over fewer needs fewer slots
        self.m = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.v = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.t = torch.zeros((1,), dtype=torch.int32, device=self.params[0].device)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def record(self, cursor, table):
        """from now on step() writes the norm before clipping to table[cursor] as well (int32 [1], f64 [n]; None, None: no record)"""
        self.cursor, self.table = cursor, table

    def step(self):
        """one Adam step of every parameter that has a gradient (as torch.optim.Adam skips the others), from the current .grad pointers;
        with max_norm the norm over those gradients first, then the clipped step"""
        live = [i for i, p in enumerate(self.params) if p.grad is not None]
        grads = [self.params[i].grad for i in live]
        if self.max_norm is not None:
            grad_norm(grads, self.max_norm, self.clip, self.cursor, self.table, self.scratch)
        adam_step([self.params[i].data for i in live], grads, [self.m[i] for i in live], [self.v[i] for i in live],
                  self.t, lr=self.lr, betas=self.betas, eps=self.eps, clip=self.clip)


class _StepBook:
    """what one policy's replayable step keeps on the device: the cursor, the statistics table, and for step="graph" the persistent copy
    of the policy batch, the schedule, the staging buffers and the captured graph"""

    def __init__(self, device, gnorm=False):
        self.device = device
        self.gnorm = torch.zeros((0,), dtype=torch.float64, device=device) if gnorm else None      # grad_clip: the norm before clipping per step
        self.cursor = torch.zeros((1,), dtype=torch.int32, device=device)
        self.n_valid = torch.zeros((1,), dtype=torch.int32, device=device)
        self.table = torch.zeros((0, len(L.PPO_STATS)), dtype=torch.float64, device=device)
        self.schedule = torch.zeros((0, 4), dtype=torch.int32, device=device)
        self.src, self.staged, self.graph, self.key, self.keep = {}, {}, None, None, None
        self.order, self.order_len = None, 0    # shuffle_sequences: the order table int32 [>= num_sgd_iter * S] and its entries in use (load_order); never allocated without it
        self.n_steps = self.cap = 0             # graph_prepare: the schedule's rows in use and the staging capacity
        self.captures = 0

    @staticmethod
    def _grown(t, n, shape, dtype, device):
        """a zeroed tensor [>= n, *shape]: t itself while it is large enough (its address stays), else one of twice the need"""
        if t is not None and t.shape[0] >= n and tuple(t.shape[1:]) == tuple(shape) and t.dtype == dtype:
            return t
        return torch.zeros((max(2 * n, 16),) + tuple(shape), dtype=dtype, device=device)

    def begin(self, n_steps, opt=None):
        """room for n_steps rows of statistics, cursor = 0; with a gnorm table, room in it too (grown with `table`), and `opt` (the
        DeviceAdam) is handed the cursor and that table"""
        self.table = self._grown(self.table, n_steps, (len(L.PPO_STATS),), torch.float64, self.device)
        if self.gnorm is not None:
            self.gnorm = self._grown(self.gnorm, self.table.shape[0], (), torch.float64, self.device)
            opt.record(self.cursor, self.gnorm)
        self.cursor.zero_()

    def load(self, cols, schedule):
        """the policy batch's columns and the schedule into the persistent buffers (the graph reads these addresses)"""
        for k, c in cols.items():
            self.src[k] = self._grown(self.src.get(k), c.shape[0], c.shape[1:], c.dtype, self.device)
            self.src[k][:c.shape[0]].copy_(c)
        sched = torch.from_numpy(np.ascontiguousarray(schedule, dtype=np.int32)).to(self.device)
        self.schedule = self._grown(self.schedule, sched.shape[0], (4,), torch.int32, self.device)
        self.schedule[:sched.shape[0]].copy_(sched)

    def load_order(self, order):
        """shuffle_sequences: the update's order table into its persistent buffer (grown like the schedule; 4 bytes per pass and chunk)"""
        order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(self.device)
        self.order = self._grown(self.order, order.shape[0], (), torch.int32, self.device)
        self.order[:order.shape[0]].copy_(order)
        self.order_len = order.shape[0]


class _PolicySGD:
    """One optimizer's minibatch steps, the same code for PPOLearner's two policies and for CommanderLearner's one: it owns the module's
    optimizer (DeviceAdam | torch.optim.Adam), the _StepBook (None with torch.optim.Adam), clip_grad_norm_'s norms of the running update
    and the policy's kl_coeff, and walks update_schedule's table — row by row from Python (step="eager") or by the cursor of ONE captured
    HIP graph (step="graph").  What differs between the learners comes in as plain callables:
      forward(mb) -> (logits, vf);  loss(logits, vf, mb, kl_coeff) -> (total, stats f64 [6]);
      stage_groups(column names) -> [(names of up to _lib.STAGE_MAX_COLS columns, rows per chunk), ...]: one stage launch each;
      policy: the index in minibatch_order's and sequence_order's keys;  noun: what a chunk is called in messages.
    cfg is the learner itself, read at every call (never written) for device, step, grad_clip, shuffle_sequences, use_kl, kl_target, num_sgd_iter,
    sgd_minibatch_size, seed and updates."""

    def __init__(self, cfg, module, lr, kl_coeff, device_adam, forward, loss, stage_groups, policy, noun):
        self.cfg, self.module, self.kl_coeff, self.gnorms = cfg, module, float(kl_coeff), []
        self.forward, self.loss, self.stage_groups, self.policy, self.noun = forward, loss, stage_groups, int(policy), noun
        if device_adam:
            self.optimizer, self.book = DeviceAdam(module.parameters(), lr=lr, max_norm=cfg.grad_clip), _StepBook(cfg.device, gnorm=cfg.grad_clip is not None)
        else:
            self.optimizer, self.book = torch.optim.Adam(module.parameters(), lr=lr), None

    def kl_term(self):
        """the KL term's coefficient as the loss takes it: ray tests config["kl_coeff"], the initial value, for the term and for update_kl"""
        return self.kl_coeff if self.cfg.use_kl else 0.0

    def schedule(self, seq_len):
        cfg = self.cfg
        return update_schedule(seq_len, cfg.sgd_minibatch_size, cfg.num_sgd_iter, cfg.seed, cfg.updates, self.policy, cfg.shuffle_sequences)

    def minibatch_step(self, mb):
        """forward, loss, backward, Adam step on one minibatch (a dict of the policy batch's columns, with n_valid) -> stats f64 [6] (device)"""
        opt, book, clip = self.optimizer, self.book, self.cfg.grad_clip
        logits, vf = self.forward(mb)
        total, stats = self.loss(logits, vf, mb, self.kl_term())
        opt.zero_grad(set_to_none=True)
        total.backward()
        if clip is not None and book is None:       # DeviceAdam: inside opt.step()
            self.gnorms.append(torch.nn.utils.clip_grad_norm_(self.module.parameters(), clip))
        opt.step()
        if book is not None:        # the statistics into the device table, cursor and Adam's t advanced: after the Adam launch
            train_commit(stats, book.table, book.cursor, opt.t)
        return stats

    # ---- the step as one HIP graph (step="graph")
    def graph_prepare(self, cols, seq_len, cap=None):
        """Everything the update needs before its first replay: the schedule of the chunks' lengths `seq_len` (host integers [S]) and the
        columns `cols` (dict of contiguous [S, ...] tensors, staged in this order) uploaded into persistent device buffers — with
        shuffle_sequences the order table beside them — the cursor set to 0, and the graph of ONE minibatch step captured unless the graph of
        an earlier call still fits: it is kept while the key is what it was — cap, kl_coeff (by value in hh_ppo_loss_params), the columns
        and the buffers' addresses; then (grad_clip, which travels by value, the norm table's address and rows) when clipping; then (True,
        the order buffer's address and rows) when shuffling.  cap: the staging capacity in chunks; default and minimum: the largest
        minibatch.  Weights, m, v, t are left bit for bit as they were.  -> (n_steps, rows)"""
        cfg, book = self.cfg, self.book
        order, sched, need = self.schedule(seq_len)
        cap = need if cap is None else int(cap)
        if cap < need:
            raise ValueError(f"cap = {cap} is smaller than the largest minibatch ({need} {self.noun})")
        book.begin(len(sched), self.optimizer)
        book.load(cols, sched)
        if order is not None:
            book.load_order(order)
        book.n_steps, book.cap = len(sched), cap
        src_chunks = min(t.shape[0] for t in book.src.values())
        names = tuple(cols)
        key = (cap, self.kl_term(), names, src_chunks, book.schedule.data_ptr(), book.schedule.shape[0], book.table.data_ptr(),
               book.table.shape[0]) + tuple(book.src[k].data_ptr() for k in names)
        if cfg.grad_clip is not None:
            key += (cfg.grad_clip, book.gnorm.data_ptr(), book.gnorm.shape[0])
        if cfg.shuffle_sequences:
            key += (True, book.order.data_ptr(), book.order.shape[0])
        if book.graph is None or book.key != key:
            self._capture(names, src_chunks)
            book.key = key
        return len(sched), int(np.sum(seq_len))

    def _capture(self, names, src_chunks):
        """stage(s) -> forward -> loss -> backward -> (norm ->) Adam -> commit on one stream as one graph, after a warm-up of the stages,
        forward and backward only"""
        book, opt, dev, shuffle = self.book, self.optimizer, self.cfg.device, self.cfg.shuffle_sequences
        if book.staged.get("obs") is None or book.staged["obs"].shape[0] != book.cap or tuple(book.staged) != names:
            book.staged = {k: torch.zeros((book.cap,) + tuple(book.src[k].shape[1:]), dtype=book.src[k].dtype, device=dev) for k in names}
        mb = dict(book.staged, n_valid=book.n_valid)
        # one launch per group; all of them only read the cursor, the schedule and the order and write the same n_valid
        groups = [([book.src[k][:src_chunks] for k in ks], [book.staged[k] for k in ks], chunk_len) for ks, chunk_len in self.stage_groups(names)]

        def stage():
            for srcs, staged, chunk_len in groups:
                if shuffle:
                    minibatch_stage_gather(srcs, staged, chunk_len, book.order, book.schedule, book.cursor, book.n_valid)
                else:
                    minibatch_stage(srcs, staged, chunk_len, book.schedule, book.cursor, book.n_valid)

        def forward_backward():
            logits, vf = self.forward(mb)
            total, stats = self.loss(logits, vf, mb, self.kl_term())
            total.backward()
            return stats
        # the warm-up: forward and backward only (rocBLAS and autograd initialise), on a side stream as torch's capture recipe has it;
        # it reads schedule[0] through the cursor and writes nothing but the staging buffers and gradients that are thrown away
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            stage()
            for _ in range(2):
                opt.zero_grad(set_to_none=True)
                forward_backward()
        torch.cuda.current_stream(dev).wait_stream(side)
        opt.zero_grad(set_to_none=True)     # backward inside the capture assigns the gradients from the graph's pool: their addresses are fixed
        book.graph = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):       # what the forward allocates (the GRU's scratch and y among it) comes from the graph's pool as well
            stage()
            stats = forward_backward()
            opt.step()
            train_commit(stats, book.table, book.cursor, opt.t)
        book.graph, book.keep = graph, stats
        book.captures += 1

    def graph_replay(self, n=1):
        """n minibatch steps from the captured graph, no host work between them"""
        graph = self.book.graph
        for _ in range(int(n)):
            graph.replay()

    def graph_stats(self, n):
        """the statistics rows f64 [n, 6] of the first n steps since graph_prepare (one device tensor; reading it synchronises)"""
        return self.book.table[:int(n)]

    def grad_gnorm(self, n):
        """grad_clip: the mean of the first n steps' norms before clipping since the update began (a float; reading it synchronises)"""
        if n == 0:
            return float("nan")
        if self.book is not None:
            return float(self.book.gnorm[:int(n)].mean())
        return float(torch.stack(self.gnorms[:int(n)]).double().mean())

    # ---- one update
    def result(self, m, steps, rows):
        """an update's dict from the means of the steps' statistics; with grad_clip also grad_gnorm"""
        clipped = {} if self.cfg.grad_clip is None else dict(grad_gnorm=self.grad_gnorm(steps))
        return dict(total_loss=m[0], policy_loss=m[1], vf_loss=m[2], kl=m[3], entropy=m[4], kl_coeff=self.kl_coeff, steps=steps, rows=rows, **clipped)

    def empty(self):
        """the dict of an update over no rows: no step, every statistic NaN"""
        return self.result([float("nan")] * 5, 0, 0)

    def run(self, cols, seq_len):
        """One update of this policy over the columns `cols` (dict of [S, ...] tensors) whose chunks hold `seq_len` (host integers [S])
        unpadded rows: every row of update_schedule's table once, in its order — replayed (step="graph": cols as graph_prepare takes them)
        or stepped from here, an unshuffled row's chunks sliced, a shuffled row's gathered by its order entries — then KLCoeffMixin.update_kl
        on the mean of the steps' mean_kl -> the update's dict."""
        cfg = self.cfg
        if cfg.step == "graph":
            n, rows = self.graph_prepare(cols, seq_len)
            self.graph_replay(n)
            table = self.graph_stats(n)
        else:
            order, sched, _ = self.schedule(seq_len)
            dev = cols["obs"].device
            n_valid = torch.from_numpy(np.ascontiguousarray(sched[:, 2])).to(dev)
            if order is not None:
                order = torch.from_numpy(order).to(dev).long()
            self.gnorms = []
            if self.book is not None:
                self.book.begin(len(sched), self.optimizer)
            all_stats = []
            for i, (c0, c1) in enumerate(sched[:, :2].tolist()):
                if order is None:
                    mb = {k: v[c0:c1] for k, v in cols.items()}
                else:
                    idx = order[c0:c1]
                    mb = {k: v.index_select(0, idx) for k, v in cols.items()}
                mb["n_valid"] = n_valid[i:i + 1]
                all_stats.append(self.minibatch_step(mb))
            n, rows = len(all_stats), int(np.sum(seq_len))
            table = torch.stack(all_stats) if all_stats else None
        m = table.mean(dim=0).tolist() if n else [float("nan")] * 6
        if cfg.use_kl and n:
            self.kl_coeff = kl_coeff_update(self.kl_coeff, m[3], cfg.kl_target)
        return self.result(m, n, rows)


def _learner_options(learner, who, device, optimizer, step, grad_clip, shuffle_sequences, kl_coeff, fused, floats, ints, heads="torch", trunk="torch"):
    """what both learners' constructors take the same way, set on `learner`: the modes, grad_clip, the flag and `heads` validated in this
    order before the device is looked at, then the device and the PPO hyper-parameters (floats and ints by name) -> the optimizer mode"""
    mode = _optimizer_mode(optimizer)
    learner.step = _step_mode(step, optimizer)
    learner.grad_clip = _grad_clip(grad_clip)
    learner.shuffle_sequences = _shuffle_flag(shuffle_sequences)
    learner.heads = _heads_mode(heads, trunk)
    if learner.heads == "fused" and not fused:
        raise ValueError('heads="fused" needs fused=True: the fused tail has the loss kernel inside')
    _need_gpu(who)
    learner.device = torch.device(device) if not isinstance(device, torch.device) else device
    for k, v in floats.items():
        setattr(learner, k, float(v))
    for k, v in ints.items():
        setattr(learner, k, int(v))
    learner.use_kl = kl_coeff > 0.0         # ray tests config["kl_coeff"], the initial value, for the KL term and for update_kl
    learner.fused, learner.updates = bool(fused), 0
    return mode


# ------------------------------------------------------------------------------------------------------------------ the learner
class PPOLearner:
    """One PPO update of train_hetero.py's two policies from the `EpisodeBatch` of a `PPORollout(batch_mode="complete_episodes")`:

        learner = PPOLearner.trainable_init(device, mode="fight", seed=0)     # the weights of PolicyBank.trainable_init(seed)
        stats = learner.update(ro.episodes, bank)
        learner.publish(bank)

    Defaults: train_hetero.py:216 (lr, clip_param, kl_target), config.py:36-37 (sgd_minibatch_size) and RLlib 2.4's PPO defaults for the
    rest.  Per policy (agent 1, then agent 2; each with its own Adam over its module's parameters, the tied shared layer in both):
      * rows: the agent's column of every emitted row — nothing is masked by `valid` (semantics = "rllib"); own observation cut to the
        kind's width, critic rows from central_critic_rows (actions filled in);
      * old_logits (RLlib's ACTION_DIST_INPUTS, which the KL term and so kl_coeff are computed from): `batch_old_logits`.  With
        PPORollout(record_logits=True) the batch carries a `logits` column — for every row the logits of the sampler call that drew its
        action and wrote its logp, whatever weights the bank held at that tick — and that column is used as it stands: no bank call,
        and rows sampled before the last publish (the head of an episode that was still running then) keep the logits of the weights
        that sampled them, so old_logp and old_logits of a row always come from one forward.
        Without the column they are recomputed once per update from `bank`, which still holds the pre-update weights, in
        ceil(R / N) greedy calls of the rollout's own shape ([N, 2] rows, the same selectors, so the row lists a captured collect
        re-uses stay what they were).  Only then does this approximation apply: rows carried over from before the last publish were
        sampled by older weights — their stored logp, and so the ratio, is exact, but their recomputed old_logits are the newer
        weights', so the KL term sees them as on-policy (`rollout.start()` after `publish` avoids it by throwing the running episodes
        away; record_logits = True makes that unnecessary);
      * advantages standardised over the policy's whole batch;
      * fight kinds: each episode cut into chunks of max_seq_len, zero-padded, mask = the unpadded rows;
      * num_sgd_iter passes; in each the chunks (escape: rows), in batch order, are split into consecutive minibatches of at least
        sgd_minibatch_size unpadded rows, visited in the order of minibatch_order(seed, update count, policy, pass).  RLlib's own
        order is drawn from an unseeded generator and shuffles the chunks themselves; this one is reproducible by construction, and
        shuffle_sequences=True shuffles the chunks themselves as well, per pass, from a seeded stream of its own (shuffled_schedule);
      * after the passes KLCoeffMixin.update_kl on the mean of the minibatches' mean_kl.
    fused = False computes the loss with torch ops (ppo_loss_torch) instead of hh_ppo_loss; nothing else differs.
    Inside a minibatch step nothing synchronises with the host (beyond what torch.optim.Adam does by itself); `update` itself synchronises
    when it reads the batch's row count, cuts the minibatches and reads the statistics.  (CommanderRollout's batches: CommanderLearner.)"""

    @_heads_keyword
    def __init__(self, kinds, state_dicts, device, lr=1e-4, clip_param=0.25, kl_target=0.025, kl_coeff=0.2, vf_clip_param=10.0,
                 vf_loss_coeff=1.0, entropy_coeff=0.0, num_sgd_iter=30, sgd_minibatch_size=256, max_seq_len=20, seed=0, fused=True, attention="torch", inputs="torch", trunk="torch",
                 optimizer="torch", step="eager", shuffle_sequences=False, grad_clip=None):
        """kinds: (kind of ac1_policy, kind of ac2_policy); state_dicts: per policy the actor and value-branch tensors in one dict (numpy or
        torch), keyed like the reference's state_dict().  The shared layer is tied to the first policy's.  attention: TrainableNet's
        argument, handed to both modules ("fused": the fight networks' chunk attention through hh_chunk_attn_* / hh_residual_normalize_*).
        inputs: TrainableNet's argument as well ("fused": everything in front of shared_layer through hh_input_stage_*).
        trunk: TrainableNet's argument too ("fused": shared_layer, bias and tanh of both sides through hh_dense_tanh_*).
        optimizer: "torch" (the default) steps with torch.optim.Adam; "fused" keeps each policy's m, v and step count on the device
        (DeviceAdam: hh_adam_step) and gathers the steps' statistics in a device table (hh_train_commit).
        step: "eager" (the default) issues every minibatch step's launches from Python; "graph" (needs optimizer="fused") captures
        stage -> forward -> loss -> backward -> Adam -> commit once per policy as ONE HIP graph and replays it per step (graph_prepare).
        grad_clip: RLlib's grad_clip.  None (the default, and the reference's value): nothing is clipped and nothing changes.  A finite float
        > 0: in every minibatch step the gradients of ONE optimizer — one policy's parameter list, the tied shared layer in it, as RLlib's
        apply_grad_clipping takes one optimizer's param groups — are scaled so that their global L2 norm does not exceed it, and every dict
        of update() also has grad_gnorm, the mean over the update's steps of the norm BEFORE clipping (RLlib reports it under the same
        condition).  optimizer="torch" calls torch.nn.utils.clip_grad_norm_ (float32 norm, scales .grad in place); "fused" computes the
        norm in float64 on the device and scales inside the Adam step (DeviceAdam(max_norm=...): .grad keeps the unscaled gradient), and
        the graph's chain becomes stage -> forward -> loss -> backward -> norm -> clipped Adam -> commit.
        shuffle_sequences: RLlib's shuffle_sequences (its default is True; here False, and then nothing changes).  True: every pass draws
        its own order of the chunks (escape: rows), sequence_order(seed, update count, policy, pass), and cuts THAT order into consecutive
        minibatches of at least sgd_minibatch_size unpadded rows (shuffled_schedule), visited in position order: the minibatches hold
        different chunks in every pass, and a pass may take one step more or fewer than another.  The eager modes gather each minibatch with
        index_select; step="graph" stages through hh_minibatch_stage_gather from an order table uploaded once per update into a persistent
        device buffer of 4 * num_sgd_iter * S bytes for S chunks, grown to twice the need so that its address outlives batches of varying
        size (30 passes: about 6.6 MB for 1.09 M fight rows in chunks of 20, about 131 MB for the same rows as escape rows).  RLlib's own
        permutation is unseeded, so equality with it is not claimed; what shuffling does to learning curves has not been measured here.
        heads (keyword only, taken by _heads_keyword in front of this signature): "torch" (the default): nothing changes.  "fused" (needs fused=True and trunk="torch"): the modules are built
        with heads="fused", every minibatch step's forward stops at shared_layer's pre-activations (TrainableNet.pre_heads) and tanh, the
        two heads, the loss and their backward run as one hh_heads_loss (heads_loss, unscaled: the step calls total.backward()), in all
        three step modes, with grad_clip and shuffle_sequences as before."""
        self.optimizer = _learner_options(
            self, "PPOLearner", device, optimizer, step, grad_clip, shuffle_sequences, kl_coeff, fused,
            dict(clip_param=clip_param, kl_target=kl_target, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff, entropy_coeff=entropy_coeff),
            dict(num_sgd_iter=num_sgd_iter, sgd_minibatch_size=sgd_minibatch_size, max_seq_len=max_seq_len, seed=seed), self._heads_arg, trunk)
        self.kinds = tuple(int(k) for k in kinds)
        assert len(self.kinds) == 2 and PN.HAS_ATT[self.kinds[0]] == PN.HAS_ATT[self.kinds[1]]
        self.attention, self.inputs, self.trunk = attention, inputs, _trunk_mode(trunk)
        # tied once, before the move: tie hands every module the first one's shared_layer MODULE, and nn.Module.to() moves a module's
        # tensors in place without ever replacing a submodule object, so the one layer stays the one layer on the device
        self.modules = tie([TrainableNet(k, attention=attention, inputs=inputs, trunk=trunk, heads=self.heads).load_numpy({k2: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k2, v in sd.items()})
                            for k, sd in zip(self.kinds, state_dicts)])
        for m in self.modules:
            m.to(self.device)
        self.recurrent = PN.HAS_ATT[self.kinds[0]]
        esc = not self.recurrent
        # per policy its own driver: the module's Adam, the step book, kl_coeff; one stage launch of every column
        # (heads="fused": the forward callable stops at the pre-activations and the loss callable is the fused tail)
        tail = self.heads == "fused"
        self._sgd = [_PolicySGD(self, m, lr, kl_coeff, self.optimizer == "fused",
                                forward=(lambda mb, m=m: m.pre_heads(mb["obs"], mb["critic"])) if tail else (lambda mb, m=m: m(mb["obs"], mb["critic"])),
                                loss=(lambda za, zc, mb, kl, a=a: self.heads_loss(a, za, zc, mb, kl)) if tail else (lambda logits, vf, mb, kl, a=a: self.loss(a, logits, vf, mb, kl)),
                                stage_groups=lambda names: [(names, 1 if esc else self.max_seq_len)], policy=a, noun="chunks")
                     for a, m in enumerate(self.modules)]
        self.optimizers = [d.optimizer for d in self._sgd]
        self._books = [d.book for d in self._sgd] if self.optimizer == "fused" else None
        self._sel = (pilots.SEL_ESC1 if esc else pilots.SEL_FIGHT1, pilots.SEL_ESC2 if esc else pilots.SEL_FIGHT2)
        self._tmp = None

    @property
    def kl_coeff(self):
        """per policy the current coefficient of the KL term (the drivers hold them; update_kl moves each after its policy's passes)"""
        return [d.kl_coeff for d in self._sgd]

    @kl_coeff.setter
    def kl_coeff(self, values):
        for d, v in zip(self._sgd, values):
            d.kl_coeff = float(v)

    @classmethod
    def trainable_init(cls, device, mode="fight", seed=0, **kw):
        """the learner whose weights equal PolicyBank.trainable_init(device, mode, seed)'s (tied shared layer)"""
        kinds = (PN.FIGHT1, PN.FIGHT2) if mode == "fight" else (PN.ESC1, PN.ESC2)
        sds = [dict(PN.random_weights(k, seed), **PN.random_critic_weights(k, seed)) for k in kinds]
        return cls(kinds, sds, device, seed=seed, **kw)

    # ---- the batch
    def old_logits(self, obs, bank, n_arenas):
        """the sampler's logits of every row of obs f32 [R, 2, D] from `bank` -> f32 [R, 2, 32]; calls of [n_arenas, 2] rows each"""
        R, _, D = obs.shape
        N = int(n_arenas)
        assert 2 * N <= bank.max_rows, "the bank serves the rollout's [N, 2] rows"
        n_calls = (R + N - 1) // N
        out = torch.zeros((max(n_calls, 1) * N, 2, OLD_LD), dtype=torch.float32, device=obs.device)
        if self._tmp is None or self._tmp[0].shape[0] != N or self._tmp[0].shape[2] != D:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=obs.device)
            self._tmp = (z((N, 2, D), torch.float32), z((N, 2, 4), torch.int8), z((N, 2), torch.float32),
                         torch.tensor(self._sel, dtype=torch.uint8, device=obs.device).repeat(N, 1).contiguous())
        stage, act, logp, sel = self._tmp
        for i in range(n_calls):
            src = obs[i * N:(i + 1) * N]
            if src.shape[0] < N:
                stage.zero_()
                stage[:src.shape[0]].copy_(src)
                src = stage
            bank.sample(src, sel, greedy=True, actions=act, logp=logp, logits=out[i * N:(i + 1) * N], want_vf=False)
        return out[:R]

    def batch_old_logits(self, rows, bank, n_arenas=None):
        """old_logits f32 [R, 2, 32] of an emitted batch (`rows`: EpisodeBatch.rows()): the batch's own `logits` column where the
        rollout recorded one (the very tensor, no bank call); otherwise recomputed from `bank` (old_logits; n_arenas: the rollout's N)"""
        if "logits" in rows:
            lg = rows["logits"]
            if lg.dtype != torch.float32 or tuple(lg.shape) != (rows["obs"].shape[0], 2, OLD_LD):
                raise ValueError(f"the batch's logits column must be f32 [R, 2, {OLD_LD}], got {lg.dtype} {tuple(lg.shape)}")
            return lg
        if bank is None or n_arenas is None:
            raise ValueError("the batch has no logits column (PPORollout(record_logits=True)): a bank and n_arenas are needed to recompute them")
        return self.old_logits(rows["obs"], bank, n_arenas)

    def policy_batch(self, rows, old_logits, agent):
        """the training batch of policy `agent` (0 | 1) from the emitted rows: dict of [S, L, ...] chunks (fight) or [R, ...] rows (escape)
        and, for chunks, seq_len [S] and mask [S, L]"""
        kind = self.kinds[agent]
        b = {"obs": rows["obs"][:, agent, :PN.OBS_DIM[kind]].contiguous(),
             "critic": central_critic_rows(rows["obs"], rows["actions"], agent + 1),
             "actions": rows["actions"][:, agent].contiguous(), "old_logp": rows["logp"][:, agent].contiguous(),
             "adv": standardize(rows["adv"][:, agent]), "target": rows["target"][:, agent].contiguous(),
             "old_logits": old_logits[:, agent].contiguous()}
        if not self.recurrent:
            return b
        seq_start, seq_len = cut_chunks(rows["ep_start"], rows["ep_len"], self.max_seq_len)
        b = {k: pad_chunks(v, seq_start, seq_len, self.max_seq_len) for k, v in b.items()}
        b["seq_len"] = seq_len
        b["mask"] = chunk_mask(seq_len, self.max_seq_len).to(torch.uint8)
        return b

    # ---- one minibatch step
    def loss(self, agent, logits, vf, mb, kl_coeff=None):
        """the policy's loss of one minibatch; kl_coeff: the KL term's coefficient, default the policy's current one"""
        kw = dict(n_comp=n_comp_of(self.kinds[agent]), clip_param=self.clip_param, vf_clip_param=self.vf_clip_param, vf_loss_coeff=self.vf_loss_coeff,
                  entropy_coeff=self.entropy_coeff, kl_coeff=self._sgd[agent].kl_term() if kl_coeff is None else kl_coeff)
        return (ppo_loss if self.fused else ppo_loss_torch)(logits, vf, mb, **kw)

    def heads_loss(self, agent, za, zc, mb, kl_coeff=None):
        """heads="fused": the policy's loss of one minibatch from pre_heads' (za, zc), through heads_loss with the module's act_out and
        val_out; the gradients are handed to total.backward() unscaled"""
        m = self.modules[agent]
        return heads_loss(za, zc, m.act_out, m.val_out, mb, n_comp=n_comp_of(self.kinds[agent]), clip_param=self.clip_param, vf_clip_param=self.vf_clip_param,
                          vf_loss_coeff=self.vf_loss_coeff, entropy_coeff=self.entropy_coeff,
                          kl_coeff=self._sgd[agent].kl_term() if kl_coeff is None else kl_coeff, scale_grad=False)

    def _columns(self, b, staged=False):
        """policy_batch's dict as the driver takes it -> (columns [S, ...], host seq_len [S]: the chunks' lengths, ones for escape rows).
        staged: as the graph's stage reads them — contiguous, the mask uint8, and for the escape kinds a mask of ones, which the padding
        rows of the staging buffers need"""
        cols = {k: (v.contiguous() if staged else v) for k, v in b.items() if k != "seq_len"}
        S = cols["obs"].shape[0]
        seq_len = b["seq_len"].cpu().numpy() if self.recurrent else np.ones(S, dtype=np.int64)
        if staged:
            if not self.recurrent:
                cols["mask"] = torch.ones((S,), dtype=torch.uint8, device=self.device)
            cols["mask"] = cols["mask"].to(torch.uint8)
        return cols, seq_len

    # the steps themselves are the driver's (_PolicySGD): one per policy
    def minibatch_step(self, agent, mb):
        """forward, loss, backward, Adam step on one minibatch (a dict sliced from policy_batch's, with n_valid) -> stats f64 [6] (device)"""
        return self._sgd[agent].minibatch_step(mb)

    def graph_prepare(self, agent, b, cap=None):
        """Everything one policy's pass needs before its first replay (_PolicySGD.graph_prepare on policy_batch `b`): the schedule and the
        batch's columns uploaded, the cursor set to 0, and the graph of ONE minibatch step — stage, forward, loss, backward, Adam, commit —
        captured unless an earlier one still fits.  cap: the staging capacity in chunks (escape: rows).  -> (n_steps, rows)"""
        if self.step != "graph":
            raise ValueError('graph_prepare needs PPOLearner(step="graph")')
        return self._sgd[agent].graph_prepare(*self._columns(b, staged=True), cap)

    def graph_replay(self, agent, n=1):
        """n minibatch steps of policy `agent` from its captured graph, no host work between them"""
        self._sgd[agent].graph_replay(n)

    def graph_stats(self, agent, n):
        """the statistics rows f64 [n, 6] of the first n steps since graph_prepare (one device tensor; reading it synchronises)"""
        return self._sgd[agent].graph_stats(n)

    def grad_gnorm(self, agent, n):
        """grad_clip: the mean of the first n steps' norms before clipping since the update began (a float; reading it synchronises)"""
        return self._sgd[agent].grad_gnorm(n)

    # ---- one update
    def update(self, episodes, bank=None):
        """one PPO update of both policies from episodes (an EpisodeBatch after a collect) -> per policy a dict: total_loss, policy_loss,
        vf_loss, kl, entropy (means over the minibatch steps), kl_coeff (after the update), steps (minibatch steps taken), rows.
        `bank` is read only when the batch has no `logits` column (batch_old_logits).  With grad_clip also grad_gnorm.
        An EpisodeBatch built with train_batch_size hands over its accumulated batch (RLlib's train_batch_size: update once
        `episodes.ready()`, e.g. after `PPORollout.collect_batch()`); nothing else changes here."""
        rows = episodes.rows()
        if rows["obs"].shape[0] == 0:
            return [d.empty() for d in self._sgd]
        with torch.no_grad():
            old = self.batch_old_logits(rows, bank, episodes.N)
            batches = [self.policy_batch(rows, old, a) for a in range(2)]
        out = [d.run(*self._columns(b, staged=self.step == "graph")) for d, b in zip(self._sgd, batches)]
        self.updates += 1
        return out

    # ---- one update from a fixed window (batch_mode = "truncate_episodes")
    def _check_window(self, rollout):
        """the refusals of window_batch / update_window -> (T, N)"""
        if getattr(rollout, "semantics", "rllib") != "rllib":
            raise ValueError("PPOLearner trains RLlib's unmasked view: a PPORollout(semantics='masked') window has its dead agents' rows cut out of adv and target")
        for k in ("obs", "actions", "logp", "adv", "target", "done", "T", "w"):
            if not hasattr(rollout, k):
                raise ValueError(f"window_batch takes a PPORollout (its [T, N] buffers); this object has no `{k}`")
        esc = rollout.w.cfg.agent_mode == L.MODE_ESCAPE
        if rollout.obs.dim() != 4 or rollout.obs.shape[2] != 2 or esc == self.recurrent or rollout.obs.shape[3] < max(PN.OBS_DIM[k] for k in self.kinds):
            raise ValueError(f"the rollout's world flies {'escape' if esc else 'fight'} mode with observations {tuple(rollout.obs.shape[2:])}; "
                             f"this learner trains kinds {self.kinds} ({'fight' if self.recurrent else 'escape'})")
        if not getattr(rollout, "collects", 0):
            raise RuntimeError("the rollout has not collected yet: its window buffers hold nothing (rollout.collect() first)")
        return rollout.T, rollout.w.N

    def _window_shared(self, rollout, bank):
        """what both policies' window batches share: the cut, the sampler's logits [T, N, 2, 32] and the advantages in arena-major rows"""
        T, N = self._check_window(rollout)
        tables = window_cut(rollout.done, self.max_seq_len if self.recurrent else 1)
        if getattr(rollout, "record_logits", False):
            logits = rollout.logits
        else:
            if bank is None:
                raise ValueError("the rollout recorded no logits (PPORollout(record_logits=True)): a bank is needed to recompute them")
            logits = self.old_logits(rollout.obs[:T].reshape(T * N, 2, rollout.obs.shape[3]), bank, N).reshape(T, N, 2, OLD_LD)
        adv_rows = rollout.adv.transpose(0, 1).reshape(N * T, 2)      # [R, 2], r = n T + t: what the episode path's rows["adv"] would hold
        return T, N, tables, logits.contiguous(), adv_rows

    def window_batch(self, rollout, bank, agent, shared=None):
        """the training batch of policy `agent` (0 | 1) from a PPORollout's [T, N] window, in policy_batch's format and — fed the same
        rows as episodes (the window's fragments, arena-major) — with policy_batch's values: fight kinds [S, L, ...] chunks with seq_len
        and mask (a chunk ends at a done row, at max_seq_len rows or at the window's end: window_cut), escape kinds [R, ...] with R = T N
        rows, arena-major (r = n T + t: the cut with max_seq_len = 1, the length-1 axis dropped).  One hh_window_gather launch of seven
        columns reads the rollout's buffers as they lie.  The trailing fragment of an arena carries RLlib's truncation bootstrap from
        vf[T] in adv and target (hh_gae_rllib).  `bank` is read only when the rollout recorded no logits.  The advantages are standardised
        over the agent's T N values (standardize).  shared: _window_shared's tuple (update_window builds it once for both policies)."""
        T, N, tables, logits, adv_rows = self._window_shared(rollout, bank) if shared is None else shared
        kind = self.kinds[agent]
        Lm = self.max_seq_len if self.recurrent else 1
        D, Dk = rollout.obs.shape[3], PN.OBS_DIM[kind]
        critic = central_critic_rows(rollout.obs[:T], rollout.actions, agent + 1).contiguous()
        adv = standardize(adv_rows[:, agent]).reshape(N, T).t().contiguous()          # back to [T, N]: where the gather reads a row (t, n)
        names = ("obs", "critic", "actions", "old_logp", "adv", "target", "old_logits")
        got = window_gather([(rollout.obs, (Dk,), agent * D * 4, False), (critic, (critic.shape[2],), 0, False),
                             (rollout.actions, (4,), agent * 4, False), (rollout.logp, (), agent * 4, False), (adv, (), 0, False),
                             (rollout.target, (), agent * 4, False), (logits, (OLD_LD,), agent * OLD_LD * 4, False)], tables, Lm)
        if not self.recurrent:
            return {k: v[:, 0] for k, v in zip(names, got)}
        b = dict(zip(names, got))
        b["seq_len"] = tables[2].long()
        b["mask"] = chunk_mask(b["seq_len"], Lm).to(torch.uint8)
        return b

    def update_window(self, rollout, bank=None):
        """one PPO update of both policies from a PPORollout's [T, N] window as the last collect left it (batch_mode =
        "truncate_episodes", the rollouts' default; the buffers are the same in both modes) -> what `update` returns, with rows = T N.
        Every row of the window was sampled by the weights the sampler holds, so nothing is carried, nothing overflows and no start()
        is needed after publish:

            ro.collect();  stats = learner.update_window(ro, bank);  learner.publish(bank)

        The batches are window_batch's; from there on it is `update`: the same _columns and driver, so fused, attention, inputs, trunk,
        heads, optimizer, step="graph", grad_clip and shuffle_sequences act as they do there, and the row count T N is the same in every
        update.  The rollout's buffers are only read."""
        with torch.no_grad():
            shared = self._window_shared(rollout, bank)
            batches = [self.window_batch(rollout, bank, a, shared) for a in range(2)]
        out = [d.run(*self._columns(b, staged=self.step == "graph")) for d, b in zip(self._sgd, batches)]
        self.updates += 1
        return out

    def publish(self, bank):
        """the new weights into the sampler's bank on the current stream (PolicyBank.refresh_trainable): captured collects replay with them"""
        bank.refresh_trainable(self.modules)


# =================================================================================================================== the commander
CMD_LD = 4      # HH_CMD_LOGITS: row width of hh_commander_sample's logits and of hh_ppo_loss_categorical's
GRU_H = 200     # HH_GRU_HIDDEN
# what CommanderLearner(step="graph") stages per minibatch: eight columns [S, L, ...] per step, then two per sequence
COMMANDER_STAGE_COLS = ("obs", "critic", "actions", "old_logp", "adv", "target", "mask", "old_logits", "state_in", "seq_len")


# ------------------------------------------------------------------------------------------------------------------ the GRU
def _gru_io(n):
    return (L.HHGruSeqIO * n)()


def _gru_scratch_bytes(G, S, Lm):
    nbytes = C.c_int64()
    L.check(L.lib().hh_gru_seq_scratch_bytes(G, S, Lm, C.byref(nbytes)))
    return nbytes.value


def gru_seq_tile(n_seq):
    """the sequences per workgroup (one of _lib.GRU_TILES) that hh_gru_seq_forward / _backward use for n_seq sequences: what the
    environment variable HH_GRU_TILE forces (read at every call; another value is an error), else the rule of DESIGN.md section 19"""
    tile = L.lib().hh_gru_seq_tile(int(n_seq))
    L.check(min(tile, 0))
    return tile


def gru_seq_forward(parts, seq_len):
    """hh_gru_seq_forward on G = len(parts) GRUs: parts = [(gi [S, L, 600], h0 [S, 200], w_hh [600, 200], b_hh [600]), ...] contiguous
    float32 CUDA tensors, seq_len i32 [S] -> (ys: list of [S, L, 200], scratch: what gru_seq_backward needs).  No autograd."""
    G = len(parts)
    S, Lm = parts[0][0].shape[:2]
    dev = parts[0][0].device
    nbytes = _gru_scratch_bytes(G, S, Lm)
    scratch = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
    ys = [torch.empty((S, Lm, GRU_H), dtype=torch.float32, device=dev) for _ in range(G)]
    io = _gru_io(G)
    for g, ((gi, h0, w_hh, b_hh), y) in enumerate(zip(parts, ys)):
        io[g].gi, io[g].h0, io[g].w_hh, io[g].b_hh, io[g].y = gi.data_ptr(), h0.data_ptr(), w_hh.data_ptr(), b_hh.data_ptr(), y.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.lib().hh_gru_seq_forward(G, S, Lm, io, _p(seq_len), _p(scratch), nbytes, st))
    return ys, scratch


def gru_seq_backward(parts, ys, dys, seq_len, scratch):
    """hh_gru_seq_backward: parts / ys / scratch of gru_seq_forward, dys = d loss / d y per GRU
    -> per GRU (d_gi [S, L, 600], d_gh [S, L, 600], d_h0 [S, 200])"""
    G = len(parts)
    S, Lm = parts[0][0].shape[:2]
    dev = parts[0][0].device
    out = [(torch.empty((S, Lm, 3 * GRU_H), dtype=torch.float32, device=dev), torch.empty((S, Lm, 3 * GRU_H), dtype=torch.float32, device=dev),
            torch.empty((S, GRU_H), dtype=torch.float32, device=dev)) for _ in range(G)]
    io = _gru_io(G)
    for g, ((gi, h0, w_hh, b_hh), y, dy, (d_gi, d_gh, d_h0)) in enumerate(zip(parts, ys, dys, out)):
        io[g].h0, io[g].w_hh, io[g].y, io[g].dy = h0.data_ptr(), w_hh.data_ptr(), y.data_ptr(), dy.data_ptr()
        io[g].d_gi, io[g].d_gh, io[g].d_h0 = d_gi.data_ptr(), d_gh.data_ptr(), d_h0.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.lib().hh_gru_seq_backward(G, S, Lm, io, _p(seq_len), _p(scratch), scratch.numel() * 4, st))
    return out


class _GruSeq(torch.autograd.Function):
    """forward: hh_gru_seq_forward over G GRUs; backward: hh_gru_seq_backward, then dW_hh = d_gh^T h_prev (one batched GEMM) and db_hh =
    the column sums of d_gh per GRU"""

    @staticmethod
    def forward(ctx, seq_len, *flat):
        parts = [tuple(t.detach().contiguous() for t in flat[4 * g:4 * g + 4]) for g in range(len(flat) // 4)]
        ys, scratch = gru_seq_forward(parts, seq_len)
        ctx.parts, ctx.seq_len, ctx.scratch = parts, seq_len, scratch
        ctx.save_for_backward(*ys)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        ys = ctx.saved_tensors
        dys = [torch.zeros_like(y) if d is None else d.contiguous() for d, y in zip(dys, ys)]
        grads = [None]
        for (gi, h0, w_hh, b_hh), y, (d_gi, d_gh, d_h0) in zip(ctx.parts, ys, gru_seq_backward(ctx.parts, ys, dys, ctx.seq_len, ctx.scratch)):
            h_prev = torch.cat((h0[:, None], y[:, :-1]), dim=1)       # beyond seq_len d_gh is 0, whatever h_prev holds there
            # dW_hh step by step (a batch of L GEMMs over the S sequences, then their sum), as autograd accumulates it for the stepped cell:
            # one reduction over all S L rows loses about three times as much in float32 (measured against float64 at S = 1000)
            d_w = torch.bmm(d_gh.permute(1, 2, 0), h_prev.transpose(0, 1)).sum(dim=0)
            grads += [d_gi, d_h0, d_w, d_gh.sum(dim=(0, 1))]
        return tuple(grads)


def _check_gru(gi, h0, w_hh, b_hh, seq_len):
    S, Lm = gi.shape[:2]
    ok = (gi.is_cuda and all(t.dtype == torch.float32 and t.device == gi.device for t in (gi, h0, w_hh, b_hh)) and seq_len.dtype == torch.int32
          and seq_len.device == gi.device and tuple(gi.shape) == (S, Lm, 3 * GRU_H) and tuple(h0.shape) == (S, GRU_H)
          and tuple(w_hh.shape) == (3 * GRU_H, GRU_H) and tuple(b_hh.shape) == (3 * GRU_H,) and tuple(seq_len.shape) == (S,))
    if not ok:
        raise ValueError("gru_sequence: float32 CUDA tensors gi [S, L, 600], h0 [S, 200], w_hh [600, 200], b_hh [600] and seq_len int32 [S] on "
                         "one device (the torch-op form for other dtypes and devices is gru_sequence_torch)")


def gru_sequence(gi, h0, w_hh, b_hh, seq_len):
    """One nn.GRU(200, 200) layer over S padded sequences with the input projection already applied, fused (hh_gru_seq_forward /
    hh_gru_seq_backward, include/hh_learner.h): gi f32 [S, L, 600] = x W_ih^T + b_ih, h0 f32 [S, 200], w_hh f32 [600, 200], b_hh f32 [600]
    (gate rows r | z | n), seq_len i32 [S] with 0 <= seq_len[s] <= L <= 32 and seq_len[0] >= 1, all CUDA -> y f32 [S, L, 200], exactly 0 at
    steps t >= seq_len; differentiable with respect to gi, h0, w_hh and b_hh.  A sequence of length 0 (a padding slot of a staged
    minibatch) gives exact zeros in y and in the gradients of its gi and h0 and changes no other sequence's bytes.  The sequences per
    workgroup (gru_seq_tile) do not change the result.  No host synchronisation; a missing library or GPU is an error."""
    _check_gru(gi, h0, w_hh, b_hh, seq_len)
    return _GruSeq.apply(seq_len.contiguous(), gi, h0, w_hh, b_hh)[0]


def gru_sequence_pair(act, val, seq_len):
    """two GRUs over the same sequences in the same two launches (CommanderGru's rnn_act and rnn_val): act, val = (gi, h0, w_hh, b_hh)
    as for gru_sequence -> (y_act, y_val)"""
    _check_gru(*act, seq_len)
    _check_gru(*val, seq_len)
    if act[0].shape != val[0].shape:
        raise ValueError("gru_sequence_pair: both GRUs run over the same [S, L] sequences")
    return _GruSeq.apply(seq_len.contiguous(), *act, *val)


def gru_cell_torch(gi_t, h, w_hh, b_hh):
    """one step of torch.nn.GRU from the projected input gi_t [S, 600] (gate columns r | z | n), with torch ops"""
    gh = h @ w_hh.T + b_hh
    ir, iz, inn = gi_t.split(GRU_H, dim=-1)
    hr, hz, hn = gh.split(GRU_H, dim=-1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(inn + r * hn)
    return (1.0 - z) * n + z * h


def gru_sequence_torch(gi, h0, w_hh, b_hh, seq_len):
    """gru_sequence with torch ops, any dtype and device (the A/B partner): the same cell stepped L times; a sequence's state stops at
    its seq_len and y is 0 from there on"""
    h, ys = h0, []
    for t in range(gi.shape[1]):
        on = (seq_len > t)[:, None]
        hn = gru_cell_torch(gi[:, t], h, w_hh, b_hh)
        h = torch.where(on, hn, h)
        ys.append(torch.where(on, hn, torch.zeros_like(hn)))
    return torch.stack(ys, dim=1)


# ------------------------------------------------------------------------------------------------------------------ the loss
class _PPOLossCat(torch.autograd.Function):
    """_PPOLoss for the commander's Categorical (hh_ppo_loss_categorical)"""

    @staticmethod
    def forward(ctx, logits, vf, old_logits, actions, old_logp, adv, target, mask, n_valid, prm):
        R = logits.shape[0]
        dev = logits.device
        stats = torch.empty((len(L.PPO_STATS),), dtype=torch.float64, device=dev)
        d_logits, d_vf = torch.empty_like(logits), torch.empty_like(vf)
        nbytes = C.c_int64()
        lib = L.lib()
        L.check(lib.hh_ppo_loss_scratch_bytes(R, C.byref(nbytes)))
        scratch = torch.empty((nbytes.value // 8,), dtype=torch.float64, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(lib.hh_ppo_loss_categorical(R, _p(logits), _p(old_logits), _p(actions), _p(old_logp), _p(adv), _p(vf), _p(target), _p(mask),
                                            _p(n_valid), C.byref(prm), _p(stats), _p(d_logits), _p(d_vf), _p(scratch), nbytes.value, st))
        ctx.save_for_backward(d_logits, d_vf)
        ctx.mark_non_differentiable(stats)
        return stats[0].float(), stats

    @staticmethod
    def backward(ctx, g_total, g_stats):
        d_logits, d_vf = ctx.saved_tensors
        return (d_logits * g_total, d_vf * g_total) + (None,) * 8


def _flat_batch_cat(logits, vf, batch):
    """_flat_batch for the commander: logits [..., 3 | 4] -> [R, 4] rows (a zero column added to 3), old_logits [R, 4], actions i8 [R]"""
    if logits.shape[-1] == CMD_LD - 1:
        logits = F.pad(logits, (0, 1))
    if logits.shape[-1] != CMD_LD:
        raise ValueError("the commander's logits are rows of 3 (or 4, the last ignored) floats")
    logits = logits.reshape(-1, CMD_LD)
    R = logits.shape[0]
    col = lambda k, dt, w=None: batch[k].reshape((R,) if w is None else (R, w)).to(dt).contiguous()
    mask = batch.get("mask")
    mask = None if mask is None else col("mask", torch.uint8)
    n_valid = batch.get("n_valid")
    if n_valid is None:
        n_valid = (torch.full((1,), R, dtype=torch.int32, device=logits.device) if mask is None
                   else mask.ne(0).sum(dtype=torch.int32).reshape(1))
    return (logits, vf.reshape(R), col("old_logits", torch.float32, CMD_LD), col("actions", torch.int8), col("old_logp", torch.float32),
            col("adv", torch.float32), col("target", torch.float32), mask, n_valid.reshape(1))


def ppo_loss_categorical(logits, vf, batch, *, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2):
    """ppo_loss for the commander's TorchCategorical over 3 actions, fused (hh_ppo_loss_categorical).  logits f32 [..., 3] or [..., 4]
    (column 3 ignored, gradient exactly 0) and vf f32 [...]: CUDA, with autograd history.  batch: old_logits f32 [..., 4] (the sampler's
    logits rows), actions i8 [...], old_logp / adv / target f32 [...]; optional mask and n_valid as for ppo_loss.
    -> (total loss, stats f64 [6]) as ppo_loss.  No host synchronisation, no fallback."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and vf.dtype == torch.float32):
        raise ValueError("ppo_loss_categorical: logits and vf are float32 CUDA tensors (the torch-op form for other dtypes is ppo_loss_categorical_torch)")
    flat = _flat_batch_cat(logits, vf.contiguous(), batch)
    prm = L.HHPpoLossParams(n_comp=1, reserved0=0, clip_param=clip_param, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff,
                            entropy_coeff=entropy_coeff, kl_coeff=kl_coeff, reserved1=0.0)
    return _PPOLossCat.apply(flat[0].contiguous(), *flat[1:], prm)


def ppo_loss_categorical_torch(logits, vf, batch, *, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2):
    """the same loss with torch ops in the dtype of `logits` (CommanderLearner(fused=False)); same arguments, same results up to rounding"""
    logits, vf, old_logits, actions, old_logp, adv, target, mask, n_valid = _flat_batch_cat(logits, vf, batch)
    dt = logits.dtype
    lp, lq = F.log_softmax(logits[:, :CMD_LD - 1], dim=1), F.log_softmax(old_logits[:, :CMD_LD - 1].to(dt), dim=1)
    a = actions.long().clamp(0, CMD_LD - 2)
    logp = lp.gather(1, a[:, None]).squeeze(1)
    ent = -(lp.exp() * lp).sum(dim=1)
    kl = (lq.exp() * (lq - lp)).sum(dim=1)
    ratio = torch.exp(logp - old_logp.to(dt))
    A = adv.to(dt)
    surrogate = torch.min(A * ratio, A * torch.clamp(ratio, 1 - clip_param, 1 + clip_param))
    vf_loss = torch.clamp(torch.pow(vf - target.to(dt), 2.0), 0, vf_clip_param)
    w = torch.ones_like(ratio) if mask is None else mask.ne(0).to(dt)
    n = n_valid.to(dt)[0]
    mean = lambda t: (t * w).sum() / n
    total = mean(-surrogate + vf_loss_coeff * vf_loss - entropy_coeff * ent)
    mean_kl = mean(kl) if kl_coeff > 0.0 else torch.zeros((), dtype=dt, device=logits.device)
    if kl_coeff > 0.0:
        total = total + kl_coeff * mean_kl
    stats = torch.stack([total, mean(-surrogate), mean(vf_loss), mean_kl, mean(ent), n]).detach().double()
    return total, stats


# ------------------------------------------------------------------------------------------------------------------ the network
class _GRUWeights(nn.Module):
    """the four tensors of an nn.GRU(200, 200) layer under nn.GRU's names and its initialisation (uniform in +- 1 / sqrt(200))"""

    def __init__(self, n_in=GRU_H, hidden=GRU_H):
        super().__init__()
        k = hidden ** -0.5
        u = lambda *shape: nn.Parameter(torch.empty(shape).uniform_(-k, k))
        self.weight_ih_l0, self.weight_hh_l0 = u(3 * hidden, n_in), u(3 * hidden, hidden)
        self.bias_ih_l0, self.bias_hh_l0 = u(3 * hidden), u(3 * hidden)


class CommanderTrainable(nn.Module):
    """models/ac_models_hier.py:CommanderGru in training form, written from commander.state_keys() and the restatement of its forward in
    tests/commander_ref.py; `state_dict()` has exactly commander.state_keys()' keys and shapes, in that order, so it goes straight into
    `CommanderNet.refresh_weights`.  ONE shared_layer object serves the actor and the value branch.

    forward(obs_own [S, L, 34], critic_row [S, L, 105], state_in [S, 2, 200], seq_len [S], fused_gru=True) -> (logits [S, L, 3], value [S, L]):
    S sequences of L steps of one agent each, sequence s holding seq_len[s] steps and then padding; state_in[:, 0] / [:, 1] are the states
    rnn_act / rnn_val start from.  critic_row is rollout.central_critic_rows_hl's layout [a_own, a_o1, a_o2 | obs_own | obs_o1 | obs_o2];
    v1..v3 see [obs_k | act_k], v4 all three.  The GRU outputs are 0 at padded steps, whose logits and values mean nothing.
    fused_gru=True runs both GRUs through gru_sequence_pair (CUDA, float32, seq_len int32); False steps the same cell with torch ops on
    any device and dtype.  return_states=True appends (h_act, h_val) [S, 200] each: the states after each sequence's last step.
    inputs = "fused" (float32 on the GPU) runs inp1..inp4 and v1..v4 as one input_stage each (commander_stage_tables()) that read obs_own and
    critic_row as they are; the default "torch" slices, concatenates and runs the eight layers one by one.  state_dict() is the same.
    trunk = "fused" (float32 on the GPU) runs shared_layer, its bias and tanh over the actor's and the critic's rows as ONE dense_tanh; the
    default "torch" applies the layer twice.  state_dict() is the same; independent of `inputs`.
    heads = "fused" (trunk="torch"): TrainableNet's argument — `pre_heads(obs_own, critic_row, state_in, seq_len, fused_gru=True) -> (za, zc)`
    [S, L, 500] is the forward up to shared_layer's pre-activations, for heads_loss(n_comp=1); `forward` and state_dict() are unchanged."""

    def __init__(self, inputs="torch", trunk="torch", heads="torch"):
        super().__init__()
        self.trunk = _trunk_mode(trunk)
        self.heads = _heads_mode(heads, self.trunk)
        if inputs not in INPUT_MODES:
            raise ValueError(f"inputs is one of {INPUT_MODES}, got {inputs!r}")
        self.inputs = inputs
        self.shared_layer = _FC(500, 500)
        self.rnn_act, self.rnn_val = _GRUWeights(), _GRUWeights()
        self.inp1, self.inp2, self.inp3, self.inp4 = _FC(4, 50), _FC(20, 200), _FC(10, 50), _FC(34, 200)
        self.act_out = _FC(500, 3)
        self.v1, self.v2, self.v3, self.v4 = _FC(35, 100), _FC(35, 100), _FC(35, 100), _FC(105, 200)
        self.val_out = _FC(500, 1)

    def _front(self, obs_own, critic_row, state_in, seq_len, fused_gru):
        """-> (the actor's rows, the critic's rows as shared_layer sees them, y_a, y_v: the GRUs' outputs)"""
        if self.inputs == "fused":
            tables = commander_stage_tables()
            x, x_full = input_stage(obs_own.contiguous(), *stage_groups(self, COMMANDER_STAGE_LAYERS["actor"], tables["actor"]))
            z, z_full = input_stage(critic_row.contiguous(), *stage_groups(self, COMMANDER_STAGE_LAYERS["critic"], tables["critic"]))
        else:
            x = torch.cat((torch.tanh(self.inp1(obs_own[..., :4])), torch.tanh(self.inp2(obs_own[..., 4:24])),
                           torch.tanh(self.inp3(obs_own[..., 24:]))), dim=-1)
            x_full = torch.tanh(self.inp4(obs_own))
            a = critic_row[..., :3]
            o = [critic_row[..., 3 + 34 * k:3 + 34 * (k + 1)] for k in range(3)]
            v = [torch.cat((o[k], a[..., k:k + 1]), dim=-1) for k in range(3)]
            z = torch.cat([torch.tanh(m(vk)) for m, vk in zip((self.v1, self.v2, self.v3), v)], dim=-1)
            z_full = torch.tanh(self.v4(torch.cat(v, dim=-1)))
        ra, rv = self.rnn_act, self.rnn_val
        gi_a = x_full @ ra.weight_ih_l0.T + ra.bias_ih_l0
        gi_v = z_full @ rv.weight_ih_l0.T + rv.bias_ih_l0
        act = (gi_a, state_in[:, 0], ra.weight_hh_l0, ra.bias_hh_l0)
        val = (gi_v, state_in[:, 1], rv.weight_hh_l0, rv.bias_hh_l0)
        if fused_gru:
            y_a, y_v = gru_sequence_pair(act, val, seq_len)
        else:
            y_a, y_v = gru_sequence_torch(*act, seq_len), gru_sequence_torch(*val, seq_len)
        x_full = F.normalize(x_full + y_a, dim=-1)
        z_full = F.normalize(z_full + y_v, dim=-1)
        return torch.cat((x, x_full), dim=-1), torch.cat((z, z_full), dim=-1), y_a, y_v

    def pre_heads(self, obs_own, critic_row, state_in, seq_len, fused_gru=True):
        """forward up to shared_layer's pre-activations -> (za, zc) [S, L, 500]: what heads_loss(n_comp=1) takes.  trunk="torch" only."""
        if self.trunk == "fused":
            raise ValueError('pre_heads needs trunk="torch": dense_tanh has the tanh inside')
        xa, xc, _, _ = self._front(obs_own, critic_row, state_in, seq_len, fused_gru)
        return self.shared_layer(xa), self.shared_layer(xc)

    def forward(self, obs_own, critic_row, state_in, seq_len, fused_gru=True, return_states=False):
        xa, xc, y_a, y_v = self._front(obs_own, critic_row, state_in, seq_len, fused_gru)
        if self.trunk == "fused":
            lin = self.shared_layer._model[0]
            h, y = dense_tanh((xa, xc), lin.weight, lin.bias)
            logits, value = self.act_out(h), self.val_out(y).squeeze(-1)
        else:
            logits = self.act_out(torch.tanh(self.shared_layer(xa)))
            value = self.val_out(torch.tanh(self.shared_layer(xc))).squeeze(-1)
        if not return_states:
            return logits, value
        last = (seq_len.long() - 1).clamp(min=0)[:, None, None].expand(-1, 1, GRU_H)
        return logits, value, y_a.gather(1, last)[:, 0], y_v.gather(1, last)[:, 0]

    load_numpy = TrainableNet.load_numpy


# ------------------------------------------------------------------------------------------------------------------ the learner
def standardize_masked(adv, mask):
    """`standardize` over the rows that `mask` keeps (RLlib standardises the train batch before it is padded); 0 elsewhere"""
    w = mask.to(adv.dtype)
    n = w.sum()
    mean = (adv * w).sum() / n
    std = torch.sqrt((((adv - mean) * w) ** 2).sum() / n)
    return (adv - mean) / torch.clamp(std, min=1e-4) * w


class CommanderLearner:
    """One PPO update of train_hier.py's commander_policy from the `CommanderEpisodeBatch` of a
    `CommanderRollout(batch_mode="complete_episodes")` — for the commander what `PPOLearner` is for the 2-vs-2 policies:

        learner = CommanderLearner.trainable_init(device, seed=6)          # the weights of commander.random_weights(6)
        stats = learner.update(ro.episodes, net)
        learner.publish(net)                                               # CommanderNet.refresh_weights: captured collects replay with them

    Defaults: train_hier.py:186 (lr 1e-4, clip_param 0.25, kl_target 0.05, sgd_minibatch_size 256) and RLlib 2.4's PPO defaults for the
    rest (kl_coeff 0.2, vf_clip_param 10, num_sgd_iter 30, max_seq_len 20 — the rollout cuts the sequences, with the same max_seq_len:
    `update` refuses a batch cut to another length).
      * the three agents map to ONE policy: one module, one Adam.  The batch is the three agents' trajectories: 3 S sequences from
        `episodes.sequences()`'s S, AGENT-MAJOR — sequence a S + s is agent a's column of arena-row sequence s, with that agent's
        state_in[s, a], its own observation, and critic rows from central_critic_rows_hl (actions filled in, while the batch's `vf` and
        the stored rnn_val states were sampled with zero action inputs: RLlib has that difference, and so does this);
      * nothing is masked by `valid`; the mask is the unpadded steps.  Advantages are standardised over the whole batch (all three
        agents' unpadded rows);
      * old_logits (RLlib's ACTION_DIST_INPUTS): `batch_old_logits`.  With CommanderRollout(record_logits=True) the sequences carry a
        `logits` column — for every step the logits of the sampler's own forward (the split-fp16 MFMA kernel that drew the action
        and wrote logp), with the weights it held at that step — and it is used as it stands, agent-major like the other columns:
        old_logp and old_logits of a row come from one forward, also for rows sampled before the last publish.
        Without the column they are recomputed once per update, under no_grad, by the module's own float32 forward with the
        pre-update weights from the stored sequence-start states.  Only then does this approximation apply: that forward is not the
        sampler's, and rows carried over from before the last publish (the head of an episode that was still running) were sampled
        by older weights — their stored logp, and so the ratio, is exact, but their recomputed old_logits are the newer weights', so
        the KL term sees them as on-policy (`rollout.start()` after `publish` avoids that part by throwing the running episodes away);
      * num_sgd_iter passes; in each the sequences, in batch order, are split into consecutive minibatches of at least
        sgd_minibatch_size unpadded rows (minibatch_partition), visited in the order of minibatch_order(seed, update count, 0, pass);
      * after the passes KLCoeffMixin.update_kl (kl_coeff_update) on the mean of the minibatches' mean_kl.
    fused = False computes the loss with torch ops (ppo_loss_categorical_torch) and steps the GRU cell with torch ops
    (gru_sequence_torch) instead of hh_ppo_loss_categorical and hh_gru_seq_*; nothing else differs.
    optimizer="fused", step="graph" replays every minibatch step from one captured HIP graph, as PPOLearner's do (graph_prepare;
    DESIGN.md section 19): the same minibatches in the same order, no Python, autograd dispatch or torch.optim.Adam between launches."""

    @_heads_keyword
    def __init__(self, state_dict, device, lr=1e-4, clip_param=0.25, kl_target=0.05, kl_coeff=0.2, vf_clip_param=10.0, vf_loss_coeff=1.0,
                 entropy_coeff=0.0, num_sgd_iter=30, sgd_minibatch_size=256, max_seq_len=20, seed=0, fused=True, inputs="torch", trunk="torch",
                 optimizer="torch", step="eager", shuffle_sequences=False, grad_clip=None):
        """state_dict: CommanderGru's tensors (numpy or torch), keyed like commander.state_keys().  inputs: CommanderTrainable's argument
        ("fused": inp1..inp4 and v1..v4 through hh_input_stage_*); trunk: its argument too ("fused": shared_layer through hh_dense_tanh_*).
        optimizer, step: PPOLearner's arguments, with its values, defaults and validation.  optimizer="fused" makes `self.optimizer` a
        DeviceAdam (m, v and the step count on the device: hh_adam_step) and gathers the steps' statistics in a device table
        (hh_train_commit); step="graph" (needs optimizer="fused") captures stage -> stage -> forward -> loss -> backward -> Adam -> commit
        once as ONE HIP graph and replays it per minibatch step (graph_prepare).  The modes are kept in `optimizer_mode` and `step`.
        grad_clip: PPOLearner's argument (None: nothing changes; else the global L2 norm of the module's gradients is clipped to it in every
        step — norm -> clipped Adam in the fused modes and in the graph — and update() also returns grad_gnorm).
        shuffle_sequences: PPOLearner's argument (False, the default: nothing changes).  True: every pass draws its own order of the 3 S
        sequences, sequence_order(seed, update count, 0, pass), and cuts that order into minibatches (shuffled_schedule); state_in and
        seq_len travel with their sequences.  The eager modes gather with index_select; the graph's two stage launches become
        hh_minibatch_stage_gather through one order table of 4 * num_sgd_iter * 3 S bytes, uploaded once per update into a persistent
        buffer (grown to twice the need).  Slot 0 of a staged minibatch is a real sequence, so seq_len[0] >= 1 holds as before.  What
        shuffling does to learning curves has not been measured here.
        heads (keyword only, taken by _heads_keyword in front of this signature): PPOLearner's argument ("torch", the default: nothing changes; "fused", with fused=True and trunk="torch": the
        step's forward stops at CommanderTrainable.pre_heads and the tail is one hh_heads_loss with n_comp = 1)."""
        self.optimizer_mode = _learner_options(
            self, "CommanderLearner", device, optimizer, step, grad_clip, shuffle_sequences, kl_coeff, fused,
            dict(clip_param=clip_param, kl_target=kl_target, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff, entropy_coeff=entropy_coeff),
            dict(num_sgd_iter=num_sgd_iter, sgd_minibatch_size=sgd_minibatch_size, max_seq_len=max_seq_len, seed=seed), self._heads_arg, trunk)
        self.inputs, self.trunk = inputs, _trunk_mode(trunk)
        self.module = CommanderTrainable(inputs=inputs, trunk=trunk, heads=self.heads).load_numpy({k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
                                                       for k, v in state_dict.items()}).to(self.device)
        # the one policy's driver.  hh_minibatch_stage takes 8 columns: the per-step columns (chunks of max_seq_len rows) in one launch, the
        # per-sequence ones (state_in, seq_len: chunks of one row) in a second
        # (heads="fused": the forward callable stops at the pre-activations and the loss callable is the fused tail)
        args = lambda mb: (mb["obs"], mb["critic"], mb["state_in"], mb["seq_len"])
        tail = self.heads == "fused"
        self._sgd = _PolicySGD(self, self.module, lr, kl_coeff, self.optimizer_mode == "fused",
                               forward=(lambda mb: self.module.pre_heads(*args(mb), fused_gru=self.fused)) if tail else (lambda mb: self.module(*args(mb), fused_gru=self.fused)),
                               loss=self.heads_loss if tail else self.loss, stage_groups=lambda names: [(names[:L.STAGE_MAX_COLS], self.max_seq_len), (names[L.STAGE_MAX_COLS:], 1)],
                               policy=0, noun="sequences")
        self.optimizer, self._book = self._sgd.optimizer, self._sgd.book

    @property
    def kl_coeff(self):
        """the current coefficient of the KL term (the driver holds it; update_kl moves it after the passes)"""
        return self._sgd.kl_coeff

    @kl_coeff.setter
    def kl_coeff(self, value):
        self._sgd.kl_coeff = float(value)

    @classmethod
    def trainable_init(cls, device, seed=0, **kw):
        """the learner whose weights equal commander.random_weights(seed)'s (what CommanderNet.set_weights(random_weights(seed)) samples with)"""
        from .commander import random_weights
        return cls(random_weights(seed), device, seed=seed, **kw)

    # ---- the batch
    @staticmethod
    def policy_batch(seqs, old_logits=None):
        """the training batch from CommanderEpisodeBatch.sequences()' dict (S arena-row sequences of L steps): dict of agent-major
        [3 S, L, ...] tensors — obs [.., 34], critic [.., 105], actions i8, old_logp, adv (standardised over all unpadded rows), target,
        mask u8, and per sequence state_in [3 S, 2, 200] and seq_len i32 [3 S]; old_logits f32 [3 S, L, 4] where given"""
        obs, actions, mask = seqs["obs"], seqs["actions"], seqs["mask"]
        agents = range(obs.shape[2])
        cat = lambda f: torch.cat([f(a) for a in agents], dim=0).contiguous()
        m3 = cat(lambda a: mask)
        b = {"obs": cat(lambda a: obs[:, :, a]),
             "critic": cat(lambda a: central_critic_rows_hl(obs, actions, a + 1)),
             "actions": cat(lambda a: actions[:, :, a]), "old_logp": cat(lambda a: seqs["logp"][:, :, a]),
             "adv": standardize_masked(cat(lambda a: seqs["adv"][:, :, a]), m3), "target": cat(lambda a: seqs["target"][:, :, a]),
             "mask": m3.to(torch.uint8), "state_in": cat(lambda a: seqs["state_in"][:, a]),
             "seq_len": cat(lambda a: seqs["seq_lens"]).to(torch.int32)}
        if old_logits is not None:
            b["old_logits"] = old_logits
        return b

    def old_logits(self, b, chunk=4096):
        """the module's logits of every row of policy_batch's dict with the weights as they stand, no autograd -> f32 [3 S, L, 4] (column 3 zero)"""
        out = []
        with torch.no_grad():
            for s0 in range(0, b["obs"].shape[0], chunk):
                sl = slice(s0, s0 + chunk)
                lg, _ = self.module(b["obs"][sl], b["critic"][sl], b["state_in"][sl], b["seq_len"][sl], fused_gru=self.fused)
                out.append(F.pad(lg, (0, 1)))
        return torch.cat(out, dim=0) if out else torch.zeros(tuple(b["obs"].shape[:2]) + (CMD_LD,), device=b["obs"].device)

    def batch_old_logits(self, seqs, b=None):
        """old_logits f32 [3 S, L, 4], agent-major, of CommanderEpisodeBatch.sequences()' dict: its own `logits` column [S, L, 3, 4] where
        the rollout recorded one (no forward); otherwise the module's (old_logits; b: policy_batch(seqs), built when not given)"""
        if "logits" in seqs:
            lg = seqs["logits"]
            if lg.dtype != torch.float32 or tuple(lg.shape) != tuple(seqs["obs"].shape[:3]) + (CMD_LD,):
                raise ValueError(f"the sequences' logits column must be f32 [S, L, 3, {CMD_LD}], got {lg.dtype} {tuple(lg.shape)}")
            return torch.cat([lg[:, :, a] for a in range(lg.shape[2])], dim=0).contiguous()
        return self.old_logits(self.policy_batch(seqs) if b is None else b)

    # ---- one minibatch step
    def loss(self, logits, vf, mb, kl_coeff=None):
        """the loss of one minibatch; kl_coeff: the KL term's coefficient, default the current one"""
        kw = dict(clip_param=self.clip_param, vf_clip_param=self.vf_clip_param, vf_loss_coeff=self.vf_loss_coeff,
                  entropy_coeff=self.entropy_coeff, kl_coeff=self._sgd.kl_term() if kl_coeff is None else kl_coeff)
        return (ppo_loss_categorical if self.fused else ppo_loss_categorical_torch)(logits, vf, mb, **kw)

    def heads_loss(self, za, zc, mb, kl_coeff=None):
        """heads="fused": the loss of one minibatch from pre_heads' (za, zc), through heads_loss(n_comp=1) with the module's act_out and
        val_out; the gradients are handed to total.backward() unscaled"""
        m = self.module
        return heads_loss(za, zc, m.act_out, m.val_out, mb, n_comp=1, clip_param=self.clip_param, vf_clip_param=self.vf_clip_param,
                          vf_loss_coeff=self.vf_loss_coeff, entropy_coeff=self.entropy_coeff,
                          kl_coeff=self._sgd.kl_term() if kl_coeff is None else kl_coeff, scale_grad=False)

    def _columns(self, b, staged=False):
        """policy_batch's dict (with old_logits) as the driver takes it -> (columns [3 S, ...], host seq_len [3 S]).  staged: as the graph's
        two stages read them — the ten COMMANDER_STAGE_COLS in that order, eight per step and then state_in and seq_len per sequence,
        contiguous, mask uint8 and seq_len int32.  The sequences of the staging buffers beyond a minibatch's are zero in every column:
        sequences of length 0 (hh_gru_seq_*'s contract) whose rows the mask drops"""
        if not staged:
            return b, b["seq_len"].cpu().numpy()
        missing = [k for k in COMMANDER_STAGE_COLS if k not in b]
        if missing:
            raise ValueError(f"graph_prepare: the policy batch lacks {missing} (policy_batch, then old_logits from batch_old_logits)")
        cols = {k: b[k].contiguous() for k in COMMANDER_STAGE_COLS}
        cols["mask"], cols["seq_len"] = cols["mask"].to(torch.uint8), cols["seq_len"].to(torch.int32)
        return cols, cols["seq_len"].cpu().numpy()

    # the steps themselves are the driver's (_PolicySGD), as PPOLearner's are
    def minibatch_step(self, mb):
        """forward, loss, backward, Adam step on one minibatch (a dict sliced from policy_batch's, with old_logits and n_valid)
        -> stats f64 [6] (device)"""
        return self._sgd.minibatch_step(mb)

    def graph_prepare(self, b, cap=None):
        """Everything one update needs before its first replay (_PolicySGD.graph_prepare on policy_batch `b` with old_logits): the schedule
        and the batch's ten columns uploaded, the cursor set to 0, and the graph of ONE minibatch step — stage (per-step columns), stage
        (per-sequence columns), forward, loss, backward, Adam, commit — captured unless an earlier one still fits.  cap: the staging
        capacity in sequences.  -> (n_steps, rows)"""
        if self.step != "graph":
            raise ValueError('graph_prepare needs CommanderLearner(step="graph")')
        return self._sgd.graph_prepare(*self._columns(b, staged=True), cap)

    def graph_replay(self, n=1):
        """n minibatch steps from the captured graph, no host work between them"""
        self._sgd.graph_replay(n)

    def graph_stats(self, n):
        """the statistics rows f64 [n, 6] of the first n steps since graph_prepare (one device tensor; reading it synchronises)"""
        return self._sgd.graph_stats(n)

    def grad_gnorm(self, n):
        """grad_clip: the mean of the first n steps' norms before clipping since the update began (a float; reading it synchronises)"""
        return self._sgd.grad_gnorm(n)

    # ---- one update
    def update(self, episodes, net=None):
        """one PPO update of commander_policy from episodes (a CommanderEpisodeBatch after a collect) -> dict: total_loss, policy_loss,
        vf_loss, kl, entropy (means over the minibatch steps), kl_coeff (after the update), steps (minibatch steps taken), rows (unpadded,
        all three agents).  `net` (the sampler's CommanderNet) is not read: the old logits are the batch's own `logits` column or, without
        one, come from the module, which holds the weights the sampler was given at the last publish (batch_old_logits).  With grad_clip
        also grad_gnorm.  A CommanderEpisodeBatch built with train_batch_size hands over its accumulated batch (update once
        `episodes.ready()`, e.g. after `CommanderRollout.collect_batch()`); nothing else changes here."""
        seqs = episodes.sequences()
        if seqs["obs"].shape[1] != self.max_seq_len:
            raise ValueError(f"CommanderLearner(max_seq_len={self.max_seq_len}) was given sequences of {seqs['obs'].shape[1]} steps: the rollout "
                             "cuts them, so both take the same max_seq_len")
        if seqs["obs"].shape[0] == 0:
            return self._sgd.empty()
        with torch.no_grad():
            b = self.policy_batch(seqs)
            b["old_logits"] = self.batch_old_logits(seqs, b)
        out = self._sgd.run(*self._columns(b, staged=self.step == "graph"))
        self.updates += 1
        return out

    # ---- one update from a fixed window (batch_mode = "truncate_episodes")
    def window_sequences(self, rollout):
        """a CommanderRollout's [T, N] window in CommanderEpisodeBatch.sequences()' format: the window cut by THIS learner's max_seq_len
        (window_cut; the rollout's own max_seq_len is not read) and whole step-rows gathered by hh_window_gather — obs f32 [S, L, 3, 34],
        actions i8 / logp / vf / adv / target [S, L, 3] (zero past seq_len), seq_lens i32 [S], mask bool [S, L], state_in f32
        [S, 3, 2, 200] = rollout.state_in[seq_t0, seq_arena] (the state the sequence's first step used: zero at an episode start, the
        carried one where the window or a length cut opens mid-episode), and logits f32 [S, L, 3, 4] where the rollout recorded them.
        Sequences arena-major, then time."""
        for k in ("obs", "actions", "logp", "vf", "adv", "target", "done", "state_in", "T"):
            if not hasattr(rollout, k):
                raise ValueError(f"window_sequences takes a CommanderRollout (its [T, N] buffers and state_in); this object has no `{k}`")
        if rollout.obs.dim() != 4 or tuple(rollout.obs.shape[2:]) != (3, 34) or tuple(rollout.state_in.shape[2:]) != (3, 2, GRU_H):
            raise ValueError(f"the rollout's observations {tuple(rollout.obs.shape[2:])} / states {tuple(rollout.state_in.shape[2:])} are not the "
                             "3-agent commander's ((3, 34) / (3, 2, 200))")
        if not getattr(rollout, "collects", 0):
            raise RuntimeError("the rollout has not collected yet: its window buffers hold nothing (rollout.collect() first)")
        Lm = self.max_seq_len
        tables = window_cut(rollout.done, Lm)
        names = ["obs", "actions", "logp", "vf", "adv", "target"] + (["logits"] if getattr(rollout, "record_logits", False) else [])
        cols = [(getattr(rollout, k), tuple(getattr(rollout, k).shape[2:]), 0, k == "state_in") for k in names + ["state_in"]]   # eight at most: one launch
        out = dict(zip(names + ["state_in"], window_gather(cols, tables, Lm)))
        out["seq_lens"] = tables[2]
        out["mask"] = chunk_mask(tables[2].long(), Lm)
        return out

    def update_window(self, rollout):
        """one PPO update of commander_policy from a CommanderRollout's [T, N] window as the last collect left it (batch_mode =
        "truncate_episodes", the rollouts' default; the buffers are the same in both modes) -> what `update` returns, rows = 3 T N:

            ro.collect();  stats = learner.update_window(ro);  learner.publish(net)

        window_sequences, then `update`'s own policy_batch, batch_old_logits and driver.  The trailing fragment of an arena carries
        RLlib's truncation bootstrap from vf[T] in adv and target.  The rollout's buffers are only read."""
        with torch.no_grad():
            seqs = self.window_sequences(rollout)
            b = self.policy_batch(seqs)
            b["old_logits"] = self.batch_old_logits(seqs, b)
        out = self._sgd.run(*self._columns(b, staged=self.step == "graph"))
        self.updates += 1
        return out

    def publish(self, net):
        """the new weights into the sampler's CommanderNet on the current stream (refresh_weights): captured collects replay with them"""
        net.refresh_weights(self.module.state_dict())
