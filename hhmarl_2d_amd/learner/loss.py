"""The PPO losses: hh_ppo_loss, hh_ppo_loss_categorical and hh_heads_loss behind autograd Functions, each with its torch twin.  All of them
shape the batch with _batch_rows and fill hh_ppo_loss_params with _loss_params; the torch twins differ in their distribution and share
_loss_tail_torch."""
import ctypes as C

import torch
import torch.nn.functional as F

from .. import _lib as L
from .. import policy_nets as PN
from ._ffi import _need_gpu, _p, _stream

OLD_LD = 32   # HH_POLICY_LOGITS: row width of the sampler's logits
CMD_LD = 4      # HH_CMD_LOGITS: row width of hh_commander_sample's logits and of hh_ppo_loss_categorical's


def n_comp_of(kind):
    """action components of the kind's MultiDiscrete: 4 ([13, 9, 2, 2], 26 logits) for type-1 aircraft, 3 ([13, 9, 2], 24) for type-2"""
    return 4 if PN.N_OUT[kind] == 26 else 3


# ------------------------------------------------------------------------------------------------------------------ what every loss shares
def _batch_rows(R, batch, old_ld, act_w, device):
    """the batch columns as contiguous rows for R rows of learner outputs -> (old_logits f32 [R, old_ld], actions i8 [R, act_w] ([R] for
    act_w None), old_logp, adv, target f32 [R], mask u8 [R] | None, n_valid i32 [1]: made on the device where the batch has none)"""
    col = lambda k, dt, w=None: batch[k].reshape((R,) if w is None else (R, w)).to(dt).contiguous()
    mask = batch.get("mask")
    mask = None if mask is None else col("mask", torch.uint8)
    n_valid = batch.get("n_valid")
    if n_valid is None:
        n_valid = (torch.full((1,), R, dtype=torch.int32, device=device) if mask is None
                   else mask.ne(0).sum(dtype=torch.int32).reshape(1))
    return (col("old_logits", torch.float32, old_ld), col("actions", torch.int8, act_w), col("old_logp", torch.float32), col("adv", torch.float32),
            col("target", torch.float32), mask, n_valid.reshape(1))


def _loss_params(n_comp, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """hh_ppo_loss_params (_lib.HHPpoLossParams) for one call; n_comp 1 is the commander's Categorical"""
    return L.HHPpoLossParams(n_comp=int(n_comp), reserved0=0, clip_param=clip_param, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff,
                             entropy_coeff=entropy_coeff, kl_coeff=kl_coeff, reserved1=0.0)


def _loss_kw(learner, sgd, kl_coeff):
    """the keywords both learners' `loss` and `heads_loss` hand on: the learner's four fixed hyper-parameters and the KL term's coefficient,
    by default the current one of the policy's driver `sgd` (_PolicySGD.kl_term)"""
    return dict(clip_param=learner.clip_param, vf_clip_param=learner.vf_clip_param, vf_loss_coeff=learner.vf_loss_coeff,
                entropy_coeff=learner.entropy_coeff, kl_coeff=sgd.kl_term() if kl_coeff is None else kl_coeff)


def _scratch(query, *dims, device):
    """the float64 scratch one of the hh_*_scratch_bytes entries asks for -> (tensor, its bytes)"""
    nbytes = C.c_int64()
    L.check(query(*dims, C.byref(nbytes)))
    return torch.empty((nbytes.value // 8,), dtype=torch.float64, device=device), nbytes.value


def _loss_tail_torch(logp, ent, kl, vf, rows, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """what the torch twins share behind their distribution: from the rows' log-probability, entropy and KL (in the dtype of the logits)
    and _batch_rows' columns to (total, stats)"""
    _, _, old_logp, adv, target, mask, n_valid = rows
    dt = logp.dtype
    ratio = torch.exp(logp - old_logp.to(dt))
    A = adv.to(dt)
    surrogate = torch.min(A * ratio, A * torch.clamp(ratio, 1 - clip_param, 1 + clip_param))
    vf_loss = torch.clamp(torch.pow(vf - target.to(dt), 2.0), 0, vf_clip_param)
    w = torch.ones_like(ratio) if mask is None else mask.ne(0).to(dt)
    n = n_valid.to(dt)[0]
    mean = lambda t: (t * w).sum() / n
    total = mean(-surrogate + vf_loss_coeff * vf_loss - entropy_coeff * ent)
    mean_kl = mean(kl) if kl_coeff > 0.0 else torch.zeros((), dtype=dt, device=logp.device)
    if kl_coeff > 0.0:
        total = total + kl_coeff * mean_kl
    stats = torch.stack([total, mean(-surrogate), mean(vf_loss), mean_kl, mean(ent), n]).detach().double()
    return total, stats


# ------------------------------------------------------------------------------------------------------------------ the loss
class _PPOLoss(torch.autograd.Function):
    """forward: hh_ppo_loss, or hh_ppo_loss_categorical where `categorical` (loss, stats and the gradients in one pass); backward: the kept
    gradients times the incoming one"""

    @staticmethod
    def forward(ctx, categorical, logits, vf, old_logits, actions, old_logp, adv, target, mask, n_valid, prm):
        R, ld = logits.shape
        dev = logits.device
        stats = torch.empty((len(L.PPO_STATS),), dtype=torch.float64, device=dev)
        d_logits, d_vf = torch.empty_like(logits), torch.empty_like(vf)
        lib = L.lib()
        scratch, nbytes = _scratch(lib.hh_ppo_loss_scratch_bytes, R, device=dev)
        entry, dims = (lib.hh_ppo_loss_categorical, (R,)) if categorical else (lib.hh_ppo_loss, (R, ld))     # the categorical's rows are CMD_LD wide
        L.check(entry(*dims, _p(logits), _p(old_logits), _p(actions), _p(old_logp), _p(adv), _p(vf), _p(target), _p(mask), _p(n_valid),
                      C.byref(prm), _p(stats), _p(d_logits), _p(d_vf), _p(scratch), nbytes, _stream(dev)))
        ctx.save_for_backward(d_logits, d_vf)
        ctx.mark_non_differentiable(stats)
        return stats[0].float(), stats

    @staticmethod
    def backward(ctx, g_total, g_stats):
        d_logits, d_vf = ctx.saved_tensors
        return (None, d_logits * g_total, d_vf * g_total) + (None,) * 8


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
    logits, vf = logits.contiguous(), vf.contiguous()
    logits = logits.reshape(-1, logits.shape[-1])
    R = logits.shape[0]
    rows = _batch_rows(R, batch, OLD_LD, 4, logits.device)
    return _PPOLoss.apply(False, logits, vf.reshape(R), *rows, _loss_params(n_comp, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff))


def ppo_loss_torch(logits, vf, batch, *, n_comp, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2):
    """the same loss with torch ops in the dtype of `logits` (PPOLearner(fused=False): the A/B and timing partner of ppo_loss; same
    arguments, same results up to rounding)"""
    logits = logits.reshape(-1, logits.shape[-1])
    R = logits.shape[0]
    rows = _batch_rows(R, batch, OLD_LD, 4, logits.device)
    old_logits, actions = rows[:2]
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
    return _loss_tail_torch(logp, ent, kl, vf.reshape(R), rows, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff)


def _categorical_rows(logits):
    """the commander's logits [..., 3 | 4] -> [R, 4] rows (a zero column added to 3)"""
    if logits.shape[-1] == CMD_LD - 1:
        logits = F.pad(logits, (0, 1))
    if logits.shape[-1] != CMD_LD:
        raise ValueError("the commander's logits are rows of 3 (or 4, the last ignored) floats")
    return logits.reshape(-1, CMD_LD)


def ppo_loss_categorical(logits, vf, batch, *, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2):
    """ppo_loss for the commander's TorchCategorical over 3 actions, fused (hh_ppo_loss_categorical).  logits f32 [..., 3] or [..., 4]
    (column 3 ignored, gradient exactly 0) and vf f32 [...]: CUDA, with autograd history.  batch: old_logits f32 [..., 4] (the sampler's
    logits rows), actions i8 [...], old_logp / adv / target f32 [...]; optional mask and n_valid as for ppo_loss.
    -> (total loss, stats f64 [6]) as ppo_loss.  No host synchronisation, no fallback."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and vf.dtype == torch.float32):
        raise ValueError("ppo_loss_categorical: logits and vf are float32 CUDA tensors (the torch-op form for other dtypes is ppo_loss_categorical_torch)")
    vf = vf.contiguous()
    logits = _categorical_rows(logits)
    R = logits.shape[0]
    rows = _batch_rows(R, batch, CMD_LD, None, logits.device)
    return _PPOLoss.apply(True, logits.contiguous(), vf.reshape(R), *rows, _loss_params(1, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff))


def ppo_loss_categorical_torch(logits, vf, batch, *, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2):
    """the same loss with torch ops in the dtype of `logits` (CommanderLearner(fused=False)); same arguments, same results up to rounding"""
    logits = _categorical_rows(logits)
    R = logits.shape[0]
    rows = _batch_rows(R, batch, CMD_LD, None, logits.device)
    old_logits, actions = rows[:2]
    dt = logits.dtype
    lp, lq = F.log_softmax(logits[:, :CMD_LD - 1], dim=1), F.log_softmax(old_logits[:, :CMD_LD - 1].to(dt), dim=1)
    a = actions.long().clamp(0, CMD_LD - 2)
    logp = lp.gather(1, a[:, None]).squeeze(1)
    ent = -(lp.exp() * lp).sum(dim=1)
    kl = (lq.exp() * (lq - lp)).sum(dim=1)
    return _loss_tail_torch(logp, ent, kl, vf.reshape(R), rows, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff)


# ------------------------------------------------------------------------------------------------------------------ the heads and the loss
HEADS_MODES = ("torch", "fused")


def _heads_mode(heads, trunk="torch"):
    if heads not in HEADS_MODES:
        raise ValueError(f"heads is one of {HEADS_MODES}, got {heads!r}")
    if heads == "fused" and trunk == "fused":
        raise ValueError('heads="fused" needs trunk="torch": dense_tanh has the tanh inside, so there are no pre-activations to hand over')
    return heads


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
        lib = L.lib()
        scratch, nbytes = _scratch(lib.hh_heads_loss_scratch_bytes, R, prm.n_comp, device=dev)
        L.check(lib.hh_heads_loss(R, _p(za), _p(zc), _p(w_act), _p(b_act), _p(w_val), _p(b_val), _p(old_logits), _p(actions), _p(old_logp), _p(adv),
                                  _p(target), _p(mask), _p(n_valid), C.byref(prm), _p(stats), *[_p(g) for g in grads], None, None, _p(scratch),
                                  nbytes, _stream(dev)))
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
    old_ld, act_w = (CMD_LD, None) if int(n_comp) == 1 else (OLD_LD, 4)
    rows = _batch_rows(za.numel() // L.HEADS_K, batch, old_ld, act_w, za.device)
    prm = _loss_params(n_comp, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff)
    return _HeadsLoss.apply(za, zc, w_act, b_act, w_val, b_val, *rows, prm, bool(scale_grad))


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
