"""The minibatch step: the mode checks, the device norm, Adam, stage and commit wrappers, DeviceAdam, the step book and the driver
that both learners share"""
import ctypes as C
import functools
import gc
import math

import numpy as np
import torch

from .. import _lib as L
from .. import checkpoint as ck
from . import ops as _ops
from ._ffi import _need_gpu, _p, _stream
from .batch import kl_coeff_update, update_schedule
from .loss import _heads_mode

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


def _shuffle_flag(shuffle_sequences):
    """RLlib's shuffle_sequences: a bool and nothing else (1, "yes" and None are refused)"""
    if not isinstance(shuffle_sequences, bool):
        raise ValueError(f"shuffle_sequences is True or False, got {shuffle_sequences!r}")
    return shuffle_sequences


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


    # ---- checkpointing (hhmarl_2d_amd/checkpoint.py)
    def _options(self):
        return {"lr": self.lr, "betas": self.betas, "eps": self.eps, "max_norm": self.max_norm, "n": len(self.params)}

    def state_dict(self):
        """m and v per parameter (in parameter order) and the step count t, with the hyper-parameters they were taken under; the clip
        pair and the norm's scratch are rewritten by every step and not saved"""
        return {"options": self._options(), "m": [ck.cpu(x) for x in self.m], "v": [ck.cpu(x) for x in self.v], "t": ck.cpu(self.t)}

    def _load_plan(self, sd):
        ck.need_keys("DeviceAdam", sd, ("options", "m", "v", "t"))
        ck.check_options("DeviceAdam", sd["options"], self._options())
        pairs = []
        for name, live in (("m", self.m), ("v", self.v)):
            if not isinstance(sd[name], (list, tuple)) or len(sd[name]) != len(live):
                raise ValueError(f"DeviceAdam: `{name}` holds one tensor per parameter ({len(live)})")
            for i, (dst, src) in enumerate(zip(live, sd[name])):
                ck.check_tensor("DeviceAdam", f"{name}[{i}]", src, dst)
                pairs.append((dst, src))
        ck.check_tensor("DeviceAdam", "t", sd["t"], self.t)
        pairs.append((self.t, sd["t"]))
        return lambda: ck.copy_pairs(pairs)

    def load_state_dict(self, sd):
        """state_dict()'s dict into the existing m, v and t (copy_: a captured step graph holds their addresses); validated first"""
        self._load_plan(sd)()


def _torch_adam_state(opt):
    """torch.optim.Adam's own state_dict with CPU tensors: a plain dict (state by parameter index, param_groups of scalars)"""
    sd = opt.state_dict()
    return {"state": {int(i): {k: (ck.cpu(v) if isinstance(v, torch.Tensor) else v) for k, v in st.items()} for i, st in sd["state"].items()},
            "param_groups": [dict(g, params=list(g["params"])) for g in sd["param_groups"]]}


def _torch_adam_plan(opt, sd):
    """the validated load of _torch_adam_state's dict into a torch.optim.Adam over the same parameters"""
    ck.need_keys("torch.optim.Adam state", sd, ("state", "param_groups"))
    params = [p for g in opt.param_groups for p in g["params"]]
    live = opt.state_dict()["param_groups"]
    if not isinstance(sd["param_groups"], list) or len(sd["param_groups"]) != len(live):
        raise ValueError("optimizer: `param_groups` differs in length from the live optimizer's")
    for i, (a, b) in enumerate(zip(sd["param_groups"], live)):
        if not isinstance(a, dict) or set(a) != set(b):
            raise ValueError(f"optimizer: `param_groups[{i}]` has other keys than the live optimizer's")
        for k in b:
            va, vb = (tuple(x) if isinstance(x, (list, tuple)) else x for x in (a[k], b[k]))
            if va != vb:
                raise ValueError(f"optimizer: `param_groups[{i}].{k}` was {a[k]!r} when saved, the live optimizer has {b[k]!r}")
    if not isinstance(sd["state"], dict):
        raise ValueError("optimizer: `state` is a dict by parameter index")
    for i, st in sd["state"].items():
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < len(params) or not isinstance(st, dict):
            raise ValueError(f"optimizer: `state[{i!r}]` names no parameter of the live optimizer")
        for k in ("exp_avg", "exp_avg_sq"):
            if k not in st:
                raise ValueError(f"optimizer: `state[{i}]` has no `{k}`")
            ck.check_tensor("optimizer", f"state[{i}].{k}", st[k], params[i])
        if "step" not in st:
            raise ValueError(f"optimizer: `state[{i}]` has no `step`")

    def commit():
        opt.load_state_dict({"state": {i: dict(st) for i, st in sd["state"].items()}, "param_groups": [dict(g) for g in sd["param_groups"]]})
    return commit


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
        self._buckets = None    # run_sharded: the shards' gradient buckets f32 [W, bucket_elems], kept between updates
        self.forward, self.loss, self.stage_groups, self.policy, self.noun = forward, loss, stage_groups, int(policy), noun
        if device_adam:
            self.optimizer, self.book = DeviceAdam(module.parameters(), lr=lr, max_norm=cfg.grad_clip), _StepBook(cfg.device, gnorm=cfg.grad_clip is not None)
        else:
            self.optimizer, self.book = torch.optim.Adam(module.parameters(), lr=lr), None

    # ---- checkpointing (hhmarl_2d_amd/checkpoint.py)
    def state_dict(self):
        """kl_coeff and the optimizer's state (DeviceAdam's own, or torch.optim.Adam's); the step book holds nothing that outlives an update"""
        opt = self.optimizer
        return {"kl_coeff": float(self.kl_coeff), "adam": opt.state_dict() if self.book is not None else _torch_adam_state(opt)}

    def _load_plan(self, sd):
        ck.need_keys("the policy's driver", sd, ("kl_coeff", "adam"))
        if isinstance(sd["kl_coeff"], bool) or not isinstance(sd["kl_coeff"], float):
            raise ValueError("`kl_coeff` is a float")
        adam = self.optimizer._load_plan(sd["adam"]) if self.book is not None else _torch_adam_plan(self.optimizer, sd["adam"])

        def commit():
            adam()
            self.kl_coeff = sd["kl_coeff"]
        return commit

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
        # no cyclic collection inside the capture: torch.cuda.graph no longer collects before it begins, and a dead object that owns another
        # captured graph (its pool is freed when it goes) must not be finalised while this stream captures — the runtime refuses the free
        # and the destructor aborts the process.  Reference counting goes on as usual.
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph):       # what the forward allocates (the GRU's scratch and y among it) comes from the graph's pool as well
                stage()
                stats = forward_backward()
                opt.step()
                train_commit(stats, book.table, book.cursor, opt.t)
        finally:
            if gc_was_on:
                gc.enable()
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

    # ---- one update over W shards (learner/shards.py)
    def run_sharded(self, group, shards):
        """`run` as one of group.W data-parallel shards' — or, with LocalShards, as all of them one after another — so that W ranks write
        the bytes one process over the W shards writes.  shards: per entry of group.local (cols, seq_len) as `run` takes them, (None, [])
        for a shard without rows.  Collective, eager modes only.
          * every shard cuts its own batch with update_schedule at max(1, sgd_minibatch_size // W) rows (RLlib's per-device split) under
            the learner's unchanged keys; the schedules' unpadded-row columns are gathered once per update (shards.step_weights): global
            step i is shard r's i-th row or empty for r, max_r len steps, weight[i, r] = n_r[i] / sum_r n_r[i] in host float64;
          * per step every local shard runs forward, loss and backward as minibatch_step does (an empty one runs nothing) and its
            gradients, over the module's parameter list — the list grad_clip takes, the tied shared layer once — go into its bucket
            (grad_pack; zeros for an empty shard); the buckets are gathered; grad_combine writes the weighted sum, added in shard order,
            into every parameter's .grad (zeros where no shard reached a parameter);
          * from there the step is minibatch_step's: clip_grad_norm_ or DeviceAdam's norm, opt.step(), train_commit (the device table
            then holds this process's first shard's rows; the result is computed from all shards').  The combined gradient is the same
            bytes on every rank, so weights, m, v, t and the norms stay identical without a broadcast;
          * the steps' statistics rows are gathered at the end of the update and combined as sum_r weight_r stat_r in shard order, slot 5
            = the step's rows over all shards (shards.combine_stats), so every rank moves kl_coeff alike.
        -> the update's dict with steps and rows over all shards and rows_local, this process's rows.  One shard with weight 1.0 is `run`
        bit for bit."""
        from .shards import combine_stats, step_weights
        cfg, opt, book, clip, dev = self.cfg, self.optimizer, self.book, self.cfg.grad_clip, self.cfg.device
        size = max(1, cfg.sgd_minibatch_size // group.W)
        plans = []
        for cols, seq_len in shards:
            if cols is None or len(seq_len) == 0:
                plans.append((None, None, np.zeros((0, 4), dtype=np.int32), None))
                continue
            order, sched, _ = update_schedule(seq_len, size, cfg.num_sgd_iter, cfg.seed, cfg.updates, self.policy, cfg.shuffle_sequences)
            n_valid = torch.from_numpy(np.ascontiguousarray(sched[:, 2])).to(dev)
            if order is not None:
                order = torch.from_numpy(order).to(dev).long()
            plans.append((cols, order, sched, n_valid))
        rows_local = int(sum(int(np.sum(seq_len)) for _, seq_len in shards))
        per_shard = group.gather_ragged([p[2][:, 2] for p in plans])
        n, n_glob, weight = step_weights(per_shard)
        steps = len(n_glob)
        if steps == 0:
            return dict(self.empty(), rows_local=rows_local)
        rows = int(sum(int(c.sum()) for c in per_shard)) // cfg.num_sgd_iter      # every pass visits every row once
        params = list(self.module.parameters())
        layout = _ops.grad_layout(params)
        if self._buckets is None or tuple(self._buckets.shape) != (group.W, layout[2]):
            self._buckets = torch.zeros((group.W, layout[2]), dtype=torch.float32, device=dev)
        buckets, none = self._buckets, [None] * len(params)
        zero6 = torch.zeros((len(L.PPO_STATS),), dtype=torch.float64, device=dev)
        self.gnorms = []
        if book is not None:
            book.begin(steps, opt)
        kept = [[] for _ in plans]
        for i in range(steps):
            targets = None
            for j, r in enumerate(group.local):
                cols, order, sched, n_valid = plans[j]
                grads, stats = none, zero6
                if i < len(sched):
                    c0, c1 = int(sched[i, 0]), int(sched[i, 1])
                    if order is None:
                        mb = {k: v[c0:c1] for k, v in cols.items()}
                    else:
                        idx = order[c0:c1]
                        mb = {k: v.index_select(0, idx) for k, v in cols.items()}
                    mb["n_valid"] = n_valid[i:i + 1]
                    logits, vf = self.forward(mb)
                    total, stats = self.loss(logits, vf, mb, self.kl_term())
                    opt.zero_grad(set_to_none=True)
                    total.backward()
                    grads = [p.grad for p in params]
                    targets = grads if targets is None else targets
                kept[j].append(stats)
                _ops.grad_pack(grads, group.pack_target(buckets, r), layout)
            group.gather_buckets(buckets)
            # the sum goes into gradient tensors that are already packed (a local shard's own), or into new ones where there is none
            for k, p in enumerate(params):
                g = None if targets is None else targets[k]
                p.grad = torch.empty_like(p, memory_format=torch.contiguous_format) if g is None else g
            _ops.grad_combine([p.grad for p in params], buckets, weight[i], layout)
            if clip is not None and book is None:       # DeviceAdam: inside opt.step()
                self.gnorms.append(torch.nn.utils.clip_grad_norm_(self.module.parameters(), clip))
            opt.step()
            if book is not None:
                train_commit(kept[0][-1], book.table, book.cursor, opt.t)
        local = torch.stack([torch.stack(k) for k in kept]).cpu().numpy().reshape(len(kept), steps * len(L.PPO_STATS))
        table = combine_stats(group.gather_host(local).reshape(group.W, steps, len(L.PPO_STATS)), weight, n_glob)
        m = torch.from_numpy(table).to(dev).mean(dim=0).tolist()        # the reduction `run` makes, on the same device
        if cfg.use_kl:
            self.kl_coeff = kl_coeff_update(self.kl_coeff, m[3], cfg.kl_target)
        return dict(self.result(m, steps, rows), rows_local=rows_local)


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


def _shard_group(group, step):
    """a learner's `group`: None (the default: one process, nothing changes) or a learner/shards.py group — LocalShards(K) | ShardGroup —,
    eager step modes only"""
    if group is None:
        return None
    if not all(hasattr(group, k) for k in ("W", "local", "gather_host", "gather_ragged", "pack_target", "gather_buckets")):
        raise ValueError(f"group is None, a LocalShards or a ShardGroup (learner/shards.py), got {group!r}")
    if step == "graph":
        raise ValueError('group needs step="eager": the shards\' gather between backward and Adam is not captured into the step graph')
    return group


LEARNER_OPTIONS = ("seed", "num_sgd_iter", "sgd_minibatch_size", "max_seq_len", "shuffle_sequences", "grad_clip", "step", "fused", "heads", "use_kl",
                   "clip_param", "kl_target", "vf_clip_param", "vf_loss_coeff", "entropy_coeff")


def _learner_saved_options(learner, mode, **more):
    """the constructor options that decide a learner's arithmetic or its schedule, as its state dict records them"""
    return dict({k: getattr(learner, k) for k in LEARNER_OPTIONS}, optimizer=mode, **more)


def _module_plan(who, module, saved, skip=()):
    """a module's parameters and buffers from `saved` (its state_dict() without the keys `skip`), copied in place: tied layers stay tied"""
    live = {k: v for k, v in module.state_dict().items() if k not in skip}
    return ck.plan_tensors(who, saved, live)


def _heads_keyword(init):
    """a learner's __init__ with one more argument, `heads`, that can only be given by keyword: it is taken off before `init` runs and
    kept as `self._heads_arg`, which `init` hands to _learner_options for validation in its place.  The constructors' own signatures stay
    as they are — grad_clip their last parameter, so no positional caller moves — and functools.wraps keeps them what introspection
    and help() show; the docstrings describe `heads`.  `group` (learner/shards.py) is taken the same way and kept as `self._group_arg`."""
    @functools.wraps(init)
    def __init__(self, *args, heads="torch", group=None, **kw):
        self._heads_arg, self._group_arg = heads, group
        init(self, *args, **kw)
    return __init__
