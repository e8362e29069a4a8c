"""The fused layer ops with their torch twins: chunk attention and residual normalize, the input stage and its layout tables,
dense_tanh, and the GRU sequence op"""
import ctypes as C

import torch
import torch.nn.functional as F

from .. import _lib as L
from .. import policy_nets as PN
from ._ffi import _fused_input, _need_gpu, _p, _stream

# ------------------------------------------------------------------------------------------------------------------ the chunk attention
ATTENTION_MODES = ("torch", "fused", "block")


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


def attention_block_tile(n_seq, seq_len, embed):
    """(sequences per workgroup tile, workgroups of the backward's first launch) of an attention_block call (hh_attn_block_tile)"""
    spt, nwg = C.c_int32(), C.c_int32()
    L.check(L.lib().hh_attn_block_tile(int(n_seq), int(seq_len), int(embed), C.byref(spt), C.byref(nwg)))
    return spt.value, nwg.value


def _attn_block_bytes(fn, S, Lm, E):
    nbytes = C.c_int64()
    L.check(fn(S, Lm, E, C.byref(nbytes)))
    return nbytes.value


class _AttnBlock(torch.autograd.Function):
    """forward: hh_attn_block_forward, keeping qkv, ctx and the norms in `save`; backward: hh_attn_block_backward.  save and scratch are
    torch allocations: inside a captured step they come from the graph's pool"""

    @staticmethod
    def forward(ctx, x, in_w, in_b, out_w, out_b):
        S, Lm, E = x.shape
        w = [t.detach().contiguous() for t in (in_w, in_b, out_w, out_b)]
        y = torch.empty_like(x)
        lib = L.lib()
        nbytes = _attn_block_bytes(lib.hh_attn_block_save_bytes, S, Lm, E)
        save = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
        L.check(lib.hh_attn_block_forward(S, Lm, E, _p(x), _p(w[0]), _p(w[1]), _p(w[2]), _p(w[3]), _p(y), _p(save), nbytes, _stream(x.device)))
        ctx.save_for_backward(x, w[0], w[2], y, save)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_y):
        x, w_in, w_out, y, save = ctx.saved_tensors
        S, Lm, E = x.shape
        dev = x.device
        new = torch.zeros if S == 0 else torch.empty        # n_seq == 0 launches nothing: the gradients of an empty call are zeros
        d_x = torch.empty_like(x)
        d_w_in, d_b_in = new((3 * E, E), dtype=torch.float32, device=dev), new((3 * E,), dtype=torch.float32, device=dev)
        d_w_out, d_b_out = new((E, E), dtype=torch.float32, device=dev), new((E,), dtype=torch.float32, device=dev)
        lib = L.lib()
        nbytes = _attn_block_bytes(lib.hh_attn_block_scratch_bytes, S, Lm, E)
        scratch = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        L.check(lib.hh_attn_block_backward(S, Lm, E, _p(x), _p(w_in), _p(w_out), _p(y), _p(save), save.numel() * 4, _p(d_y.contiguous()), _p(d_x),
                                           _p(d_w_in), _p(d_b_in), _p(d_w_out), _p(d_b_out), _p(scratch), nbytes, _stream(dev)))
        return d_x, d_w_in, d_b_in, d_w_out, d_b_out


def attention_block(x, in_w, in_b, out_w, out_b):
    """F.normalize(x + nn.MultiheadAttention(E, 2, batch_first=True)(x, x, x)[0], dim=-1) as ONE launch forward and two backward
    (hh_attn_block_forward / hh_attn_block_backward, include/hh_learner.h): x f32 [S, L, E], contiguous, CUDA, E = 100 | 150,
    1 <= L <= 32; in_w [3E, E], in_b [3E], out_w [E, E], out_b [E] the module's in_proj_weight, in_proj_bias, out_proj.weight and
    out_proj.bias -> f32 [S, L, E].  No mask: a zero-padded row is a key like any other.  Differentiable with respect to all five (first
    order); the same inputs give the same bytes.  No host synchronisation; a missing library or GPU is an error."""
    _need_gpu("attention_block")
    _fused_input("attention_block", x, "x")
    if x.dim() != 3 or x.shape[2] not in L.ATTN_WIDTHS or not 1 <= x.shape[1] <= L.ATTN_MAX_LEN:
        raise ValueError(f"attention_block: x is [S, L, E] with E in {L.ATTN_WIDTHS} and 1 <= L <= {L.ATTN_MAX_LEN}, got {tuple(x.shape)}")
    E = x.shape[2]
    for what, t, shape in (("in_w", in_w, (3 * E, E)), ("in_b", in_b, (3 * E,)), ("out_w", out_w, (E, E)), ("out_b", out_b, (E,))):
        if not (t.is_cuda and t.dtype == torch.float32 and t.device == x.device and tuple(t.shape) == shape):
            raise ValueError(f"attention_block: {what} is a float32 CUDA tensor {shape} on x's device (the torch-op form is attention_block_torch)")
    return _AttnBlock.apply(x, in_w, in_b, out_w, out_b)


def attention_block_torch(x, in_w, in_b, out_w, out_b):
    """attention_block with torch ops, any dtype and device (the A/B partner): the two projections around chunk_attention_torch, then
    residual_normalize_torch"""
    return residual_normalize_torch(x, F.linear(chunk_attention_torch(F.linear(x, in_w, in_b)), out_w, out_b))


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


# ------------------------------------------------------------------------------------------------------------------ the GRU
GRU_H = 200     # HH_GRU_HIDDEN


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


# ------------------------------------------------------------------------------------------------------------------ gradients of W shards
def grad_layout(tensors):
    """where a list of gradients lies in its bucket: tensors (or their element counts) in list order, each starting at the next multiple
    of 4 elements -> (ns, offs, bucket_elems), bucket_elems a multiple of 4"""
    ns = [int(t.numel()) if isinstance(t, torch.Tensor) else int(t) for t in tensors]
    offs, at = [], 0
    for n in ns:
        if n < 0:
            raise ValueError("grad_layout: an element count is >= 0")
        offs.append(at)
        at += (n + 3) // 4 * 4
    return ns, offs, at


def _grad_desc(who, grads, layout, dev):
    ns, offs, _ = layout
    if not (len(grads) == len(ns) == len(offs)):
        raise ValueError(f"{who}: one layout entry per gradient ({len(grads)} gradients, {len(ns)} entries)")
    desc = (L.HHGradTensor * max(len(grads), 1))()
    for i, (g, n, off) in enumerate(zip(grads, ns, offs)):
        if g is not None and not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.device == dev and g.numel() == n):
            raise ValueError(f"{who}: a gradient is None or a contiguous float32 CUDA tensor of its layout entry's {n} elements on the bucket's device "
                             f"(the torch-op form is {who}_torch)")
        desc[i].g, desc[i].n, desc[i].off = (None if g is None else g.data_ptr()), n, off
    return desc


def grad_pack(grads, bucket, layout=None):
    """A module's gradients into one flat bucket, the block an all-gather moves (hh_grad_pack, include/hh_learner.h): grads is a list of
    contiguous float32 CUDA tensors or None (a parameter without .grad), layout grad_layout's triple for them (default: grad_layout(grads),
    then without None), bucket a contiguous float32 [bucket_elems] CUDA tensor, 16-byte aligned.  Gradient i goes to
    bucket[offs[i] : offs[i] + ns[i]] byte for byte; the range of a None and all padding are written as +0.0.  -> bucket.
    ceil(n / 64) launches, no host synchronisation, HIP-graph capturable; a missing library or GPU is an error."""
    _need_gpu("grad_pack")
    grads = list(grads)
    layout = grad_layout(grads) if layout is None else layout
    if not (isinstance(bucket, torch.Tensor) and bucket.is_cuda and bucket.dtype == torch.float32 and bucket.is_contiguous() and bucket.dim() == 1
            and bucket.numel() == layout[2]):
        raise ValueError(f"grad_pack: bucket is a contiguous float32 [{layout[2]}] CUDA tensor (the torch-op form is grad_pack_torch)")
    desc = _grad_desc("grad_pack", grads, layout, bucket.device)
    L.check(L.lib().hh_grad_pack(len(grads), desc, _p(bucket), bucket.numel(), _stream(bucket.device)))
    return bucket


def grad_pack_torch(grads, layout=None, device=None):
    """grad_pack with torch ops, any device -> a new bucket float32 [bucket_elems]: zeros, then every gradient that is not None copied in"""
    grads = list(grads)
    ns, offs, E = grad_layout(grads) if layout is None else layout
    if device is None:
        device = next((g.device for g in grads if g is not None), "cpu")
    bucket = torch.zeros((E,), dtype=torch.float32, device=device)
    for g, n, off in zip(grads, ns, offs):
        if g is not None:
            bucket[off:off + n] = g.detach().reshape(-1)
    return bucket


def _shard_weights(who, weight, W):
    w = [float(x) for x in weight]
    if len(w) != W or not 1 <= W <= L.GRAD_MAX_SHARDS:
        raise ValueError(f"{who}: one weight per shard, 1 .. {L.GRAD_MAX_SHARDS} shards (got {len(w)} weights for {W} buckets)")
    return w


def grad_combine(grads, buckets, weight, layout=None):
    """The gathered buckets of W shards back into the gradients, added in shard order (hh_grad_combine, include/hh_learner.h): buckets a
    contiguous float32 [W, bucket_elems] CUDA tensor, weight W host floats (float64), grads the tensors to write — contiguous float32 CUDA
    tensors, or None for a parameter that receives nothing — and layout their grad_layout (default: grad_layout(grads)).  Per element
        acc = float64(b[0]) * weight[0];  acc = acc + float64(b[r]) * weight[r]  for r = 1 .. W-1;  g = float32(acc)
    with every product and sum rounded on its own: the same bytes on every rank and for every W that presents the same shards; W = 1 with
    weight 1.0 returns the bucket's bytes.  In place on grads.  ceil(n / 64) launches, no host synchronisation, HIP-graph capturable."""
    _need_gpu("grad_combine")
    grads = list(grads)
    layout = grad_layout(grads) if layout is None else layout
    if not (isinstance(buckets, torch.Tensor) and buckets.is_cuda and buckets.dtype == torch.float32 and buckets.is_contiguous() and buckets.dim() == 2
            and buckets.shape[1] == layout[2]):
        raise ValueError(f"grad_combine: buckets is a contiguous float32 [W, {layout[2]}] CUDA tensor (the torch-op form is grad_combine_torch)")
    W = buckets.shape[0]
    w = (C.c_double * max(W, 1))(*_shard_weights("grad_combine", weight, W))
    desc = _grad_desc("grad_combine", grads, layout, buckets.device)
    L.check(L.lib().hh_grad_combine(len(grads), desc, _p(buckets), buckets.shape[1], W, w, _stream(buckets.device)))


def grad_combine_torch(buckets, weight, layout):
    """grad_combine with torch ops, any device (the A/B partner): float64 products and sums in shard order, rounded to float32 once
    -> per layout entry a new flat float32 tensor [ns[i]]"""
    ns, offs, E = layout
    w = _shard_weights("grad_combine_torch", weight, buckets.shape[0])
    acc = buckets[0].double() * w[0]
    for r in range(1, len(w)):
        acc = acc + buckets[r].double() * w[r]
    flat = acc.float()
    return [flat[off:off + n].clone() for n, off in zip(ns, offs)]
