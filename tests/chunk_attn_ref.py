"""Inputs and float64 references for the chunk-attention tests (test_chunk_attention_host.py, test_gpu_chunk_attention.py): the core
between nn.MultiheadAttention's two projections (learner.chunk_attention_torch) and normalize(x + a) (learner.residual_normalize_torch),
each with its autograd.  References are computed once per case and shared: callers must not write into what they get."""
import functools

import torch

from hhmarl_2d_amd import learner as LR

HEADS = 2
SCALES = (1.0, 3.0)


@functools.lru_cache(maxsize=None)
def core_inputs(S, Lm, E, scale, seed=0):
    """qkv [S, L, 3E] = randn * scale with a constant tail in sequence 1 (what zero-padded rows give after the in-projection: equal rows)
    and sequence 2 all rows equal (uniform probabilities); d_ctx [S, L, E] = randn"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * S + 3 * Lm + E + int(10 * scale))
    qkv = torch.randn((S, Lm, 3 * E), generator=g) * scale
    if S > 1:
        qkv[1, Lm // 2:] = 0.25
    if S > 2:
        qkv[2] = qkv[2, :1].clone()
    return qkv, torch.randn((S, Lm, E), generator=g)


def core_run(qkv, d_ctx, dtype, device, fn=None):
    """fn (default: the torch-op restatement) and its autograd in `dtype` on `device` -> (ctx, d_qkv), float64 on the CPU"""
    q = qkv.to(device=device, dtype=dtype).requires_grad_(True)
    ctx = (fn or LR.chunk_attention_torch)(q)
    ctx.backward(d_ctx.to(device=device, dtype=dtype))
    return ctx.detach().double().cpu(), q.grad.double().cpu()


@functools.lru_cache(maxsize=None)
def core_reference(S, Lm, E, scale, seed=0):
    return core_run(*core_inputs(S, Lm, E, scale, seed), torch.float64, "cpu")


@functools.lru_cache(maxsize=None)
def norm_inputs(R, E, zero_row, seed=0):
    """x, a, d_y [R, E]; zero_row: the row where a = -x (None: no such row)"""
    g = torch.Generator().manual_seed(1000 * seed + 5 * R + E)
    x, a, d_y = (torch.randn((R, E), generator=g) for _ in range(3))
    if zero_row is not None:
        a[zero_row] = -x[zero_row]
    return x, a, d_y


def norm_run(x, a, d_y, dtype, device, fn=None):
    """-> (y, d_x, d_a), float64 on the CPU"""
    xs, as_ = (t.to(device=device, dtype=dtype).requires_grad_(True) for t in (x, a))
    y = (fn or LR.residual_normalize_torch)(xs, as_)
    y.backward(d_y.to(device=device, dtype=dtype))
    return y.detach().double().cpu(), xs.grad.double().cpu(), as_.grad.double().cpu()


@functools.lru_cache(maxsize=None)
def norm_reference(R, E, zero_row, seed=0):
    return norm_run(*norm_inputs(R, E, zero_row, seed), torch.float64, "cpu")


def rel_err(got, want):
    """max |difference| / max |reference| of one compared tensor"""
    return (got - want).abs().max().item() / want.abs().max().item()
