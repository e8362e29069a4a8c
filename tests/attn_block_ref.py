"""One attention block of a fight network, y = normalize(x + out_proj(attention(in_proj(x)))), and its backward, restated step by step
in torch (float64 unless told otherwise) — what learner.attention_block is measured against.  Shared by test_attn_block_host.py, which
pins it to nn.MultiheadAttention + F.normalize and autograd, and by the GPU tests."""
import torch

HEADS, EPS = 2, 1e-12
NAMES = ("y", "d_x", "d_in_w", "d_in_b", "d_out_w", "d_out_b")


def _heads(t):
    """[S, L, E] -> [S, HEADS, L, E / HEADS]"""
    S, Lm, E = t.shape
    return t.reshape(S, Lm, HEADS, E // HEADS).transpose(1, 2)


def _merge(t):
    """[S, HEADS, L, d] -> [S, L, HEADS d]"""
    S, H, Lm, d = t.shape
    return t.transpose(1, 2).reshape(S, Lm, H * d)


def forward(x, in_w, in_b, out_w, out_b):
    """-> (y, what backward needs)"""
    E = x.shape[-1]
    d = E // HEADS
    qkv = x @ in_w.T + in_b
    q, k, v = (_heads(t) for t in qkv.split(E, dim=-1))
    s = (q @ k.transpose(-1, -2)) / d ** 0.5
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    p = p / p.sum(dim=-1, keepdim=True)
    ctx = _merge(p @ v)
    a = ctx @ out_w.T + out_b
    sm = x + a
    nrm = (sm * sm).sum(dim=-1, keepdim=True).sqrt()
    y = sm / nrm.clamp_min(EPS)
    return y, (x, in_w, out_w, q, k, v, p, ctx, y, nrm)


def backward(kept, d_y):
    """-> (d_x, d_in_w, d_in_b, d_out_w, d_out_b); below a norm of EPS the clamp holds the denominator: d_s = d_y / EPS"""
    x, in_w, out_w, q, k, v, p, ctx, y, nrm = kept
    E = x.shape[-1]
    d = E // HEADS
    d_s = torch.where(nrm >= EPS, (d_y - y * (y * d_y).sum(dim=-1, keepdim=True)) / nrm.clamp_min(EPS), d_y / EPS)
    flat = lambda t: t.reshape(-1, t.shape[-1])
    d_out_w, d_out_b = flat(d_s).T @ flat(ctx), flat(d_s).sum(dim=0)
    dO = _heads(d_s @ out_w)
    d_v = p.transpose(-1, -2) @ dO
    d_p = dO @ v.transpose(-1, -2)
    d_sc = p * (d_p - (p * d_p).sum(dim=-1, keepdim=True)) / d ** 0.5
    d_qkv = torch.cat([_merge(d_sc @ k), _merge(d_sc.transpose(-1, -2) @ q), _merge(d_v)], dim=-1)
    d_in_w, d_in_b = flat(d_qkv).T @ flat(x), flat(d_qkv).sum(dim=0)
    return d_s + d_qkv @ in_w, d_in_w, d_in_b, d_out_w, d_out_b


def make_case(E, Lm, S, seed, padded=True):
    """float64 CPU tensors (x, in_w, in_b, out_w, out_b, d_y): weights at nn.MultiheadAttention's scale, biases that are not zero, and
    (padded) every third sequence zero from some step on, as pad_chunks leaves a ragged chunk"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float64)
    x = rn(S, Lm, E)
    if padded:
        for s in range(0, S, 3):
            x[s, (s // 3) % Lm:] = 0.0
    return x, rn(3 * E, E) * (2.0 / (4 * E)) ** 0.5 * 1.7, rn(3 * E) * 0.3, rn(E, E) * E ** -0.5, rn(E) * 0.3, rn(S, Lm, E)


def reference(args, dtype=torch.float64, device=None):
    """the block and its backward on make_case's tensors in `dtype` -> {name: tensor in float64} for NAMES"""
    x, in_w, in_b, out_w, out_b, d_y = (t.to(device=device, dtype=dtype) for t in args)
    y, kept = forward(x, in_w, in_b, out_w, out_b)
    return dict(zip(NAMES, (t.double() for t in (y,) + backward(kept, d_y))))
