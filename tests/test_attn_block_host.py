"""learner.attention_block / TrainableNet(attention="block") without a GPU: the torch-op twin and the float64 restatement that the GPU
tests measure the kernels against are pinned to the reference's own module class (nn.MultiheadAttention) with F.normalize and to
autograd, and the `attention` argument leaves the state dict alone and refuses what it cannot serve."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import attn_block_ref as REF
from hhmarl_2d_amd import learner as LR
from hhmarl_2d_amd import policy_nets as PN


def _close(got, want, what):
    """to 1e-12 of the tensor's scale (at least 1)"""
    err, scale = (got - want).abs().max().item(), max(1.0, want.abs().max().item())
    assert got.shape == want.shape and err <= 1e-12 * scale, (what, err, scale)


@pytest.mark.parametrize("Lm", (1, 7, 20))
@pytest.mark.parametrize("E", (100, 150))
def test_torch_twin_and_restatement_equal_multihead_attention(E, Lm):
    """attention_block_torch in float64, values and all five gradients, against F.normalize(x + nn.MultiheadAttention(E, 2,
    batch_first=True)(x, x, x)[0]) of the same parameters under autograd; zero-padded rows are keys like any other.  The hand-written
    backward of tests/attn_block_ref.py is held to the same."""
    x, in_w, in_b, out_w, out_b, d_y = REF.make_case(E, Lm, 7, 100 * E + Lm)
    assert not x[0].any() and x[1].all()
    att = nn.MultiheadAttention(E, 2, batch_first=True).double()
    with torch.no_grad():
        for p, t in ((att.in_proj_weight, in_w), (att.in_proj_bias, in_b), (att.out_proj.weight, out_w), (att.out_proj.bias, out_b)):
            p.copy_(t)
    xa = x.clone().requires_grad_(True)
    want = F.normalize(xa + att(xa, xa, xa, need_weights=False)[0], dim=-1)
    want.backward(d_y)
    want_g = (xa.grad, att.in_proj_weight.grad, att.in_proj_bias.grad, att.out_proj.weight.grad, att.out_proj.bias.grad)
    leaves = [t.clone().requires_grad_(True) for t in (x, in_w, in_b, out_w, out_b)]
    got = LR.attention_block_torch(*leaves)
    got.backward(d_y)
    ref = REF.reference((x, in_w, in_b, out_w, out_b, d_y))
    _close(got.detach(), want.detach(), "y")
    _close(ref["y"], want.detach(), "restated y")
    for name, leaf, w in zip(REF.NAMES[1:], leaves, want_g):
        _close(leaf.grad, w, name)
        _close(ref[name], w, "restated " + name)


def test_restatement_takes_the_clamp_branch_where_autograd_does():
    """a row whose x + a is exactly zero: y = 0 there and d_s = d_y / 1e-12"""
    E = 100
    x, in_w, in_b, out_w, out_b, d_y = REF.make_case(E, 4, 2, 5, padded=False)
    x[1], in_b, out_b = 0.0, torch.zeros_like(in_b), torch.zeros_like(out_b)
    leaves = [t.clone().requires_grad_(True) for t in (x, in_w, in_b, out_w, out_b)]
    y = LR.attention_block_torch(*leaves)
    y.backward(d_y)
    ref = REF.reference((x, in_w, in_b, out_w, out_b, d_y))
    assert not y[1].any() and not ref["y"][1].any()
    for name, leaf in zip(REF.NAMES[1:], leaves):
        _close(ref[name], leaf.grad, name)
    assert ref["d_out_b"].abs().max().item() > 1e11


@pytest.mark.parametrize("kind", (PN.FIGHT1, PN.FIGHT2))
def test_block_attention_keeps_the_state_dict(kind):
    want = {k: tuple(v.shape) for k, v in LR.TrainableNet(kind).state_dict().items()}
    m = LR.TrainableNet(kind, attention="block")
    assert m.attention == "block" and LR.TrainableNet(kind).attention == "torch" and LR.ATTENTION_MODES == ("torch", "fused", "block")
    assert list(want) == list(m.state_dict()) and want == {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert want == {k: tuple(v) for k, v in dict(PN.actor_keys(kind), **PN.critic_keys(kind)).items()}
    assert isinstance(m.att_act, nn.MultiheadAttention) and isinstance(m.att_val, nn.MultiheadAttention)


def test_block_is_refused_for_the_escape_kinds():
    for kind in (PN.ESC1, PN.ESC2):
        with pytest.raises(ValueError, match="has no attention"):
            LR.TrainableNet(kind, attention="block")
        with pytest.raises(ValueError, match="has no attention"):
            LR.TrainableNet(kind, attention="fused")


def test_block_function_refuses_cpu_tensors():
    """without a GPU a RuntimeError as PPOLearner raises; with one, CPU tensors are a ValueError: there is no CPU fallback either way"""
    err = ValueError if torch.cuda.is_available() else RuntimeError
    E = 100
    with pytest.raises(err):
        LR.attention_block(torch.zeros((2, 20, E)), torch.zeros((3 * E, E)), torch.zeros(3 * E), torch.zeros((E, E)), torch.zeros(E))
    m = LR.TrainableNet(PN.FIGHT1, attention="block")
    with pytest.raises(err):
        m(torch.zeros((2, 20, PN.OBS_DIM[PN.FIGHT1])), torch.zeros((2, 20, 57)))
