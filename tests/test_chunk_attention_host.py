"""The chunk attention of learner.TrainableNet(attention="fused") without a GPU: the torch-op restatements that the GPU tests measure the
kernels against are pinned to the reference's own module class (nn.MultiheadAttention: column order q | k | v, head split, scale) and to
F.normalize, and the `attention` argument leaves the state dict alone and refuses what it cannot serve."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from hhmarl_2d_amd import learner as LR
from hhmarl_2d_amd import policy_nets as PN


@pytest.mark.parametrize("Lm", (1, 2, 20))
@pytest.mark.parametrize("E", (100, 150))
def test_restatement_equals_multihead_attention(E, Lm):
    """F.linear + chunk_attention_torch + F.linear in float64 against nn.MultiheadAttention(E, 2, batch_first=True) of the same parameters;
    rtol 1e-12 (atol 1e-13), the project's bound for float64 restatements (test_learner_host.test_torch_loss_equals_restatement)"""
    torch.manual_seed(E + Lm)
    att = nn.MultiheadAttention(E, 2, batch_first=True).double()
    with torch.no_grad():
        att.in_proj_bias.normal_(0.0, 0.3)        # the module starts them at zero
        att.out_proj.bias.normal_(0.0, 0.3)
    x = torch.randn((7, Lm, E), dtype=torch.float64)
    x[1, Lm // 2:] = 0.0                          # zero-padded rows are keys like any other
    with torch.no_grad():
        want, _ = att(x, x, x, need_weights=False)
        qkv = F.linear(x, att.in_proj_weight, att.in_proj_bias)
        got = F.linear(LR.chunk_attention_torch(qkv), att.out_proj.weight, att.out_proj.bias)
    assert got.shape == want.shape
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-13), (got - want).abs().max().item()


def test_restatement_of_one_key_returns_the_v_columns():
    qkv = torch.randn((5, 1, 300))
    assert torch.equal(LR.chunk_attention_torch(qkv), qkv[..., 200:])


@pytest.mark.parametrize("E", (100, 150))
def test_residual_normalize_restatement_is_f_normalize(E):
    g = torch.Generator().manual_seed(E)
    x, a = torch.randn((9, 4, E), generator=g, dtype=torch.float64), torch.randn((9, 4, E), generator=g, dtype=torch.float64)
    a[3, 2] = -x[3, 2]
    got = LR.residual_normalize_torch(x, a)
    assert torch.equal(got, F.normalize(x + a, dim=-1))
    assert torch.equal(got[3, 2], torch.zeros(E, dtype=torch.float64))


@pytest.mark.parametrize("kind", (PN.FIGHT1, PN.FIGHT2))
def test_fused_attention_keeps_the_state_dict(kind):
    want = {k: tuple(v.shape) for k, v in LR.TrainableNet(kind).state_dict().items()}
    m = LR.TrainableNet(kind, attention="fused")
    assert m.attention == "fused" and LR.TrainableNet(kind).attention == "torch"
    assert list(want) == list(m.state_dict()) and want == {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert want == {k: tuple(v) for k, v in dict(PN.actor_keys(kind), **PN.critic_keys(kind)).items()}


def test_attention_argument_is_checked():
    with pytest.raises(ValueError):
        LR.TrainableNet(PN.FIGHT1, attention="flash")
    for kind in (PN.ESC1, PN.ESC2):
        with pytest.raises(ValueError):
            LR.TrainableNet(kind, attention="fused")
        assert LR.TrainableNet(kind, attention="torch").attention == "torch"


def test_fused_functions_refuse_cpu_tensors():
    """without a GPU a RuntimeError as PPOLearner raises; with one, CPU tensors are a ValueError: there is no CPU fallback either way"""
    err = ValueError if torch.cuda.is_available() else RuntimeError
    with pytest.raises(err):
        LR.chunk_attention(torch.zeros((2, 20, 300)))
    with pytest.raises(err):
        LR.residual_normalize(torch.zeros((2, 100)), torch.zeros((2, 100)))
    m = LR.TrainableNet(PN.FIGHT1, attention="fused")
    with pytest.raises(err):
        m(torch.zeros((2, 20, PN.OBS_DIM[PN.FIGHT1])), torch.zeros((2, 20, 57)))
