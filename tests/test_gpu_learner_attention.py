"""learner.TrainableNet(attention="fused") and PPOLearner(attention="fused") on the MI355X: the forward against the reference's recorded
training-form outputs, every parameter's gradient and the loss statistics against a float64 run (the fused path at most 4 x as far
from it as the default path), and collect -> update -> publish rounds with the fused attention."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP, VCLIP = 0.25, 10.0
KW = dict(clip_param=CLIP, vf_clip_param=VCLIP, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)


def _weights(kind, seed):
    from hhmarl_2d_amd import policy_nets as PN
    return dict(PN.random_weights(kind, seed), **PN.random_critic_weights(kind, seed))


@pytest.mark.parametrize("kind", (0, 1))
def test_fused_forward_equals_reference_recording(kind):
    """tests/golden/fight_sequence_forward.npz (the reference's own Fight1 / Fight2 forward + value_function on padded chunks) within the
    1.5e-4 that tests/test_learner_host.py established for the file; padded rows are outputs like any other and are compared too"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    g = np.load(os.path.join(ROOT, "tests", "golden", "fight_sequence_forward.npz"))
    name = PN.KIND_NAMES[kind]
    seed = json.loads(str(g["meta"]))["seed"]
    m = LR.TrainableNet(kind, attention="fused").load_numpy(_weights(kind, seed)).cuda().eval()
    with torch.no_grad():
        logits, value = m(torch.from_numpy(g[f"{name}_obs"]).cuda(), torch.from_numpy(g[f"{name}_critic"]).cuda())
    dl = np.abs(logits.cpu().numpy() - g[f"{name}_logits"]).max()
    dv = np.abs(value.cpu().numpy() - g[f"{name}_value"]).max()
    print(f"{name}: max |logits - reference| = {dl:.3e}, max |value - reference| = {dv:.3e}")
    assert logits.shape == g[f"{name}_logits"].shape and value.shape == g[f"{name}_value"].shape
    assert dl <= 1.5e-4 and dv <= 1.5e-4


@pytest.mark.parametrize("flat", (False, True))
@pytest.mark.parametrize("kind", (0, 1))
def test_gradients_fused_against_torch_attention(kind, flat):
    """shaped like test_gpu_ppo_loss.test_autograd_into_the_network_fused_against_unfused (S = 96 chunks of 20, masked; flat: the same rows
    as 1920 chunks of length 1, the 2-D form): gradients and the first five statistics through attention="fused" and through
    attention="torch", each against a float64 run of the same module and loss (ppo_loss_torch in all three, so the attention is the only
    difference); the fused path's largest error is at most 4 x the torch path's"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(60 + kind)
    d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
    S, Lc = 96, 20
    n_comp = LR.n_comp_of(kind)
    own = torch.rand((S, Lc, d1), generator=g)
    crit = torch.cat([torch.rand((S, Lc, a1 + a2), generator=g), own, torch.rand((S, Lc, d2), generator=g)], dim=-1)
    mask = LR.chunk_mask(torch.randint(1, Lc + 1, (S,), generator=g), Lc)
    own, crit = own * mask[..., None], crit * mask[..., None]
    if flat:
        own, crit, mask = own.reshape(S * Lc, -1), crit.reshape(S * Lc, -1), mask.reshape(S * Lc)
    lead = tuple(own.shape[:-1])
    w = _weights(kind, 9)
    nets = {a: LR.TrainableNet(kind, attention=a).load_numpy(w).to(dev) for a in ("torch", "fused")}
    net64 = LR.TrainableNet(kind).load_numpy(w).double().to(dev)
    with torch.no_grad():
        old, _ = nets["torch"](own.to(dev), crit.to(dev))
    splits = PN.ACTION_SPLIT[:n_comp]
    old = old + 0.3 * torch.randn(old.shape, generator=g).to(dev)
    actions = torch.zeros(lead + (4,), dtype=torch.int8)
    for i, wd in enumerate(splits):
        actions[..., i] = torch.randint(0, wd, lead, generator=g).to(torch.int8)
    old32 = torch.zeros(lead + (32,), device=dev)
    old32[..., :old.shape[-1]] = old
    lo, old_logp = 0, torch.zeros(lead, device=dev)
    for i, wd in enumerate(splits):
        old_logp += torch.log_softmax(old[..., lo:lo + wd], dim=-1).gather(-1, actions[..., i:i + 1].long().to(dev)).squeeze(-1)
        lo += wd
    batch = {"old_logits": old32, "actions": actions.to(dev), "old_logp": old_logp, "adv": torch.randn(lead, generator=g).to(dev),
             "target": torch.randn(lead, generator=g).to(dev) * 2.0, "mask": mask.to(dev)}

    def grads(module, dt):
        module.zero_grad(set_to_none=True)
        logits, vf = module(own.to(dev, dt), crit.to(dev, dt))
        total, stats = LR.ppo_loss_torch(logits, vf, batch, n_comp=n_comp, **KW)
        total.backward()
        return {k: p.grad.double().clone() for k, p in module.named_parameters()}, stats.clone()

    g64, s64 = grads(net64, torch.float64)
    gto, sto = grads(nets["torch"], torch.float32)
    gfu, sfu = grads(nets["fused"], torch.float32)
    assert set(gfu) == set(g64) and all(torch.isfinite(v).all() for v in gfu.values())
    e_to = max((gto[k] - g64[k]).abs().max().item() for k in g64)
    e_fu = max((gfu[k] - g64[k]).abs().max().item() for k in g64)
    s_to, s_fu = (sto - s64).abs()[:5].max().item(), (sfu - s64).abs()[:5].max().item()
    print(f"{PN.KIND_NAMES[kind]} flat={flat}: largest parameter gradient {max(g64[k].abs().max().item() for k in g64):.3e}; error against float64: "
          f"attention=torch {e_to:.3e}, attention=fused {e_fu:.3e}; stats error torch {s_to:.3e}, fused {s_fu:.3e}")
    assert e_fu <= 4.0 * e_to
    assert s_fu <= 4.0 * s_to


def _setup(attention, N=256, T=32, horizon=30, seed=23):
    from hhmarl_2d_amd.learner import PPOLearner
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    dev = torch.device("cuda", 0)
    w = World(make_config(n_arenas=N, level=3, seed=seed, auto_reset=True, horizon=horizon), device=0)
    bank = PolicyBank.trainable_init(dev, mode="fight", seed=5, max_rows=2 * N)
    ro = PPORollout(w, bank, T, batch_mode="complete_episodes")
    learner = PPOLearner.trainable_init(dev, mode="fight", seed=5, num_sgd_iter=1, sgd_minibatch_size=1 << 30, attention=attention)
    return ro, bank, learner


STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy")


def test_one_update_with_fused_attention():
    """one PPOLearner.update with num_sgd_iter = 1 and one minibatch over the whole batch, so the reported statistics are those of one
    forward per policy.  Policy 0's is the first forward of the update: its statistics through attention="fused" and through "torch"
    (identically seeded learners, the same batch) are each compared with a float64 module's, the fused error at most 4 x the torch
    error.  Policy 1's forward follows policy 0's Adam step on the tied shared layer, whose first step moves every weight by about
    +- lr whatever the size of its gradient, so round-off in a near-zero gradient can flip a whole step: no float64 module stands for
    both learners there, and its statistics are only required to be finite.  Then publish: the bank's packed bytes equal a
    refresh_trainable of the learner's modules; and a second update on a new collect runs."""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    from hhmarl_2d_amd.rollout import central_critic_rows
    ro, bank, fused = _setup("fused")
    _, _, plain = _setup("torch")
    assert fused.attention == "fused" and all(m.attention == "fused" for m in fused.modules) and all(m.attention == "torch" for m in plain.modules)
    ro.collect()
    rows = ro.episodes.rows()
    assert rows["obs"].shape[0] > 1000
    with torch.no_grad():
        old = plain.batch_old_logits(rows, bank, ro.episodes.N)
        b = plain.policy_batch(rows, old, 0)
    m64 = LR.TrainableNet(plain.kinds[0]).load_numpy({k: v.detach().cpu().numpy() for k, v in plain.modules[0].state_dict().items()}).double().cuda()
    with torch.no_grad():
        logits, vf = m64(b["obs"].double(), b["critic"].double())
        _, s64 = LR.ppo_loss_torch(logits, vf, {k: v for k, v in b.items() if k != "seq_len"}, n_comp=LR.n_comp_of(plain.kinds[0]),
                                   clip_param=plain.clip_param, vf_clip_param=plain.vf_clip_param, vf_loss_coeff=plain.vf_loss_coeff,
                                   entropy_coeff=plain.entropy_coeff, kl_coeff=plain.kl_coeff[0])
    s64 = s64[:5].tolist()
    st_f, st_t = fused.update(ro.episodes, bank), plain.update(ro.episodes, bank)
    for st in (st_f, st_t):
        assert len(st) == 2 and all(s["steps"] == 1 and s["rows"] == rows["obs"].shape[0] for s in st)
        assert all(np.isfinite(s[k]) for s in st for k in STAT_KEYS + ("kl_coeff",))
    e_f = max(abs(st_f[0][k] - w) for k, w in zip(STAT_KEYS, s64))
    e_t = max(abs(st_t[0][k] - w) for k, w in zip(STAT_KEYS, s64))
    print(f"policy 0 statistics against float64 {s64}: error attention=torch {e_t:.3e}, attention=fused {e_f:.3e}")
    assert e_f <= 4.0 * e_t
    # publish: the bank's packed bytes are what refresh_trainable packs from the fused learner's modules, and its sampler reproduces their
    # length-1 forward (the 2-D form of the fused path) within the policy kernels' bound, as test_gpu_learner.py checks for the default
    fused.publish(bank)
    got = [[bank.packed(slot, part).clone() for part in range(5)] for slot in (0, 1)]
    bank.refresh_trainable(plain.modules)
    bank.refresh_trainable(fused.modules)
    for slot in (0, 1):
        for part in range(5):
            assert torch.equal(got[slot][part], bank.packed(slot, part))
    assert fused.modules[1].shared_layer._model[0].weight is fused.modules[0].shared_layer._model[0].weight
    probe = rows["obs"][:ro.episodes.N].contiguous()
    sel = torch.tensor(fused._sel, dtype=torch.uint8, device=probe.device).repeat(probe.shape[0], 1).contiguous()
    logits = torch.zeros((probe.shape[0], 2, 32), device=probe.device)
    act = torch.zeros((probe.shape[0], 2, 4), dtype=torch.int8, device=probe.device)
    bank.sample(probe, sel, greedy=True, actions=act, logits=logits)
    for a, kind in enumerate(fused.kinds):
        with torch.no_grad():
            want_l, _ = fused.modules[a](probe[:, a, :PN.OBS_DIM[kind]].contiguous(), central_critic_rows(probe, torch.zeros_like(act), a + 1))
        assert (logits[:, a, :PN.N_OUT[kind]] - want_l).abs().max().item() <= 1e-5
    # a second round on a new collect
    ro.start()
    ro.collect()
    st2 = fused.update(ro.episodes, bank)
    assert fused.updates == 2
    for s in st2:
        assert s["steps"] >= 1 and all(np.isfinite(s[k]) for k in STAT_KEYS)
