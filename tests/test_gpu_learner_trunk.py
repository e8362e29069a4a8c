"""learner.TrainableNet(trunk="fused"), CommanderTrainable(trunk="fused") and the two learners with trunk="fused" on the MI355X: every
parameter's gradient and the loss statistics against a float64 run (the fused path at most 4 x as far from it as the default path),
the fight forward against the reference's recorded training-form outputs, and collect -> update -> publish rounds."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP, VCLIP = 0.25, 10.0
KW = dict(clip_param=CLIP, vf_clip_param=VCLIP, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)
STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy")
ALL_FUSED = dict(attention="fused", inputs="fused", trunk="fused")


def _weights(kind, seed):
    from hhmarl_2d_amd import policy_nets as PN
    return dict(PN.random_weights(kind, seed), **PN.random_critic_weights(kind, seed))


@pytest.mark.parametrize("kind", (0, 1))
def test_fused_forward_equals_reference_recording(kind):
    """tests/golden/fight_sequence_forward.npz within the 1.5e-4 that tests/test_learner_host.py established for the file"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    g = np.load(os.path.join(ROOT, "tests", "golden", "fight_sequence_forward.npz"))
    name = PN.KIND_NAMES[kind]
    seed = json.loads(str(g["meta"]))["seed"]
    m = LR.TrainableNet(kind, trunk="fused").load_numpy(_weights(kind, seed)).cuda().eval()
    with torch.no_grad():
        logits, value = m(torch.from_numpy(g[f"{name}_obs"]).cuda(), torch.from_numpy(g[f"{name}_critic"]).cuda())
    dl = np.abs(logits.cpu().numpy() - g[f"{name}_logits"]).max()
    dv = np.abs(value.cpu().numpy() - g[f"{name}_value"]).max()
    print(f"{name}: max |logits - reference| = {dl:.3e}, max |value - reference| = {dv:.3e}")
    assert logits.shape == g[f"{name}_logits"].shape and value.shape == g[f"{name}_value"].shape
    assert dl <= 1.5e-4 and dv <= 1.5e-4


def _compare(name, runs, g64, s64):
    """runs: {label: (gradients, stats)} with the labels "torch" and the fused ones; every fused label is held to 4 x the torch error"""
    err = {}
    for label, (gr, st) in runs.items():
        assert set(gr) == set(g64) and all(torch.isfinite(v).all() for v in gr.values())
        err[label] = (max((gr[k] - g64[k]).abs().max().item() for k in g64), (st - s64).abs()[:5].max().item())
    print(f"{name}: largest parameter gradient {max(g64[k].abs().max().item() for k in g64):.3e}; (gradient, statistics) error against float64: "
          + ", ".join(f"{label} ({e[0]:.3e}, {e[1]:.3e})" for label, e in err.items())
          + "; ratios to torch: " + ", ".join(f"{label} ({e[0] / err['torch'][0]:.2f}, {e[1] / err['torch'][1]:.2f})" for label, e in err.items() if label != "torch"))
    for label, e in err.items():
        if label != "torch":
            assert e[0] <= 4.0 * err["torch"][0], label
            assert e[1] <= 4.0 * err["torch"][1], label


@pytest.mark.parametrize("kind,flat", [(0, False), (0, True), (1, False), (1, True), (2, True), (3, True)])
def test_gradients_fused_against_torch_trunk(kind, flat):
    """shaped like test_gpu_learner_inputs.test_gradients_fused_against_torch_inputs (fight kinds: 96 chunks of 20, masked, and the same
    rows flat; escape kinds: 1920 rows, no mask): gradients and the first five statistics through trunk="fused" and through
    trunk="torch", each against a float64 run of the same module and loss (ppo_loss_torch in all, so the shared layer is the only
    difference); once more with inputs="fused" (and, for the fight kinds, attention="fused") on top"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(80 + kind)
    d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
    S, Lc = 96, 20
    att = PN.HAS_ATT[kind]
    n_comp = LR.n_comp_of(kind)
    own = torch.rand((S, Lc, d1), generator=g)
    crit = torch.cat([torch.rand((S, Lc, a1 + a2), generator=g), own, torch.rand((S, Lc, d2), generator=g)], dim=-1)
    mask = LR.chunk_mask(torch.randint(1, Lc + 1, (S,), generator=g), Lc) if att else torch.ones((S, Lc), dtype=torch.bool)
    own, crit = own * mask[..., None], crit * mask[..., None]
    if flat:
        own, crit, mask = own.reshape(S * Lc, -1), crit.reshape(S * Lc, -1), mask.reshape(S * Lc)
    lead = tuple(own.shape[:-1])
    w = _weights(kind, 9)
    on_top = ALL_FUSED if att else dict(inputs="fused", trunk="fused")
    nets = {"torch": LR.TrainableNet(kind).load_numpy(w).to(dev), "trunk=fused": LR.TrainableNet(kind, trunk="fused").load_numpy(w).to(dev),
            "all fused": LR.TrainableNet(kind, **on_top).load_numpy(w).to(dev)}
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
             "target": torch.randn(lead, generator=g).to(dev) * 2.0}
    if att:
        batch["mask"] = mask.to(dev)

    def grads(module, dt):
        module.zero_grad(set_to_none=True)
        logits, vf = module(own.to(dev, dt), crit.to(dev, dt))
        total, stats = LR.ppo_loss_torch(logits, vf, batch, n_comp=n_comp, **KW)
        total.backward()
        return {k: p.grad.double().clone() for k, p in module.named_parameters()}, stats.clone()

    g64, s64 = grads(net64, torch.float64)
    _compare(f"{PN.KIND_NAMES[kind]} flat={flat}", {label: grads(m, torch.float32) for label, m in nets.items()}, g64, s64)


def test_commander_gradients_fused_against_torch_trunk():
    """64 sequences of 20 steps with ragged seq_len; the float32 modules run the fused GRU, the float64 module the stepped cell"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.commander import random_weights
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(91)
    S, Lc = 64, 20
    seq_len = torch.randint(1, Lc + 1, (S,), generator=g).to(torch.int32)
    seq_len[0], seq_len[1] = Lc, 1
    mask = LR.chunk_mask(seq_len, Lc)
    obs = torch.rand((S, Lc, 34), generator=g) * mask[..., None]
    crit = torch.cat([torch.randint(0, 3, (S, Lc, 3), generator=g).float(), obs, torch.rand((S, Lc, 68), generator=g)], dim=-1) * mask[..., None]
    state = 0.3 * torch.randn((S, 2, 200), generator=g)
    w = random_weights(6)
    nets = {"torch": LR.CommanderTrainable().load_numpy(w).to(dev), "trunk=fused": LR.CommanderTrainable(trunk="fused").load_numpy(w).to(dev),
            "all fused": LR.CommanderTrainable(inputs="fused", trunk="fused").load_numpy(w).to(dev)}
    net64 = LR.CommanderTrainable().load_numpy(w).double().to(dev)
    with torch.no_grad():
        old, _ = nets["torch"](obs.to(dev), crit.to(dev), state.to(dev), seq_len.to(dev))
    old = torch.nn.functional.pad(old + 0.3 * torch.randn(old.shape, generator=g).to(dev), (0, 1))
    actions = torch.randint(0, 3, (S, Lc), generator=g).to(torch.int8).to(dev)
    old_logp = torch.log_softmax(old[..., :3], dim=-1).gather(-1, actions.long()[..., None])[..., 0]
    batch = {"old_logits": old, "actions": actions, "old_logp": old_logp, "adv": torch.randn((S, Lc), generator=g).to(dev),
             "target": torch.randn((S, Lc), generator=g).to(dev) * 2.0, "mask": mask.to(dev)}

    def grads(module, dt):
        module.zero_grad(set_to_none=True)
        logits, vf = module(obs.to(dev, dt), crit.to(dev, dt), state.to(dev, dt), seq_len.to(dev), fused_gru=dt == torch.float32)
        total, stats = LR.ppo_loss_categorical_torch(logits, vf, batch, **KW)
        total.backward()
        return {k: p.grad.double().clone() for k, p in module.named_parameters()}, stats.clone()

    g64, s64 = grads(net64, torch.float64)
    _compare("commander", {label: grads(m, torch.float32) for label, m in nets.items()}, g64, s64)


def test_tied_layer_takes_gradients_only_from_the_module_that_ran():
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    dev = torch.device("cuda", 0)
    a, b = LR.tie([LR.TrainableNet(PN.ESC1, trunk="fused").to(dev), LR.TrainableNet(PN.ESC2, trunk="fused").to(dev)])
    assert b.shared_layer is a.shared_layer
    d1, a1, d2, a2 = PN.CRITIC_DIMS[PN.ESC1]
    logits, value = a(torch.rand((70, PN.OBS_DIM[PN.ESC1]), device=dev), torch.rand((70, d1 + a1 + d2 + a2), device=dev))
    (logits.sum() + value.sum()).backward()
    lin = a.shared_layer._model[0]
    assert lin.weight.grad is not None and lin.weight.grad.abs().max() > 0 and lin.bias.grad.abs().max() > 0
    assert all(p.grad is None for k, p in b.named_parameters() if not k.startswith("shared_layer."))
    assert all(p.grad is not None for p in a.parameters())


def _setup(trunk, N=64, T=32, horizon=30, seed=23):
    from hhmarl_2d_amd.learner import PPOLearner
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    dev = torch.device("cuda", 0)
    w = World(make_config(n_arenas=N, level=3, seed=seed, auto_reset=True, horizon=horizon), device=0)
    bank = PolicyBank.trainable_init(dev, mode="fight", seed=5, max_rows=2 * N)
    ro = PPORollout(w, bank, T, batch_mode="complete_episodes")
    learner = PPOLearner.trainable_init(dev, mode="fight", seed=5, num_sgd_iter=2, sgd_minibatch_size=256, trunk=trunk)
    return ro, bank, learner


def test_one_update_with_fused_trunk():
    """one collect -> update -> publish round at 64 arenas: finite statistics, the step counts of the torch learner on the same batch, and
    after publish the bank serves the bytes that refresh_trainable packs from the module"""
    ro, bank, fused = _setup("fused")
    _, _, plain = _setup("torch")
    assert fused.trunk == "fused" and all(m.trunk == "fused" for m in fused.modules) and all(m.trunk == "torch" for m in plain.modules)
    ro.collect()
    rows = ro.episodes.rows()
    assert rows["obs"].shape[0] > 256
    st_f, st_t = fused.update(ro.episodes, bank), plain.update(ro.episodes, bank)
    for st in (st_f, st_t):
        assert len(st) == 2 and all(s["rows"] == rows["obs"].shape[0] for s in st)
        assert all(np.isfinite(s[k]) for s in st for k in STAT_KEYS + ("kl_coeff",))
    assert [s["steps"] for s in st_f] == [s["steps"] for s in st_t] and all(s["steps"] >= 2 for s in st_f)
    print("statistics fused", st_f, "torch", st_t)
    fused.publish(bank)
    got = [[bank.packed(slot, part).clone() for part in range(5)] for slot in (0, 1)]
    bank.refresh_trainable(plain.modules)
    bank.refresh_trainable(fused.modules)
    for slot in (0, 1):
        for part in range(5):
            assert torch.equal(got[slot][part], bank.packed(slot, part))
    assert fused.modules[1].shared_layer._model[0].weight is fused.modules[0].shared_layer._model[0].weight


def test_one_commander_update_with_fused_trunk():
    """set up the way tests/test_gpu_commander_learner.py sets its rounds up, at 64 arenas; the torch learner runs the same batch"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    N = 64
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True, horizon=150), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    ro = CommanderRollout(w, net, VariantNetPilot(w, seed=8), 16, batch_mode="complete_episodes", max_seq_len=20)
    learner = LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, num_sgd_iter=2, trunk="fused")
    plain = LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, num_sgd_iter=2)
    assert learner.trunk == "fused" and learner.module.trunk == "fused" and plain.module.trunk == "torch"
    ro.start()
    for _ in range(6):
        ro.collect()
    before = {k: v.clone() for k, v in learner.module.state_dict().items()}
    stats, stats_t = learner.update(ro.episodes, net), plain.update(ro.episodes, net)
    assert stats["steps"] > 0 and stats["rows"] > 0 and all(np.isfinite(stats[k]) for k in STAT_KEYS)
    assert stats["steps"] == stats_t["steps"] and stats["rows"] == stats_t["rows"]
    after = learner.module.state_dict()
    assert all(not torch.equal(after[k], before[k]) for k in before) and all(torch.isfinite(v).all() for v in after.values())
    learner.publish(net)
    packed = [net.packed(part).clone() for part in (0, 1)]
    net.refresh_weights(plain.module.state_dict())
    assert not all(torch.equal(want, net.packed(part)) for part, want in enumerate(packed))
    net.refresh_weights(learner.module.state_dict())
    for part, want in enumerate(packed):
        assert torch.equal(want, net.packed(part))
