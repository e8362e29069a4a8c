"""learner.TrainableNet(heads="fused"), CommanderTrainable(heads="fused") and the two learners with heads="fused" on the MI355X: every
parameter's gradient and the loss statistics through pre_heads + heads_loss against a float64 run (the fused tail at most 4 x as far from
it as the default path), the unchanged forward and state_dict, the tied shared layer, the scaling of the kept gradients, collect -> update
-> publish rounds in all three step modes against the heads="torch" learner, and the refused combinations."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CLIP, VCLIP = 0.25, 10.0
KW = dict(clip_param=CLIP, vf_clip_param=VCLIP, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)
STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy")
MODES = {"eager": {}, "device-adam": dict(optimizer="fused"), "graph": dict(optimizer="fused", step="graph")}


def _weights(kind, seed):
    from hhmarl_2d_amd import policy_nets as PN
    return dict(PN.random_weights(kind, seed), **PN.random_critic_weights(kind, seed))


def _compare(name, runs, g64, s64):
    """runs: {label: (gradients, stats)} with the label "torch" and the fused ones; every fused label is held to 4 x the torch error"""
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


def _fight_case(kind, flat):
    """test_gpu_learner_trunk's case: 96 chunks of 20 with a ragged mask (fight kinds), the same rows flat, 1920 unmasked rows (escape)"""
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
    with torch.no_grad():
        old, _ = LR.TrainableNet(kind).load_numpy(w).to(dev)(own.to(dev), crit.to(dev))
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
    return w, own.to(dev), crit.to(dev), batch, n_comp


@pytest.mark.parametrize("kind,flat", [(0, False), (0, True), (1, False), (1, True), (2, True), (3, True)])
def test_gradients_fused_against_torch_heads(kind, flat):
    """gradients of every parameter and the first five statistics through heads="fused" (pre_heads + heads_loss) and through the default
    path (forward + ppo_loss_torch), each against a float64 run of the same module; once more with inputs="fused" (and, for the fight
    kinds, attention="fused") under the fused tail"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    dev = torch.device("cuda", 0)
    w, own, crit, batch, n_comp = _fight_case(kind, flat)
    on_top = dict(attention="fused", inputs="fused") if PN.HAS_ATT[kind] else dict(inputs="fused")
    nets = {"torch": LR.TrainableNet(kind).load_numpy(w).to(dev), "heads=fused": LR.TrainableNet(kind, heads="fused").load_numpy(w).to(dev),
            "all fused": LR.TrainableNet(kind, heads="fused", **on_top).load_numpy(w).to(dev)}
    net64 = LR.TrainableNet(kind).load_numpy(w).double().to(dev)

    def grads(module, dt):
        module.zero_grad(set_to_none=True)
        if module.heads == "fused":
            za, zc = module.pre_heads(own, crit)
            total, stats = LR.heads_loss(za, zc, module.act_out, module.val_out, batch, n_comp=n_comp, **KW)
        else:
            logits, vf = module(own.to(dt), crit.to(dt))
            total, stats = LR.ppo_loss_torch(logits, vf, batch, n_comp=n_comp, **KW)
        total.backward()
        return {k: p.grad.double().clone() for k, p in module.named_parameters()}, stats.clone()

    g64, s64 = grads(net64, torch.float64)
    _compare(f"{PN.KIND_NAMES[kind]} flat={flat}", {label: grads(m, torch.float32) for label, m in nets.items()}, g64, s64)


def _commander_case():
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
    with torch.no_grad():
        old, _ = LR.CommanderTrainable().load_numpy(w).to(dev)(obs.to(dev), crit.to(dev), state.to(dev), seq_len.to(dev))
    old = torch.nn.functional.pad(old + 0.3 * torch.randn(old.shape, generator=g).to(dev), (0, 1))
    actions = torch.randint(0, 3, (S, Lc), generator=g).to(torch.int8).to(dev)
    old_logp = torch.log_softmax(old[..., :3], dim=-1).gather(-1, actions.long()[..., None])[..., 0]
    batch = {"old_logits": old, "actions": actions, "old_logp": old_logp, "adv": torch.randn((S, Lc), generator=g).to(dev),
             "target": torch.randn((S, Lc), generator=g).to(dev) * 2.0, "mask": mask.to(dev)}
    return w, (obs.to(dev), crit.to(dev), state.to(dev), seq_len.to(dev)), batch


def test_commander_gradients_fused_against_torch_heads():
    """64 sequences of 20 steps with ragged seq_len; the float32 modules run the fused GRU, the float64 module the stepped cell"""
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    w, (obs, crit, state, seq_len), batch = _commander_case()
    nets = {"torch": LR.CommanderTrainable().load_numpy(w).to(dev), "heads=fused": LR.CommanderTrainable(heads="fused").load_numpy(w).to(dev),
            "all fused": LR.CommanderTrainable(inputs="fused", heads="fused").load_numpy(w).to(dev)}
    net64 = LR.CommanderTrainable().load_numpy(w).double().to(dev)

    def grads(module, dt):
        module.zero_grad(set_to_none=True)
        if module.heads == "fused":
            za, zc = module.pre_heads(obs, crit, state, seq_len)
            total, stats = LR.heads_loss(za, zc, module.act_out, module.val_out, batch, n_comp=1, **KW)
        else:
            logits, vf = module(obs.to(dt), crit.to(dt), state.to(dt), seq_len, fused_gru=dt == torch.float32)
            total, stats = LR.ppo_loss_categorical_torch(logits, vf, batch, **KW)
        total.backward()
        return {k: p.grad.double().clone() for k, p in module.named_parameters()}, stats.clone()

    g64, s64 = grads(net64, torch.float64)
    _compare("commander", {label: grads(m, torch.float32) for label, m in nets.items()}, g64, s64)


def test_forward_and_state_dict_do_not_depend_on_heads():
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    for kind, flat in ((0, False), (1, True), (2, True)):
        w, own, crit, _, _ = _fight_case(kind, flat)
        a, b = LR.TrainableNet(kind).load_numpy(w).to(dev), LR.TrainableNet(kind, heads="fused").load_numpy(w).to(dev)
        assert a.heads == "torch" and b.heads == "fused" and list(a.state_dict()) == list(b.state_dict())
        with torch.no_grad():
            (la, va), (lb, vb) = a(own, crit), b(own, crit)
            za, zc = b.pre_heads(own, crit)
        assert torch.equal(la, lb) and torch.equal(va, vb)
        assert tuple(za.shape) == tuple(own.shape[:-1]) + (500,) and za.is_contiguous() and zc.is_contiguous()
        # the heads on pre_heads' outputs are forward's logits and values
        assert torch.equal(b.act_out(torch.tanh(za)), lb) and torch.equal(b.val_out(torch.tanh(zc)).squeeze(-1), vb)
    w, args, _ = _commander_case()
    a, b = LR.CommanderTrainable().load_numpy(w).to(dev), LR.CommanderTrainable(heads="fused").load_numpy(w).to(dev)
    assert list(a.state_dict()) == list(b.state_dict())
    with torch.no_grad():
        (la, va), (lb, vb) = a(*args), b(*args)
    assert torch.equal(la, lb) and torch.equal(va, vb)


def test_kept_gradients_are_scaled_by_the_upstream_gradient_unless_switched_off():
    """on leaf tensors, so that nothing but heads_loss's own backward runs: an upstream gradient of 3 gives exactly 3 x the gradients of
    an upstream gradient of 1 (one float32 multiply of the kept tensors); scale_grad=False hands the kept tensors over as they are"""
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    w, own, crit, batch, n_comp = _fight_case(2, True)
    m = LR.TrainableNet(2, heads="fused").load_numpy(w).to(dev)
    with torch.no_grad():
        za0, zc0 = m.pre_heads(own, crit)
    heads = [p.detach() for p in (*m.act_out.parameters(), *m.val_out.parameters())]

    def run(factor, **kw):
        leaves = [t.clone().requires_grad_(True) for t in (za0, zc0, *heads)]
        za, zc, w_act, b_act, w_val, b_val = leaves
        total, stats = LR.heads_loss(za, zc, (w_act, b_act), (w_val, b_val), batch, n_comp=n_comp, **KW, **kw)
        assert total.dtype == torch.float32 and total.dim() == 0 and total.item() == np.float32(stats[0].item()) and not stats.requires_grad
        (total * factor).backward()
        assert all(t.grad is not None and t.grad.shape == t.shape and t.grad.abs().max() > 0 for t in leaves)
        return [t.grad.clone() for t in leaves]

    one, three, raw = run(1.0), run(3.0), run(3.0, scale_grad=False)
    assert all(torch.equal(a, b) for a, b in zip(raw, one)), "scale_grad=False hands the kept gradients over as they are"
    assert all(torch.equal(a, b * 3.0) for a, b in zip(three, one))
    with pytest.raises(ValueError, match="heads_loss"):
        LR.heads_loss(za0.double(), zc0.double(), m.act_out, m.val_out, batch, n_comp=n_comp, **KW)
    with pytest.raises(ValueError, match="heads_loss"):
        LR.heads_loss(za0[:, :496], zc0[:, :496], m.act_out, m.val_out, batch, n_comp=n_comp, **KW)
    with pytest.raises(ValueError, match="n_comp"):
        LR.heads_loss(za0, zc0, m.act_out, m.val_out, batch, n_comp=2, **KW)


def test_tied_layer_takes_gradients_only_from_the_module_that_ran():
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    dev = torch.device("cuda", 0)
    a, b = LR.tie([LR.TrainableNet(PN.ESC1, heads="fused").to(dev), LR.TrainableNet(PN.ESC2, heads="fused").to(dev)])
    assert b.shared_layer is a.shared_layer
    w, own, crit, batch, n_comp = _fight_case(PN.ESC1, True)
    za, zc = a.pre_heads(own, crit)
    total, _ = LR.heads_loss(za, zc, a.act_out, a.val_out, batch, n_comp=n_comp, **KW)
    total.backward()
    lin = a.shared_layer._model[0]
    assert lin.weight.grad is not None and lin.weight.grad.abs().max() > 0 and lin.bias.grad.abs().max() > 0
    assert all(p.grad is None for k, p in b.named_parameters() if not k.startswith("shared_layer."))
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in a.parameters())


def _world(mode, N=64, T=32, horizon=30, seed=23):
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    dev = torch.device("cuda", 0)
    w = World(make_config(n_arenas=N, level=3, seed=seed, auto_reset=True, horizon=horizon, agent_mode=1 if mode == "escape" else 0), device=0)
    bank = PolicyBank.trainable_init(dev, mode=mode, seed=5, max_rows=2 * N)
    return PPORollout(w, bank, T, batch_mode="complete_episodes"), bank


def _learner(mode, **kw):
    from hhmarl_2d_amd.learner import PPOLearner
    return PPOLearner.trainable_init(torch.device("cuda", 0), mode=mode, seed=5, **{**dict(num_sgd_iter=2, sgd_minibatch_size=256), **kw})


@pytest.fixture(scope="module", params=("fight", "escape"))
def round_(request):
    """one collect at 64 arenas and, on that batch, the eager fused=True and fused=False learners' updates: their gap is the yardstick
    of tests/test_gpu_learner_graph.py; read only"""
    mode = request.param
    ro, bank = _world(mode)
    ro.collect()
    st_f, st_p = _learner(mode).update(ro.episodes, bank), _learner(mode, fused=False).update(ro.episodes, bank)
    yard = [max(abs(x[k] - y[k]) for k in STAT_KEYS) for x, y in zip(st_f, st_p)]
    return mode, ro, bank, yard


@pytest.mark.parametrize("step_mode", list(MODES))
def test_update_rounds_against_the_torch_heads(round_, step_mode):
    """collect -> update -> publish at 64 arenas in each step mode: steps and rows of the heads="torch" learner of the same mode on the same
    batch, mean statistics within 4 x the fused = True / False yardstick of it; once with grad_clip, once with shuffle_sequences"""
    mode, ro, bank, yard = round_
    extra = {"eager": {}, "device-adam": dict(grad_clip=2.0), "graph": dict(shuffle_sequences=True)}[step_mode]
    R = ro.episodes.rows()["obs"].shape[0]
    assert R > 256
    for kw in ({}, extra) if extra else ({},):
        fused, plain = _learner(mode, heads="fused", **MODES[step_mode], **kw), _learner(mode, **MODES[step_mode], **kw)
        assert fused.heads == "fused" and all(m.heads == "fused" for m in fused.modules) and plain.heads == "torch"
        st_h, st_t = fused.update(ro.episodes, bank), plain.update(ro.episodes, bank)
        for st in (st_h, st_t):
            assert len(st) == 2 and all(s["rows"] == R for s in st) and all(np.isfinite(s[k]) for s in st for k in STAT_KEYS + ("kl_coeff",))
        assert [s["steps"] for s in st_h] == [s["steps"] for s in st_t] and all(s["steps"] >= 2 for s in st_h)
        assert set(st_h[0]) == set(st_t[0])
        got = [max(abs(x[k] - y[k]) for k in STAT_KEYS) for x, y in zip(st_h, st_t)]
        print(f"{mode} {step_mode} {kw}: per policy max |difference| of the mean statistics, heads fused vs torch {got[0]:.3e}, {got[1]:.3e}; "
              f"yardstick (eager fused=True vs fused=False) {yard[0]:.3e}, {yard[1]:.3e}")
        assert all(g <= 4.0 * y for g, y in zip(got, yard)), (got, yard)
        if "grad_clip" in kw:
            assert all(np.isfinite(s["grad_gnorm"]) and s["grad_gnorm"] > 0 for s in st_h + st_t)
    fused.publish(bank)
    got = [[bank.packed(slot, part).clone() for part in range(5)] for slot in (0, 1)]
    bank.refresh_trainable(plain.modules)
    bank.refresh_trainable(fused.modules)
    for slot in (0, 1):
        for part in range(5):
            assert torch.equal(got[slot][part], bank.packed(slot, part))
    assert fused.modules[1].shared_layer._model[0].weight is fused.modules[0].shared_layer._model[0].weight
    bank.refresh_trainable(_learner(mode).modules)      # the fixture's bank goes back to the initial weights


@pytest.fixture(scope="module")
def commander_round():
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    N = 64
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True, horizon=150), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    ro = CommanderRollout(w, net, VariantNetPilot(w, seed=8), 16, batch_mode="complete_episodes", max_seq_len=20, record_logits=True)
    ro.start()
    for _ in range(6):
        ro.collect()
    make = lambda **kw: LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, num_sgd_iter=2, sgd_minibatch_size=256, **kw)
    st_f, st_p = make().update(ro.episodes, net), make(fused=False).update(ro.episodes, net)
    return ro, net, make, max(abs(st_f[k] - st_p[k]) for k in STAT_KEYS)


@pytest.mark.parametrize("step_mode", list(MODES))
def test_commander_update_rounds_against_the_torch_heads(commander_round, step_mode):
    ro, net, make, yard = commander_round
    extra = {"eager": dict(shuffle_sequences=True), "device-adam": {}, "graph": dict(grad_clip=2.0)}[step_mode]
    rows = int(ro.episodes.sequences()["mask"].sum()) * 3
    for kw in ({}, extra) if extra else ({},):
        fused, plain = make(heads="fused", **MODES[step_mode], **kw), make(**MODES[step_mode], **kw)
        assert fused.heads == "fused" and fused.module.heads == "fused" and plain.heads == "torch" and plain.module.heads == "torch"
        before = {k: v.clone() for k, v in fused.module.state_dict().items()}
        st_h, st_t = fused.update(ro.episodes, net), plain.update(ro.episodes, net)
        assert st_h["rows"] == st_t["rows"] == rows and st_h["steps"] == st_t["steps"] >= 4 and set(st_h) == set(st_t)
        assert all(np.isfinite(st_h[k]) for k in STAT_KEYS + ("kl_coeff",))
        got = max(abs(st_h[k] - st_t[k]) for k in STAT_KEYS)
        print(f"commander {step_mode} {kw}: max |difference| of the mean statistics, heads fused vs torch {got:.3e}; yardstick {yard:.3e}")
        assert got <= 4.0 * yard
        after = fused.module.state_dict()
        assert all(not torch.equal(after[k], before[k]) for k in before) and all(torch.isfinite(v).all() for v in after.values())
    fused.publish(net)
    packed = [net.packed(part).clone() for part in (0, 1)]
    net.refresh_weights(fused.module.state_dict())
    assert all(torch.equal(want, net.packed(part)) for part, want in enumerate(packed))
    net.refresh_weights(make().module.state_dict())


def test_refused_combinations_and_defaults():
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    assert LR.TrainableNet(0).heads == "torch" and LR.CommanderTrainable().heads == "torch"
    assert _learner("fight").heads == "torch" and LR.CommanderLearner.trainable_init(dev, seed=6).heads == "torch"
    for make in (lambda **kw: _learner("fight", **kw), lambda **kw: _learner("escape", **kw), lambda **kw: LR.CommanderLearner.trainable_init(dev, seed=6, **kw)):
        with pytest.raises(ValueError, match="heads"):
            make(heads="fused", trunk="fused")
        with pytest.raises(ValueError, match="heads"):
            make(heads="fused", fused=False)
        with pytest.raises(ValueError, match="heads"):
            make(heads="hip")
    with pytest.raises(ValueError, match="pre_heads"):
        LR.TrainableNet(2, trunk="fused").to(dev).pre_heads(torch.zeros((4, 30), device=dev), torch.zeros((4, 66), device=dev))
    with pytest.raises(TypeError):
        LR.PPOLearner((0, 1), ({}, {}), dev, 1e-4, 0.25, 0.025, 0.2, 10.0, 1.0, 0.0, 30, 256, 20, 0, True, "torch", "torch", "torch", "torch", "eager", False,
                      None, "fused")     # heads is keyword only
