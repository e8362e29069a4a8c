"""PPOLearner(optimizer="fused", step="graph") on the MI355X: the first replayed step against the eager step and a float64 run, whole
updates against the eager learner with the fused = True / False difference as the yardstick, re-capture when kl_coeff and cap change,
and the escape surrogate.  Weights after many Adam steps are never compared between paths: m / (sqrt(v) + eps) amplifies rounding
differences, so that comparison is ill-conditioned."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy")
GRAPH = dict(optimizer="fused", step="graph")


def _weights(kind, seed):
    from hhmarl_2d_amd import policy_nets as PN
    return dict(PN.random_weights(kind, seed), **PN.random_critic_weights(kind, seed))


def _policy_batch(kind, net, seed):
    """a policy batch as PPOLearner.policy_batch makes it: fight kinds 14 chunks of 20 with ragged seq_len and a mask, escape kinds 271 rows"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(seed)
    d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
    att = PN.HAS_ATT[kind]
    lead = (14, 20) if att else (271,)
    own = torch.rand(lead + (d1,), generator=g)
    crit = torch.cat([torch.rand(lead + (a1 + a2,), generator=g), own, torch.rand(lead + (d2,), generator=g)], dim=-1)
    b = {}
    if att:
        seq_len = torch.randint(1, 21, (14,), generator=g)
        seq_len[0], seq_len[1] = 20, 1
        mask = LR.chunk_mask(seq_len, 20)
        own, crit = own * mask[..., None], crit * mask[..., None]
        b["seq_len"], b["mask"] = seq_len.to(dev), mask.to(torch.uint8).to(dev)
    n_comp = LR.n_comp_of(kind)
    splits = PN.ACTION_SPLIT[:n_comp]
    with torch.no_grad():
        old, _ = net(own.to(dev), crit.to(dev))
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
    b.update({"obs": own.to(dev), "critic": crit.to(dev), "actions": actions.to(dev), "old_logp": old_logp, "adv": torch.randn(lead, generator=g).to(dev),
              "target": (torch.randn(lead, generator=g) * 2.0).to(dev), "old_logits": old32})
    if att:       # what pad_chunks leaves in the padded rows: zeros in every column
        for k in ("actions", "old_logp", "adv", "target", "old_logits"):
            b[k] = b[k] * b["mask"].reshape(b["mask"].shape + (1,) * (b[k].dim() - 2)).to(b[k].dtype)
    return b


def _state_bytes(learner, agent):
    opt, book = learner.optimizers[agent], learner._books[agent]
    torch.cuda.synchronize()
    return ([p.detach().cpu().numpy().tobytes() for p in learner.modules[agent].parameters()] + [x.cpu().numpy().tobytes() for x in opt.m + opt.v]
            + [opt.t.cpu().numpy().tobytes(), book.cursor.cpu().numpy().tobytes()])


@pytest.mark.parametrize("kind,opts", [(0, {}), (1, {}), (2, {}), (0, dict(attention="fused", inputs="fused"))])
def test_first_replayed_step_against_the_eager_step_and_float64(kind, opts):
    """Fight1 / Fight2: 14 chunks staged into cap = 16 (two chunks of pure padding); Esc1: 271 rows in cap = 288.  From identical weights the
    gradients the graph's first replay leaves in p.grad and its five statistics, and the eager step's on the unpadded minibatch, each
    against a float64 run of the same module and loss: the graph at most 4 x as far from it as the eager step"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    dev = torch.device("cuda", 0)
    att = PN.HAS_ATT[kind]
    kinds = (PN.FIGHT1, PN.FIGHT2) if att else (PN.ESC1, PN.ESC2)
    agent = kinds.index(kind)
    sds = [_weights(k, 9) for k in kinds]
    kw = dict(entropy_coeff=0.01, num_sgd_iter=1, sgd_minibatch_size=100000, seed=9, **opts)
    graph, eager = LR.PPOLearner(kinds, sds, dev, **kw, **GRAPH), LR.PPOLearner(kinds, sds, dev, **kw)
    assert graph.optimizer == "fused" and graph.step == "graph" and eager.optimizer == "torch" and eager.step == "eager"
    net64 = LR.TrainableNet(kind)
    net64.load_state_dict(eager.modules[agent].state_dict())
    net64 = net64.double().to(dev)
    b = _policy_batch(kind, eager.modules[agent], 40 + kind)
    cap = 16 if att else 288

    before = _state_bytes(graph, agent)
    n_steps, n_rows = graph.graph_prepare(agent, b, cap=cap)
    assert _state_bytes(graph, agent) == before, "warm-up and capture leave weights, m, v, t and the cursor bit for bit as they were"
    valid = int(b["seq_len"].sum()) if att else 271
    assert (n_steps, n_rows) == (1, valid) and graph._books[agent].cap == cap
    graph.graph_replay(agent, 1)
    torch.cuda.synchronize()
    g_graph = {k: p.grad.double().clone() for k, p in graph.modules[agent].named_parameters()}
    s_graph = graph.graph_stats(agent, 1)[0].clone()
    opt, book = graph.optimizers[agent], graph._books[agent]
    assert int(opt.t.item()) == 1 and int(book.cursor.item()) == 1 and int(book.n_valid.item()) == valid and s_graph[5].item() == valid
    staged = book.staged
    assert staged["obs"].shape[0] == cap and int(staged["mask"].sum()) == valid and not staged["obs"][cap - 2:].any()
    changed = [k for (k, p), old in zip(graph.modules[agent].named_parameters(), before) if p.detach().cpu().numpy().tobytes() != old]
    assert len(changed) == len(list(graph.modules[agent].parameters())), "one replay is one Adam step of every tensor"

    mb = {k: v for k, v in b.items() if k != "seq_len"}
    mb["n_valid"] = torch.tensor([valid], dtype=torch.int32, device=dev)

    def grads(learner, module, dt):
        module.zero_grad(set_to_none=True)
        logits, vf = module(mb["obs"].to(dt), mb["critic"].to(dt))
        if dt == torch.float64:
            total, stats = LR.ppo_loss_torch(logits, vf, mb, n_comp=LR.n_comp_of(kind), clip_param=learner.clip_param, vf_clip_param=learner.vf_clip_param,
                                             vf_loss_coeff=learner.vf_loss_coeff, entropy_coeff=learner.entropy_coeff, kl_coeff=learner.kl_coeff[agent])
        else:
            total, stats = learner.loss(agent, logits, vf, mb)
        total.backward()
        return {k: p.grad.double().clone() for k, p in module.named_parameters()}, stats.clone()

    g64, s64 = grads(eager, net64, torch.float64)
    g_eager, s_eager = grads(eager, eager.modules[agent], torch.float32)
    err = {}
    for label, (gr, st) in (("eager", (g_eager, s_eager)), ("graph", (g_graph, s_graph))):
        assert set(gr) == set(g64) and all(torch.isfinite(v).all() for v in gr.values())
        err[label] = (max((gr[k] - g64[k]).abs().max().item() for k in g64), (st - s64).abs()[:5].max().item())
    print(f"{PN.KIND_NAMES[kind]} {opts}: largest parameter gradient {max(g64[k].abs().max().item() for k in g64):.3e}; (gradient, statistics) error "
          f"against float64: eager ({err['eager'][0]:.3e}, {err['eager'][1]:.3e}), graph ({err['graph'][0]:.3e}, {err['graph'][1]:.3e}); ratios "
          f"({err['graph'][0] / err['eager'][0]:.2f}, {err['graph'][1] / err['eager'][1]:.2f})")
    assert err["graph"][0] <= 4.0 * err["eager"][0]
    assert err["graph"][1] <= 4.0 * err["eager"][1]


def _world(mode="fight", N=64, T=32, horizon=30, seed=23):
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    dev = torch.device("cuda", 0)
    w = World(make_config(n_arenas=N, level=3, seed=seed, auto_reset=True, horizon=horizon, agent_mode=1 if mode == "escape" else 0), device=0)
    bank = PolicyBank.trainable_init(dev, mode=mode, seed=5, max_rows=2 * N)
    return PPORollout(w, bank, T, batch_mode="complete_episodes"), bank


def _learner(mode="fight", **kw):
    from hhmarl_2d_amd.learner import PPOLearner
    return PPOLearner.trainable_init(torch.device("cuda", 0), mode=mode, seed=5, **{**dict(num_sgd_iter=2, sgd_minibatch_size=256), **kw})


def _gap(a, b):
    """per policy the largest difference over the five mean statistics of two learners' update results"""
    return [max(abs(x[k] - y[k]) for k in STAT_KEYS) for x, y in zip(a, b)]


def _check_update(what, st_graph, st_fused, st_plain, graph, n_rows):
    """the graph learner's statistics differ from the eager fused=True learner's by at most 4 x what the eager fused=True and
    fused=False learners — two accepted float32 forms of the same update — differ by on this batch"""
    for st in (st_graph, st_fused, st_plain):
        assert len(st) == 2 and all(s["rows"] == n_rows for s in st)
        assert all(np.isfinite(s[k]) for s in st for k in STAT_KEYS + ("kl_coeff",))
    assert [s["steps"] for s in st_graph] == [s["steps"] for s in st_fused] and all(s["steps"] >= 2 for s in st_graph)
    for a in range(2):
        book = graph._books[a]
        steps = st_graph[a]["steps"]
        assert int(book.cursor.item()) == steps == book.n_steps and int(graph.optimizers[a].t.item()) >= steps
        nv = graph.graph_stats(a, steps)[:, 5].reshape(graph.num_sgd_iter, -1).sum(dim=1)
        assert all(int(x) == n_rows for x in nv.tolist()), "every pass visits every row once"
    yard, got = _gap(st_fused, st_plain), _gap(st_graph, st_fused)
    print(f"{what}: per policy max |difference| over the five mean statistics: eager fused=True vs fused=False (the yardstick) "
          f"{yard[0]:.3e}, {yard[1]:.3e}; graph vs eager fused=True {got[0]:.3e}, {got[1]:.3e}")
    for a in range(2):
        assert got[a] <= 4.0 * yard[a], (what, a, got, yard)


def test_one_update_against_the_eager_learner():
    """64 arenas, T = 32, two passes of minibatches of 256: the same batch for a graph learner and two eager ones"""
    ro, bank = _world()
    graph, fused, plain = _learner(**GRAPH), _learner(), _learner(fused=False)
    ro.collect()
    R = ro.episodes.rows()["obs"].shape[0]
    assert R > 256
    st_g, st_f, st_p = graph.update(ro.episodes, bank), fused.update(ro.episodes, bank), plain.update(ro.episodes, bank)
    print("statistics graph", st_g, "eager", st_f)
    _check_update("one update", st_g, st_f, st_p, graph, R)
    assert set(st_g[0]) == set(st_f[0]) and graph.updates == 1 and [b.captures for b in graph._books] == [1, 1]
    graph.publish(bank)
    got = [[bank.packed(slot, part).clone() for part in range(5)] for slot in (0, 1)]
    bank.refresh_trainable(plain.modules)
    bank.refresh_trainable(graph.modules)
    for slot in (0, 1):
        for part in range(5):
            assert torch.equal(got[slot][part], bank.packed(slot, part))
    assert graph.modules[1].shared_layer._model[0].weight is graph.modules[0].shared_layer._model[0].weight
    assert list(graph.modules[0].state_dict()) == list(plain.modules[0].state_dict())


def test_two_updates_recapture_when_kl_coeff_and_cap_change():
    """kl_target = 1e-9 makes kl_coeff grow after the first update, and the second collect cuts other minibatches: the graph of the first
    update bakes both in, so the second update must capture again — with the first update's graph it misses the yardstick.  horizon = 20
    under T = 32: the first collect completes one episode per arena, the second two, so the schedule doubles"""
    ro, bank = _world(horizon=20)
    kw = dict(kl_target=1e-9)
    graph, fused, plain = _learner(**GRAPH, **kw), _learner(**kw), _learner(fused=False, **kw)
    seen = []
    for rnd in range(2):
        ro.collect()
        R = ro.episodes.rows()["obs"].shape[0]
        st = [ln.update(ro.episodes, bank) for ln in (graph, fused, plain)]
        _check_update(f"update {rnd + 1} of two", *st, graph, R)
        seen.append(([b.cap for b in graph._books], [b.n_steps for b in graph._books], list(graph.kl_coeff)))
    (cap0, steps0, kl0), (cap1, steps1, kl1) = seen
    assert kl0 == [0.2 * 1.5] * 2 and kl1 == [0.2 * 1.5 * 1.5] * 2 and graph.kl_coeff == fused.kl_coeff
    assert cap0 != cap1 or steps0 != steps1, "the two collects must differ in cap or in the schedule length for this test to bite"
    assert [b.captures for b in graph._books] == [2, 2]


def test_the_graph_is_kept_while_nothing_baked_into_it_changes():
    """kl_coeff = 0 (no KL term, no update_kl) and the same batch twice: one capture serves both updates"""
    ro, bank = _world()
    graph = _learner(kl_coeff=0.0, **GRAPH)
    ro.collect()
    graph.update(ro.episodes, bank)
    st = graph.update(ro.episodes, bank)
    assert [b.captures for b in graph._books] == [1, 1] and graph.updates == 2
    assert all(np.isfinite(s[k]) for s in st for k in STAT_KEYS) and all(int(o.t.item()) == 2 * s["steps"] for o, s in zip(graph.optimizers, st))


def test_eager_step_with_the_device_adam():
    """optimizer="fused" in the eager step: the same step counts, statistics within 4 x the fused = True / False yardstick"""
    ro, bank = _world()
    dev_adam, fused, plain = _learner(optimizer="fused"), _learner(), _learner(fused=False)
    ro.collect()
    st_d, st_f, st_p = (ln.update(ro.episodes, bank) for ln in (dev_adam, fused, plain))
    yard, got = _gap(st_f, st_p), _gap(st_d, st_f)
    print(f"eager + device Adam vs eager + torch Adam {got}, yardstick {yard}")
    assert [s["steps"] for s in st_d] == [s["steps"] for s in st_f]
    assert all(int(o.t.item()) == s["steps"] for o, s in zip(dev_adam.optimizers, st_d))
    assert all(g <= 4.0 * y for g, y in zip(got, yard))


def _surrogate_objective(learner, batch, agent, clip):
    """mean over the whole batch of min(adv ratio, adv clamp(ratio)) with the module's current weights (float64 accumulate)"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    with torch.no_grad():
        logits, _ = learner.modules[agent](batch["obs"], batch["critic"])
        lo, lp = 0, 0.0
        for i, w in enumerate(PN.ACTION_SPLIT[:LR.n_comp_of(learner.kinds[agent])]):
            lp = lp + torch.log_softmax(logits[:, lo:lo + w].double(), dim=1).gather(1, batch["actions"][:, i:i + 1].long()).squeeze(1)
            lo += w
        ratio = torch.exp(lp - batch["old_logp"].double())
        adv = batch["adv"].double()
        return torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean().item()


def test_escape_update_raises_the_clipped_surrogate():
    ro, bank = _world("escape", N=256)
    learner = _learner("escape", num_sgd_iter=4, sgd_minibatch_size=512, **GRAPH)
    ro.collect()
    rows = ro.episodes.rows()
    old = learner.old_logits(rows["obs"], bank, ro.episodes.N)
    batches = [learner.policy_batch(rows, old, a) for a in range(2)]
    before = [_surrogate_objective(learner, batches[a], a, learner.clip_param) for a in range(2)]
    st = learner.update(ro.episodes, bank)
    after = [_surrogate_objective(learner, batches[a], a, learner.clip_param) for a in range(2)]
    print("clipped surrogate objective before / after one graph update:", before, after, st)
    assert all(x1 > x0 for x0, x1 in zip(before, after))
    assert all(s["rows"] == rows["obs"].shape[0] and s["steps"] % 4 == 0 for s in st)
