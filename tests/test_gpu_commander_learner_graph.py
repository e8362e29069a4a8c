"""CommanderLearner(optimizer="fused", step="graph") on the MI355X: the first replayed step against the eager step and a float64 run,
one whole update against the eager learners with the fused = True / False difference as the yardstick, re-capture when kl_coeff or cap
change, and the eager step with the device Adam.  Weights after many Adam steps are never compared between paths: m / (sqrt(v) + eps)
amplifies rounding differences, so that comparison is ill-conditioned."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy")
GRAPH = dict(optimizer="fused", step="graph")
S, LM = 14, 20


def _learner(**kw):
    from hhmarl_2d_amd import learner as LR
    return LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, **kw)


def _policy_batch(module, seed):
    """a policy batch as CommanderLearner.policy_batch makes it, with old_logits: 14 sequences of 20 steps, ragged seq_len with
    seq_len[0] = 20 and seq_len[1] = 1, random non-zero state_in, padded rows zero in every column"""
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(seed)
    seq_len = torch.randint(1, LM + 1, (S,), generator=g)
    seq_len[0], seq_len[1] = LM, 1
    mask = LR.chunk_mask(seq_len, LM)
    actions = torch.randint(0, 3, (S, LM), generator=g).to(torch.int8)
    obs = torch.rand((S, LM, 34), generator=g)
    others = torch.randint(0, 3, (S, LM, 2), generator=g).float()
    critic = torch.cat([actions[..., None].float(), others, obs, torch.rand((S, LM, 68), generator=g)], dim=-1)
    state_in = 0.5 * torch.randn((S, 2, 200), generator=g)
    assert state_in.abs().min() > 0
    b = {"obs": obs, "critic": critic, "actions": actions, "adv": torch.randn((S, LM), generator=g), "target": 2.0 * torch.randn((S, LM), generator=g)}
    b = {k: (v * mask.reshape(mask.shape + (1,) * (v.dim() - 2)).to(v.dtype)).to(dev) for k, v in b.items()}
    b.update({"mask": mask.to(torch.uint8).to(dev), "state_in": state_in.to(dev), "seq_len": seq_len.to(torch.int32).to(dev)})
    with torch.no_grad():
        lg, _ = module(b["obs"], b["critic"], b["state_in"], b["seq_len"])
    old = lg + 0.3 * torch.randn(lg.shape, generator=g).to(dev)
    m = b["mask"].bool()
    b["old_logp"] = torch.log_softmax(old, dim=-1).gather(-1, b["actions"].long()[..., None])[..., 0] * m
    b["old_logits"] = torch.nn.functional.pad(old, (0, 1)) * m[..., None]
    return b


def _state_bytes(learner):
    opt, book = learner.optimizer, learner._book
    torch.cuda.synchronize()
    return ([p.detach().cpu().numpy().tobytes() for p in learner.module.parameters()] + [x.cpu().numpy().tobytes() for x in opt.m + opt.v]
            + [opt.t.cpu().numpy().tobytes(), book.cursor.cpu().numpy().tobytes()])


def _grads64(learner, mb):
    """gradients and statistics of a float64 run of the learner's weights as they stand: torch-op GRU cell, torch-op loss"""
    from hhmarl_2d_amd import learner as LR
    net64 = LR.CommanderTrainable()
    net64.load_state_dict(learner.module.state_dict())
    net64 = net64.double().to(mb["obs"].device)
    logits, vf = net64(mb["obs"].double(), mb["critic"].double(), mb["state_in"].double(), mb["seq_len"], fused_gru=False)
    total, stats = LR.ppo_loss_categorical_torch(logits, vf, mb, clip_param=learner.clip_param, vf_clip_param=learner.vf_clip_param,
                                                 vf_loss_coeff=learner.vf_loss_coeff, entropy_coeff=learner.entropy_coeff, kl_coeff=learner.kl_coeff)
    total.backward()
    return {k: p.grad.clone() for k, p in net64.named_parameters()}, stats.clone(), net64


@pytest.mark.parametrize("opts", [{}, dict(inputs="fused")])
def test_first_replayed_step_against_the_eager_step_and_float64(opts):
    """14 sequences staged into cap = 16 (two sequences of pure padding: length 0, zero inputs, zero states).  From identical weights the
    gradients the graph's first replay leaves in p.grad and its five statistics, and the eager step's on the unpadded minibatch, each
    against a float64 run of the same module and loss: the graph at most 4 x as far from it as the eager step"""
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    kw = dict(entropy_coeff=0.01, num_sgd_iter=1, sgd_minibatch_size=100000, **opts)
    graph, eager = _learner(**kw, **GRAPH), _learner(**kw)
    assert graph.optimizer_mode == "fused" and graph.step == "graph" and eager.optimizer_mode == "torch" and eager.step == "eager"
    assert isinstance(graph.optimizer, LR.DeviceAdam) and isinstance(eager.optimizer, torch.optim.Adam)
    b = _policy_batch(eager.module, 41)
    valid, cap = int(b["seq_len"].sum()), 16
    mb = dict(b, n_valid=torch.tensor([valid], dtype=torch.int32, device=dev))
    g64, s64, _ = _grads64(eager, mb)

    before = _state_bytes(graph)
    n_steps, n_rows = graph.graph_prepare(b, cap=cap)
    assert _state_bytes(graph) == before, "warm-up and capture leave weights, m, v, t and the cursor bit for bit as they were"
    assert (n_steps, n_rows) == (1, valid) and graph._book.cap == cap and graph._book.captures == 1
    graph.graph_replay(1)
    torch.cuda.synchronize()
    g_graph = {k: p.grad.double().clone() for k, p in graph.module.named_parameters()}
    s_graph = graph.graph_stats(1)[0].clone()
    opt, book = graph.optimizer, graph._book
    assert int(opt.t.item()) == 1 and int(book.cursor.item()) == 1 and int(book.n_valid.item()) == valid and s_graph[5].item() == valid
    staged = book.staged
    assert tuple(staged) == LR.COMMANDER_STAGE_COLS and len(staged) == 10
    assert tuple(staged["state_in"].shape) == (cap, 2, 200) and staged["seq_len"].dtype == torch.int32 and tuple(staged["seq_len"].shape) == (cap,)
    for k, v in staged.items():
        assert v.shape[0] == cap and not v[S:].any(), f"staged sequences 14 and 15 are zero in {k}"
        assert torch.equal(v[:S], b[k].to(v.dtype)), f"the staged {k} is the minibatch's"
    assert staged["seq_len"][S:].tolist() == [0, 0] and int(staged["mask"].sum()) == valid
    changed = [k for (k, p), old in zip(graph.module.named_parameters(), before) if p.detach().cpu().numpy().tobytes() != old]
    assert len(changed) == len(list(graph.module.parameters())), "one replay is one Adam step of every tensor"

    eager.module.zero_grad(set_to_none=True)
    logits, vf = eager.module(mb["obs"], mb["critic"], mb["state_in"], mb["seq_len"], fused_gru=True)
    total, s_eager = eager.loss(logits, vf, mb)
    total.backward()
    g_eager = {k: p.grad.double().clone() for k, p in eager.module.named_parameters()}
    err = {}
    for label, (gr, st) in (("eager", (g_eager, s_eager)), ("graph", (g_graph, s_graph))):
        assert set(gr) == set(g64) and all(torch.isfinite(v).all() for v in gr.values())
        err[label] = (max((gr[k] - g64[k]).abs().max().item() for k in g64), (st - s64).abs()[:5].max().item())
    print(f"commander {opts}: largest parameter gradient {max(g64[k].abs().max().item() for k in g64):.3e}; (gradient, statistics) error "
          f"against float64: eager ({err['eager'][0]:.3e}, {err['eager'][1]:.3e}), graph ({err['graph'][0]:.3e}, {err['graph'][1]:.3e}); ratios "
          f"({err['graph'][0] / err['eager'][0]:.2f}, {err['graph'][1] / err['eager'][1]:.2f})")
    assert err["graph"][0] <= 4.0 * err["eager"][0]
    assert err["graph"][1] <= 4.0 * err["eager"][1]


def test_prepare_keeps_the_graph_and_refuses_a_small_cap():
    """a second graph_prepare with nothing changed keeps the graph and the state; another cap captures again; a cap below the largest
    minibatch is refused"""
    graph = _learner(num_sgd_iter=1, sgd_minibatch_size=100, **GRAPH)
    b = _policy_batch(graph.module, 43)
    n_steps, n_rows = graph.graph_prepare(b)
    need, kept = graph._book.cap, graph._book.graph
    assert n_steps >= 2 and n_rows == int(b["seq_len"].sum()) and need < S and graph._book.captures == 1
    before = _state_bytes(graph)
    assert graph.graph_prepare(b) == (n_steps, n_rows)
    assert graph._book.captures == 1 and graph._book.graph is kept and _state_bytes(graph) == before
    with pytest.raises(ValueError, match="largest minibatch"):
        graph.graph_prepare(b, cap=need - 1)
    graph.graph_prepare(b, cap=need + 3)
    assert graph._book.captures == 2 and graph._book.cap == need + 3 and _state_bytes(graph) == before
    graph.graph_replay(n_steps)
    st = graph.graph_stats(n_steps)
    assert int(graph._book.cursor.item()) == n_steps and int(st[:, 5].sum()) == n_rows and torch.isfinite(st).all()
    with pytest.raises(ValueError, match="graph_prepare needs"):
        _learner(optimizer="fused").graph_prepare(b)


@pytest.fixture(scope="module")
def episodes():
    """64 arenas, T = 16, horizon 150 with the sampler's logits recorded, collected until whole episodes have arrived; read only"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    N = 64
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True, horizon=150),
              device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    ro = CommanderRollout(w, net, VariantNetPilot(w, seed=8), 16, batch_mode="complete_episodes", max_seq_len=20, record_logits=True)
    ro.start()
    for _ in range(6):
        ro.collect()
    torch.cuda.synchronize()
    assert "logits" in ro.episodes.sequences()
    return ro.episodes, net, ro


def _gap(a, b):
    return max(abs(a[k] - b[k]) for k in STAT_KEYS)


def test_one_update_against_the_eager_learners(episodes):
    """two passes of minibatches of 256 over the same batch for a graph learner and two eager ones: the graph learner's mean statistics
    differ from the eager fused=True learner's by at most 4 x what fused=True and fused=False — two accepted float32 forms — differ by"""
    ep, net, _ = episodes
    kw = dict(num_sgd_iter=2, sgd_minibatch_size=256)
    graph, fused, plain = _learner(**kw, **GRAPH), _learner(**kw), _learner(fused=False, **kw)
    rows = int(ep.sequences()["mask"].sum()) * 3
    st_g, st_f, st_p = graph.update(ep, net), fused.update(ep, net), plain.update(ep, net)
    print("statistics graph", st_g, "eager", st_f)
    assert set(st_g) == set(st_f) and graph.updates == 1 and graph._book.captures == 1
    for st in (st_g, st_f, st_p):
        assert st["rows"] == rows and all(np.isfinite(st[k]) for k in STAT_KEYS + ("kl_coeff",))
    assert st_g["steps"] == st_f["steps"] == st_p["steps"] and st_g["steps"] >= 4
    steps = st_g["steps"]
    assert int(graph._book.cursor.item()) == steps == graph._book.n_steps and int(graph.optimizer.t.item()) == steps
    nv = graph.graph_stats(steps)[:, 5].reshape(graph.num_sgd_iter, -1).sum(dim=1)
    assert all(int(x) == rows for x in nv.tolist()), "every pass visits every row once"
    yard, got = _gap(st_f, st_p), _gap(st_g, st_f)
    print(f"max |difference| over the five mean statistics: eager fused=True vs fused=False (the yardstick) {yard:.3e}; graph vs eager "
          f"fused=True {got:.3e}")
    assert got <= 4.0 * yard
    assert list(graph.module.state_dict()) == list(plain.module.state_dict())
    graph.publish(net)


def test_two_updates_recapture_when_kl_coeff_changes(episodes):
    """kl_target = 1e-9 makes kl_coeff grow after the first update; it travels by value in hh_ppo_loss_params, so the second update
    captures again.  With kl_coeff = 0 (no KL term, no update_kl) one capture serves both updates"""
    ep, net, _ = episodes
    kw = dict(num_sgd_iter=1, sgd_minibatch_size=256)
    graph, fused = _learner(kl_target=1e-9, **kw, **GRAPH), _learner(kl_target=1e-9, **kw)
    for rnd in range(2):
        st_g, st_f = graph.update(ep, net), fused.update(ep, net)
        assert st_g["steps"] == st_f["steps"] and st_g["rows"] == st_f["rows"] and all(np.isfinite(st_g[k]) for k in STAT_KEYS)
        assert graph._book.captures == rnd + 1 and graph.kl_coeff == fused.kl_coeff == pytest.approx(0.2 * 1.5 ** (rnd + 1))
    steady = _learner(kl_coeff=0.0, **kw, **GRAPH)
    steady.update(ep, net)
    st = steady.update(ep, net)
    assert steady._book.captures == 1 and steady.updates == 2 and int(steady.optimizer.t.item()) == 2 * st["steps"]
    assert all(np.isfinite(st[k]) for k in STAT_KEYS)


def test_eager_step_with_the_device_adam():
    """optimizer="fused", step="eager": one minibatch step from the same weights as torch.optim.Adam's.  Both float32 steps against a
    float64 restatement (float64 gradients, adam_step_torch on float64 tensors): the device Adam's parameters at most 4 x as far from it
    as torch.optim.Adam's"""
    from hhmarl_2d_amd import learner as LR
    dev = torch.device("cuda", 0)
    kw = dict(entropy_coeff=0.01, lr=1e-3)
    device_adam, torch_adam = _learner(optimizer="fused", **kw), _learner(**kw)
    assert device_adam.step == "eager" and device_adam._book is not None and torch_adam._book is None
    b = _policy_batch(torch_adam.module, 47)
    mb = dict(b, n_valid=torch.tensor([int(b["seq_len"].sum())], dtype=torch.int32, device=dev))
    g64, _, net64 = _grads64(torch_adam, mb)
    p64 = [p.data for p in net64.parameters()]
    LR.adam_step_torch(p64, [g64[k] for k, _ in net64.named_parameters()], [torch.zeros_like(p) for p in p64], [torch.zeros_like(p) for p in p64], 0, lr=1e-3)
    start = [p.detach().clone() for p in torch_adam.module.parameters()]
    device_adam._book.begin(1)
    s_d, s_t = device_adam.minibatch_step(mb), torch_adam.minibatch_step(mb)
    torch.cuda.synchronize()
    assert s_d[5].item() == s_t[5].item() == mb["n_valid"].item() and int(device_adam.optimizer.t.item()) == 1 and int(device_adam._book.cursor.item()) == 1
    assert torch.equal(device_adam._book.table[0], s_d)
    err = {}
    for label, ln in (("torch", torch_adam), ("device", device_adam)):
        ps = list(ln.module.parameters())
        assert all(not torch.equal(p.detach(), p0) for p, p0 in zip(ps, start)), "one step moves every tensor"
        err[label] = max((p.detach().double() - q).abs().max().item() for p, q in zip(ps, p64))
    print(f"parameters after one Adam step (lr 1e-3) against the float64 restatement: torch.optim.Adam {err['torch']:.3e}, device Adam "
          f"{err['device']:.3e}, ratio {err['device'] / err['torch']:.2f}")
    assert err["device"] <= 4.0 * err["torch"]


def test_argument_validation():
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.commander import random_weights
    dev, sd = torch.device("cuda", 0), random_weights(6)
    with pytest.raises(ValueError, match='needs optimizer="fused"'):
        LR.CommanderLearner(sd, dev, step="graph")
    with pytest.raises(ValueError, match='needs optimizer="fused"'):
        LR.CommanderLearner(sd, dev, optimizer="torch", step="graph")
    with pytest.raises(ValueError, match="optimizer is one of"):
        LR.CommanderLearner(sd, dev, optimizer="adam")
    with pytest.raises(ValueError, match="step is one of"):
        LR.CommanderLearner(sd, dev, optimizer="fused", step="replay")
