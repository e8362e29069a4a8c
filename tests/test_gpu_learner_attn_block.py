"""learner.TrainableNet(attention="block") and PPOLearner(attention="block") on the MI355X: every parameter's gradient and the loss
statistics against a float64 run (at most 4 x as far from it as the default path), alone and under the fused input stage and the fused
tail; the forward against the reference's recorded training-form outputs; the first replay of the captured minibatch step; one update on
a real collect and publish."""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_learner_graph import _policy_batch, _state_bytes, _weights
from test_gpu_learner_heads import _compare, _fight_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)
STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy")
VARIANTS = {"block": {}, "block + inputs": dict(inputs="fused"), "block + inputs + heads": dict(inputs="fused", heads="fused")}


@pytest.mark.parametrize("flat", (False, True))
@pytest.mark.parametrize("kind", (0, 1))
def test_gradients_block_against_torch_attention(kind, flat):
    """test_gpu_learner_attention.test_gradients_fused_against_torch_attention's construction (S = 96 chunks of 20, masked; flat: the same
    rows as 1920 chunks of length 1) with attention="block" alone, with inputs="fused", and with inputs="fused", heads="fused" (pre_heads +
    heads_loss): gradients of every parameter and the first five statistics, each path against a float64 run of the default module"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    dev = torch.device("cuda", 0)
    w, own, crit, batch, n_comp = _fight_case(kind, flat)
    nets = {"torch": LR.TrainableNet(kind).load_numpy(w).to(dev)}
    nets.update({label: LR.TrainableNet(kind, attention="block", **kw).load_numpy(w).to(dev) for label, kw in VARIANTS.items()})
    assert all(m.attention == "block" for label, m in nets.items() if label != "torch")
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


@pytest.mark.parametrize("kind", (0, 1))
def test_block_forward_equals_reference_recording(kind):
    """tests/golden/fight_sequence_forward.npz (the reference's own Fight1 / Fight2 forward + value_function on padded chunks) within the
    1.5e-4 that tests/test_learner_host.py established for the file"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    g = np.load(os.path.join(ROOT, "tests", "golden", "fight_sequence_forward.npz"))
    name = PN.KIND_NAMES[kind]
    seed = json.loads(str(g["meta"]))["seed"]
    m = LR.TrainableNet(kind, attention="block").load_numpy(_weights(kind, seed)).cuda().eval()
    with torch.no_grad():
        logits, value = m(torch.from_numpy(g[f"{name}_obs"]).cuda(), torch.from_numpy(g[f"{name}_critic"]).cuda())
    dl = np.abs(logits.cpu().numpy() - g[f"{name}_logits"]).max()
    dv = np.abs(value.cpu().numpy() - g[f"{name}_value"]).max()
    print(f"{name}: max |logits - reference| = {dl:.3e}, max |value - reference| = {dv:.3e}")
    assert logits.shape == g[f"{name}_logits"].shape and value.shape == g[f"{name}_value"].shape
    assert dl <= 1.5e-4 and dv <= 1.5e-4


@pytest.mark.parametrize("kind", (0, 1))
def test_first_replayed_step_with_block_attention(kind):
    """test_gpu_learner_graph.test_first_replayed_step_against_the_eager_step_and_float64's construction for PPOLearner(attention="block",
    inputs="fused", optimizer="fused", step="graph"): 14 ragged chunks staged into cap = 16 (two chunks of pure padding).  Capture leaves
    weights, m, v, t and the cursor bit for bit; the first replay's gradients and statistics are at most 4 x as far from float64 as the
    default eager step's; a second replay of the same schedule row from the restored state writes the same bytes"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    dev = torch.device("cuda", 0)
    kinds = (PN.FIGHT1, PN.FIGHT2)
    agent = kinds.index(kind)
    sds = [_weights(k, 9) for k in kinds]
    kw = dict(entropy_coeff=0.01, num_sgd_iter=1, sgd_minibatch_size=100000, seed=9)
    graph = LR.PPOLearner(kinds, sds, dev, **kw, attention="block", inputs="fused", optimizer="fused", step="graph")
    eager = LR.PPOLearner(kinds, sds, dev, **kw)
    assert graph.attention == "block" and all(m.attention == "block" for m in graph.modules) and eager.attention == "torch"
    net64 = LR.TrainableNet(kind)
    net64.load_state_dict(eager.modules[agent].state_dict())
    net64 = net64.double().to(dev)
    b = _policy_batch(kind, eager.modules[agent], 40 + kind)
    cap = 16

    before = _state_bytes(graph, agent)
    n_steps, n_rows = graph.graph_prepare(agent, b, cap=cap)
    assert _state_bytes(graph, agent) == before, "warm-up and capture leave weights, m, v, t and the cursor bit for bit as they were"
    valid = int(b["seq_len"].sum())
    assert (n_steps, n_rows) == (1, valid) and graph._books[agent].cap == cap
    opt, book = graph.optimizers[agent], graph._books[agent]
    params = list(graph.modules[agent].parameters())
    kept = [[t.detach().clone() for t in ts] for ts in (params, opt.m, opt.v, [opt.t])]

    def replay():
        graph.graph_replay(agent, 1)
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in graph.modules[agent].named_parameters()}
        return grads, graph.graph_stats(agent, 1)[0].clone(), _state_bytes(graph, agent)

    g_graph, s_graph, after = replay()
    assert int(opt.t.item()) == 1 and int(book.cursor.item()) == 1 and int(book.n_valid.item()) == valid and s_graph[5].item() == valid
    staged = book.staged
    assert staged["obs"].shape[0] == cap and int(staged["mask"].sum()) == valid and not staged["obs"][cap - 2:].any()
    assert all(x != y for x, y in zip(after[:len(params)], before[:len(params)])), "one replay is one Adam step of every tensor"
    with torch.no_grad():
        for ts, olds in zip((params, opt.m, opt.v, [opt.t]), kept):
            for t, old in zip(ts, olds):
                t.copy_(old)
        book.cursor.zero_()
    assert _state_bytes(graph, agent) == before
    g_again, s_again, after_again = replay()
    assert after_again == after and torch.equal(s_again, s_graph) and all(torch.equal(g_again[k], g_graph[k]) for k in g_graph)

    mb = {k: v for k, v in b.items() if k != "seq_len"}
    mb["n_valid"] = torch.tensor([valid], dtype=torch.int32, device=dev)

    def grads(module, dt):
        module.zero_grad(set_to_none=True)
        logits, vf = module(mb["obs"].to(dt), mb["critic"].to(dt))
        if dt == torch.float64:
            total, stats = LR.ppo_loss_torch(logits, vf, mb, n_comp=LR.n_comp_of(kind), clip_param=eager.clip_param, vf_clip_param=eager.vf_clip_param,
                                             vf_loss_coeff=eager.vf_loss_coeff, entropy_coeff=eager.entropy_coeff, kl_coeff=eager.kl_coeff[agent])
        else:
            total, stats = eager.loss(agent, logits, vf, mb)
        total.backward()
        return {k: p.grad.double().clone() for k, p in module.named_parameters()}, stats.clone()

    g64, s64 = grads(net64, torch.float64)
    _compare(f"{PN.KIND_NAMES[kind]} graph step", {"torch": grads(eager.modules[agent], torch.float32),
                                                  "graph, block": ({k: v.double() for k, v in g_graph.items()}, s_graph)}, g64, s64)


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


def test_one_update_with_block_attention():
    """test_gpu_learner_attention.test_one_update_with_fused_attention with "block": one update of one minibatch over a real collect (256
    arenas, T = 32, horizon 30); every statistic finite, policy 0's (the first forward of the update) at most 4 x as far from a float64
    module's as the default learner's; publish gives the bank the packed bytes that refresh_trainable gives"""
    from hhmarl_2d_amd import learner as LR
    ro, bank, block = _setup("block")
    _, _, plain = _setup("torch")
    assert block.attention == "block" and all(m.attention == "block" for m in block.modules) and block.state_dict()["options"]["attention"] == "block"
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
    st_b, st_t = block.update(ro.episodes, bank), plain.update(ro.episodes, bank)
    for st in (st_b, st_t):
        assert len(st) == 2 and all(s["steps"] == 1 and s["rows"] == rows["obs"].shape[0] for s in st)
        assert all(np.isfinite(s[k]) for s in st for k in STAT_KEYS + ("kl_coeff",))
    e_b = max(abs(st_b[0][k] - w) for k, w in zip(STAT_KEYS, s64))
    e_t = max(abs(st_t[0][k] - w) for k, w in zip(STAT_KEYS, s64))
    print(f"policy 0 statistics against float64 {s64}: error attention=torch {e_t:.3e}, attention=block {e_b:.3e}")
    assert e_b <= 4.0 * e_t
    block.publish(bank)
    got = [[bank.packed(slot, part).clone() for part in range(5)] for slot in (0, 1)]
    bank.refresh_trainable(plain.modules)
    bank.refresh_trainable(block.modules)
    for slot in (0, 1):
        for part in range(5):
            assert torch.equal(got[slot][part], bank.packed(slot, part))
    assert block.modules[1].shared_layer._model[0].weight is block.modules[0].shared_layer._model[0].weight
