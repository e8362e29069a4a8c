"""PPOLearner(grad_clip=...) and CommanderLearner(grad_clip=...) on the MI355X: the first replayed step of the graph (norm -> clipped Adam
inside it) against hh_adam_step on the gradients the replay left, one update in all three modes with the fused = True / False difference
as the yardstick, graph reuse, and the unchanged default.  The batches are built as tests/test_gpu_learner_graph.py and
tests/test_gpu_commander_learner_graph.py build theirs."""
import functools
import math

import numpy as np
import pytest
import torch

import grad_clip_ref as GR

pytestmark = pytest.mark.gpu
STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy")
FORMER_KEYS = set(STAT_KEYS) | {"kl_coeff", "steps", "rows"}
GRAPH = dict(optimizer="fused", step="graph")
LM = 20


# ---------------------------------------------------------------------------------------------------------------- the batches
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
    lead = (14, LM) if att else (271,)
    own = torch.rand(lead + (d1,), generator=g)
    crit = torch.cat([torch.rand(lead + (a1 + a2,), generator=g), own, torch.rand(lead + (d2,), generator=g)], dim=-1)
    b = {}
    if att:
        seq_len = torch.randint(1, LM + 1, (14,), generator=g)
        seq_len[0], seq_len[1] = LM, 1
        mask = LR.chunk_mask(seq_len, LM)
        own, crit = own * mask[..., None], crit * mask[..., None]
        b["seq_len"], b["mask"] = seq_len.to(dev), mask.to(torch.uint8).to(dev)
    splits = PN.ACTION_SPLIT[:LR.n_comp_of(kind)]
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


def _commander_batch(module, seed, S=17):
    """a policy batch as CommanderLearner.policy_batch makes it, with old_logits: S sequences of 20 steps, ragged seq_len with
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


class _Fight:
    """one policy of a PPOLearner behind the commander learner's argument-free interface"""

    def __init__(self, kind, grad_clip):
        from hhmarl_2d_amd import learner as LR
        from hhmarl_2d_amd import policy_nets as PN
        att = PN.HAS_ATT[kind]
        kinds = (PN.FIGHT1, PN.FIGHT2) if att else (PN.ESC1, PN.ESC2)
        self.agent, self.cap, self.kind = kinds.index(kind), 16 if att else 288, kind
        self.ln = LR.PPOLearner(kinds, [_weights(k, 9) for k in kinds], torch.device("cuda", 0), entropy_coeff=0.01, num_sgd_iter=1,
                                sgd_minibatch_size=100000, seed=9, grad_clip=grad_clip, **GRAPH)
        self.opt, self.book, self.module = self.ln.optimizers[self.agent], self.ln._books[self.agent], self.ln.modules[self.agent]

    def batch(self):
        return _policy_batch(self.kind, self.module, 40 + self.kind)

    def prepare(self, b):
        return self.ln.graph_prepare(self.agent, b, cap=self.cap)

    def replay(self):
        self.ln.graph_replay(self.agent, 1)


class _Commander:
    def __init__(self, _, grad_clip):
        from hhmarl_2d_amd import learner as LR
        self.ln = LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, entropy_coeff=0.01, num_sgd_iter=1, sgd_minibatch_size=100000,
                                                     grad_clip=grad_clip, **GRAPH)
        self.opt, self.book, self.module, self.cap = self.ln.optimizer, self.ln._book, self.ln.module, 20

    def batch(self):
        return _commander_batch(self.module, 41)

    def prepare(self, b):
        return self.ln.graph_prepare(b, cap=self.cap)

    def replay(self):
        self.ln.graph_replay(1)


def _state_bytes(x):
    torch.cuda.synchronize()
    return ([p.detach().cpu().numpy().tobytes() for p in x.module.parameters()] + [t.cpu().numpy().tobytes() for t in x.opt.m + x.opt.v]
            + [x.opt.t.cpu().numpy().tobytes(), x.book.cursor.cpu().numpy().tobytes()])


# ---------------------------------------------------------------------------------------------------------------- the first replayed step
@functools.lru_cache(maxsize=None)
def _unclipped_first_step(make, kind):
    """a learner with grad_clip = 1e30 takes one replay of its batch: N0, the first step's norm from its gnorm table, with a coefficient of
    exactly 1 -> dict(n0, batch, before: the state's bytes before the prepare, m: the first moments' bytes after the step).  Computed once."""
    free = make(kind, 1e30)
    b = free.batch()
    before = _state_bytes(free)
    assert free.prepare(b)[0] == 1 and _state_bytes(free) == before
    free.replay()
    torch.cuda.synchronize()
    n0 = float(free.book.gnorm[0].item())
    assert free.opt.clip.tolist() == [n0, 1.0] and math.isfinite(n0) and n0 > 0.0
    return dict(n0=n0, batch=b, before=before, m=[m.cpu().numpy().tobytes() for m in free.opt.m])


@pytest.mark.parametrize("make,kind", [(_Fight, 0), (_Fight, 2), (_Commander, None)], ids=["fight1", "esc1", "commander"])
def test_first_replayed_step_clips_inside_the_graph(make, kind):
    """Fight1: 14 chunks of 20 in cap 16; Esc1: 271 rows; the commander: 17 sequences in cap 20.  A learner with grad_clip = 1e30 gives the
    first step's norm N0 (coefficient exactly 1); a second one from the same weights with grad_clip = N0 / 2 takes one replay: its clip is
    the float64 norm of the p.grad it left, and m and v of every parameter are, bit for bit, hh_adam_step's from zero state on
    float32(float64(p.grad) clip[1]).  (m and v, not p: Adam's first step is nearly invariant to the gradient's scale.)"""
    from hhmarl_2d_amd import learner as LR
    free = _unclipped_first_step(make, kind)
    n0, b = free["n0"], free["batch"]
    half = make(kind, n0 / 2.0)
    assert _state_bytes(half)[:-2] == free["before"][:-2], "the same weights"
    before = _state_bytes(half)
    assert half.prepare(b)[0] == 1
    assert _state_bytes(half) == before, "warm-up and capture leave weights, m, v, t and the cursor bit for bit as they were"
    assert not half.opt.clip.any() and not half.book.gnorm.any(), "no norm launch ran outside the capture"
    half.replay()
    torch.cuda.synchronize()
    opt, book = half.opt, half.book
    assert int(opt.t.item()) == 1 and int(book.cursor.item()) == 1 and book.captures == 1
    assert all(p.grad is not None for p in opt.params)
    grads = [p.grad.detach().cpu().numpy().reshape(-1) for p in opt.params]
    norm, coef = opt.clip.tolist()
    want, _ = GR.norm_coef(grads, n0 / 2.0)
    print(f"N0 {n0!r}; clipped learner: clip {norm!r}, {coef!r}; float64 norm of the gradients it left {want!r} "
          f"(relative difference {abs(norm - want) / want:.3e}, bound {GR.bound(grads):.3e})")
    assert abs(norm - want) <= GR.bound(grads) * want
    assert coef < 1.0 and abs(coef - min(1.0, (n0 / 2.0) / (norm + 1e-6))) <= 2 * np.spacing(coef)
    assert float(book.gnorm[0].item()) == norm and not book.gnorm[1:].any()
    # hh_adam_step from zero state on the host-scaled gradients
    dev = opt.params[0].device
    scaled = [torch.from_numpy(s).to(dev) for s in GR.scaled(grads, coef)]
    p0 = [torch.zeros_like(s) for s in scaled]
    m0, v0 = [torch.zeros_like(s) for s in scaled], [torch.zeros_like(s) for s in scaled]
    LR.adam_step(p0, scaled, m0, v0, torch.zeros((1,), dtype=torch.int32, device=dev), lr=opt.lr)
    torch.cuda.synchronize()
    for i, (m, v) in enumerate(zip(opt.m, opt.v)):
        assert m.cpu().numpy().tobytes() == m0[i].cpu().numpy().tobytes(), f"m of parameter {i}"
        assert v.cpu().numpy().tobytes() == v0[i].cpu().numpy().tobytes(), f"v of parameter {i}"
    differ = sum(m.cpu().numpy().tobytes() != mf for m, mf in zip(opt.m, free["m"]))
    assert differ == len(opt.m), "the clip changed every first moment"


# ---------------------------------------------------------------------------------------------------------------- one update, three modes
def _fight_world(N=64, T=32, horizon=30, seed=23):
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, level=3, seed=seed, auto_reset=True, horizon=horizon, agent_mode=0), device=0)
    bank = PolicyBank.trainable_init(torch.device("cuda", 0), mode="fight", seed=5, max_rows=2 * N)
    return PPORollout(w, bank, T, batch_mode="complete_episodes"), bank


@pytest.fixture(scope="module")
def fight():
    """64 arenas, T = 32, horizon 30: one collect, read only"""
    ro, bank = _fight_world()
    ro.collect()
    torch.cuda.synchronize()
    return ro.episodes, bank


@pytest.fixture(scope="module")
def commander():
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
    return ro.episodes, net


def _fight_learner(**kw):
    from hhmarl_2d_amd.learner import PPOLearner
    return PPOLearner.trainable_init(torch.device("cuda", 0), mode="fight", seed=5, **{**dict(num_sgd_iter=2, sgd_minibatch_size=256), **kw})


def _commander_learner(**kw):
    from hhmarl_2d_amd.learner import CommanderLearner
    return CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, **{**dict(num_sgd_iter=2, sgd_minibatch_size=256), **kw})


def _gap(a, b, keys):
    return max(abs(a[k] - b[k]) for k in keys)


def _check_three_modes(what, clip, results):
    """results: per learner (graph, eager with the device Adam, eager fused=True, eager fused=False) the list of its policies' dicts.
    grad_clip is N0 / 2 with N0 the first replayed step's norm of the test above (Fight1's for the fight update, the commander's for the
    commander's).  The first step of THESE updates is no substitute: measured unclipped, the norm of a fresh learner's very first step is
    5.50 / 5.23 (fight policies) and 12.46 (commander) and falls at once, the means over the update's 16 / 28 steps are 2.39 / 2.75 and
    3.38 — half of that first norm is a threshold that the mean of the norms does not reach (fight policy 0, commander)."""
    keys = STAT_KEYS + ("grad_gnorm",)
    for p, (g, d, f, pl) in enumerate(zip(*results)):
        for st in (g, d, f, pl):
            assert set(st) == FORMER_KEYS | {"grad_gnorm"} and all(np.isfinite(st[k]) for k in keys)
            assert st["grad_gnorm"] > clip, "the mean norm before clipping is above grad_clip: the clip bound at least once"
        assert g["steps"] == d["steps"] == f["steps"] == pl["steps"] >= 2 and g["rows"] == f["rows"]
        yard, got, got_d = _gap(f, pl, keys), _gap(g, f, keys), _gap(d, f, keys)
        print(f"{what} policy {p}: grad_clip {clip:.6e}; grad_gnorm graph {g['grad_gnorm']!r}, device Adam {d['grad_gnorm']!r}, fused=True "
              f"{f['grad_gnorm']!r}, fused=False {pl['grad_gnorm']!r}; max |difference| over the five statistics and grad_gnorm: fused=True vs "
              f"fused=False (the yardstick) {yard:.3e} (statistics {_gap(f, pl, STAT_KEYS):.3e}, grad_gnorm {_gap(f, pl, ('grad_gnorm',)):.3e}); "
              f"graph vs fused=True {got:.3e} (statistics {_gap(g, f, STAT_KEYS):.3e}, grad_gnorm {_gap(g, f, ('grad_gnorm',)):.3e}); "
              f"eager device Adam vs fused=True {got_d:.3e}")
        assert got <= 4.0 * yard


def test_one_fight_update_in_all_three_modes(fight):
    ep, bank = fight
    clip = _unclipped_first_step(_Fight, 0)["n0"] / 2.0
    learners = [_fight_learner(grad_clip=clip, **GRAPH), _fight_learner(grad_clip=clip, optimizer="fused"), _fight_learner(grad_clip=clip),
                _fight_learner(grad_clip=clip, fused=False)]
    results = [ln.update(ep, bank) for ln in learners]
    _check_three_modes("fight", clip, results)
    graph = learners[0]
    for a in range(2):
        steps = results[0][a]["steps"]
        assert int(graph._books[a].cursor.item()) == steps and float(graph._books[a].gnorm[:steps].mean()) == results[0][a]["grad_gnorm"]
        assert bool((graph._books[a].gnorm[:steps] > 0).all()) and not graph._books[a].gnorm[steps:].any()
        print(f"fight policy {a}, graph: norms before clipping per step {[round(x, 4) for x in graph._books[a].gnorm[:steps].tolist()]}")


def test_one_commander_update_in_all_three_modes(commander):
    ep, net = commander
    clip = _unclipped_first_step(_Commander, None)["n0"] / 2.0
    learners = [_commander_learner(grad_clip=clip, **GRAPH), _commander_learner(grad_clip=clip, optimizer="fused"), _commander_learner(grad_clip=clip),
                _commander_learner(grad_clip=clip, fused=False)]
    results = [[ln.update(ep, net)] for ln in learners]
    _check_three_modes("commander", clip, results)
    steps = results[0][0]["steps"]
    assert steps >= 4 and int(learners[0]._book.cursor.item()) == steps and int(learners[0].optimizer.t.item()) == steps
    print(f"commander, graph: norms before clipping per step {[round(x, 4) for x in learners[0]._book.gnorm[:steps].tolist()]}")


# ---------------------------------------------------------------------------------------------------------------- reuse and the default
def test_graph_reuse_and_the_default(fight, commander):
    """kl_coeff = 0 and the same batch twice: one capture; grad_clip is part of the capture's key (it travels by value); with grad_clip =
    None the result has exactly its former keys and nothing of the feature exists"""
    ep, bank = fight
    a, b, none = (_fight_learner(kl_coeff=0.0, grad_clip=c, **GRAPH) for c in (0.5, 0.25, None))
    a.update(ep, bank)
    st = a.update(ep, bank)
    assert [bk.captures for bk in a._books] == [1, 1] and a.updates == 2 and all(set(s) == FORMER_KEYS | {"grad_gnorm"} for s in st)
    b.update(ep, bank)
    assert [bk.captures for bk in b._books] == [1, 1]
    assert a._books[0].key[-3] == 0.5 and b._books[0].key[-3] == 0.25 and a._books[0].key[-2] == a._books[0].gnorm.data_ptr()
    st = none.update(ep, bank)
    assert all(set(s) == FORMER_KEYS for s in st) and len(none._books[0].key) == len(a._books[0].key) - 3
    assert all(bk.gnorm is None for bk in none._books) and all(o.clip is None and o.scratch is None and o.max_norm is None for o in none.optimizers)
    for kw in (dict(), dict(optimizer="fused")):
        assert all(set(s) == FORMER_KEYS for s in _fight_learner(num_sgd_iter=1, **kw).update(ep, bank))

    ep, net = commander
    c, none = _commander_learner(kl_coeff=0.0, grad_clip=0.5, **GRAPH), _commander_learner(kl_coeff=0.0, **GRAPH)
    c.update(ep, net)
    st = c.update(ep, net)
    assert c._book.captures == 1 and set(st) == FORMER_KEYS | {"grad_gnorm"} and c._book.key[-3] == 0.5
    st = none.update(ep, net)
    assert set(st) == FORMER_KEYS and none._book.gnorm is None and none.optimizer.clip is None and len(none._book.key) == len(c._book.key) - 3
    # a changed grad_clip on a learner whose graph exists: the next prepare captures again
    c.grad_clip = c.optimizer.max_norm = 0.125
    c.update(ep, net)
    assert c._book.captures == 2 and c._book.key[-3] == 0.125
