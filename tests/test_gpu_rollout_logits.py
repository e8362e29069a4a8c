"""record_logits=True on the MI355X: the logits of the sampler call that drew a row's action travel with the row through the carry into the
whole-episode batch (PPORollout / EpisodeBatch, CommanderRollout / CommanderEpisodeBatch), and the learners use that column.
  (a) row order: every emitted row's (arena, episode, t) names the tick it was sampled in; its logits and logp are byte-equal to that
      tick's in the host copies of the collects — a consistency check between two outputs of the same sampler call;
  (b) two weight versions: other weights are published after two collects; an emitted episode that spans the publish carries, in its
      earlier rows, the logits of the weights that sampled them, not what a recompute after the publish gives;
  (c) the learners take the column as it stands (no bank call / no module forward) and an update on such a batch completes;
  (d) record_logits=False: no buffer, no column, and collects byte-equal to those of a rollout built by the earlier signature."""
import numpy as np
import pytest
import torch

from episodes_ref import pad_sequences

pytestmark = pytest.mark.gpu
K, PUBLISH_AFTER = 6, 2


# ------------------------------------------------------------------------------------------------------------------ helpers
def _tick_of_rows(rows, done_all):
    """global tick (over the concatenated collects) of every emitted row, from its arena / episode / t columns and the done stream"""
    arena, episode, t = (rows[k].astype(np.int64) for k in ("arena", "episode", "t"))
    g = np.empty(len(t), dtype=np.int64)
    for n in np.unique(arena):
        ends = np.nonzero(done_all[:, n])[0]
        first = np.concatenate([[0], ends + 1])              # first tick of episode e of this arena
        m = arena == n
        g[m] = first[episode[m]] + t[m]
    return g


def _run(ro, publish, cols):
    """K collects with `publish()` after the second -> (host copies of the [T, N] buffers concatenated over the collects, emitted batches
    (numpy) with the global tick of every row and the index of the collect that emitted it)"""
    host = {k: [] for k in cols}
    emitted = []
    for c in range(K):
        if c == PUBLISH_AFTER:
            publish()
        ro.collect()
        torch.cuda.synchronize()
        for k in cols:
            host[k].append(getattr(ro, k)[: ro.T].cpu().numpy().copy())
        emitted.append({k: v.cpu().numpy() for k, v in ro.episodes.rows().items()})
    host = {k: np.concatenate(v, axis=0) for k, v in host.items()}
    for c, b in enumerate(emitted):
        b["tick"] = _tick_of_rows(b, host["done"][: (c + 1) * ro.T])
    return host, emitted


def _check_rows_carry_their_ticks_outputs(host, emitted, T):
    """(a) for every emitted row: logits, logp and actions of the tick it was sampled in, bit for bit"""
    n_rows = 0
    for c, b in enumerate(emitted):
        g, n = b["tick"], b["arena"]
        assert (g >= 0).all() and (g < (c + 1) * T).all()
        assert np.array_equal(b["logits"].view(np.uint32), host["logits"][g, n].view(np.uint32)), f"collect {c}: logits are not their tick's"
        assert np.array_equal(b["logp"].view(np.uint32), host["logp"][g, n].view(np.uint32)), f"collect {c}: logp is not its tick's"
        assert np.array_equal(b["actions"], host["actions"][g, n])
        n_rows += len(g)
    return n_rows


def _spanning_rows(emitted, T):
    """per emitted batch: mask of the rows sampled before the publish that belong to an episode emitted after it"""
    cut = PUBLISH_AFTER * T                       # ticks [0, cut) were sampled with the first weights
    out = []
    for c, b in enumerate(emitted):
        out.append((b["tick"] < cut) if c >= PUBLISH_AFTER else np.zeros(len(b["tick"]), dtype=bool))
    return out


# ------------------------------------------------------------------------------------------------------------------ the 2-vs-2 policies
def _ppo(use_graph=True, record=True, new_signature=True, N=64, T=8, horizon=20):
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, level=1, seed=23, auto_reset=True, horizon=horizon), device=0)
    bank = PolicyBank.trainable_init(torch.device("cuda", 0), mode="fight", seed=5, max_rows=2 * N)
    if not new_signature:
        return PPORollout(w, bank, T, use_graph=use_graph, batch_mode="complete_episodes")
    return PPORollout(w, bank, T, use_graph=use_graph, batch_mode="complete_episodes", record_logits=record)


class _CountingBank:
    """a PolicyBank whose sample calls are counted"""

    def __init__(self, bank):
        self._bank, self.calls = bank, 0

    def sample(self, *a, **kw):
        self.calls += 1
        return self._bank.sample(*a, **kw)

    def __getattr__(self, name):
        return getattr(self._bank, name)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_ppo_rows_carry_the_logits_of_their_own_forward(use_graph):
    from hhmarl_2d_amd.learner import PPOLearner
    ro = _ppo(use_graph)
    assert ro.logits.shape == (8, 64, 2, 32) and ro.logits.dtype == torch.float32
    other = PPOLearner.trainable_init(torch.device("cuda", 0), mode="fight", seed=1)      # visibly different weights
    host, emitted = _run(ro, lambda: other.publish(ro.bank), ("logits", "actions", "logp", "done"))
    T = ro.T
    # (a)
    assert _check_rows_carry_their_ticks_outputs(host, emitted, T) > 64 * T
    assert host["logits"][..., :26].any() and not host["logits"][:, :, 0, 26:].any() and not host["logits"][:, :, 1, 24:].any()
    # (b) in a batch emitted after the publish every episode ends after it, so its rows sampled before it belong to an episode that spans it
    cut = PUBLISH_AFTER * T
    span = _spanning_rows(emitted, T)
    assert sum(int(m.sum()) for m in span) > 0, "no emitted episode spans the publish: choose another seed / horizon"
    for c, (b, m) in enumerate(zip(emitted, span)):
        if not m.any():
            continue
        ep_key = b["arena"].astype(np.int64) * 1_000_000 + b["episode"]
        assert set(ep_key[m]) <= set(ep_key[b["tick"] >= cut]), "the t / tick columns: these episodes have rows on both sides of the publish"
        recomputed = other.old_logits(torch.from_numpy(b["obs"]).cuda(), ro.bank, ro.w.N).cpu().numpy()   # the bank holds the published weights
        got, rec, want = b["logits"][m], recomputed[m], host["logits"][b["tick"][m], b["arena"][m]]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "pre-publish rows must carry the pre-publish logits"
        late = b["tick"] >= cut
        d_pre, d_late = np.abs(got - rec).reshape(len(got), -1).max(axis=1), np.abs(b["logits"][late] - recomputed[late]).max()
        print(f"collect {c}: {int(m.sum())} pre-publish rows, |recorded - recomputed| min {d_pre.min():.3e} max {d_pre.max():.3e}; "
              f"{int(late.sum())} post-publish rows, max {d_late:.3e}")
        assert (d_pre > 0).all() and d_pre.max() > 1e-3, "a pre-publish row carries the post-publish weights' logits"
        # rows sampled after the publish: the recompute is the same weights' forward in another launch shape (the forms' last bits)
        assert d_late < 1e-4


def test_ppo_learner_uses_the_column_and_makes_no_bank_call():
    from hhmarl_2d_amd.learner import PPOLearner
    ro = _ppo()
    for _ in range(4):
        ro.collect()
    rows = ro.episodes.rows()
    assert rows["logits"].shape == (rows["obs"].shape[0], 2, 32) and rows["obs"].shape[0] > 0
    learner = PPOLearner.trainable_init(torch.device("cuda", 0), mode="fight", seed=5, num_sgd_iter=1, sgd_minibatch_size=128)
    bank = _CountingBank(ro.bank)
    old = learner.batch_old_logits(rows, bank, ro.w.N)
    assert old is rows["logits"] and bank.calls == 0
    stats = learner.update(ro.episodes, bank)
    assert bank.calls == 0
    for s in stats:
        assert s["steps"] > 0 and s["rows"] == rows["obs"].shape[0]
        assert all(np.isfinite(s[k]) for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "kl_coeff"))
    # without the column the same learner recomputes from the bank, in ceil(R / N) calls
    plain = {k: v for k, v in rows.items() if k != "logits"}
    rec = learner.batch_old_logits(plain, bank, ro.w.N)
    assert bank.calls == -(-rows["obs"].shape[0] // ro.w.N) and rec.shape == rows["logits"].shape


def test_ppo_default_is_unchanged():
    """(d) record_logits=False: no buffer, no column; two collects byte-equal to those of a rollout built by the earlier signature"""
    a, b = _ppo(record=False), _ppo(new_signature=False)
    assert not hasattr(a, "logits") and a.episodes.aux_name is None and not hasattr(a.episodes, "logits")
    bufs = ("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target")
    for c in range(2):
        ra, rb = a.collect().episodes.rows(), b.collect().episodes.rows()
        assert "logits" not in ra and set(ra) == set(rb)
        for k in bufs:
            assert torch.equal(getattr(a, k), getattr(b, k)), (c, k)
        for k in ra:
            assert torch.equal(ra[k], rb[k]), (c, k)
    # and recording changes nothing else: the same buffers and batch with the column on
    r = _ppo(record=True)
    a2 = _ppo(record=False)
    for c in range(2):
        rr, ra = r.collect().episodes.rows(), a2.collect().episodes.rows()
        for k in bufs:
            assert torch.equal(getattr(r, k), getattr(a2, k)), (c, k)
        for k in ra:
            assert torch.equal(rr[k], ra[k]), (c, k)


# ------------------------------------------------------------------------------------------------------------------ the commander
def _cmd(use_graph=True, record=True, N=16, T=4, horizon=100, L=4):
    from hhmarl_2d_amd import _lib as LB
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, env_kind=LB.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True,
                          horizon=horizon), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    return CommanderRollout(w, net, VariantNetPilot(w, seed=8), T, use_graph=use_graph, batch_mode="complete_episodes", max_seq_len=L,
                            record_logits=record)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_commander_rows_carry_the_logits_of_their_own_forward(use_graph):
    from hhmarl_2d_amd.learner import CommanderLearner
    ro = _cmd(use_graph)
    assert ro.logits.shape == (4, 16, 3, 4)
    other = CommanderLearner.trainable_init(torch.device("cuda", 0), seed=1, max_seq_len=4)
    host, emitted = _run(ro, lambda: other.publish(ro.net), ("logits", "actions", "logp", "done"))
    T = ro.T
    assert _check_rows_carry_their_ticks_outputs(host, emitted, T) > 16 * T
    assert host["logits"][..., :3].any() and not host["logits"][..., 3].any()
    # the sampler's logp is the log-softmax of these very logits at the drawn action
    lsm = torch.log_softmax(torch.from_numpy(host["logits"][..., :3]).double(), dim=-1)
    lp = torch.gather(lsm, -1, torch.from_numpy(host["actions"]).long()[..., None])[..., 0]
    assert (lp - torch.from_numpy(host["logp"]).double()).abs().max().item() <= 1e-6
    # (b) against the recompute with the published weights: the learner's float32 forward from the emitted sequence-start states
    cut, Lq = PUBLISH_AFTER * T, ro.max_seq_len
    span = _spanning_rows(emitted, T)
    assert sum(int(m.sum()) for m in span) > 0, "no emitted episode spans the publish: choose another seed / horizon"
    for c, (b, m) in enumerate(zip(emitted, span)):
        if not m.any():
            continue
        ep_key = b["arena"].astype(np.int64) * 1_000_000 + b["episode"]
        assert set(ep_key[m]) <= set(ep_key[b["tick"] >= cut]), "the t / tick columns: these episodes have rows on both sides of the publish"
        got, want = b["logits"][m], host["logits"][b["tick"][m], b["arena"][m]]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "pre-publish rows must carry the pre-publish logits"
        p = pad_sequences(b, Lq)
        for k in ("logits", "tick"):
            p[k] = np.zeros((len(b["seq_start"]), Lq) + b[k].shape[1:], dtype=b[k].dtype)
            for i, (s0, n) in enumerate(zip(b["seq_start"], b["seq_len"])):
                p[k][i, :n] = b[k][s0:s0 + n]
        seqs = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in p.items()}
        col = other.batch_old_logits(seqs)
        rec = other.old_logits(other.policy_batch(seqs))
        d = (col[..., :3] - rec[..., :3]).abs().amax(dim=-1)                             # [3 S, L], agent-major
        pre = torch.cat([(seqs["tick"] < cut) & seqs["mask"]] * 3, dim=0)
        fresh = torch.cat([(seqs["tick"][:, :1] - torch.from_numpy(b["t"][b["seq_start"]]).cuda()[:, None] >= cut) & seqs["mask"]] * 3, dim=0)
        print(f"collect {c}: {int(pre.sum())} pre-publish rows, |recorded - recomputed| min {d[pre].min().item():.3e} max {d[pre].max().item():.3e}; "
              f"{int(fresh.sum())} rows of episodes begun after the publish" + (f", max {d[fresh].max().item():.3e}" if fresh.any() else ""))
        assert (d[pre] > 0).all() and d[pre].max().item() > 1e-3, "a pre-publish row carries the post-publish weights' logits"
        # episodes begun after the publish: the same weights in the module's float32 forward, not the sampler's split-fp16 one: close
        if fresh.any():
            assert d[fresh].max().item() < 1e-3


def test_commander_learner_uses_the_column_and_runs_no_forward_for_it():
    from hhmarl_2d_amd.learner import CommanderLearner
    ro = _cmd()
    for c in range(12):      # 16 arenas, 4 steps per collect: not every collect ends an episode; take the first batch after the third that has one
        ro.collect()
        if c >= 3 and int(ro.episodes.n_rows) > 0:
            break
    seqs = ro.episodes.sequences()
    rows = ro.episodes.rows()
    S, Lq = seqs["mask"].shape
    assert S > 0 and seqs["logits"].shape == (S, Lq, 3, 4)
    # the padded column: the rows' logits up to seq_len, zero past it
    for i in range(S):
        s0, n = int(rows["seq_start"][i]), int(rows["seq_len"][i])
        assert torch.equal(seqs["logits"][i, :n], rows["logits"][s0:s0 + n]) and not seqs["logits"][i, n:].any()
    learner = CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, num_sgd_iter=1, sgd_minibatch_size=64, max_seq_len=4)
    calls = []
    recompute = learner.old_logits
    learner.old_logits = lambda *a, **kw: (calls.append(1), recompute(*a, **kw))[1]
    old = learner.batch_old_logits(seqs)
    assert not calls and old.shape == (3 * S, Lq, 4)
    for a in range(3):
        assert torch.equal(old[a * S:(a + 1) * S], seqs["logits"][:, :, a])
    stats = learner.update(ro.episodes, ro.net)
    assert not calls and stats["steps"] > 0 and stats["rows"] == 3 * int(seqs["mask"].sum())
    assert all(np.isfinite(stats[k]) for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "kl_coeff"))


def test_commander_default_is_unchanged():
    a = _cmd(record=False)
    assert not hasattr(a, "logits") and a.episodes.aux_name is None
    r = _cmd(record=True)
    for c in range(3):
        ra, rr = a.collect().episodes.rows(), r.collect().episodes.rows()
        assert "logits" not in ra and "logits" in rr
        assert "logits" not in a.episodes.sequences()
        for k in ("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target", "state_in"):
            assert torch.equal(getattr(a, k), getattr(r, k)), (c, k)
        for k in ra:
            assert torch.equal(ra[k], rr[k]), (c, k)
