"""CommanderLearner on the MI355X: collect -> update -> publish -> start() rounds on a small 3-vs-3 world, fused (hh_gru_seq_* and
hh_ppo_loss_categorical) and unfused (torch ops), set up the way tests/test_gpu_commander_episodes.py sets its rollouts up."""
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4          # sampler (split-fp16 MFMA, sequences of length 1) against learner (float32, whole sequences from the stored states)


def _setup(fused, N=64, T=16, horizon=150, num_sgd_iter=2, **kw):
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True,
                          horizon=horizon), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    ro = CommanderRollout(w, net, VariantNetPilot(w, seed=8), T, batch_mode="complete_episodes", max_seq_len=20)
    learner = LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, num_sgd_iter=num_sgd_iter, fused=fused, **kw)
    return ro, net, learner


def _logp_at(logits, actions):
    return torch.log_softmax(logits[..., :3].double(), dim=-1).gather(-1, actions.long()[..., None])[..., 0]


def _surrogate(learner, b):
    """the clipped surrogate of the module as it stands over the whole batch (mean over the unpadded rows)"""
    with torch.no_grad():
        logits, _ = learner.module(b["obs"], b["critic"], b["state_in"], b["seq_len"], fused_gru=learner.fused)
    m = b["mask"].bool()
    ratio = torch.exp(_logp_at(logits, b["actions"]) - b["old_logp"].double())
    A = b["adv"].double()
    s = torch.min(A * ratio, A * torch.clamp(ratio, 1 - learner.clip_param, 1 + learner.clip_param))
    return s[m].mean().item()


def _rounds(fused, n_rounds=3):
    ro, net, learner = _setup(fused)
    out = []
    for rnd in range(n_rounds):
        ro.start()
        for _ in range(8):                            # until whole episodes have arrived (horizon 150: an episode lasts at most 13 steps)
            ro.collect()
            if ro.episodes.sequences()["obs"].shape[0] >= 32:
                break
        assert ro.episodes.sequences()["obs"].shape[0] >= 32, "8 collects of 16 steps brought fewer than 32 sequences"
        graph = ro._graph
        assert graph is not None
        seqs = ro.episodes.sequences()
        before = {k: v.clone() for k, v in ro.episodes.rows().items()}
        with torch.no_grad():
            b = learner.policy_batch(seqs)
            old = learner.old_logits(b)
        m = b["mask"].bool()
        # the recomputed old logits reproduce the logp the sampler recorded at the recorded actions
        e_logp = (_logp_at(old, b["actions"])[m] - b["old_logp"][m].double()).abs().max().item()
        assert torch.equal(old[..., 3], torch.zeros_like(old[..., 3]))
        # the first minibatch, before any step: ratio 1 and no KL
        b["old_logits"] = old
        import numpy as np
        from hhmarl_2d_amd import learner as LR
        seq_len = b["seq_len"].cpu().numpy()
        s0, s1 = LR.minibatch_partition(seq_len, learner.sgd_minibatch_size)[0]
        mb = {k: v[s0:s1] for k, v in b.items()}
        mb["n_valid"] = torch.tensor([int(seq_len[s0:s1].sum())], dtype=torch.int32, device="cuda")
        with torch.no_grad():
            lg, vf = learner.module(mb["obs"], mb["critic"], mb["state_in"], mb["seq_len"], fused_gru=fused)
            _, st0 = learner.loss(lg, vf, mb)
        mm = mb["mask"].bool()
        e_ratio = (torch.exp(_logp_at(lg, mb["actions"]) - mb["old_logp"].double()) - 1.0)[mm].abs().max().item()
        print(f"fused={fused} round {rnd}: {int(m.sum())} rows in {b['obs'].shape[0]} sequences; |logp(old logits) - stored logp| {e_logp:.3e}; "
              f"first minibatch |ratio - 1| {e_ratio:.3e}, mean KL {st0[3].item():.3e}")
        assert e_logp <= TOL and e_ratio <= TOL and abs(st0[3].item()) <= TOL
        params = {k: v.clone() for k, v in learner.module.state_dict().items()}
        stats = learner.update(ro.episodes, net)
        assert stats["steps"] == 2 * len(LR.minibatch_partition(seq_len, learner.sgd_minibatch_size)) and stats["rows"] == int(m.sum())
        assert all(np.isfinite(stats[k]) for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy"))
        after = learner.module.state_dict()
        assert all(not torch.equal(after[k], params[k]) for k in params), [k for k in params if torch.equal(after[k], params[k])]
        assert all(torch.isfinite(v).all() for v in after.values())
        rows = ro.episodes.rows()
        assert all(torch.equal(rows[k], before[k]) for k in before), "update changed the batch"
        learner.publish(net)
        # the sampler with the published weights against the module's length-1 forward
        obs = seqs["obs"][:, 0].contiguous()                                # [S, 3, 34], each sequence's first step
        S = obs.shape[0]
        h_in = seqs["state_in"].clone().contiguous()
        logits = torch.zeros((S, 3, 4), dtype=torch.float32, device="cuda")
        big = net if 3 * S <= net.max_rows else None
        if big is None:
            obs, h_in, logits, S = obs[:net.max_rows // 3], h_in[:net.max_rows // 3], logits[:net.max_rows // 3], net.max_rows // 3
        net.sample(obs.contiguous(), h_in.contiguous(), torch.empty_like(h_in), greedy=True, logits=logits)
        one = torch.ones((S,), dtype=torch.int32, device="cuda")
        zeros = torch.zeros((S, 1, 3), dtype=torch.int8, device="cuda")
        from hhmarl_2d_amd.rollout import central_critic_rows_hl
        for a in range(3):
            with torch.no_grad():
                lg, _ = learner.module(obs[:, None, a], central_critic_rows_hl(obs[:, None], zeros, a + 1), h_in[:, a], one, fused_gru=fused)
            e = (lg[:, 0] - logits[:, a, :3]).abs().max().item()
            assert e <= TOL, f"round {rnd}, agent {a}: sampler against module after publish {e:.3e}"
        out.append(stats)
        # the captured collect keeps replaying, with the new weights
        ro.start()
        ro.collect()
        assert ro._graph is graph, "publish made the rollout capture again"
    return out


@pytest.mark.parametrize("fused", (True, False))
def test_three_rounds_of_collect_update_publish(fused):
    stats = _rounds(fused)
    assert len(stats) == 3 and all(s["steps"] > 0 for s in stats)


def test_fused_and_unfused_learners_agree_from_the_same_start():
    ro, net, fu = _setup(True)
    _, _, un = _setup(False)
    ro.start()
    for _ in range(6):
        ro.collect()
    a, b = fu.update(ro.episodes, net), un.update(ro.episodes, net)
    print(f"fused {a}\nunfused {b}")
    assert a["steps"] == b["steps"] > 0 and a["rows"] == b["rows"]
    for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy"):
        assert abs(a[k] - b[k]) <= 1e-4 * max(abs(b[k]), 1e-30), (k, a[k], b[k])


def test_more_passes_raise_the_clipped_surrogate():
    ro, net, learner = _setup(True, num_sgd_iter=8)
    ro.start()
    for _ in range(6):
        ro.collect()
    with torch.no_grad():
        b = learner.policy_batch(ro.episodes.sequences())
    s_before = _surrogate(learner, b)
    stats = learner.update(ro.episodes, net)
    s_after = _surrogate(learner, b)
    print(f"clipped surrogate over the batch: {s_before:.6f} before, {s_after:.6f} after {stats['steps']} steps")
    assert stats["steps"] > 0 and s_after > s_before
