"""PPOLearner on the MI355X: collect -> update -> publish rounds on a small world, fight and escape — the published bank equals the
modules' length-1 forward, the recomputed old logits reproduce the batch's logp, the shared layer stays one tensor, the batch is not
touched — and, in escape mode (where the training and the sampling forward coincide), the first minibatch has ratio 1 and zero KL and
one update raises the clipped surrogate objective."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BOUND = 1e-5     # the policy kernels' documented bound on logits against the float32 PyTorch forward (include/hh_policy.h)


def _setup(mode, N=256, T=32, horizon=30, seed=23, **kw):
    from hhmarl_2d_amd.learner import PPOLearner
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    dev = torch.device("cuda", 0)
    w = World(make_config(n_arenas=N, level=3, seed=seed, auto_reset=True, horizon=horizon, agent_mode=1 if mode == "escape" else 0), device=0)
    bank = PolicyBank.trainable_init(dev, mode=mode, seed=5, max_rows=2 * N)
    ro = PPORollout(w, bank, T, batch_mode="complete_episodes")
    learner = PPOLearner.trainable_init(dev, mode=mode, seed=5, **kw)
    return ro, bank, learner


def _snapshot(episodes):
    return {k: v.clone() for k, v in episodes.rows().items()}


def _multicategorical_logp(logits, actions, n_comp):
    from hhmarl_2d_amd import policy_nets as PN
    lo, out = 0, 0.0
    for i, w in enumerate(PN.ACTION_SPLIT[:n_comp]):
        out = out + torch.log_softmax(logits[:, lo:lo + w].double(), dim=1).gather(1, actions[:, i:i + 1].long()).squeeze(1)
        lo += w
    return out


@pytest.mark.parametrize("mode", ["fight", "escape"])
@pytest.mark.parametrize("fused", [True, False])
def test_collect_update_publish_rounds(mode, fused):
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    from hhmarl_2d_amd.rollout import central_critic_rows
    ro, bank, learner = _setup(mode, num_sgd_iter=2, sgd_minibatch_size=256, fused=fused)
    shared = learner.modules[0].shared_layer._model[0].weight
    for rnd in range(3):
        ro.collect()
        before = _snapshot(ro.episodes)
        rows = ro.episodes.rows()
        R = rows["obs"].shape[0]
        assert R > 1000
        # the old logits the learner recomputes from the bank give back the batch's logp at the stored actions
        old = learner.old_logits(rows["obs"], bank, ro.episodes.N)
        for a, kind in enumerate(learner.kinds):
            lp = _multicategorical_logp(old[:, a], rows["actions"][:, a], LR.n_comp_of(kind))
            assert (lp - rows["logp"][:, a].double()).abs().max().item() <= BOUND
        params = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in learner.modules]
        stats = learner.update(ro.episodes, bank)
        assert len(stats) == 2
        for a, st in enumerate(stats):
            assert all(np.isfinite(st[k]) for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "kl_coeff")), st
            assert st["rows"] == R and st["steps"] >= 2 and st["steps"] % 2 == 0 and st["kl"] >= -1e-6 and st["entropy"] > 0
            assert st["kl_coeff"] == learner.kl_coeff[a]
            changed = [k for k, v in learner.modules[a].state_dict().items() if not torch.equal(v, params[a][k])]
            assert len(changed) == len(params[a]), "every tensor of the policy is trained"
        # the batch is the rollout's: byte-identical whether or not a learner read it
        after = _snapshot(ro.episodes)
        assert set(before) == set(after) and all(torch.equal(before[k].view(torch.uint8), after[k].view(torch.uint8)) for k in before)
        learner.publish(bank)
        # RLlib samples every episode under ONE weight version (complete_episodes, weights synced between sample() calls).  A carried
        # episode head was sampled before this publish: its stored logp is the old policy's, which the bank no longer holds.  Fresh
        # episodes after every publish keep the batch strictly on-policy, which is what the old_logits / logp check above states.
        ro.start()
        # one shared layer: still one parameter object; both bank slots carry it (each slot reproduces its module, which holds it)
        assert learner.modules[1].shared_layer._model[0].weight is shared
        probe = rows["obs"][:ro.episodes.N].contiguous()      # the rollout's own call shape: its row lists stay valid
        sel = torch.tensor(learner._sel, dtype=torch.uint8, device=probe.device).repeat(probe.shape[0], 1).contiguous()
        logits = torch.zeros((probe.shape[0], 2, 32), device=probe.device)
        act = torch.zeros((probe.shape[0], 2, 4), dtype=torch.int8, device=probe.device)
        _, _, vf = bank.sample(probe, sel, greedy=True, actions=act, logits=logits)
        for a, kind in enumerate(learner.kinds):
            with torch.no_grad():
                crit0 = central_critic_rows(probe, torch.zeros_like(act), a + 1)      # the sampler's critic sees zero action inputs
                want_l, want_v = learner.modules[a](probe[:, a, :PN.OBS_DIM[kind]].contiguous()[:, None] if PN.HAS_ATT[kind] else probe[:, a, :PN.OBS_DIM[kind]],
                                                    crit0[:, None] if PN.HAS_ATT[kind] else crit0)
            want_l, want_v = want_l.reshape(probe.shape[0], -1), want_v.reshape(-1)
            assert (logits[:, a, :PN.N_OUT[kind]] - want_l).abs().max().item() <= BOUND
            print(f"round {rnd} policy {a}: value difference bank / module {(vf[:, a] - want_v).abs().max().item():.3e}")
    assert learner.updates == 3


def test_same_seed_same_weights_other_seed_other_order():
    """two learners with the same seed on the same batch end with the same minibatch order (the keyed permutation), another seed with
    another; the weights of equal-order runs agree to float32 round-off of the GEMMs' atomics-free kernels"""
    from hhmarl_2d_amd import learner as LR
    assert not np.array_equal(LR.minibatch_order(50, 0, 0, 0, 0), LR.minibatch_order(50, 1, 0, 0, 0))
    ro, bank, l1 = _setup("escape", num_sgd_iter=1)
    _, _, l2 = _setup("escape", num_sgd_iter=1)
    ro.collect()
    s1, s2 = l1.update(ro.episodes, bank), l2.update(ro.episodes, bank)
    for a in range(2):
        assert s1[a]["steps"] == s2[a]["steps"] and abs(s1[a]["total_loss"] - s2[a]["total_loss"]) <= 1e-4 * max(1.0, abs(s1[a]["total_loss"]))


def _surrogate_objective(learner, batch, agent, clip):
    """mean over the whole batch of min(adv ratio, adv clamp(ratio)) with the module's current weights (float64 accumulate)"""
    from hhmarl_2d_amd import learner as LR
    with torch.no_grad():
        logits, _ = learner.modules[agent](batch["obs"], batch["critic"])
        lp = _multicategorical_logp(logits, batch["actions"], LR.n_comp_of(learner.kinds[agent]))
        ratio = torch.exp(lp - batch["old_logp"].double())
        adv = batch["adv"].double()
        return torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean().item(), ratio


def test_escape_first_minibatch_is_on_policy_and_an_update_improves_the_surrogate():
    ro, bank, learner = _setup("escape", num_sgd_iter=4, sgd_minibatch_size=512)
    ro.collect()
    rows = ro.episodes.rows()
    old = learner.old_logits(rows["obs"], bank, ro.episodes.N)
    batches = [learner.policy_batch(rows, old, a) for a in range(2)]
    for a in range(2):
        mb = {k: v[:512] for k, v in batches[a].items()}
        with torch.no_grad():
            logits, vf = learner.modules[a](mb["obs"], mb["critic"])
        _, stats = learner.loss(a, logits, vf, mb)
        obj0, ratio = _surrogate_objective(learner, batches[a], a, learner.clip_param)
        # the learner's forward is the sampler's: ratio 1 and KL 0 within the kernels' bound on the logits (4 components x 1e-5 in logp)
        assert (ratio - 1.0).abs().max().item() <= 4 * BOUND
        assert abs(stats[3].item()) <= BOUND
        assert abs(stats[1].item() + batches[a]["adv"][:512].double().mean().item()) <= 1e-4     # -mean(adv x 1)
    before = [_surrogate_objective(learner, batches[a], a, learner.clip_param)[0] for a in range(2)]
    learner.update(ro.episodes, bank)
    after = [_surrogate_objective(learner, batches[a], a, learner.clip_param)[0] for a in range(2)]
    print("clipped surrogate objective before / after one update:", before, after)
    assert all(x1 > x0 for x0, x1 in zip(before, after))
