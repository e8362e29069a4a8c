"""The commander's learner without a GPU (hhmarl_2d_amd.learner: CommanderTrainable, gru_sequence_torch, ppo_loss_categorical_torch,
CommanderLearner.policy_batch): the module against tests/commander_ref.forward in float64, padding, the loss against a float64
restatement of include/hh_learner.h's formulas, the batch builder on a synthetic sequences() dict, and the library's new symbols."""
import ctypes as C
import os
import re

import numpy as np
import torch

import commander_ref as REF
from hhmarl_2d_amd import commander as CM
from hhmarl_2d_amd import learner as LR
from hhmarl_2d_amd.rollout import central_critic_rows_hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(seed=3):
    return LR.CommanderTrainable().load_numpy(CM.random_weights(seed)).double()


def _inputs(S, Lm, seed, ragged=True):
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((S, Lm, 3, 34), generator=g).double()      # float32 values: central_critic_rows_hl's rows are float32
    actions = torch.randint(0, 3, (S, Lm, 3), generator=g).to(torch.int8)
    state = 0.5 * torch.randn((S, 2, 200), generator=g, dtype=torch.float64)
    seq_len = torch.randint(1, Lm + 1, (S,), generator=g) if ragged else torch.full((S,), Lm)
    seq_len[0] = Lm
    return obs, actions, state, seq_len.to(torch.int32)


def _ref_step(sd, obs_t, act_t, h_act, h_val):
    """commander_ref.forward on agent 1's rows of obs_t [S, 3, 34] with the actions filled in as central_critic_rows_hl does"""
    a = [act_t[:, k:k + 1].double() / 2.0 for k in range(3)]
    return REF.forward(sd, obs_t[:, 0], obs_t[:, 1], obs_t[:, 2], a[0], a[1], a[2], h_act, h_val)


def test_state_dict_has_the_commanders_keys_and_one_shared_layer():
    m = LR.CommanderTrainable()
    sd = m.state_dict()
    keys = CM.state_keys()
    assert list(sd.keys()) == list(keys.keys())
    assert all(tuple(sd[k].shape) == tuple(shp) for k, shp in keys.items())
    names = [n for n, _ in m.named_parameters()]
    assert len(names) == len(keys) and names.count("shared_layer._model.0.weight") == 1
    assert sum(p.numel() for p in m.parameters()) == sum(int(np.prod(s)) for s in keys.values())
    # load_numpy round trip
    w = CM.random_weights(5)
    m.load_numpy(w)
    assert all(np.array_equal(m.state_dict()[k].numpy(), w[k]) for k in keys)


def test_length_one_sequences_equal_the_reference_forward():
    m, sd = _module(), REF.to_torch(CM.random_weights(3))
    obs, actions, state, _ = _inputs(37, 1, 0)
    crit = central_critic_rows_hl(obs, actions, 1).double()
    one = torch.ones((37,), dtype=torch.int32)
    logits, value, ha, hv = m(obs[:, :, 0], crit, state, one, fused_gru=False, return_states=True)
    wl, wv, wha, whv = _ref_step(sd, obs[:, 0], actions[:, 0], state[:, 0], state[:, 1])
    for got, want in ((logits[:, 0], wl), (value[:, 0], wv), (ha, wha), (hv, whv)):
        assert (got - want).abs().max().item() <= 1e-12


def test_padded_ragged_batch_equals_the_reference_stepped_with_chained_states():
    m, sd = _module(), REF.to_torch(CM.random_weights(3))
    S, Lm = 23, 7
    obs, actions, state, seq_len = _inputs(S, Lm, 1)
    mask = LR.chunk_mask(seq_len, Lm)
    obs, actions = obs * mask[..., None, None], actions * mask[..., None].to(torch.int8)
    crit = central_critic_rows_hl(obs, actions, 1).double()
    logits, value, ha, hv = m(obs[:, :, 0], crit, state, seq_len, fused_gru=False, return_states=True)
    h_act, h_val = state[:, 0], state[:, 1]
    checked = 0
    for t in range(Lm):
        wl, wv, h_act, h_val = _ref_step(sd, obs[:, t], actions[:, t], h_act, h_val)
        on = mask[:, t]
        assert (logits[:, t][on] - wl[on]).abs().max().item() <= 1e-12 and (value[:, t][on] - wv[on]).abs().max().item() <= 1e-12
        last = seq_len == t + 1
        if last.any():
            assert (ha[last] - h_act[last]).abs().max().item() <= 1e-12 and (hv[last] - h_val[last]).abs().max().item() <= 1e-12
        checked += int(on.sum())
    assert checked == int(seq_len.sum()) and checked < S * Lm


def test_padded_rows_reach_no_unpadded_output_and_no_parameter_gradient():
    S, Lm = 11, 6
    obs, actions, state, seq_len = _inputs(S, Lm, 2)
    mask = LR.chunk_mask(seq_len, Lm)
    assert not mask.all()
    g = torch.Generator().manual_seed(9)
    obs2 = torch.where(mask[..., None, None], obs, torch.rand(obs.shape, generator=g).double() * 5.0)
    act2 = torch.where(mask[..., None], actions, torch.randint(0, 3, actions.shape, generator=g).to(torch.int8))
    wts = torch.randn((S, Lm, 4), generator=g, dtype=torch.float64)

    def run(o, a):
        m = _module()
        logits, value = m(o[:, :, 0], central_critic_rows_hl(o, a, 1).double(), state, seq_len, fused_gru=False)
        loss = ((logits * wts[..., :3]).sum(-1) + value * wts[..., 3])[mask].sum()
        loss.backward()
        return logits, value, {k: p.grad.clone() for k, p in m.named_parameters()}

    l1, v1, g1 = run(obs, actions)
    l2, v2, g2 = run(obs2, act2)
    assert torch.equal(l1[mask], l2[mask]) and torch.equal(v1[mask], v2[mask])
    assert not torch.equal(l1[~mask], l2[~mask])
    assert all(torch.equal(g1[k], g2[k]) for k in g1) and all(g1[k].abs().max() > 0 for k in g1)


def loss_restatement(logits, vf, old_logits, actions, old_logp, adv, target, mask, clip, vf_clip, vf_coeff, ent_coeff, kl_coeff):
    """include/hh_learner.h's formulas for one Categorical over 3 logits, float64 numpy, row by row -> (total, policy, vf, kl, entropy, n)"""
    tot = np.zeros(4)
    n = 0
    for i in range(len(vf)):
        if mask is not None and not mask[i]:
            continue
        n += 1
        lp = logits[i, :3] - logits[i, :3].max()
        lp = lp - np.log(np.exp(lp).sum())
        lq = old_logits[i, :3] - old_logits[i, :3].max()
        lq = lq - np.log(np.exp(lq).sum())
        ratio = np.exp(lp[actions[i]] - old_logp[i])
        surr = min(adv[i] * ratio, adv[i] * min(max(ratio, 1 - clip), 1 + clip))
        tot += (-surr, min(max((vf[i] - target[i]) ** 2, 0.0), vf_clip), (np.exp(lq) * (lq - lp)).sum(), -(np.exp(lp) * lp).sum())
    total = (tot[0] + vf_coeff * tot[1] - ent_coeff * tot[3]) / n
    kl = tot[2] / n if kl_coeff > 0 else 0.0
    return np.array([total + kl_coeff * kl, tot[0] / n, tot[1] / n, kl, tot[3] / n, n])


def cat_inputs(R, masked, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((R, 4), generator=g, dtype=torch.float64)
    old = torch.zeros((R, 4), dtype=torch.float64)
    old[:, :3] = logits[:, :3] + 0.3 * torch.randn((R, 3), generator=g, dtype=torch.float64)
    actions = torch.randint(0, 3, (R,), generator=g).to(torch.int8)
    old_logp = torch.log_softmax(old[:, :3], dim=1).gather(1, actions.long()[:, None])[:, 0]
    b = {"old_logits": old.float(), "actions": actions, "old_logp": old_logp.float(), "adv": torch.randn((R,), generator=g),
         "target": 2.0 * torch.randn((R,), generator=g)}
    if masked:
        b["mask"] = torch.rand((R,), generator=g) < 0.8
        b["mask"][0] = True
    return logits.float(), (3.0 * torch.randn((R,), generator=g)).float(), b


def test_torch_categorical_loss_equals_the_float64_restatement():
    for masked, klc, ec in ((False, 0.2, 0.0), (True, 0.2, 0.01), (True, 0.0, 0.01)):
        logits, vf, b = cat_inputs(301, masked, 4)
        kw = dict(clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=0.7, entropy_coeff=ec, kl_coeff=klc)
        l64 = logits.double().requires_grad_(True)
        total, stats = LR.ppo_loss_categorical_torch(l64, vf.double(), b, **kw)
        np64 = lambda t: t.double().numpy()
        want = loss_restatement(np64(logits), np64(vf), np64(b["old_logits"]), b["actions"].long().numpy(), np64(b["old_logp"]), np64(b["adv"]),
                                np64(b["target"]), b["mask"].numpy() if masked else None, 0.25, 10.0, 0.7, ec, klc)
        assert np.abs(stats.numpy() - want).max() <= 1e-12 and abs(total.item() - want[0]) <= 1e-12
        total.backward()
        assert torch.equal(l64.grad[:, 3], torch.zeros(301, dtype=torch.float64))
        if masked:
            assert torch.equal(l64.grad[~b["mask"]], torch.zeros((int((~b["mask"]).sum()), 4), dtype=torch.float64))
        # three-column logits give the same loss
        total3, _ = LR.ppo_loss_categorical_torch(logits.double()[:, :3], vf.double(), b, **kw)
        assert total3.item() == total.item()


def test_policy_batch_on_a_synthetic_sequences_dict():
    S, Lm = 9, 5
    g = torch.Generator().manual_seed(6)
    seq_len = torch.randint(1, Lm + 1, (S,), generator=g).to(torch.int32)
    mask = LR.chunk_mask(seq_len, Lm)
    z3 = lambda t: t * mask[..., None].to(t.dtype)
    seqs = {"obs": torch.rand((S, Lm, 3, 34), generator=g) * mask[..., None, None], "actions": z3(torch.randint(0, 3, (S, Lm, 3), generator=g).to(torch.int8)),
            "logp": z3(-torch.rand((S, Lm, 3), generator=g)), "vf": z3(torch.randn((S, Lm, 3), generator=g)),
            "adv": z3(torch.randn((S, Lm, 3), generator=g) * 3 + 1), "target": z3(torch.randn((S, Lm, 3), generator=g)),
            "seq_lens": seq_len, "mask": mask, "state_in": torch.randn((S, 3, 2, 200), generator=g)}
    before = {k: v.clone() for k, v in seqs.items()}
    b = LR.CommanderLearner.policy_batch(seqs)
    assert all(torch.equal(seqs[k], before[k]) for k in seqs)
    assert b["obs"].shape == (3 * S, Lm, 34) and b["critic"].shape == (3 * S, Lm, 105) and b["state_in"].shape == (3 * S, 2, 200)
    assert b["seq_len"].dtype == torch.int32 and b["actions"].dtype == torch.int8 and b["mask"].dtype == torch.uint8
    seen = set()
    for a in range(3):
        for s in range(S):
            i = a * S + s                                  # agent-major
            seen.add((s, a))
            assert torch.equal(b["obs"][i], seqs["obs"][s, :, a]) and torch.equal(b["actions"][i], seqs["actions"][s, :, a])
            assert torch.equal(b["critic"][i], central_critic_rows_hl(seqs["obs"][s], seqs["actions"][s], a + 1))
            assert torch.equal(b["state_in"][i], seqs["state_in"][s, a]) and torch.equal(b["mask"][i].bool(), mask[s])
            assert b["seq_len"][i] == seq_len[s]
            assert torch.equal(b["old_logp"][i], seqs["logp"][s, :, a]) and torch.equal(b["target"][i], seqs["target"][s, :, a])
    assert len(seen) == 3 * S == b["obs"].shape[0]
    # advantages: standardised over every unpadded row of the three agents, zero in the padding
    raw = torch.cat([seqs["adv"][:, :, a] for a in range(3)], dim=0)
    m3 = b["mask"].bool()
    want = LR.standardize(raw[m3].double())
    assert (b["adv"][m3].double() - want).abs().max().item() <= 1e-5 and torch.equal(b["adv"][~m3], torch.zeros(int((~m3).sum())))


def test_learner_defaults_are_train_hiers():
    import inspect
    d = {k: v.default for k, v in inspect.signature(LR.CommanderLearner.__init__).parameters.items()}
    assert (d["lr"], d["clip_param"], d["kl_target"], d["sgd_minibatch_size"]) == (1e-4, 0.25, 0.05, 256)
    assert (d["kl_coeff"], d["vf_clip_param"], d["num_sgd_iter"], d["max_seq_len"], d["fused"]) == (0.2, 10.0, 30, 20, True)
    for name in ("trainable_init", "policy_batch", "loss", "minibatch_step", "update", "publish"):
        assert callable(getattr(LR.CommanderLearner, name))


def test_library_exports_the_learners_symbols_and_the_struct_matches_the_header():
    from hhmarl_2d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "hh_learner.h")).read()
    declared = set(re.findall(r"^int (hh_[a-z_]+)\s*\(", txt, re.M))
    assert declared == set(_lib.LEARNER_EXPORTS)
    assert {"hh_ppo_loss_categorical", "hh_gru_seq_scratch_bytes", "hh_gru_seq_forward", "hh_gru_seq_backward"} <= declared
    for s in declared:
        assert hasattr(lib, s), f"libhh_world.so does not export {s}"
    body = re.search(r"typedef struct hh_gru_seq_io \{(.*?)\} hh_gru_seq_io;", txt, re.S).group(1)
    names = re.findall(r"^\s*(?:const )?float \*([a-z_0-9]+);", body, re.M)
    assert names == [f[0] for f in _lib.HHGruSeqIO._fields_] and C.sizeof(_lib.HHGruSeqIO) == 8 * len(names)
