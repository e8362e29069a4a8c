"""From one level of the curriculum to the next on the MI355X (INTEGRATION.md "From one level to the next"): a level-3 run is saved and
exported; fresh level-4 objects, their opponents loaded from the exported files by name, take the learner over with
checkpoint.load_subset — weights, Adam state, step counts, KL coefficients and update count bit for bit —, publish it to the level-4
sampler and train on.  64 arenas, windows of 8 ticks, horizon 40, one pass of minibatches of 128 rows, the device-side Adam."""
import math

import pytest
import torch

from lowlevel_eval_ref import actor_weights
from resume_harness import _host, same

pytestmark = pytest.mark.gpu

N, T, HORIZON = 64, 8, 40
LEARN = dict(num_sgd_iter=1, sgd_minibatch_size=128, optimizer="fused")
WINDOW = ("obs", "actions", "reward", "done", "adv")


def _dev():
    return torch.device("cuda", 0)


def _level(level, opponents=None):
    """world, sampler bank, rollout and learner of one level, from the same learner options at every level; opponents: the bank the
    level's frozen opponents fly (levels 4-5)"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.config import make_args
    from hhmarl_2d_amd.env_hetero import config_from_args
    from hhmarl_2d_amd.pilots import OpponentNets, PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World
    w = World(config_from_args(make_args(0, level=level, horizon=HORIZON), L.ENV_LOWLEVEL, N, 23, auto_reset=True), device=0)
    bank = PolicyBank.trainable_init(_dev(), mode="fight", seed=5, max_rows=2 * N)
    opp = OpponentNets(w, bank=opponents, bind=True, skip_first=False) if opponents is not None else None
    ro = PPORollout(w, bank, T, opponents=opp, record_logits=True)
    learner = LR.PPOLearner.trainable_init(_dev(), mode="fight", seed=5, **LEARN)
    return dict(world=w, bank=bank, rollout=ro, learner=learner, _keep=opp)


def _packed(bank):
    torch.cuda.synchronize()
    return [bank.packed(slot, part).cpu() for slot in (0, 1) for part in range(5)]


def _window(ro):
    torch.cuda.synchronize()
    return {k: _host(getattr(ro, k)) for k in WINDOW}


def _finite(stats):
    assert len(stats) == 2
    for s in stats:
        assert s["steps"] >= 1 and s["rows"] == T * N
        for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "kl_coeff"):
            assert math.isfinite(s[k]), (k, s[k])


def test_level_3_hands_its_learner_to_level_4(tmp_path):
    from hhmarl_2d_amd import checkpoint
    from hhmarl_2d_amd import pilots as P
    from hhmarl_2d_amd.config import make_args
    path, pdir = str(tmp_path / "L3.ckpt"), str(tmp_path / "policies")
    # ---- level 3: one iteration, then the checkpoint and the policy files
    l3 = _level(3)
    l3["rollout"].collect()
    _finite(l3["learner"].update_window(l3["rollout"], l3["bank"]))
    l3["learner"].publish(l3["bank"])
    objs3 = {k: v for k, v in l3.items() if not k.startswith("_")}
    checkpoint.save(path, **objs3)
    assert checkpoint.contents(path) == {"world": "World", "bank": "PolicyBank", "rollout": "PPORollout", "learner": "PPOLearner"}
    l3["learner"].export_policies(pdir, 3)
    saved_learner, saved_packed = _host(l3["learner"].state_dict()), _packed(l3["bank"])
    assert saved_learner["updates"] == 1 and all(int(p["adam"]["t"]) >= 1 for p in saved_learner["policies"])
    # ---- level 4: fresh objects, the opponents from the exported files by name
    args4 = make_args(0, level=4, horizon=HORIZON)
    l4 = _level(4, P.PolicyBank.from_reference_dir(_dev(), pdir, "LowLevel", args4, max_rows=2 * N))
    objs4 = {k: v for k, v in l4.items() if not k.startswith("_")}
    fresh = _host(l4["learner"].state_dict())
    assert same(fresh["modules"], saved_learner["modules"]) is not None and fresh["updates"] == 0
    # the whole file does not fit a level-4 run, and `load` takes no part of it
    with pytest.raises(ValueError, match="the file holds"):
        checkpoint.load(path, learner=l4["learner"])
    assert same(_host(l4["learner"].state_dict()), fresh) is None
    checkpoint.load_subset(path, learner=l4["learner"])
    got = _host(l4["learner"].state_dict())
    assert same(got, saved_learner) is None, same(got, saved_learner)
    assert l4["learner"].updates == 1 and l4["learner"].kl_coeff == l3["learner"].kl_coeff
    assert l4["learner"].modules[0].shared_layer is l4["learner"].modules[1].shared_layer
    # publish: the level-4 sampler holds the bytes the level-3 sampler held at the save (actor and value branch)
    assert any(not torch.equal(a, b) for a, b in zip(_packed(l4["bank"]), saved_packed))
    l4["learner"].publish(l4["bank"])
    for i, (a, b) in enumerate(zip(_packed(l4["bank"]), saved_packed)):
        assert torch.equal(a, b), f"slot {i // 5} part {i % 5}"
    # ---- a second level-4 run whose opponents come from a bank built by hand from the level-3 modules, with the same selector table
    hand = P.PolicyBank(_dev(), 2 * N)
    for slot, (kind, sd) in enumerate(actor_weights(l3["learner"])):
        hand.set_net(slot, kind, sd)
    hand.set_lut({P.SEL_FIGHT1: 0, P.SEL_FIGHT2: 1})
    l4b = _level(4, hand)
    checkpoint.load_subset(path, learner=l4b["learner"])
    l4b["learner"].publish(l4b["bank"])
    for run in (l4, l4b):
        run["rollout"].start()
        run["rollout"].collect()
    wa, wb = _window(l4["rollout"]), _window(l4b["rollout"])
    assert same(wa, wb) is None, same(wa, wb)
    assert bool(wa["done"].any()) or HORIZON > T              # (windows of 8 ticks: episodes of 40 need not end in the first)
    assert float(wa["obs"].abs().sum()) > 0 and len(torch.unique(wa["actions"].reshape(-1, 4), dim=0)) > 4
    # ---- and the level-4 run trains on
    stats = l4["learner"].update_window(l4["rollout"], l4["bank"])
    _finite(stats)
    assert l4["learner"].updates == 2
    after = _host(l4["learner"].state_dict())
    assert same(after["modules"], saved_learner["modules"]) is not None
    assert all(int(p["adam"]["t"]) > int(q["adam"]["t"]) for p, q in zip(after["policies"], saved_learner["policies"]))
    l4["learner"].publish(l4["bank"])
    l4["rollout"].collect()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(l4["rollout"].adv).all())


def test_load_subset_refuses_what_the_learner_refuses(tmp_path):
    """the learner's own validation runs before anything is touched: other learner options than the saved run's"""
    from hhmarl_2d_amd import checkpoint
    from hhmarl_2d_amd import learner as LR
    path = str(tmp_path / "L3.ckpt")
    src = LR.PPOLearner.trainable_init(_dev(), mode="fight", seed=5, **LEARN)
    checkpoint.save(path, learner=src, twin=LR.PPOLearner.trainable_init(_dev(), mode="fight", seed=6, **LEARN))
    other = LR.PPOLearner.trainable_init(_dev(), mode="fight", seed=5, **dict(LEARN, sgd_minibatch_size=64))
    before = _host(other.state_dict())
    with pytest.raises(ValueError, match="`sgd_minibatch_size` was 128 when saved, the live object has 64"):
        checkpoint.load_subset(path, learner=other)
    esc = LR.PPOLearner.trainable_init(_dev(), mode="escape", seed=5, **LEARN)
    with pytest.raises(ValueError, match="`kinds`"):
        checkpoint.load_subset(path, learner=esc)
    with pytest.raises(ValueError, match=r"not \['bank'\]"):
        checkpoint.load_subset(path, learner=other, bank=other)
    assert same(_host(other.state_dict()), before) is None
