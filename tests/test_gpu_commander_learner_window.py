"""CommanderLearner.window_sequences / update_window on the MI355X: a CommanderRollout in its default batch_mode ("truncate_episodes"),
set up the way tests/test_gpu_commander_learner.py sets its rollouts up, whose second window opens mid-episode — so sequences that start
at t = 0 carry the GRU state of the collect before.  window_sequences equals the reference (tests/window_batch_ref.py) byte for byte, and
update_window equals the driver run on the reference's policy batch."""
import numpy as np
import pytest
import torch

import window_batch_ref as WR

pytestmark = pytest.mark.gpu
T = 16


def _learner(L, **kw):
    from hhmarl_2d_amd import learner as LR
    return LR.CommanderLearner.trainable_init(torch.device("cuda", 0), seed=6, num_sgd_iter=2, max_seq_len=L, **kw)


def _setup(N, record_logits=False):
    from hhmarl_2d_amd import _lib as L_
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, env_kind=L_.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True, horizon=150), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    ro = CommanderRollout(w, net, VariantNetPilot(w, seed=8), T, max_seq_len=7, record_logits=record_logits)     # its own max_seq_len is not read
    assert ro.batch_mode == "truncate_episodes" and ro.episodes is None
    return ro, net


@pytest.mark.parametrize("N,L,record_logits", [(64, 20, False), (16, 4, True)])
def test_window_sequences_and_update_window(N, L, record_logits):
    ro, net = _setup(N, record_logits)
    l1, l2 = _learner(L), _learner(L)
    with pytest.raises(RuntimeError, match="has not collected yet"):
        l1.update_window(ro)
    ro.collect()
    ro.collect()
    torch.cuda.synchronize()
    with torch.no_grad():
        got = l1.window_sequences(ro)
    want = WR.window_sequences_ref(ro, L)
    opened = want["seq_lens"].new_tensor(WR.window_cut_ref(ro.done, L)[0]) == 0
    assert want["state_in"][opened].abs().sum(dim=(1, 2, 3)).gt(0).any().item(), "a sequence that starts at t = 0 carries a state from the collect before"
    assert (~want["state_in"].abs().sum(dim=(1, 2, 3)).gt(0)).any().item(), "a sequence at an episode start has zero state"
    assert set(got) == set(want) and ("logits" in got) == record_logits
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].contiguous().view(torch.uint8), want[k].contiguous().view(torch.uint8)), f"N {N} L {L}: {k}"
    S = got["obs"].shape[0]
    assert got["obs"].shape == (S, L, 3, 34) and got["state_in"].shape == (S, 3, 2, 200) and int(got["seq_lens"].sum()) == T * N
    print(f"N {N} L {L}: {S} sequences over {T * N} rows")

    names = ("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target", "state_in") + (("logits",) if record_logits else ())
    before = {k: getattr(ro, k).clone() for k in names}
    params = {k: v.detach().clone() for k, v in l1.module.state_dict().items()}
    st = l1.update_window(ro)
    with torch.no_grad():
        b = l2.policy_batch(want)
        b["old_logits"] = l2.batch_old_logits(want, b)
    rf = l2._sgd.run(*l2._columns(b))
    print(f"update_window {st}\nthe driver on the reference batch {rf}")
    assert l1.updates == 1 and st["rows"] == 3 * T * N == rf["rows"] and st["steps"] == rf["steps"] >= 2
    assert all(np.isfinite(st[k]) for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "kl_coeff")), st
    assert abs(st["total_loss"] - rf["total_loss"]) <= 1e-4 * max(1.0, abs(rf["total_loss"]))
    changed = [k for k, v in l1.module.state_dict().items() if not torch.equal(v, params[k])]
    assert len(changed) == len(params), "every tensor of the policy is trained"
    assert all(torch.equal(before[k].view(torch.uint8), getattr(ro, k).view(torch.uint8)) for k in names), "the window is only read"
    l1.publish(net)
    ro.collect()                      # no start(): the next window is sampled by the published weights
    torch.cuda.synchronize()
    assert ro.collects == 3 and np.isfinite(l1.update_window(ro)["total_loss"])


def test_update_window_replays_the_captured_step():
    """optimizer="fused", step="graph" next to fused eager on one window, compared the way tests/test_gpu_learner_driver.py compares the
    step modes: the same steps and rows, each step's unpadded rows update_schedule's column 2"""
    from hhmarl_2d_amd import learner as LR
    ro, net = _setup(32)
    kw = dict(kl_coeff=0.0, optimizer="fused", sgd_minibatch_size=128)
    eager, graph = _learner(20, step="eager", **kw), _learner(20, step="graph", **kw)
    ro.collect()
    ro.collect()
    with torch.no_grad():
        seq_len = eager.policy_batch(eager.window_sequences(ro))["seq_len"].cpu().numpy()
    st_e, st_g = eager.update_window(ro), graph.update_window(ro)
    torch.cuda.synchronize()
    _, sched, _ = LR.update_schedule(seq_len, 128, 2, eager.seed, 0, 0, False)
    steps = len(sched)
    print(f"eager {st_e}\ngraph {st_g}")
    assert st_e["steps"] == st_g["steps"] == steps >= 6 and st_e["rows"] == st_g["rows"] == 3 * T * 32
    for what, ln in (("eager", eager), ("graph", graph)):
        assert ln._sgd.book.table[:steps, 5].tolist() == sched[:, 2].tolist(), f"{what} visited update_schedule's rows in its order"
    assert graph._sgd.book.captures == 1 and np.isfinite(st_g["total_loss"])
