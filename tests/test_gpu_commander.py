"""The trainable commander on the MI355X: hh_commander_sample (the fused CommanderGru sampler kernel) against the golden vectors recorded
from the reference's own class and against the float64 PyTorch restatement, the world-keyed draws, and CommanderRollout (one HIP graph per
collect) against a step-by-step eager replay."""
import json
import os

import numpy as np
import pytest
import torch

import commander_ref as CR
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN, "commander_gru.npz"))
META = json.loads(str(G["meta"]))
TOL = 1e-5


def _net(seed=META["seed"], max_rows=3 * 8192):
    from hhmarl_2d_amd.commander import CommanderNet, random_weights
    return CommanderNet(0, max_rows).set_weights(random_weights(seed))


def _ck(t):
    return int(np.nonzero(G["ck_steps"] == t)[0][0])


def _run(net, obs, h, fresh=None, uniforms=None, crit_act=None, greedy=False, want_vf=True):
    N = obs.shape[0]
    h_in = h.clone().contiguous()
    h_out = torch.full_like(h_in, float("nan"))
    logits = torch.zeros((N, 3, 4), dtype=torch.float32, device="cuda")
    a, lp, vf = net.sample(obs.contiguous(), h_in, h_out, fresh=fresh, uniforms=uniforms, crit_act=crit_act, greedy=greedy, logits=logits,
                           want_vf=want_vf)
    torch.cuda.synchronize()
    return a, lp, vf, h_in, h_out, logits


def _check_draws(logits, u, actions, logp, need_clear=1.0):
    """actions against the float64 inverse CDF on the kernel's own logits (exact wherever no running sum lies within 1e-6 of the target)"""
    lg = logits[..., :3].double().cpu().numpy()
    want, want_lp = CR.inverse_cdf(lg, u)
    m = lg.max(-1, keepdims=True)
    e = np.exp(lg - m)
    S = e.sum(-1)
    margin = np.abs(np.cumsum(e, -1)[..., :2] - (u * S)[..., None]).min(-1) / S
    clear = margin > 1e-6
    assert clear.mean() >= need_clear
    assert np.array_equal(actions.cpu().numpy().astype(np.int64)[clear], want[clear])
    assert np.abs(logp.double().cpu().numpy() - want_lp).max() <= TOL
    assert (logits[..., 3] == 0).all()


def test_teacher_forced_fixture_steps():
    """each step from the reference's own state in (zero where fresh — given the non-zero state, the kernel must zero it itself).  The
    fixture stores the reference's state_out only at CK_STEPS (the whole chain's would add 2.4 MB), so the teacher-forced steps are step 0
    and the steps that follow a stored state (0, 1, 8, 9, 16, 17), plus part (b); every other step is covered by test_free_running_chain"""
    net = _net()
    steps = [0] + [int(c) + 1 for c in G["ck_steps"] if c + 1 < META["K"]]
    for t in steps:
        h = torch.zeros((META["n_arenas"], 3, 2, 200)) if t == 0 else torch.from_numpy(G["h_out_ck"][_ck(t - 1)])
        fresh = torch.from_numpy(G["fresh"][t]).cuda()
        a, lp, vf, h_in, h_out, lg = _run(net, torch.from_numpy(G["obs"][t]).cuda(), h.cuda(), fresh=fresh,
                                          uniforms=torch.from_numpy(G["uniforms"][t]).cuda())
        assert np.abs(lg[..., :3].cpu().numpy() - G["logits"][t]).max() <= TOL, t
        assert np.abs(vf.cpu().numpy() - G["value"][t]).max() <= TOL, t
        assert np.abs(lp.cpu().numpy() - G["logp"][t]).max() <= TOL, t
        _check_draws(lg, G["uniforms"][t], a, lp)
        f = fresh.bool().cpu()
        assert (h_in.cpu()[f] == 0).all() and torch.equal(h_in.cpu()[~f], h[~f])
        if t in G["ck_steps"]:
            assert np.abs(h_out.cpu().numpy() - G["h_out_ck"][_ck(t)]).max() <= TOL, t
    # the value branch's action columns (fixture part b)
    t = META["b_step"]
    h = torch.from_numpy(G["h_out_ck"][_ck(t - 1)]).cuda()
    a, lp, vf, h_in, h_out, lg = _run(net, torch.from_numpy(G["obs"][t]).cuda(), h, fresh=torch.from_numpy(G["fresh"][t]).cuda(),
                                      crit_act=torch.from_numpy(G["b_act"]).cuda(), greedy=True)
    assert np.abs(vf.cpu().numpy() - G["b_value"]).max() <= TOL and np.abs(h_out.cpu().numpy() - G["b_hout"]).max() <= TOL
    assert np.abs(lg[..., :3].cpu().numpy() - G["b_logits"]).max() <= TOL


def test_free_running_chain():
    """the kernel's own state fed back over all K steps; the largest deviation per step is printed (error growth over the chain)"""
    net = _net()
    N = META["n_arenas"]
    h = torch.zeros((N, 3, 2, 200), device="cuda")
    errs = []
    for t in range(META["K"]):
        a, lp, vf, h_in, h, lg = _run(net, torch.from_numpy(G["obs"][t]).cuda(), h, fresh=torch.from_numpy(G["fresh"][t]).cuda(),
                                      uniforms=torch.from_numpy(G["uniforms"][t]).cuda())
        e = max(np.abs(lg[..., :3].cpu().numpy() - G["logits"][t]).max(), np.abs(vf.cpu().numpy() - G["value"][t]).max())
        if t in G["ck_steps"]:
            e = max(e, np.abs(h.cpu().numpy() - G["h_out_ck"][_ck(t)]).max())
        errs.append(float(e))
        _check_draws(lg, G["uniforms"][t], a, lp)
    print("free-running chain: max |kernel - reference| per step", " ".join(f"{x:.1e}" for x in errs))
    assert max(errs) <= 1e-4


@pytest.mark.parametrize("N", [1, 2, 33, 8192])
def test_shapes_fresh_greedy_and_action_inputs_against_float64(N):
    net = _net(seed=3)
    from hhmarl_2d_amd.commander import random_weights
    sd = CR.to_torch(random_weights(3), torch.float64, "cuda")
    g = torch.Generator(device="cuda").manual_seed(N)
    obs = torch.rand((N, 3, 34), device="cuda", generator=g)
    obs[:, :, 4:24] *= (torch.rand((N, 3, 1), device="cuda", generator=g) > 0.2)
    obs *= (torch.rand((N, 3, 1), device="cuda", generator=g) > 0.1)
    h = torch.rand((N, 3, 2, 200), device="cuda", generator=g) * 2 - 1
    fresh = (torch.rand((N,), device="cuda", generator=g) < 0.3).to(torch.uint8)
    crit = (torch.randint(0, 3, (N, 3), device="cuda", generator=g) / 2.0).float()
    u = torch.rand((N, 3), device="cuda", generator=g, dtype=torch.float64)
    h0 = torch.where(fresh.bool()[:, None, None, None], torch.zeros_like(h), h)
    for crit_act in (None, crit):
        lg_ref, v_ref, h_ref = CR.arena_forward(sd, obs.double(), h0.double(), None if crit_act is None else crit_act.double())
        a, lp, vf, h_in, h_out, lg = _run(net, obs, h, fresh=fresh, uniforms=u, crit_act=crit_act)
        assert (lg[..., :3].double() - lg_ref).abs().max() <= TOL
        assert (vf.double() - v_ref).abs().max() <= TOL
        assert (h_out.double() - h_ref).abs().max() <= TOL
        assert torch.equal(h_in, h0)
        _check_draws(lg, u.cpu().numpy(), a, lp, need_clear=0.99)
    # greedy: arg-max and its log-probability; vf = NULL leaves the state update alone
    a, lp, vf, h_in, h_out2, lg = _run(net, obs, h, fresh=fresh, greedy=True, want_vf=False)
    assert vf is None and torch.equal(h_out2, _run(net, obs, h, fresh=fresh, uniforms=u)[4])   # the action inputs were zero: same states
    l64 = lg[..., :3].double()
    assert torch.equal(a.long(), torch.argmax(lg[..., :3], dim=-1))
    assert (lp.double() - torch.log_softmax(l64, -1).gather(-1, a.long()[..., None])[..., 0]).abs().max() <= TOL
    _, _, _, _, h_out3, _ = _run(net, obs, h, fresh=fresh, greedy=True)
    assert torch.equal(h_out2, h_out3)


def test_logits_output_needs_no_16_byte_alignment():
    net = _net(seed=2, max_rows=96)
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.rand((32, 3, 34), device="cuda", generator=g)
    h = torch.rand((32, 3, 2, 200), device="cuda", generator=g) - 0.5
    _, _, _, _, _, lg = _run(net, obs, h, greedy=True)
    buf = torch.full((32 * 3 * 4 + 1,), 7.0, device="cuda")
    off = buf[1:]                                                       # 4-byte aligned only
    net.sample(obs, h.clone(), torch.empty_like(h), greedy=True, logits=off)
    torch.cuda.synchronize()
    assert torch.equal(off.reshape(32, 3, 4), lg) and buf[0] == 7.0


def test_argument_errors():
    from hhmarl_2d_amd.commander import CommanderNet
    net = _net(max_rows=96)
    obs = torch.zeros((32, 3, 34), device="cuda")
    h, h2 = torch.zeros((32, 3, 2, 200), device="cuda"), torch.zeros((32, 3, 2, 200), device="cuda")
    u = torch.zeros((32, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="max_rows"):
        net.sample(torch.zeros((33, 3, 34), device="cuda"), torch.zeros((33, 3, 2, 200), device="cuda"),
                   torch.zeros((33, 3, 2, 200), device="cuda"), uniforms=torch.zeros((33, 3), dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError, match="alias"):
        net.sample(obs, h, h, uniforms=u)
    hb = torch.zeros((33, 3, 2, 200), device="cuda")
    with pytest.raises(RuntimeError, match="alias"):                   # overlapping by one row, not identical
        net.sample(obs, hb[:32], hb[1:], uniforms=u)
    with pytest.raises(RuntimeError, match="exactly one"):
        net.sample(obs, h, h2)
    empty = CommanderNet(0, 96)
    with pytest.raises(RuntimeError, match="no weights"):
        empty.sample(obs, h, h2, greedy=True)
    assert net.kernel_name(32) == "hh_k_commander"


def _hl_world(N, seed=11, horizon=None):
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.world import World, make_config
    kw = dict(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=seed, arena_offset=500, auto_reset=True)
    if horizon is not None:
        kw["horizon"] = horizon
    return World(make_config(**kw), device=0)


def test_keyed_draws_at_rollout_size(oracle):
    """8192 arenas x 3 agents of a real world a few commander steps in: draws keyed by (seed, arena, episode, steps, agent, site 27, 0)"""
    from hhmarl_2d_amd.env_hier import macro_step
    from hhmarl_2d_amd.pilots import RandomPilot
    N = 8192
    w = _hl_world(N)
    net = _net(seed=4)
    obs = w.reset()
    pilot = RandomPilot(w.device, seed=2)
    for _ in range(2):
        obs = macro_step(w, torch.randint(0, 3, (N, 3), device="cuda", dtype=torch.int8), pilot)[0]
    h, h2 = torch.zeros((N, 3, 2, 200), device="cuda"), torch.zeros((N, 3, 2, 200), device="cuda")
    logits = torch.zeros((N, 3, 4), device="cuda")
    a, lp, vf = net.sample(obs.contiguous(), h, h2, world=w, logits=logits)
    torch.cuda.synchronize()
    st = w.get_state()["ar_i"]          # steps, ..., episode (column 5)
    lib = oracle.lib()
    sub = np.arange(0, N, 7)
    u = np.array([[lib.hho_rng_u01(11, 500 + int(n), int(st[n, 5]), int(st[n, 0]), s + 1, 27, 0) for s in range(3)] for n in sub])
    _check_draws(logits[sub], u, a[sub], lp[sub], need_clear=0.99)
    for k in range(3):
        assert len(torch.unique(a[:, k])) == 3
    a2, _, _ = net.sample(obs.contiguous(), h, h2, world=w)
    assert torch.equal(a, a2)                                          # keyed, not a stream


def test_every_agent_has_a_reward_key_every_commander_step():
    """RLlib fills rewards.get(agent_id, 0.0); HighLevelEnv gives every agent id a reward key every step (env_hier.py:154,188), dead
    agents included.  hh_hl_end writes reward 0.0 wherever it reports valid = 0 (an arena that did not take part), and in an
    auto-resetting world every arena takes part in every macro step: valid is 1 on every row, so CommanderRollout masks nothing"""
    from hhmarl_2d_amd.env_hier import macro_step
    from hhmarl_2d_amd.pilots import RandomPilot
    N = 2048
    w = _hl_world(N, seed=5, horizon=4)
    w.reset()
    pilot = RandomPilot(w.device, seed=3)
    dones = 0
    for _ in range(10):
        obs, rew, val, done = macro_step(w, torch.randint(0, 3, (N, 3), device="cuda", dtype=torch.int8), pilot)
        assert (val == 1).all() and (rew[val == 0] == 0).all() and torch.isfinite(rew).all()
        dones += int(done.sum())
    assert dones > 0


def _rollout_buffers(r):
    return {k: getattr(r, k).clone() for k in ("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target", "state_in")}


def _replay_step_by_step(w, net, pilot, T, collects):
    """the collect's semantics spelled out call by call: fresh = previous done, zero state at fresh arenas, bootstrap from scratch"""
    from hhmarl_2d_amd.env_hier import macro_step
    N = w.N
    obs = w.reset()
    h = torch.zeros((N, 3, 2, 200), device="cuda")
    fresh = torch.ones((N,), dtype=torch.uint8, device="cuda")
    out = []
    for _ in range(collects):
        B = {"obs": [obs.clone()], "actions": [], "logp": [], "vf": [], "reward": [], "valid": [], "done": [], "state_in": []}
        for t in range(T):
            h_out = torch.zeros_like(h)
            a, lp, vf = net.sample(obs.contiguous(), h, h_out, fresh=fresh, world=w)
            B["state_in"].append(h.clone())
            obs, rew, val, done = macro_step(w, a, pilot, early_exit=False)
            for k, v in zip(("actions", "logp", "vf", "reward", "valid", "done"), (a, lp, vf, rew, val, done)):
                B[k].append(v.clone())
            B["obs"].append(obs.clone())
            h, fresh = h_out, done.clone()
        scratch = torch.zeros_like(h)
        _, _, vf = net.sample(obs.contiguous(), h, scratch, fresh=fresh, greedy=True)
        B["vf"].append(vf.clone())
        B["state_in"].append(h.clone())
        out.append({k: torch.stack(v) for k, v in B.items()})
    return out


@pytest.mark.parametrize("form", ["graph_variants", "graph_variants_trace", "eager_variants", "eager_tape"])
def test_commander_rollout_equals_a_step_by_step_replay(form):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import gae_ref
    from hhmarl_2d_amd.commander import CommanderRollout
    from hhmarl_2d_amd.pilots import TapePilot, VariantNetPilot
    N, T = 64, 6
    nets = [_net(seed=6, max_rows=3 * N) for _ in range(2)]
    results = []
    for i in range(2):
        w = _hl_world(N, seed=21, horizon=9)              # short horizon: episodes end and restart inside a collect
        if form == "eager_tape":
            pilot = TapePilot(w.device, N, w.A, seed=4)
        else:
            pilot = VariantNetPilot(w, seed=8)
        if i == 0:
            roll = CommanderRollout(w, nets[0], pilot, T, use_graph=form.startswith("graph"))
            res = []
            for c in range(2):
                if c == 1 and form == "graph_variants_trace":
                    # trace_enable frees and reallocates the world's trace ring: the captured graph holds the old one and must be re-captured
                    gen0 = roll._graph_gen
                    w.trace_enable(n_arenas=4, capacity=256)
                roll.collect()
                res.append(_rollout_buffers(roll))
            if form == "graph_variants_trace":
                assert roll._graph_gen != gen0
                tr = w.trace_read()
                assert len(tr) == 4 and all(len(r) > 0 for r, _ in tr)   # the second collect's graph writes the new ring
            torch.cuda.synchronize()
            results.append(res)
        else:
            results.append(_replay_step_by_step(w, nets[1], pilot, T, 2))
    got, want = results
    for c in range(2):
        g, r = got[c], want[c]
        for k in ("obs", "actions", "logp", "vf", "reward", "valid", "done", "state_in"):
            assert torch.equal(g[k], r[k].reshape(g[k].shape)), (c, k)
        assert g["done"].any(), "no episode ended inside the collect"
        fresh_rows = torch.cat([torch.ones_like(g["done"][:1]) if c == 0 else got[c - 1]["done"][-1:], g["done"]])  # [T+1, N]
        assert (g["state_in"][fresh_rows.bool()] == 0).all()
        h = [x.cpu().numpy() for x in (g["reward"], g["valid"], g["vf"], g["done"])]
        a_ref, r_ref = gae_ref.rllib_stream(h[0], h[1], h[2], h[3], 0.99, 1.0)
        assert np.array_equal(g["adv"].cpu().numpy(), a_ref) and np.array_equal(g["target"].cpu().numpy(), r_ref)
    if form.startswith("graph"):
        from hhmarl_2d_amd.rollout import central_critic_rows_hl
        for agent in (1, 2, 3):
            assert torch.equal(roll.critic_rows(agent), central_critic_rows_hl(roll.obs[:T], roll.actions, agent))
