"""hh_commander_act_chain (the commander as evaluation.py:40-48 runs it) on the MI355X: bit for bit a slot-by-slot replay with
hh_commander_sample(greedy=True), within the commander tolerance of the float64 restatement chained the same way, its argument checks,
and a captured call against an eager one."""
import ctypes as C

import numpy as np
import pytest
import torch

import commander_ref as CR

pytestmark = pytest.mark.gpu

TOL = 1e-5          # test_gpu_commander.py's tolerance against the float64 forward
SEED = 5
NS = [1, 31, 32, 33, 1000, 8192]


def _net(max_rows=5 * 8192):
    from hhmarl_2d_amd.commander import CommanderNet, random_weights
    return CommanderNet(0, max_rows).set_weights(random_weights(SEED))


def _obs(N, nA, seed):
    """observations in [0, 1] with the sparsity of real ones: opponent blocks missing, dead agents as zero rows"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = torch.rand((N, nA, 34), device="cuda", generator=g)
    obs[:, :, 4:24] *= (torch.rand((N, nA, 1), device="cuda", generator=g) > 0.2)
    obs *= (torch.rand((N, nA, 1), device="cuda", generator=g) > 0.15)
    return obs.contiguous()


def _chain(net, obs):
    N, nA = obs.shape[:2]
    h = torch.full((N, nA, 200), float("nan"), device="cuda")
    lg = torch.full((N, nA, 4), float("nan"), device="cuda")
    a = net.act_chain(obs, h_out=h, logits=lg)
    torch.cuda.synchronize()
    return a, h, lg


def _replay(net, obs):
    """slot by slot with the sampler: slot 0 fresh, slot k's h_in (rnn_act) = slot k-1's h_out; the N rows of a slot packed three to a
    sampler arena (the actor reads its own row only)"""
    N, nA = obs.shape[:2]
    M = -(-N // 3)
    acts, hs, lgs = [], [], []
    h_prev = torch.zeros((3 * M, 2, 200), device="cuda")
    for k in range(nA):
        o = torch.zeros((3 * M, 34), device="cuda")
        o[:N] = obs[:, k]
        h_in = h_prev.clone()
        h_out = torch.full((3 * M, 2, 200), float("nan"), device="cuda")
        lg = torch.full((M, 3, 4), float("nan"), device="cuda")
        fresh = torch.ones((M,), dtype=torch.uint8, device="cuda") if k == 0 else None
        a, _, _ = net.sample(o.view(M, 3, 34), h_in, h_out, fresh=fresh, greedy=True, logits=lg, want_vf=False)
        acts.append(a.view(-1)[:N])
        hs.append(h_out[:N, 0])
        lgs.append(lg.view(-1, 4)[:N])
        h_prev = h_out
    torch.cuda.synchronize()
    return torch.stack(acts, 1), torch.stack(hs, 1), torch.stack(lgs, 1)


@pytest.mark.parametrize("N", NS)
def test_chain_equals_slot_by_slot_sampler_replay_bitwise(N):
    net = _net()
    for nA in range(1, 6):
        obs = _obs(N, nA, 100 * N + nA)
        a, h, lg = _chain(net, obs)
        ra, rh, rlg = _replay(net, obs)
        assert torch.equal(lg, rlg), (N, nA)
        assert torch.equal(a, ra), (N, nA)
        assert torch.equal(h, rh), (N, nA)
        assert (lg[..., 3] == 0).all() and int(a.min()) >= 0 and int(a.max()) <= 2


@pytest.mark.parametrize("N", [1, 33, 1000])
def test_chain_against_float64_reference(N):
    from hhmarl_2d_amd.commander import random_weights
    net = _net()
    sd = CR.to_torch(random_weights(SEED), torch.float64, "cuda")
    checked = 0
    for nA in range(1, 6):
        obs = _obs(N, nA, 7 * N + nA)
        a, h, lg = _chain(net, obs)
        z34 = torch.zeros((N, 34), dtype=torch.float64, device="cuda")
        z1 = torch.zeros((N, 1), dtype=torch.float64, device="cuda")
        ha = torch.zeros((N, 200), dtype=torch.float64, device="cuda")
        hv = torch.zeros_like(ha)
        for k in range(nA):
            ref, _, ha, _ = CR.forward(sd, obs[:, k].double(), z34, z34, z1, z1, z1, ha, hv)
            assert (lg[:, k, :3].double() - ref).abs().max() <= TOL, (N, nA, k)
            assert (h[:, k].double() - ha).abs().max() <= TOL, (N, nA, k)
            top2 = ref.topk(2, dim=1).values
            clear = (top2[:, 0] - top2[:, 1]) > TOL
            want = ref.argmax(dim=1)
            assert torch.equal(a[:, k].long()[clear], want[clear]), (N, nA, k)
            checked += int(clear.sum())
    assert checked >= 0.9 * N * 15


def test_argument_errors():
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.commander import CommanderNet
    net = _net(max_rows=100)
    obs = _obs(20, 3, 1)
    for bad in (torch.zeros((4, 0, 34), device="cuda"), torch.zeros((4, 6, 34), device="cuda"), torch.zeros((4, 3, 33), device="cuda"),
                torch.zeros((4, 3, 34), device="cuda", dtype=torch.float64), torch.zeros((0, 3, 34), device="cuda")):
        with pytest.raises(ValueError):
            net.act_chain(bad)
    with pytest.raises(ValueError):
        net.act_chain(obs, actions=torch.zeros((20, 2), dtype=torch.int8, device="cuda"))
    with pytest.raises(ValueError):
        net.act_chain(obs, h_out=torch.zeros((20, 3, 199), device="cuda"))
    with pytest.raises(ValueError):
        net.act_chain(obs, logits=torch.zeros((20, 3, 3), device="cuda"))
    with pytest.raises(RuntimeError, match="max_rows"):
        net.act_chain(_obs(34, 3, 2))                       # 102 rows > max_rows 100
    act = torch.zeros((20, 3), dtype=torch.int8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    for nA in (0, 6, -1):                                   # the C entry point checks on its own
        assert L.lib().hh_commander_act_chain(net.h, p(obs), 20, nA, p(act), None, None, None) != 0
    assert L.lib().hh_commander_act_chain(net.h, None, 20, 3, p(act), None, None, None) != 0
    assert L.lib().hh_commander_act_chain(net.h, p(obs), 0, 3, p(act), None, None, None) != 0
    assert L.lib().hh_commander_act_chain(None, p(obs), 20, 3, p(act), None, None, None) != 0
    empty = CommanderNet(0, 100)                            # no weights loaded
    with pytest.raises(RuntimeError, match="no weights"):
        empty.act_chain(obs)
    assert net.chain_kernel_name(20, 3) == "hh_k_commander_chain"
    with pytest.raises(RuntimeError):
        net.chain_kernel_name(20, 6)


def test_captured_call_equals_eager():
    net = _net()
    N, nA = 1000, 4
    obs = _obs(N, nA, 9)
    a_e, h_e, lg_e = _chain(net, obs)
    src = torch.zeros_like(obs)
    a_g = torch.zeros((N, nA), dtype=torch.int8, device="cuda")
    h_g = torch.zeros((N, nA, 200), device="cuda")
    lg_g = torch.zeros((N, nA, 4), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            net.act_chain(src, actions=a_g, h_out=h_g, logits=lg_g)
    torch.cuda.current_stream().wait_stream(side)
    src.copy_(obs)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a_g, a_e) and torch.equal(h_g, h_e) and torch.equal(lg_g, lg_e)
    src.copy_(_obs(N, nA, 10))                              # the graph reads the buffer as it is at replay
    graph.replay()
    a2, h2, lg2 = _chain(net, src)
    assert torch.equal(a_g, a2) and torch.equal(lg_g, lg2) and torch.equal(h_g, h2)
