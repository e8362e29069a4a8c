"""The samplers' weight packer on the MI355X, by both ways in — a load (set_net + set_critic, set_weights) and a device refresh
(hh_policy_refresh / hh_commander_refresh_weights): every packed form byte-equal to the recorded digests of packed_weight_digests.py;
a reload with another kind, the caller's arrays free on return, set_net's invalidation of the value branch; captured rollout graphs
that keep working across a refresh; a refresh captured into one graph with a collect; and the error paths, which leave the packed bytes
as they were."""
import ctypes as C

import numpy as np
import pytest
import torch

import packed_weight_digests as PWD
from hhmarl_2d_amd import _lib as L
from hhmarl_2d_amd import commander as CM
from hhmarl_2d_amd import pilots
from hhmarl_2d_amd import policy_nets as PN
from hhmarl_2d_amd.pilots import PolicyBank

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
POLICY_PARTS = (0, 1, 2, 3, 4)
ROLLOUT_BUFS = ("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target")


def _dicts(mode, seed, tie, edges=False):
    """what trainable_init(mode, seed, tie_shared=tie) loads: (kinds, actor dicts, critic dicts), numpy"""
    kinds = (PN.FIGHT1, PN.FIGHT2) if mode == "fight" else (PN.ESC1, PN.ESC2)
    sds = [PN.random_weights(k, seed) for k in kinds]
    if tie:
        pilots.tie_shared_layer(sds)
    csds = [PN.random_critic_weights(k, seed) for k in kinds]
    if edges:   # fp16 subnormals, fp32 subnormals, signed zero, rounding ties and the top of the fp16 range in every kind of section
        vals = np.array([1e-39, -3e-41, 2.0 ** -25, -(2.0 ** -24) * 1.5, 6.1e-5, -0.0, 65504.0, 1.0 + 2.0 ** -11], dtype=np.float32)
        for sd in sds[:1] if tie else sds:
            sd["shared_layer._model.0.weight"][3, :8] = vals
        for sd, csd in zip(sds, csds):
            sd["inp1._model.0.weight"][0, :4] = vals[:4]
            sd["act_out._model.0.weight"][1, 10:18] = vals
            for k in ("att_act.in_proj_weight", "att_act.out_proj.weight", "att_val.in_proj_weight", "att_val.out_proj.weight"):
                if k in sd:
                    sd[k][250 if "in_proj" in k else 5, :8] = vals * 1e-3
                if k in csd:
                    csd[k][400 if "in_proj" in k else 5, :8] = vals * 1e-3
            csd["val_out._model.0.weight"][0, :8] = vals
    return kinds, sds, csds


def _cuda(dicts):
    """numpy dicts -> CUDA tensors; a numpy array shared by several dicts (a tied shared layer) becomes ONE tensor"""
    cache = {}
    out = []
    for d in dicts:
        out.append({k: cache.setdefault(id(v), torch.from_numpy(np.ascontiguousarray(v)).to(DEV)) for k, v in d.items()})
    return out


def _policy_parts(bank, slots=(0, 1)):
    return {(s, p): bank.packed(s, p) for s in slots for p in POLICY_PARTS}


@pytest.mark.parametrize("mode", ["fight", "escape"])
@pytest.mark.parametrize("seeds", [(3, 11), (17, 5)])
@pytest.mark.parametrize("tie", [True, False])
def test_policy_refresh_is_byte_identical_to_the_host_path(mode, seeds, tie):
    s1, s2 = seeds
    kinds, sds, csds = _dicts(mode, s2, tie, edges=seeds == (17, 5))
    fix = PWD.load()["policy"][PWD.policy_case(mode, seeds, tie)]
    assert PWD.weights_digest(sds + csds) == fix["weights_sha256"]           # else: the weight generator drifted, not the packer
    want = fix["parts"]
    host = PolicyBank(DEV, 64)
    for slot in (0, 1):
        host.load_trainable(slot, kinds[slot], sds[slot], csds[slot])
    dev = PolicyBank.trainable_init(DEV, mode=mode, seed=s1, max_rows=64, tie_shared=tie)
    d_sd, d_csd = _cuda(sds), _cuda(csds)
    if tie:
        assert d_sd[0]["shared_layer._model.0.weight"] is d_sd[1]["shared_layer._model.0.weight"]
    before = PWD.policy_digests(dev)
    gen, kinds_before = dev.generation, dict(dev.kinds)
    for slot in (0, 1):
        dev.refresh(slot, d_sd[slot], d_csd[slot])
    loaded, got = PWD.policy_digests(host), PWD.policy_digests(dev)
    for key in want:
        assert before[key] != want[key], key                                 # the refresh had something to change
        assert loaded[key] == want[key], key
        assert got[key] == want[key], key
    assert dev.generation == gen and dev.kinds == kinds_before               # nothing a captured graph holds by value changed


@pytest.mark.parametrize("seeds", [(2, 9), (9, 4)])
def test_commander_refresh_is_byte_identical_to_the_host_path(seeds):
    s1, s2 = seeds
    sd = CM.random_weights(s2)
    if seeds == (9, 4):
        sd["rnn_act.bias_ih_l0"][:4] = np.array([1e-39, 3.0, -0.0, 2.0 ** -25], np.float32)
        sd["rnn_act.bias_hh_l0"][:4] = np.array([-1e-39, 2.0 ** -24, 0.0, 1e-7], np.float32)
        sd["shared_layer._model.0.weight"][7, 295:305] = 6.1e-5
    fix = PWD.load()["commander"][PWD.commander_case(seeds)]
    assert PWD.weights_digest([sd]) == fix["weights_sha256"]
    want = fix["parts"]
    host = CM.CommanderNet(0, 96).set_weights(sd)
    dev = CM.CommanderNet(0, 96).set_weights(CM.random_weights(s1))
    before = PWD.commander_digests(dev)
    dev.refresh_weights(_cuda([sd])[0])
    loaded, got = PWD.commander_digests(host), PWD.commander_digests(dev)
    for p in want:
        assert before[p] != want[p] and loaded[p] == want[p] and got[p] == want[p], p


def _recorded(mode, seeds=(3, 11), tie=True):
    """a recorded policy case: its weights (kinds, actor dicts, critic dicts) and the digests of its packed parts"""
    return _dicts(mode, seeds[1], tie), PWD.load()["policy"][PWD.policy_case(mode, seeds, tie)]["parts"]


@pytest.mark.parametrize("first, then", [("fight", "escape"), ("escape", "fight")])
def test_reload_with_another_kind_leaves_nothing_of_the_old_one(first, then):
    """the packer writes no padding and only fight nets have attention sections: a load has to clear what the slot held (a fresh
    allocation is usually zero and would hide a missing clear; a slot that held the other kind does not)"""
    bank = PolicyBank(DEV, 64)
    for mode in (first, then):
        (kinds, sds, csds), want = _recorded(mode)
        for slot in (0, 1):
            bank.load_trainable(slot, kinds[slot], sds[slot], csds[slot])
    assert PWD.policy_digests(bank) == want


def _own_and_poison(d):
    """after a load returned: the arrays were the caller's own (no copy stood in between) and may be overwritten at once"""
    for v in d.values():
        assert v.dtype == np.float32 and v.flags["C_CONTIGUOUS"]          # set_net / set_critic / set_weights pass such an array through
        v.fill(np.nan)


def test_the_callers_arrays_are_free_when_a_load_returns():
    """every source array is overwritten with NaN right after the call that read it returns, with no synchronisation; the packed parts,
    read on another stream than the default one, are the recorded ones"""
    (kinds, sds, csds), want = _recorded("fight", tie=False)
    bank = PolicyBank(DEV, 64)
    for slot in (0, 1):
        shared = {k: sds[slot][k].copy() for k in ("shared_layer._model.0.weight", "shared_layer._model.0.bias")}   # set_critic's
        bank.set_net(slot, kinds[slot], sds[slot])
        _own_and_poison(sds[slot])
        bank.set_critic(slot, kinds[slot], shared, csds[slot])
        _own_and_poison(csds[slot])
        _own_and_poison(shared)
    sd = PWD.commander_weights((2, 9))
    net = CM.CommanderNet(0, 96).set_weights(sd)
    _own_and_poison(sd)
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        assert PWD.policy_digests(bank) == want
        assert PWD.commander_digests(net) == PWD.load()["commander"]["2-9"]["parts"]


def _fight_rows(n_arenas=16):
    obs = torch.zeros((n_arenas, 2, 30), dtype=torch.float32, device=DEV)
    sel = torch.tensor([pilots.SEL_FIGHT1, pilots.SEL_FIGHT2], dtype=torch.uint8, device=DEV).repeat(n_arenas, 1).contiguous()
    return obs, sel


def test_set_net_alone_invalidates_the_value_branch():
    (kinds, sds, csds), want = _recorded("fight")
    bank = PolicyBank.trainable_init(DEV, mode="fight", seed=3, max_rows=64)
    obs, sel = _fight_rows()
    bank.sample(obs, sel, greedy=True)                                          # both value branches loaded: vf is given
    bank.set_net(0, kinds[0], sds[0])
    with pytest.raises(RuntimeError, match=r"vf asked for, but a loaded network has no value branch \(hh_policy_set_critic\)"):
        bank.sample(obs, sel, greedy=True)
    bank.sample(obs, sel, greedy=True, want_vf=False)
    bank.set_critic(0, kinds[0], sds[0], csds[0])
    _, _, vf = bank.sample(obs, sel, greedy=True)
    assert torch.isfinite(vf).all()
    got = PWD.policy_digests(bank, slots=(0,))
    assert got["0/3"] == want["0/3"] and got["0/4"] == want["0/4"]


def test_load_error_paths_leave_the_packed_bytes_unchanged():
    """a missing pointer on a LOADED slot / commander: HH_E_ARG with the message of the check, every packed part as it was, and the value
    branch still loaded (validation comes before anything is touched)"""
    bank = PolicyBank.trainable_init(DEV, mode="fight", seed=5, max_rows=64)
    before = PWD.policy_digests(bank)
    kinds, sds, csds = _dicts("fight", 9, True)
    lib = L.lib()
    hp = lambda d: (lambda k: d[k].ctypes.data_as(C.c_void_p) if k in d else None)
    crit = {**csds[0], **{k: sds[0][k] for k in ("shared_layer._model.0.weight", "shared_layer._model.0.bias")}}

    def refused(call, struct, field, index, msg):
        w = struct()
        if index is None:
            setattr(w, field, None)
        else:
            getattr(w, field)[index] = None
        assert call(w) == -1 and lib.hh_last_error().decode() == msg, (field, lib.hh_last_error().decode())

    set_net = lambda w: lib.hh_policy_set_net(bank.h, 0, C.byref(w))
    set_critic = lambda w: lib.hh_policy_set_critic(bank.h, 0, C.byref(w))
    refused(set_net, lambda: pilots._net_struct(PN.FIGHT1, hp(sds[0])), "att_out_w", None, "hh_policy_set_net: missing weight pointer")
    refused(set_net, lambda: pilots._net_struct(PN.FIGHT1, hp(sds[0])), "inp_b", 2, "hh_policy_set_net: missing input layer")
    refused(set_critic, lambda: pilots._critic_struct(PN.FIGHT1, hp(crit)), "v_w", 2, "hh_policy_set_critic: missing weight pointer")
    refused(set_critic, lambda: pilots._critic_struct(PN.FIGHT1, hp(crit)), "val_b", None, "hh_policy_set_critic: missing weight pointer")
    assert PWD.policy_digests(bank) == before
    _, _, vf = bank.sample(*_fight_rows(), greedy=True)
    assert torch.isfinite(vf).all()
    sd = CM.random_weights(2)
    net = CM.CommanderNet(0, 96).set_weights(CM.random_weights(1))
    cb = PWD.commander_digests(net)
    set_weights = lambda w: lib.hh_commander_set_weights(net.h, C.byref(w))
    refused(set_weights, lambda: CM._weights_struct(lambda k: sd[k].ctypes.data), "val_w_hh", None, "hh_commander_set_weights: missing weight pointer")
    refused(set_weights, lambda: CM._weights_struct(lambda k: sd[k].ctypes.data), "v_b", 3, "hh_commander_set_weights: missing input layer")
    assert PWD.commander_digests(net) == cb


def _ppo(N, T, seed_w, graph):
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, level=3, seed=23, auto_reset=True, horizon=30), device=0)
    bank = PolicyBank.trainable_init(DEV, mode="fight", seed=seed_w, max_rows=2 * N)
    return PPORollout(w, bank, T, use_graph=graph)


def test_ppo_rollout_graph_survives_a_refresh():
    """captured with w1, refreshed to w2 on the device: the same graph object replays and gives what a rollout host-loaded with w2 gives
    from the same world state"""
    N, T = 256, 12
    a, b, c = _ppo(N, T, 5, True), _ppo(N, T, 5, False), _ppo(N, T, 5, True)
    for r in (a, b, c):
        r.collect()
    g0 = a._graph
    kinds, sds, csds = _dicts("fight", 8, True)
    d_sd, d_csd = _cuda(sds), _cuda(csds)
    a.bank.refresh_trainable([{**d_sd[s], **d_csd[s]} for s in (0, 1)])
    for s in (0, 1):
        b.bank.load_trainable(s, kinds[s], sds[s], csds[s])
    for r in (a, b, c):
        r.collect()
    torch.cuda.synchronize()
    assert a._graph is g0
    for k in ROLLOUT_BUFS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert not torch.equal(a.logp, c.logp)                                   # c kept w1: the new weights are in use


def _commander(N, T, seed_w, graph):
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=21, arena_offset=500, auto_reset=True, horizon=9),
              device=0)
    net = CM.CommanderNet(0, 3 * N).set_weights(CM.random_weights(seed_w))
    return CM.CommanderRollout(w, net, VariantNetPilot(w, seed=8), T, use_graph=graph)


def test_commander_rollout_graph_survives_a_refresh():
    N, T = 64, 6
    a, b, c = _commander(N, T, 6, True), _commander(N, T, 6, False), _commander(N, T, 6, True)
    for r in (a, b, c):
        r.collect()
    g0, gen0 = a._graph, a._graph_gen
    sd2 = CM.random_weights(12)
    a.net.refresh_weights(_cuda([sd2])[0])
    b.net.set_weights(sd2)
    for r in (a, b, c):
        r.collect()
    torch.cuda.synchronize()
    assert a._graph is g0 and a._graph_gen == gen0
    for k in ROLLOUT_BUFS + ("state_in",):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert not torch.equal(a.logp, c.logp)


def test_refresh_and_collect_in_one_captured_graph():
    """refresh of both trainable slots + a whole PPORollout collect in ONE torch.cuda.graph; the source parameters are updated in place
    between replays, and after each replay the packed bytes are the host path's for the new values"""
    N, T = 128, 8
    ro = _ppo(N, T, 5, False)
    ro.start()
    bank = ro.bank
    kinds, sds, csds = _dicts("fight", 30, True)
    src_sd, src_csd = _cuda(sds), _cuda(csds)
    for s in (0, 1):                                                          # first launches outside the capture
        bank.refresh(s, src_sd[s], src_csd[s])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for s in (0, 1):
            bank.refresh(s, src_sd[s], src_csd[s])
        ro.collect()
    host = PolicyBank(DEV, 64)
    for seed in (40, 41):
        kinds, sds, csds = _dicts("fight", seed, True)
        with torch.no_grad():
            for src, new in zip(src_sd + src_csd, sds + csds):
                for k, v in new.items():
                    src[k].copy_(torch.from_numpy(v))
        g.replay()
        for s in (0, 1):
            host.load_trainable(s, kinds[s], sds[s], csds[s])
        want, got = _policy_parts(host), _policy_parts(bank)
        torch.cuda.synchronize()
        for key in want:
            assert torch.equal(got[key], want[key]), (seed, key)
        assert torch.isfinite(ro.logp).all() and torch.isfinite(ro.vf).all()


def test_commander_refresh_in_a_captured_graph():
    net = CM.CommanderNet(0, 96).set_weights(CM.random_weights(1))
    src = _cuda([CM.random_weights(2)])[0]
    net.refresh_weights(src)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        net.refresh_weights(src)
    for seed in (3, 4):
        new = CM.random_weights(seed)
        with torch.no_grad():
            for k, v in new.items():
                src[k].copy_(torch.from_numpy(v))
        g.replay()
        host = CM.CommanderNet(0, 96).set_weights(new)
        for p in (0, 1):
            want, got = host.packed(p), net.packed(p)
            torch.cuda.synchronize()
            assert torch.equal(got, want), (seed, p)


def test_error_paths_leave_the_packed_bytes_unchanged():
    bank = PolicyBank.trainable_init(DEV, mode="fight", seed=5, max_rows=64)    # slots 0, 1 with value branches
    esc = PN.random_weights(PN.ESC1, 1)
    bank.set_net(2, PN.ESC1, esc)                                               # slot 2: an actor only
    before = {**_policy_parts(bank), **{(2, p): bank.packed(2, p) for p in (0, 1, 2)}}
    kinds, sds, csds = _dicts("fight", 9, True)
    d_sd, d_csd = _cuda(sds), _cuda(csds)
    lib, st = L.lib(), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ptr = lambda d: (lambda k: d[k].data_ptr() if k in d else None)
    w0 = pilots._net_struct(PN.FIGHT1, ptr(d_sd[0]))
    shared = {k: d_sd[0][k] for k in ("shared_layer._model.0.weight", "shared_layer._model.0.bias")}
    cw0 = pilots._critic_struct(PN.FIGHT1, ptr({**d_csd[0], **shared}))
    # an empty slot
    with pytest.raises(ValueError, match="empty"):
        bank.refresh(5, d_sd[0], d_csd[0])
    assert lib.hh_policy_refresh(bank.h, 5, C.byref(w0), C.byref(cw0), st) == -1
    # a kind other than the loaded one (Fight1 weights into the Fight2 slot)
    assert lib.hh_policy_refresh(bank.h, 1, C.byref(w0), C.byref(cw0), st) == -1
    assert "kind" in lib.hh_last_error().decode()
    # the value branch is loaded but no critic is given; a critic for a slot without a value branch
    with pytest.raises(RuntimeError, match="value branch"):
        bank.refresh(0, d_sd[0])
    d_esc = _cuda([esc, PN.random_critic_weights(PN.ESC1, 1)])
    with pytest.raises(RuntimeError, match="value branch"):
        bank.refresh(2, d_esc[0], d_esc[1])
    # a missing pointer
    w_bad = pilots._net_struct(PN.FIGHT1, ptr(d_sd[0]))
    w_bad.att_out_w = None
    assert lib.hh_policy_refresh(bank.h, 0, C.byref(w_bad), C.byref(cw0), st) == -1
    # wrong shape / dtype / device in Python
    for k, v in (("shared_layer._model.0.weight", d_sd[0]["shared_layer._model.0.weight"][:, :499]),
                 ("inp1._model.0.bias", d_sd[0]["inp1._model.0.bias"].double()),
                 ("act_out._model.0.weight", d_sd[0]["act_out._model.0.weight"].cpu())):
        with pytest.raises(ValueError):
            bank.refresh(0, {**d_sd[0], k: v}, d_csd[0])
    with pytest.raises(ValueError, match="shape"):
        bank.refresh(0, d_sd[0], {**d_csd[0], "v3._model.0.weight": d_csd[0]["v3._model.0.weight"].t()})
    after = {**_policy_parts(bank), **{(2, p): bank.packed(2, p) for p in (0, 1, 2)}}
    torch.cuda.synchronize()
    for key in before:
        assert torch.equal(before[key], after[key]), key
    # the commander: a wrong shape, an unloaded commander, a missing pointer
    net = CM.CommanderNet(0, 96).set_weights(CM.random_weights(1))
    cb = [net.packed(p) for p in (0, 1)]
    d = _cuda([CM.random_weights(2)])[0]
    with pytest.raises(ValueError, match="shape"):
        net.refresh_weights({**d, "rnn_act.weight_hh_l0": d["rnn_act.weight_hh_l0"][:599]})
    with pytest.raises(RuntimeError, match="no weights loaded"):
        CM.CommanderNet(0, 96).refresh_weights(d)
    wc = CM._weights_struct(lambda k: d[k].data_ptr())
    wc.val_w_hh = None
    assert lib.hh_commander_refresh_weights(net.h, C.byref(wc), st) == -1
    ca = [net.packed(p) for p in (0, 1)]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(cb, ca))
