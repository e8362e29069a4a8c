"""hh_policy_snapshot / hh_policy_restore and hh_commander_snapshot / hh_commander_restore on the MI355X (PolicyBank / CommanderNet
.snapshot, .restore, .state_dict, .load_state_dict): snapshot, refresh with other weights, restore — actions, logp, vf and logits on a
fixed observation block are bitwise what they were, every packed part is byte for byte what it was, and a blob of another slot layout
is refused with the bank unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N = 70          # [N, 2] = 140 sampler rows: more than one 64-row tile, not a multiple of the 32-row tile


def _cuda(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sd.items()}


def _bank(seed=5, frozen=True, max_rows=2 * N):
    """the two trainable fight policies (slots 0, 1: actor and value branch) and, with frozen, two frozen escape actors (slots 2, 3)"""
    from hhmarl_2d_amd import pilots, policy_nets as PN
    b = pilots.PolicyBank.trainable_init(torch.device("cuda", 0), mode="fight", seed=seed, max_rows=max_rows)
    lut = {pilots.SEL_FIGHT1: 0, pilots.SEL_FIGHT2: 1}
    if frozen:
        b.set_net(2, PN.ESC1, PN.random_weights(PN.ESC1, seed + 1))
        b.set_net(3, PN.ESC2, PN.random_weights(PN.ESC2, seed + 1))
        lut.update({pilots.SEL_ESC1: 2, pilots.SEL_ESC2: 3})
    b.set_lut(lut)
    return b


def _outputs(b, frozen=True):
    """the sampler on a fixed block (keyed by explicit uniforms) and the greedy forward of the frozen slots, with logits; vf where every
    loaded slot has a value branch (hh_policy_sample refuses it otherwise: the frozen slots have none)"""
    from hhmarl_2d_amd import pilots
    g = torch.Generator().manual_seed(3)
    obs = torch.randn((N, 2, 26), generator=g).cuda()
    u = torch.rand((N, 2, 4), generator=g, dtype=torch.float64).cuda()
    obs30 = torch.randn((N, 2, 30), generator=g).cuda()
    out = []
    if frozen:
        sel_e = torch.tensor([pilots.SEL_ESC1, pilots.SEL_ESC2], dtype=torch.uint8).repeat(N, 1).contiguous().cuda()
        lg_e = torch.zeros((N, 2, 32), device="cuda")
        out += [b.act(obs30, sel_e, logits=lg_e), lg_e]
    sel = torch.tensor([pilots.SEL_FIGHT1, pilots.SEL_FIGHT2], dtype=torch.uint8).repeat(N, 1).contiguous().cuda()
    lg = torch.zeros((N, 2, 32), device="cuda")
    out += [x for x in b.sample(obs, sel, uniforms=u, logits=lg, want_vf=not frozen) if x is not None] + [lg]
    out += [x.clone() for x in b.sample(obs, None, uniforms=u, want_vf=not frozen) if x is not None]   # sel = NULL: the row lists of the call before
    torch.cuda.synchronize()
    return [x.cpu() for x in out]


def _parts(b):
    return [b.packed(s, p).cpu() for s in sorted(b.kinds) for p in range(5 if s in b._critics else 3)]


def _refresh_with_other_weights(b, seed):
    from hhmarl_2d_amd import pilots, policy_nets as PN
    sds = pilots.tie_shared_layer([PN.random_weights(k, seed) for k in (PN.FIGHT1, PN.FIGHT2)])
    b.refresh_trainable([_cuda(dict(sd, **PN.random_critic_weights(k, seed))) for k, sd in zip((PN.FIGHT1, PN.FIGHT2), sds)])
    for slot in (2, 3):
        if slot in b.kinds:
            b.refresh(slot, _cuda(PN.random_weights(b.kinds[slot], seed)))


def _equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("frozen", [True, False])
def test_bank_snapshot_refresh_restore(frozen):
    b = _bank(frozen=frozen)
    _outputs = lambda bank: globals()["_outputs"](bank, frozen)
    want, parts = _outputs(b), _parts(b)
    assert frozen or (want[2].dtype == torch.float32 and tuple(want[2].shape) == (N, 2)), "the trainable slots alone: vf is among the outputs"
    blob = b.snapshot()
    assert bytes(blob[:4].tolist()) == b"HHSP" and blob.device.type == "cpu" and blob.dtype == torch.uint8
    assert torch.equal(b.snapshot(), blob), "the same state gives the same bytes"
    gen = b.generation
    _refresh_with_other_weights(b, 77)
    assert not _equal(_outputs(b), want) and not _equal(_parts(b), parts), "the refresh changed what the bank computes"
    b.restore(blob)
    assert b.generation == gen, "in place: no address a captured graph holds has changed"
    assert _equal(_parts(b), parts), "every packed part is byte for byte what it was"
    assert _equal(_outputs(b), want), "actions, logp, vf and logits are bitwise what they were"


def test_bank_restore_into_a_fresh_bank_and_sel_null_reuse():
    from hhmarl_2d_amd import pilots
    b = _bank()
    want = _outputs(b)
    sd = b.state_dict()
    fresh = _bank(seed=9)                       # the same layout, other weights
    assert not _equal(_outputs(fresh), want)
    fresh2 = _bank(seed=9)
    fresh2.load_state_dict(sd)
    assert _equal(_parts(fresh2), _parts(b))
    # the row lists travel with the blob: a sel = NULL call right after the load re-uses the saved lists
    g = torch.Generator().manual_seed(3)
    obs = torch.randn((N, 2, 26), generator=g).cuda()
    u = torch.rand((N, 2, 4), generator=g, dtype=torch.float64).cuda()
    got = [x.cpu() for x in fresh2.sample(obs, None, uniforms=u, want_vf=False)[:2]]
    # (the saved lists are those of the sampler's call with selectors, the last one that binned before the save)
    ref = [x.cpu() for x in b.sample(obs, None, uniforms=u, want_vf=False)[:2]]
    assert _equal(got, ref)
    assert _equal(_outputs(fresh2), want)
    assert np.array_equal(fresh2._lut, b._lut) and fresh2._lut[pilots.SEL_ESC2] == 4


def test_bank_of_another_slot_layout_is_refused_and_unchanged():
    from hhmarl_2d_amd import _lib as L, policy_nets as PN
    b = _bank()
    blob, sd = b.snapshot(), b.state_dict()
    others = {"no frozen slots": _bank(frozen=False), "another max_rows": _bank(max_rows=2 * N + 2)}
    k = _bank()
    k.set_net(3, PN.ESC1, PN.random_weights(PN.ESC1, 1))     # slot 3 holds another kind
    others["another kind in a slot"] = k
    c = _bank()
    c.set_net(1, PN.FIGHT2, PN.random_weights(PN.FIGHT2, 5))  # slot 1's value branch is invalidated (set_net without set_critic)
    others["a value branch on one side only"] = c
    for what, o in others.items():
        frozen, can_sample = 2 in o.kinds, what != "a value branch on one side only"      # (its sampler refuses vf until set_critic)
        before = _outputs(o, frozen) if can_sample else None
        parts, own = _parts(o), o.snapshot()
        rc = L.lib().hh_policy_restore(o.h, C.c_void_p(blob.data_ptr()), blob.numel(), None)
        assert rc == -1, what
        assert L.lib().hh_last_error().decode().startswith("hh_policy_restore: "), what
        with pytest.raises(ValueError):
            o.restore(blob)
        with pytest.raises(ValueError, match="PolicyBank"):
            o.load_state_dict(sd)
        assert torch.equal(o.snapshot(), own) and _equal(_parts(o), parts), f"{what}: nothing was written"
        if can_sample:
            assert _equal(_outputs(o, frozen), before), what
    for bad, match in ((blob[:blob.numel() // 2].clone(), "truncated|shorter"), (torch.cat([torch.zeros(4, dtype=torch.uint8), blob[4:]]), "magic")):
        before = _parts(b)
        with pytest.raises(ValueError, match=match):
            b.restore(bad)
        assert _equal(_parts(b), before)
    with pytest.raises(ValueError, match="`slots` was"):
        others["no frozen slots"].load_state_dict(sd)
    with pytest.raises(ValueError, match="`max_rows` was"):
        others["another max_rows"].load_state_dict(sd)


def _commander(seed):
    from hhmarl_2d_amd import commander as CM
    return CM.CommanderNet(0, 3 * N).set_weights(CM.random_weights(seed))


def _commander_outputs(net):
    g = torch.Generator().manual_seed(4)
    obs = torch.randn((N, 3, 34), generator=g).cuda()
    h_in = (0.1 * torch.randn((N, 3, 2, 200), generator=g)).cuda()
    u = torch.rand((N, 3), generator=g, dtype=torch.float64).cuda()
    h_out, lg = torch.zeros_like(h_in), torch.zeros((N, 3, 4), device="cuda")
    act, logp, vf = net.sample(obs, h_in, h_out, uniforms=u, logits=lg)
    chain = net.act_chain(obs)
    torch.cuda.synchronize()
    return [x.cpu() for x in (act, logp, vf, lg, h_out, chain)]


def test_commander_snapshot_refresh_restore():
    from hhmarl_2d_amd import commander as CM
    net = _commander(6)
    want, parts = _commander_outputs(net), [net.packed(p).cpu() for p in (0, 1)]
    blob = net.snapshot()
    assert bytes(blob[:4].tolist()) == b"HHSC"
    net.refresh_weights(_cuda(CM.random_weights(7)))
    assert not _equal(_commander_outputs(net), want)
    net.restore(blob)
    assert _equal([net.packed(p).cpu() for p in (0, 1)], parts) and _equal(_commander_outputs(net), want)
    other = _commander(8)
    other.load_state_dict({"blob": blob})
    assert _equal(_commander_outputs(other), want) and torch.equal(other.state_dict()["blob"], blob)


def test_commander_refusals_leave_the_net_unchanged():
    from hhmarl_2d_amd import _lib as L, commander as CM
    net = _commander(6)
    blob, want = net.snapshot(), _commander_outputs(net)
    empty = CM.CommanderNet(0, 3 * N)            # no weights loaded: nothing to restore into
    rc = L.lib().hh_commander_restore(empty.h, C.c_void_p(blob.data_ptr()), blob.numel(), None)
    assert rc == -1 and L.lib().hh_last_error().decode().startswith("hh_commander_restore: ")
    with pytest.raises(ValueError):
        empty.load_state_dict({"blob": blob})
    bank_blob = _bank(frozen=False).snapshot()
    for bad in (blob[:blob.numel() - 64].clone(), bank_blob, torch.cat([blob[:4], torch.full((4,), 9, dtype=torch.uint8), blob[8:]])):
        with pytest.raises(ValueError):
            net.restore(bad)
        with pytest.raises(ValueError):
            net.load_state_dict({"blob": bad})
        assert torch.equal(net.snapshot(), blob) and _equal(_commander_outputs(net), want)
