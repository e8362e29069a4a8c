"""What tests/test_gpu_heads_loss.py and tests/test_gpu_learner_heads.py rely on, shown without a GPU: every table of
tests/heads_loss_ref.py keeps every unmasked row away from every kink (so no row has to be left out of a comparison), the float32
restatement's error is positive and representative on every case, the masked rows of the restatement are inert, and
learner.heads_loss_torch is autograd through TrainableNet.forward / CommanderTrainable.forward + ppo_loss_torch in float64 — the gradients
of every head parameter and of za, zc, for all three instances."""
import pytest
import torch

import heads_loss_ref as H

NC = pytest.mark.parametrize("n_comp", H.INSTANCES)


def test_geometry_and_row_counts():
    for n_comp in H.INSTANCES:
        tile, one = H.geometry(1, n_comp)
        assert tile >= 2 and one == 1
        counts = H.row_counts(n_comp)
        assert {1, tile - 1, tile, tile + 1, 280, 5003} <= set(counts)
        cap = H.geometry(1 << 30, n_comp)[1]
        assert H.geometry(cap * tile, n_comp)[1] == cap and (cap + 1) * tile in counts
        for R in counts:
            t, w = H.geometry(R, n_comp)
            assert t == tile and w == min((R + tile - 1) // tile, cap)


@pytest.mark.parametrize("n_comp,R,masked", H.grid())
def test_every_table_stays_clear_of_every_kink(n_comp, R, masked):
    inp, want, e32 = H.case(n_comp, R, masked)
    k = H.kw()
    d_ratio, d_sq, d_min = H.kink_distances(want, k)
    assert len(d_ratio) == H.n_valid_of(inp) >= 1
    print(f"n_comp={n_comp} R={R} masked={masked}: least distance to a kink: ratio {d_ratio.min():.3e}, value {d_sq.min():.3e}, min {d_min.min():.3e}")
    assert d_ratio.min() >= H.KINK_MARGIN and d_sq.min() >= H.KINK_MARGIN and d_min.min() >= H.KINK_MARGIN
    assert H.representative(inp, want, e32, H.restate(inp, torch.float32, n_comp, k), k)
    # positive wherever the float64 quantity is not identically zero (a single row beyond the value clip has no value gradient at all)
    assert all(e32[key] > 0.0 for key in H.QUANTITIES[1:] if want[key].abs().max() > 0) and e32["stats"] > 0.0
    if R >= 280:                                             # both sides of the clip range and of the value clip occur
        a = want["aux"]
        assert (a["ratio"] > 1 + H.CLIP).any() and (a["ratio"] < 1 - H.CLIP).any() and ((a["ratio"] > 1 - H.CLIP) & (a["ratio"] < 1 + H.CLIP)).any()
        assert (a["sq"] > k["vf_clip_param"]).any() and (a["sq"] < k["vf_clip_param"]).any()


@NC
def test_masked_tile_table(n_comp):
    zero, _, e32, nan = H.masked_tile_case(n_comp)
    assert all(e32[key] > 0.0 for key in H.QUANTITIES)
    tile, _ = H.geometry(1, n_comp)
    assert not zero["mask"][tile:2 * tile].any() and zero["mask"][:tile].any() and zero["mask"][2 * tile:].any()
    off = ~nan["mask"]
    assert all(torch.isnan(nan[key][off]).all() for key in H.ROW_KEYS if nan[key].dtype == torch.float32)
    k = H.kw()
    a, b = H.restate(zero, torch.float64, n_comp, k), H.restate(nan, torch.float64, n_comp, k)
    assert a["stats"] == b["stats"] and all(torch.equal(a[key], b[key]) for key in H.QUANTITIES[1:])
    assert all(torch.isfinite(b[key]).all() for key in H.QUANTITIES[1:])
    assert torch.equal(b["d_za"][off], torch.zeros_like(b["d_za"][off])) and (b["d_za"][~off] != 0).any(dim=1).all()
    d = H.kink_distances(a, k)
    assert min(x.min().item() for x in d) >= H.KINK_MARGIN


@NC
def test_reorder_bound_is_far_below_the_float32_error(n_comp):
    """the bound the equivalence test falls back on is a float64 reordering bound: at least three orders of magnitude under e32"""
    inp, want, e32 = H.case(n_comp, 5003, True)
    bound = H.stats_reorder_bound(want, H.kw())
    assert all(b > 0.0 for b in bound) and max(bound) < 1e-3 * e32["stats"]


def _module_case(kind, seed=4):
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    g = torch.Generator().manual_seed(seed)
    R = 37
    if kind is None:
        m = LR.CommanderTrainable(heads="fused").double()
        S, Lc = 3, 6
        seq_len = torch.tensor([6, 4, 1], dtype=torch.int32)
        args = (torch.rand((S, Lc, 34), generator=g).double(), torch.rand((S, Lc, 105), generator=g).double(),
                0.3 * torch.randn((S, 2, 200), generator=g).double(), seq_len)
        kwargs = dict(fused_gru=False)
        lead, n_comp = (S, Lc), 1
        batch = {"old_logits": torch.randn(lead + (4,), generator=g), "actions": torch.randint(0, 3, lead, generator=g).to(torch.int8),
                 "mask": LR.chunk_mask(seq_len, Lc)}
    else:
        m = LR.TrainableNet(kind, heads="fused").double()
        d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
        args = (torch.rand((R, PN.OBS_DIM[kind]), generator=g).double(), torch.rand((R, d1 + a1 + d2 + a2), generator=g).double())
        kwargs = {}
        lead, n_comp = (R,), LR.n_comp_of(kind)
        act = torch.zeros(lead + (4,), dtype=torch.int8)
        for i, wd in enumerate(PN.ACTION_SPLIT[:n_comp]):
            act[..., i] = torch.randint(0, wd, lead, generator=g).to(torch.int8)
        batch = {"old_logits": torch.randn(lead + (32,), generator=g), "actions": act, "mask": torch.rand(lead, generator=g) < 0.8}
    batch.update(old_logp=-3.0 + 0.3 * torch.randn(lead, generator=g), adv=torch.randn(lead, generator=g), target=torch.randn(lead, generator=g))
    return LR, m, args, kwargs, batch, n_comp


@pytest.mark.parametrize("kind", (0, 1, 2, 3, None), ids=("Fight1", "Fight2", "Esc1", "Esc2", "commander"))
def test_heads_loss_torch_is_forward_plus_loss(kind):
    """float64 on the CPU: pre_heads + heads_loss_torch against forward + ppo_loss_torch — the statistics, every parameter's gradient, and
    the gradients of za and zc against those that autograd delivers at shared_layer's outputs in the plain run"""
    LR, m, args, kwargs, batch, n_comp = _module_case(kind)
    k = dict(clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)
    m.zero_grad(set_to_none=True)
    za, zc = m.pre_heads(*args, **kwargs)
    za.retain_grad(), zc.retain_grad()
    total, stats = LR.heads_loss_torch(za, zc, m.act_out, m.val_out, batch, n_comp=n_comp, **k)
    total.backward()
    got = {key: p.grad.clone() for key, p in m.named_parameters()}
    d_za, d_zc = za.grad.clone(), zc.grad.clone()
    # the plain run, with a hook on shared_layer that keeps the gradient of its two outputs
    m.zero_grad(set_to_none=True)
    kept = []

    def keep(module, inputs, output):
        output.retain_grad()
        kept.append(output)
    handle = m.shared_layer.register_forward_hook(keep)
    logits, vf = m(*args, **kwargs)
    handle.remove()
    loss = LR.ppo_loss_categorical_torch if n_comp == 1 else (lambda lg, v, b, **kk: LR.ppo_loss_torch(lg, v, b, n_comp=n_comp, **kk))
    total2, stats2 = loss(logits, vf, batch, **k)
    total2.backward()
    assert torch.allclose(stats, stats2, rtol=1e-13, atol=1e-15) and len(kept) == 2
    assert set(got) == {key for key, _ in m.named_parameters()}
    for key, p in m.named_parameters():
        assert torch.allclose(got[key], p.grad, rtol=1e-11, atol=1e-14), key
    assert got["act_out._model.0.weight"].abs().max() > 0 and got["val_out._model.0.weight"].abs().max() > 0
    assert torch.allclose(d_za, kept[0].grad.reshape(d_za.shape), rtol=1e-11, atol=1e-15)
    assert torch.allclose(d_zc, kept[1].grad.reshape(d_zc.shape), rtol=1e-11, atol=1e-15)
    assert d_za.abs().max() > 0 and d_zc.abs().max() > 0


@NC
def test_restatement_is_heads_loss_torch(n_comp):
    """the ref module's own restatement and learner.heads_loss_torch agree in float64 on a masked table (independent spellings)"""
    from hhmarl_2d_amd import learner as LR
    inp, want, _ = H.case(n_comp, 280, True)
    k = H.kw()
    leaf = lambda key: inp[key].double().clone().requires_grad_(True)
    za, zc, w_act, b_act, w_val, b_val = (leaf(key) for key in ("za", "zc") + H.WEIGHT_KEYS)
    batch = {key: inp[key] for key in ("old_logits", "actions", "old_logp", "adv", "target", "mask")}
    total, stats = LR.heads_loss_torch(za, zc, (w_act, b_act), (w_val, b_val), batch, n_comp=n_comp, **k)
    total.backward()
    assert max(abs(float(a) - b) for a, b in zip(stats[:5], want["stats"][:5])) < 1e-13 and float(stats[5]) == want["stats"][5]
    for key, t in zip(H.GRADS, (za, zc, w_act, b_act, w_val, b_val)):
        assert torch.allclose(t.grad, want[key].reshape(t.shape), rtol=1e-10, atol=1e-16), key


def test_options_are_validated_without_a_gpu():
    from hhmarl_2d_amd import learner as LR
    assert LR.TrainableNet(0).heads == "torch" and LR.CommanderTrainable().heads == "torch" and LR.HEADS_MODES == ("torch", "fused")
    assert list(LR.TrainableNet(0, heads="fused").state_dict()) == list(LR.TrainableNet(0).state_dict())
    assert list(LR.CommanderTrainable(heads="fused").state_dict()) == list(LR.CommanderTrainable().state_dict())
    for make in (lambda **kw: LR.TrainableNet(2, **kw), LR.CommanderTrainable):
        with pytest.raises(ValueError, match="heads"):
            make(heads="hip")
        with pytest.raises(ValueError, match="heads"):
            make(heads="fused", trunk="fused")
    sd = {}
    for make in (lambda **kw: LR.PPOLearner((0, 1), (sd, sd), "cuda:0", **kw), lambda **kw: LR.CommanderLearner(sd, "cuda:0", **kw)):
        with pytest.raises(ValueError, match="heads"):
            make(heads="hip")
        with pytest.raises(ValueError, match="heads"):
            make(heads="fused", trunk="fused")
        with pytest.raises(ValueError, match="heads"):
            make(heads="fused", fused=False)
