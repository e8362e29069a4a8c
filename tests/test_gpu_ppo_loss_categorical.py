"""hh_ppo_loss_categorical on the MI355X (include/hh_learner.h) against a float64 restatement of the header's formulas written here, at
the tolerances tests/test_gpu_ppo_loss.py holds hh_ppo_loss to: e32 = the largest error of the same restatement in float32 against the
float64 one, per compared quantity (the five statistics together; d_logits; d_vf), and the kernel may be at most 4 x e32 away.  Rows
within 1e-4 of a clip boundary of the ratio or within 1e-3 of vf_clip_param in the squared value error are left out of the gradient
comparison (min and clamp make it discontinuous there)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
CLIP, VCLIP = 0.25, 10.0
CASES = [(R, masked, klc, ec) for R in (1, 63, 4096, 100003) for masked in (False, True) for klc in (0.0, 0.2) for ec in (0.0, 0.01)]


def make_inputs(R, masked, seed):
    """logits near the sampler's, ratios on both sides of the clip range (advantages of both signs), value errors on both sides of vf_clip"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((R, 4), generator=g)
    logits[:, 3] = 7.0                                   # the ignored column holds junk
    old = torch.zeros((R, 4))
    old[:, :3] = logits[:, :3] + 0.4 * torch.randn((R, 3), generator=g)
    actions = torch.randint(0, 3, (R,), generator=g).to(torch.int8)
    old_logp = torch.log_softmax(old[:, :3].double(), dim=1).gather(1, actions.long()[:, None])[:, 0].float()
    adv, target = torch.randn((R,), generator=g), 2.0 * torch.randn((R,), generator=g)
    vf = target + 3.0 * torch.randn((R,), generator=g)
    mask = None
    if masked:
        mask = torch.rand((R,), generator=g) < 0.8
        mask[0] = True
    return dict(logits=logits, vf=vf, old_logits=old, actions=actions, old_logp=old_logp, adv=adv, target=target, mask=mask)


def restatement(inp, dtype, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """-> (stats [6], d_logits [R, 4], d_vf [R], ratio, squared value error)"""
    logits = inp["logits"].to(dtype).clone().requires_grad_(True)
    vf = inp["vf"].to(dtype).clone().requires_grad_(True)
    x, y = logits[:, :3], inp["old_logits"][:, :3].to(dtype)
    lp = x - torch.logsumexp(x, dim=1, keepdim=True)
    lq = y - torch.logsumexp(y, dim=1, keepdim=True)
    logp = lp.gather(1, inp["actions"].long()[:, None])[:, 0]
    ratio = torch.exp(logp - inp["old_logp"].to(dtype))
    A = inp["adv"].to(dtype)
    surr = torch.min(A * ratio, A * torch.clamp(ratio, 1 - clip_param, 1 + clip_param))
    kl = (lq.exp() * (lq - lp)).sum(dim=1)
    ent = -(lp.exp() * lp).sum(dim=1)
    sq = (vf - inp["target"].to(dtype)) ** 2
    vl = torch.clamp(sq, 0, vf_clip_param)
    w = torch.ones_like(ratio) if inp["mask"] is None else inp["mask"].to(dtype)
    n = w.sum()
    mean = lambda t: (t * w).sum() / n
    total = mean(-surr + vf_loss_coeff * vl - entropy_coeff * ent)
    mkl = mean(kl) if kl_coeff > 0 else torch.zeros((), dtype=dtype)
    if kl_coeff > 0:
        total = total + kl_coeff * mkl
    total.backward()
    stats = [float(v) for v in (total, mean(-surr), mean(vl), mkl, mean(ent), n)]
    return stats, logits.grad, vf.grad, ratio.detach(), sq.detach()


def _kernel(inp, kw):
    from hhmarl_2d_amd import learner as LR
    logits, vf = inp["logits"].cuda().requires_grad_(True), inp["vf"].cuda().requires_grad_(True)
    b = {k: inp[k].cuda() for k in ("old_logits", "actions", "old_logp", "adv", "target")}
    if inp["mask"] is not None:
        b["mask"] = inp["mask"].cuda()
    total, stats = LR.ppo_loss_categorical(logits, vf, b, **kw)
    total.backward()
    torch.cuda.synchronize()
    return stats.cpu(), logits.grad.cpu(), vf.grad.cpu(), total.item()


@pytest.mark.parametrize("R,masked,klc,ec", CASES)
def test_kernel_against_float64_restatement(R, masked, klc, ec):
    kw = dict(clip_param=CLIP, vf_clip_param=VCLIP, vf_loss_coeff=1.0, entropy_coeff=ec, kl_coeff=klc)
    inp = make_inputs(R, masked, R % 97)
    ws, wdl, wdv, ratio, sq = restatement(inp, torch.float64, **kw)
    s32, dl32, dv32, _, _ = restatement(inp, torch.float32, **kw)
    keep = ~(((ratio - (1 - CLIP)).abs() < 1e-4) | ((ratio - (1 + CLIP)).abs() < 1e-4) | ((sq - VCLIP).abs() < 1e-3))
    assert (~keep).sum().item() <= 0.01 * R
    if R >= 4096:   # the cases hold clipped and unclipped ratios and value errors
        assert ((ratio < 1 - CLIP) | (ratio > 1 + CLIP)).float().mean() > 0.05 and ((ratio - 1).abs() < CLIP).float().mean() > 0.3
        assert (sq > VCLIP).float().mean() > 0.05
    stats, dl, dv, total = _kernel(inp, kw)
    assert torch.isfinite(stats).all() and torch.isfinite(dl).all() and torch.isfinite(dv).all()
    assert stats[5].item() == ws[5] and abs(total - stats[0].item()) <= 1e-6 * max(1.0, abs(total))
    assert torch.equal(dl[:, 3], torch.zeros(R))                       # exactly zero: the ignored column
    if masked:
        off = ~inp["mask"]
        assert torch.equal(dl[off], torch.zeros((int(off.sum()), 4))) and torch.equal(dv[off], torch.zeros(int(off.sum())))
    if klc == 0.0:
        assert stats[3].item() == 0.0

    def errors(s, a, b):
        e_s = max(abs(float(x) - y) for x, y in zip(s[:5], ws[:5]))
        return e_s, (a.double()[keep] - wdl[keep]).abs().max().item() if keep.any() else 0.0, (b.double()[keep] - wdv[keep]).abs().max().item() if keep.any() else 0.0
    e32, err = errors(s32, dl32, dv32), errors(stats, dl, dv)
    print(f"R={R} masked={masked} kl_coeff={klc} entropy_coeff={ec}: e32 (stats, d_logits, d_vf) = {e32[0]:.3e} {e32[1]:.3e} {e32[2]:.3e}; "
          f"kernel = {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}")
    for name, e, b in zip(("stats", "d_logits", "d_vf"), err, e32):
        assert e <= 4.0 * b, f"{name}: kernel error {e:.3e} above 4 x e32 = {4 * b:.3e}"


def test_same_bytes_every_run_and_the_torch_form_agrees():
    from hhmarl_2d_amd import learner as LR
    kw = dict(clip_param=CLIP, vf_clip_param=VCLIP, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)
    inp = make_inputs(100003, True, 5)
    a, b = _kernel(inp, kw), _kernel(inp, kw)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    batch = {k: inp[k].cuda() for k in ("old_logits", "actions", "old_logp", "adv", "target", "mask")}
    _, st = LR.ppo_loss_categorical_torch(inp["logits"].cuda()[:, :3], inp["vf"].cuda(), batch, **kw)
    assert (st.cpu() - a[0]).abs()[:5].max().item() <= 1e-4


def test_gradients_under_an_upstream_gradient_of_one_half():
    """learner.ppo_loss_categorical under (0.5 * total).backward() — _kernel only ever sends an upstream gradient of exactly 1 — on the
    smallest shape that reaches the pad-to-4 path ([3, 4, 3] logits, a mask): the gradients of logits and vf are exactly half those of
    total.backward() and agree with learner.ppo_loss_categorical_torch's under the same upstream gradient within the 1e-4 that
    test_same_bytes_every_run_and_the_torch_form_agrees holds the two forms to."""
    from hhmarl_2d_amd import learner as LR
    kw = dict(clip_param=CLIP, vf_clip_param=VCLIP, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)
    inp = make_inputs(12, True, 7)
    shaped = lambda t: t.reshape((3, 4) + tuple(t.shape[1:])).cuda()
    batch = {k: shaped(inp[k]) for k in ("old_logits", "actions", "old_logp", "adv", "target", "mask")}

    def grads(loss_fn, upstream):
        logits, vf = shaped(inp["logits"][:, :3]).requires_grad_(True), shaped(inp["vf"]).requires_grad_(True)
        total, _ = loss_fn(logits, vf, batch, **kw)
        (upstream * total).backward()
        assert logits.grad.shape == (3, 4, 3) and vf.grad.shape == (3, 4)
        return logits.grad, vf.grad

    fused, torch_form, one = grads(LR.ppo_loss_categorical, 0.5), grads(LR.ppo_loss_categorical_torch, 0.5), grads(LR.ppo_loss_categorical, 1.0)
    assert all(torch.isfinite(g).all() for g in fused) and fused[0].abs().max().item() > 0 and fused[1].abs().max().item() > 0
    assert torch.equal(2.0 * fused[0], one[0]) and torch.equal(2.0 * fused[1], one[1])
    err = [(a - b).abs().max().item() for a, b in zip(fused, torch_form)]
    print(f"upstream 0.5: fused against the torch form, d_logits {err[0]:.3e}, d_vf {err[1]:.3e}")
    assert max(err) <= 1e-4


def test_bad_arguments_are_refused():
    import ctypes as C
    from hhmarl_2d_amd import _lib as L
    lib = L.lib()
    R = 63
    inp = make_inputs(R, False, 0)
    t = {k: v.cuda().contiguous() for k, v in inp.items() if v is not None}
    n_valid = torch.tensor([R], dtype=torch.int32, device="cuda")
    stats, dl, dv = torch.empty(6, dtype=torch.float64, device="cuda"), torch.empty((R, 4), device="cuda"), torch.empty(R, device="cuda")
    scratch = torch.empty(4, dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(n_comp=1, nbytes=32, logits=p(t["logits"])):
        prm = L.HHPpoLossParams(n_comp=n_comp, reserved0=0, clip_param=CLIP, vf_clip_param=VCLIP, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2,
                                reserved1=0.0)
        return lib.hh_ppo_loss_categorical(R, logits, p(t["old_logits"]), p(t["actions"]), p(t["old_logp"]), p(t["adv"]), p(t["vf"]), p(t["target"]),
                                           None, p(n_valid), C.byref(prm), p(stats), p(dl), p(dv), p(scratch), nbytes, st)
    assert call() == 0
    assert call(n_comp=3) == -1 and call(n_comp=4) == -1 and call(nbytes=8) == -1 and call(logits=None) == -1
    assert call(logits=C.c_void_p(t["logits"].data_ptr() + 4)) == -1
    assert b"hh_ppo_loss_categorical" in lib.hh_last_error()
    torch.cuda.synchronize()
