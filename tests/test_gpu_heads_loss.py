"""hh_heads_loss on the MI355X through the C ABI, its three instances (n_comp 4, 3 and 1), on the tables of tests/heads_loss_ref.py: row
counts at the edges of the geometry the library reports (one row, either side of a tile, one tile more than a full round of the
workgroups, 280 and about 5000 rows), a ragged mask, a whole masked tile with NaN in every input, n_valid = 0, the equivalence with
hh_ppo_loss / hh_ppo_loss_categorical on the very logits and values the call wrote, determinism, guards around every output, and the
refusals.

The bound is the project's: e32 = the error of the float32 restatement against the float64 one on the same inputs, per compared quantity
(the five statistics together; d_za; d_zc; d_w_act; d_b_act; d_w_val; d_b_val; logits; vf), and the kernel may be at most 4 x e32 away
from float64.  No row is left out of any comparison; tests/test_heads_loss_host.py shows that none has to be.  Every call runs on
outputs that are views into sentinel-filled buffers and checks the guards and all inputs bitwise afterwards."""
import ctypes as C

import pytest
import torch

import heads_loss_ref as H

pytestmark = pytest.mark.gpu
NC = pytest.mark.parametrize("n_comp", H.INSTANCES)
SENT = -12345.678
GUARD = 16                       # elements either side of an output: 64 B of floats, 128 B of doubles, so the views keep 16-byte alignment
IN_KEYS = ("za", "zc") + H.WEIGHT_KEYS + ("old_logits", "actions", "old_logp", "adv", "target", "mask", "n_valid")
OUT_KEYS = ("stats",) + H.GRADS + ("logits", "vf", "scratch")
OPTIONAL = ("mask", "logits", "vf")


def bits(x):
    return x.contiguous().view({8: torch.int64, 4: torch.int32, 1: torch.int8}[x.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Run:
    """one call of the C ABI on device buffers: outputs are views into sentinel-filled buffers, inputs are kept for a bitwise check"""

    def __init__(self, inp, n_comp, k, n_valid=None, want_heads=True):
        from hhmarl_2d_amd import _lib as L
        dev = torch.device("cuda", 0)
        self.L, self.n_comp, self.R = L, n_comp, inp["za"].shape[0]
        R, n_out = self.R, H.N_OUT[n_comp]
        host = {key: inp[key].contiguous() for key in H.ROW_KEYS + H.WEIGHT_KEYS}
        host["mask"] = None if inp["mask"] is None else inp["mask"].to(torch.uint8)
        host["n_valid"] = torch.tensor([H.n_valid_of(inp) if n_valid is None else n_valid], dtype=torch.int32)
        self.host = host
        self.t = {key: (None if v is None else v.to(dev)) for key, v in host.items()}
        self.prm = L.HHPpoLossParams(n_comp=n_comp, reserved0=0, clip_param=k["clip_param"], vf_clip_param=k["vf_clip_param"],
                                     vf_loss_coeff=k["vf_loss_coeff"], entropy_coeff=k["entropy_coeff"], kl_coeff=k["kl_coeff"], reserved1=0.0)
        nb = C.c_int64()
        L.check(L.lib().hh_heads_loss_scratch_bytes(R, n_comp, C.byref(nb)))
        self.nb = nb.value
        _, wgs = H.geometry(R, n_comp)
        assert self.nb == wgs * ((4 + n_out + 1) * 8 + (n_out + 1) * H.K * 4)
        sizes = {"stats": (6, torch.float64), "d_za": (R * H.K, torch.float32), "d_zc": (R * H.K, torch.float32),
                 "d_w_act": (n_out * H.K, torch.float32), "d_b_act": (n_out, torch.float32), "d_w_val": (H.K, torch.float32),
                 "d_b_val": (1, torch.float32), "logits": (R * n_out, torch.float32), "vf": (R, torch.float32),
                 "scratch": (self.nb // 8, torch.float64)}
        self.big = {key: torch.full((n + 2 * GUARD,), SENT, dtype=dt, device=dev) for key, (n, dt) in sizes.items()}
        self.out = {key: self.big[key][GUARD:GUARD + n] for key, (n, _) in sizes.items()}
        self.null = set() if want_heads else {"logits", "vf"}    # names passed as NULL
        self.ptr_off = {}                                         # name -> bytes added to the pointer passed
        self.n_rows = R

    def run(self):
        def p(name):
            x = self.out[name] if name in self.out else self.t[name]
            return None if x is None or name in self.null else C.c_void_p(x.data_ptr() + self.ptr_off.get(name, 0))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return self.L.lib().hh_heads_loss(self.n_rows, *[p(key) for key in IN_KEYS], C.byref(self.prm), *[p(key) for key in OUT_KEYS], self.nb, st)

    def outputs(self):
        """-> dict of the outputs on the host, after checking the guards and the inputs"""
        torch.cuda.synchronize()
        for key, big in self.big.items():
            g = torch.cat([big[:GUARD], big[-GUARD:]]).cpu()
            assert torch.equal(g, torch.full_like(g, SENT)), f"{key}: a guard element was overwritten"
        for key, v in self.host.items():
            if v is not None:
                assert same_bits(self.t[key].cpu(), v), f"input {key} was modified"
        R, n_out = self.R, H.N_OUT[self.n_comp]
        shape = {"d_za": (R, H.K), "d_zc": (R, H.K), "d_w_act": (n_out, H.K), "d_w_val": (1, H.K), "logits": (R, n_out)}
        out = {key: self.out[key].cpu().clone().reshape(shape.get(key, (-1,))) for key in OUT_KEYS[:-1]}
        for key in self.null:
            assert torch.equal(out[key], torch.full_like(out[key], SENT)), f"{key} was written though NULL was passed"
            out[key] = None
        return out

    def untouched(self):
        torch.cuda.synchronize()
        return all(torch.equal(b.cpu(), torch.full_like(b.cpu(), SENT)) for b in self.big.values())


def call(inp, n_comp, k, **kwargs):
    r = Run(inp, n_comp, k, **kwargs)
    assert r.run() == 0, r.L.lib().hh_last_error()
    return r.outputs()


def finite(out):
    return all(torch.isfinite(v).all() for v in out.values() if v is not None)


def hold_to_rule(label, got, want, e32):
    """print every (e32, kernel) pair, then: the kernel at most 4 x e32 from float64, per quantity"""
    err = H.errors(got, want)
    print(f"{label}: " + "; ".join(f"{key} e32 {e32[key]:.3e} kernel {err[key]:.3e}" for key in H.QUANTITIES))
    for key in H.QUANTITIES:
        assert err[key] <= 4.0 * e32[key], f"{label} {key}: kernel error {err[key]:.3e} above 4 x e32 = {4 * e32[key]:.3e}"


def exact_zeros(inp, out):
    """the masked rows of d_za and d_zc (and of the optional logits and vf) are exactly zero"""
    if inp["mask"] is not None:
        off = ~inp["mask"]
        for key in ("d_za", "d_zc", "logits", "vf"):
            if out[key] is not None:
                assert torch.equal(out[key][off], torch.zeros_like(out[key][off])), key


@pytest.mark.parametrize("n_comp,R,masked", H.grid(), ids=[f"n{n}-R{R}-{'m' if m else 'u'}" for n, R, m in H.grid()])
def test_grid(n_comp, R, masked):
    inp, want, e32 = H.case(n_comp, R, masked)
    out = call(inp, n_comp, H.kw())
    assert finite(out) and out["stats"][5].item() == want["stats"][5] == H.n_valid_of(inp)
    exact_zeros(inp, out)
    hold_to_rule(f"grid n_comp={n_comp} R={R} masked={masked}", out, want, e32)


@NC
def test_without_kl_term_and_without_the_optional_outputs(n_comp):
    inp, want, e32 = H.case(n_comp, 280, True, 0.0)
    out = call(inp, n_comp, H.kw(0.0), want_heads=False)
    assert out["logits"] is None and out["vf"] is None and out["stats"][3].item() == 0.0
    full = call(inp, n_comp, H.kw(0.0))
    assert all(same_bits(out[key], full[key]) for key in ("stats",) + H.GRADS)
    hold_to_rule(f"kl_coeff=0 n_comp={n_comp}", full, want, e32)


@NC
def test_whole_masked_tile_with_nan_in_every_input(n_comp):
    zero, want, e32, nan = H.masked_tile_case(n_comp)
    k = H.kw()
    a, b = call(zero, n_comp, k), call(nan, n_comp, k)
    assert finite(b) and all(same_bits(a[key], b[key]) for key in OUT_KEYS[:-1])
    exact_zeros(nan, b)
    hold_to_rule(f"masked tile n_comp={n_comp}", b, want, e32)


@NC
def test_n_valid_zero(n_comp):
    """every row masked, NaN in all of them: every gradient exactly 0.0f, stats as hh_ppo_loss documents"""
    tile, _ = H.geometry(1, n_comp)
    R = 2 * tile + 3
    inp = H.make_inputs(n_comp, R, True, 1, nan=True, mask=torch.zeros(R, dtype=torch.bool))
    for klc in (0.2, 0.0):
        out = call(inp, n_comp, H.kw(klc))
        for key in H.GRADS + ("logits", "vf"):
            assert torch.equal(out[key], torch.zeros_like(out[key])), key
        s = out["stats"]
        assert s[5].item() == 0.0 and torch.isnan(s[[0, 1, 2, 4]]).all() and (torch.isnan(s[3]) if klc > 0 else s[3].item() == 0.0)


@NC
def test_statistics_equal_those_of_the_loss_kernel_on_the_same_logits(n_comp):
    """hh_ppo_loss / hh_ppo_loss_categorical on the logits and values this call wrote: the same row terms by the same device code; the
    float64 sums run over other tiles, so the statistics agree bit for bit or within heads_loss_ref.stats_reorder_bound"""
    from hhmarl_2d_amd import _lib as L
    inp, want, _ = H.case(n_comp, 5003, True)
    k = H.kw()
    out = call(inp, n_comp, k)
    dev = torch.device("cuda", 0)
    R, n_out = inp["za"].shape[0], H.N_OUT[n_comp]
    ld = 4 if n_comp == 1 else n_out
    logits = torch.zeros((R, ld))
    logits[:, :n_out] = out["logits"]
    t = {key: inp[key].contiguous().to(dev) for key in ("old_logits", "actions", "old_logp", "adv", "target")}
    mask, n_valid = inp["mask"].to(torch.uint8).to(dev), torch.tensor([H.n_valid_of(inp)], dtype=torch.int32, device=dev)
    lg, vf = logits.to(dev), out["vf"].to(dev)
    stats, d_logits, d_vf = torch.zeros(6, dtype=torch.float64, device=dev), torch.empty_like(lg), torch.empty_like(vf)
    nb = C.c_int64()
    L.check(L.lib().hh_ppo_loss_scratch_bytes(R, C.byref(nb)))
    scratch = torch.empty(nb.value // 8, dtype=torch.float64, device=dev)
    prm = L.HHPpoLossParams(n_comp=n_comp, reserved0=0, clip_param=k["clip_param"], vf_clip_param=k["vf_clip_param"], vf_loss_coeff=k["vf_loss_coeff"],
                            entropy_coeff=k["entropy_coeff"], kl_coeff=k["kl_coeff"], reserved1=0.0)
    p = lambda x: C.c_void_p(x.data_ptr())
    rows = [p(lg), p(t["old_logits"]), p(t["actions"]), p(t["old_logp"]), p(t["adv"]), p(vf), p(t["target"]), p(mask), p(n_valid)]
    tail = [C.byref(prm), p(stats), p(d_logits), p(d_vf), p(scratch), nb.value, C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    L.check(L.lib().hh_ppo_loss_categorical(R, *rows, *tail) if n_comp == 1 else L.lib().hh_ppo_loss(R, ld, *rows, *tail))
    ref = stats.cpu()
    bound = H.stats_reorder_bound(want, k)
    diff = (out["stats"] - ref).abs()[:5].tolist()
    print(f"n_comp={n_comp}: bit-equal {same_bits(out['stats'], ref)}; |difference| {diff}; reordering bound {bound}")
    assert out["stats"][5].item() == ref[5].item()
    assert same_bits(out["stats"], ref) or all(d <= b for d, b in zip(diff, bound))
    # and the head gradients are what that kernel's d_logits and d_vf give: d_b_act and d_b_val are their float64 column sums
    assert torch.allclose(out["d_b_act"].double(), d_logits.cpu()[:, :n_out].double().sum(dim=0), rtol=1e-6, atol=1e-12)
    assert torch.allclose(out["d_b_val"].double(), d_vf.cpu().double().sum().reshape(1), rtol=1e-6, atol=1e-12)


@NC
def test_two_calls_give_the_same_bytes(n_comp):
    inp, _, _ = H.case(n_comp, 5003, True)
    a, b = call(inp, n_comp, H.kw()), call(inp, n_comp, H.kw())
    assert all(same_bits(a[key], b[key]) for key in OUT_KEYS[:-1])


@NC
def test_refusals_write_nothing(n_comp):
    inp, _, _ = H.case(n_comp, 280, True)
    k = H.kw()

    def refused(what, change):
        r = Run(inp, n_comp, k)
        change(r)
        assert r.run() == -1, what                               # HH_E_ARG
        assert b"hh_heads_loss" in r.L.lib().hh_last_error(), what
        assert r.untouched(), what

    for name in IN_KEYS + OUT_KEYS:
        if name not in OPTIONAL:
            refused(f"NULL {name}", lambda r, name=name: r.null.add(name))
    for name in ("za", "zc", "d_za", "d_zc"):
        for off in (4, 8):
            refused(f"{name} + {off} bytes", lambda r, name=name, off=off: r.ptr_off.update({name: off}))
    for bad in (0, 2, 5, -1):
        refused(f"n_comp = {bad}", lambda r, bad=bad: setattr(r.prm, "n_comp", bad))
    refused("reserved0", lambda r: setattr(r.prm, "reserved0", 1))
    refused("reserved1", lambda r: setattr(r.prm, "reserved1", 1.0))
    for bad in (0, -1):
        refused(f"n_rows = {bad}", lambda r, bad=bad: setattr(r, "n_rows", bad))
    refused("small scratch", lambda r: setattr(r, "nb", r.nb - 1))
    from hhmarl_2d_amd import _lib as L
    nb, tile, wgs = C.c_int64(7), C.c_int32(7), C.c_int32(7)
    for bad_rows, bad_comp in ((0, n_comp), (280, 2)):
        assert L.lib().hh_heads_loss_scratch_bytes(bad_rows, bad_comp, C.byref(nb)) == -1 and nb.value == 7
        assert L.lib().hh_heads_loss_geometry(bad_rows, bad_comp, C.byref(tile), C.byref(wgs)) == -1 and (tile.value, wgs.value) == (7, 7)
    assert call(inp, n_comp, k)["stats"][5].item() == H.n_valid_of(inp)      # and the unchanged call goes through
