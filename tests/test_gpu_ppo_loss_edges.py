"""hh_ppo_loss (n_comp 4 and 3) and hh_ppo_loss_categorical (n_comp 1 below) on the MI355X at their edges, on the tables of
tests/ppo_loss_edges_ref.py: row counts either side of the 256-row tile and of the final sum's 256 partials, every row width, rows placed
on and around the kinks of min and clamp, logits 200 apart and 8192 away from 0, out-of-range action bytes, whole masked tiles with NaN in
them, NaN in the ignored columns, guards around every output, and the refusals.

The bound is the project's: e32 = the largest error of the float32 restatement against the float64 one on the same inputs, per compared
quantity (the five statistics together; d_logits; d_vf), and the kernel may be at most 4 x e32 away from float64.  No row is left out of
any comparison; tests/test_ppo_loss_edges_host.py proves that none has to be.  Every call runs on outputs that are views into larger
sentinel-filled buffers and checks the sentinels and all nine inputs afterwards."""
import ctypes as C

import pytest
import torch

import ppo_loss_edges_ref as E

pytestmark = pytest.mark.gpu
NC = pytest.mark.parametrize("n_comp", E.INSTANCES)
SENT = -12345.678
GUARD = 16                       # floats (64 B) and doubles (128 B) either side of an output: offsets keep the 16-byte alignment rule
FN = {4: "hh_ppo_loss", 3: "hh_ppo_loss", 1: "hh_ppo_loss_categorical"}


def bits(x):
    return x.contiguous().view({8: torch.int64, 4: torch.int32, 1: torch.int8}[x.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Run:
    """one call of the C ABI on device buffers: outputs are views into sentinel-filled buffers, inputs are kept for a bitwise check"""

    def __init__(self, inp, n_comp, k, n_valid=None, act_off=0):
        from hhmarl_2d_amd import _lib as L
        dev = torch.device("cuda", 0)
        self.L, self.n_comp = L, n_comp
        R, ld = inp["logits"].shape
        self.R, self.ld = R, ld
        assert inp["old_logits"].shape == (R, E.OLD_LD[n_comp]) and inp["actions"].shape == ((R,) if n_comp == 1 else (R, 4))
        host = {key: inp[key].contiguous() for key in E.ROW_KEYS}
        host["mask"] = None if inp["mask"] is None else inp["mask"].to(torch.uint8)
        host["n_valid"] = torch.tensor([E.n_valid_of(inp) if n_valid is None else n_valid], dtype=torch.int32)
        self.host = host
        self.t = {key: (None if v is None else v.to(dev)) for key, v in host.items()}
        if act_off:                                   # the Categorical's actions at an odd address
            buf = torch.zeros(R + 8, dtype=torch.int8, device=dev)
            buf[act_off:act_off + R] = self.t["actions"]
            self.t["actions"] = buf[act_off:act_off + R]
            assert self.t["actions"].data_ptr() % 4 == act_off
        self.prm = L.HHPpoLossParams(n_comp=n_comp, reserved0=0, clip_param=k["clip_param"], vf_clip_param=k["vf_clip_param"],
                                     vf_loss_coeff=k["vf_loss_coeff"], entropy_coeff=k["entropy_coeff"], kl_coeff=k["kl_coeff"], reserved1=0.0)
        nb = C.c_int64()
        L.check(L.lib().hh_ppo_loss_scratch_bytes(R, C.byref(nb)))
        self.nb = nb.value
        assert self.nb == (R + 255) // 256 * 32
        sizes = {"d_logits": (R * ld, torch.float32), "d_vf": (R, torch.float32), "stats": (6, torch.float64), "scratch": (self.nb // 8, torch.float64)}
        self.big = {key: torch.full((n + 2 * GUARD,), SENT, dtype=dt, device=dev) for key, (n, dt) in sizes.items()}
        self.out = {key: self.big[key][GUARD:GUARD + n] for key, (n, _) in sizes.items()}
        self.ptr_off = {}                             # name -> bytes added to the pointer passed (the refusals)

    def run(self):
        def p(name):
            x = self.out[name] if name in self.out else self.t[name]
            return None if x is None else C.c_void_p(x.data_ptr() + self.ptr_off.get(name, 0))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rows = [p(key) for key in ("logits", "old_logits", "actions", "old_logp", "adv", "vf", "target", "mask", "n_valid")]
        tail = [C.byref(self.prm), p("stats"), p("d_logits"), p("d_vf"), p("scratch"), self.nb, st]
        if self.n_comp == 1:
            return self.L.lib().hh_ppo_loss_categorical(self.R, *rows, *tail)
        return self.L.lib().hh_ppo_loss(self.R, self.ld, *rows, *tail)

    def outputs(self):
        """-> (stats, d_logits [R, ld], d_vf) on the host, after checking the guards and the inputs"""
        torch.cuda.synchronize()
        for key, big in self.big.items():
            g = torch.cat([big[:GUARD], big[-GUARD:]]).cpu()
            assert torch.equal(g, torch.full_like(g, SENT)), f"{key}: a guard element was overwritten"
        for key, v in self.host.items():
            if v is not None:
                assert same_bits(self.t[key].cpu(), v), f"input {key} was modified"
        return self.out["stats"].cpu().clone(), self.out["d_logits"].cpu().reshape(self.R, self.ld).clone(), self.out["d_vf"].cpu().clone()

    def untouched(self):
        torch.cuda.synchronize()
        return all(torch.equal(b.cpu(), torch.full_like(b.cpu(), SENT)) for b in self.big.values())


def call(inp, n_comp, k, **kwargs):
    r = Run(inp, n_comp, k, **kwargs)
    assert r.run() == 0, r.L.lib().hh_last_error()
    return r.outputs()


def hold_to_rule(label, got, want, e32, rows=None, which=(0, 1, 2)):
    """print the (e32, kernel) pairs as the existing tests do, then: the kernel at most 4 x e32 from float64"""
    err = E.errors(got, want, rows)
    print(f"{label}: e32 (stats, d_logits, d_vf) = {e32[0]:.3e} {e32[1]:.3e} {e32[2]:.3e}; kernel = {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}")
    for i in which:
        assert err[i] <= 4.0 * e32[i], f"{label} {('stats', 'd_logits', 'd_vf')[i]}: kernel error {err[i]:.3e} above 4 x e32 = {4 * e32[i]:.3e}"


def exact_zeros(inp, n_comp, dl, dv):
    """masked rows and the columns at or beyond the policy's logits are exactly zero"""
    n_out = E.N_OUT[n_comp]
    assert torch.equal(dl[:, n_out:], torch.zeros_like(dl[:, n_out:]))
    if inp["mask"] is not None:
        off = ~inp["mask"]
        assert torch.equal(dl[off], torch.zeros_like(dl[off])) and torch.equal(dv[off], torch.zeros_like(dv[off]))


GRID = [(n_comp, case) for n_comp in E.INSTANCES for case in E.grid_cases(n_comp)]


@pytest.mark.parametrize("n_comp,case", GRID, ids=[f"n{n}-R{c[0]}-ld{c[1]}-{'m' if c[2] else 'u'}-kl{c[3]}" for n, c in GRID])
def test_ragged_grid(n_comp, case):
    inp, want, e32 = E.grid_case(n_comp, case)
    assert all(e > 0.0 for e, must in zip(e32, E.e32_must_be_positive(inp)) if must)
    stats, dl, dv = call(inp, n_comp, E.kw(case[3], case[4]))
    assert torch.isfinite(stats).all() and torch.isfinite(dl).all() and torch.isfinite(dv).all()
    assert stats[5].item() == want[0][5] == E.n_valid_of(inp)
    if case[3] == 0.0:
        assert stats[3].item() == 0.0
    exact_zeros(inp, n_comp, dl, dv)
    hold_to_rule(f"grid n_comp={n_comp} R={case[0]} ld={case[1]} masked={case[2]} kl_coeff={case[3]}", (stats, dl, dv), want, e32)


@NC
@pytest.mark.parametrize("offsets", (False, True))
def test_wide_logit_table(n_comp, offsets):
    inp, _ = E.wide_table(n_comp, offsets)
    k = E.kw()
    want = E.restate(inp, torch.float64, n_comp, k)
    e32 = E.errors(E.restate(inp, torch.float32, n_comp, k), want)
    stats, dl, dv = call(inp, n_comp, k)
    assert torch.isfinite(stats).all() and torch.isfinite(dl).all() and torch.isfinite(dv).all()
    exact_zeros(inp, n_comp, dl, dv)
    hold_to_rule(f"wide n_comp={n_comp} offsets={offsets}", (stats, dl, dv), want, e32)


@NC
def test_kink_table(n_comp):
    inp, meta = E.kink_table(n_comp)
    pol, val = E.kink_expect(n_comp)
    # with entropy and KL terms: every row against float64, the host test having shown that both are on the same side of every kink
    k = E.kink_kw(0.2, 0.01)
    want = E.restate(inp, torch.float64, n_comp, k)
    e32 = E.errors(E.restate(inp, torch.float32, n_comp, k), want)
    got = call(inp, n_comp, k)
    assert all(torch.isfinite(x).all() for x in got)
    hold_to_rule(f"kink n_comp={n_comp}", got, want, e32, which=(0, 1))
    # the policy gradient alone: the rows it passes on against float64, exactly 0.0f in all others
    k0 = E.kink_kw(0.0, 0.0)
    want0 = E.restate(inp, torch.float64, n_comp, k0)
    e32_0 = E.errors(E.restate(inp, torch.float32, n_comp, k0), want0, rows=pol)
    stats0, dl0, dv0 = call(inp, n_comp, k0)
    assert e32_0[0] > 0.0 and e32_0[1] > 0.0
    hold_to_rule(f"kink n_comp={n_comp} policy gradient alone, passing rows", (stats0, dl0, dv0), want0, e32_0, rows=pol, which=(0, 1))
    assert torch.equal(dl0[~pol], torch.zeros_like(dl0[~pol]))
    assert (dl0[pol] != 0).any(dim=1).all()
    exact_zeros(inp, n_comp, dl0, dv0)
    # the value gradient: exactly 0.0f beyond the kink, exactly vf_coeff / n * 2 * dv at and inside it
    exact = (E.KINK_VFC / E.KINK_R * 2 * meta["dv"]).float()
    inside = meta["dv"].abs() <= 2.0
    for dv in (got[2], dv0):
        assert torch.equal(dv[~inside], torch.zeros_like(dv[~inside]))
        assert same_bits(dv[inside], exact[inside])
        assert torch.equal(dv != 0, val)


@NC
def test_action_table(n_comp):
    inp, K = E.action_table(n_comp)
    k = E.kw()
    stats, dl, dv = call(inp, n_comp, k)
    assert same_bits(dl[:K], dl[K:]) and same_bits(dv[:K], dv[K:])
    twin = dict(inp, actions=torch.cat([inp["actions"][K:], inp["actions"][K:]]))
    want = E.restate(twin, torch.float64, n_comp, k)
    e32 = E.errors(E.restate(twin, torch.float32, n_comp, k), want)
    hold_to_rule(f"actions n_comp={n_comp}", (stats, dl, dv), want, e32)
    stats_t, dl_t, dv_t = call(twin, n_comp, k)
    assert same_bits(stats, stats_t) and same_bits(dl, dl_t) and same_bits(dv, dv_t)


@NC
def test_rows_do_not_depend_on_their_position(n_comp):
    lds = E.LDS[n_comp]
    inp = E.base_inputs(n_comp, 513, lds[len(lds) // 2], True, 2)
    perm = torch.randperm(513, generator=torch.Generator().manual_seed(1))
    assert (perm != torch.arange(513)).float().mean() > 0.9 and (perm // 256 != torch.arange(513) // 256).any()
    k = E.kw()
    want = E.restate(inp, torch.float64, n_comp, k)
    e32 = E.errors(E.restate(inp, torch.float32, n_comp, k), want)
    stats, dl, dv = call(inp, n_comp, k)
    stats_p, dl_p, dv_p = call(E.permuted(inp, perm), n_comp, k)
    assert same_bits(dl_p, dl[perm]) and same_bits(dv_p, dv[perm])
    hold_to_rule(f"position n_comp={n_comp}", (stats, dl, dv), want, e32)
    hold_to_rule(f"position n_comp={n_comp} permuted", (stats_p, dl, dv), want, e32, which=(0,))


@NC
def test_a_row_changes_no_other_rows_gradient(n_comp):
    lds = E.LDS[n_comp]
    R, ld = 513, lds[len(lds) // 2]
    inp, donor = E.base_inputs(n_comp, R, ld, False, 6), E.base_inputs(n_comp, R, ld, False, 7)
    k = E.kw()
    _, dl, dv = call(inp, n_comp, k)
    for row in (0, 255, 256, R - 1):
        _, dl_r, dv_r = call(E.replace_row(inp, row, donor, 300), n_comp, k)
        others = torch.arange(R) != row
        assert same_bits(dl_r[others], dl[others]) and same_bits(dv_r[others], dv[others]), row
        assert not same_bits(dl_r[row], dl[row]), row


@NC
def test_the_divisor_is_the_callers_n_valid(n_comp):
    inp = E.base_inputs(n_comp, 513, E.LDS[n_comp][0], True, 8)
    n = E.n_valid_of(inp)
    k = E.kw()
    stats, dl, dv = call(inp, n_comp, k)
    stats2, dl2, dv2 = call(inp, n_comp, k, n_valid=2 * n)
    assert stats[5].item() == n and stats2[5].item() == 2 * n
    assert same_bits(dl2 * 2, dl) and same_bits(dv2 * 2, dv) and (dl != 0).any() and (dv != 0).any()
    assert torch.allclose(stats2[:5] * 2, stats[:5], rtol=1e-14, atol=0)


@NC
@pytest.mark.parametrize("name", E.MASK_PATTERNS)
def test_mask_patterns_with_nan_in_the_masked_rows(n_comp, name):
    zero, nan = E.mask_case(n_comp, name, False), E.mask_case(n_comp, name, True)
    k = E.kw()
    stats, dl, dv = call(zero, n_comp, k)
    stats_n, dl_n, dv_n = call(nan, n_comp, k)
    assert same_bits(stats, stats_n) and same_bits(dl, dl_n) and same_bits(dv, dv_n)
    exact_zeros(zero, n_comp, dl, dv)
    assert stats[5].item() == E.n_valid_of(zero)
    if name == "all_off":
        # include/hh_learner.h: with n_valid = 0 the gradients are 0.0f, stats[5] is 0 and the five means are 0 / 0
        assert torch.equal(dl, torch.zeros_like(dl)) and torch.equal(dv, torch.zeros_like(dv)) and stats[5].item() == 0.0
        assert torch.isnan(stats[:5]).all()
        s0 = call(zero, n_comp, E.kw(klc=0.0))[0]
        assert torch.isnan(s0[[0, 1, 2, 4]]).all() and s0[3].item() == 0.0 and s0[5].item() == 0.0
        return
    want = E.restate(zero, torch.float64, n_comp, k)
    e32 = E.errors(E.restate(zero, torch.float32, n_comp, k), want)
    assert torch.isfinite(stats).all() and torch.isfinite(dl).all() and torch.isfinite(dv).all()
    hold_to_rule(f"mask {name} n_comp={n_comp}", (stats, dl, dv), want, e32)


@NC
def test_nan_in_the_ignored_columns(n_comp):
    zero, nan = E.ignored_columns_case(n_comp, False), E.ignored_columns_case(n_comp, True)
    k = E.kw()
    stats, dl, dv = call(zero, n_comp, k)
    stats_n, dl_n, dv_n = call(nan, n_comp, k)
    assert same_bits(stats, stats_n) and same_bits(dl, dl_n) and same_bits(dv, dv_n)
    assert torch.isfinite(stats).all() and torch.isfinite(dl).all()
    exact_zeros(nan, n_comp, dl_n, dv_n)
    want = E.restate(zero, torch.float64, n_comp, k)
    hold_to_rule(f"ignored columns n_comp={n_comp}", (stats_n, dl_n, dv_n), want, E.errors(E.restate(zero, torch.float32, n_comp, k), want))


@NC
def test_misaligned_pointers_are_refused_and_nothing_is_written(n_comp):
    inp = E.base_inputs(n_comp, 63, E.LDS[n_comp][0], False, 0)
    k = E.kw()
    refused = [("logits", 4), ("old_logits", 4), ("d_logits", 4)] + ([("actions", 1)] if n_comp != 1 else [])
    for name, off in refused:
        r = Run(inp, n_comp, k)
        r.ptr_off[name] = off
        assert r.run() == -1, (name, off)             # HH_E_ARG
        assert FN[n_comp].encode() in r.L.lib().hh_last_error() and b"aligned" in r.L.lib().hh_last_error()
        assert r.untouched(), (name, off)
    if n_comp == 1:                                   # "no alignment requirement": the same bytes from every address
        first = call(inp, n_comp, k)
        for off in (1, 2, 3):
            assert all(same_bits(a, b) for a, b in zip(first, call(inp, n_comp, k, act_off=off))), off
