"""hh_gae and hh_gae_rllib on the MI355X at their edges (tables: tests/gae_edges_ref.py; what they rest on: tests/test_gae_edges_host.py):
column counts either side of the 256-lane block with 1, 2 and 3 agents, T from 1, a done on every row, on the first or the last row only
and a ragged pattern tied to the arena, gamma and lambda at 0 and 1.  hh_gae_rllib is bit-exact against oracle/gae_ref.py's rllib_stream;
hh_gae is held to 4 x e32 of the float64 masked recursion (e32 = the float32 numpy form's error against it, per case) and to the exact
bits where the recursion is exact in float32.  Every call writes into views of sentinel-filled buffers and leaves its inputs alone."""
import ctypes as C

import numpy as np
import pytest

import gae_edges_ref as G
import gae_ref

pytestmark = pytest.mark.gpu
SENT = -12345.678
GUARD = 64


def run(kind, x, gamma, lam, reward=None):
    """hh_gae ("masked") or hh_gae_rllib ("rllib") through the C ABI -> (adv, ret) as numpy, after checking guards and inputs"""
    import torch
    from hhmarl_2d_amd import _lib as L
    reward = x["reward"] if reward is None else reward
    T, N, nA = reward.shape
    host = dict(reward=reward, value=x["value"], valid=x["valid"], done=x["done"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    n = T * N * nA
    big = [torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device="cuda") for _ in range(2)]
    adv, ret = (b[GUARD:GUARD + n] for b in big)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if kind == "masked":
        L.check(L.lib().hh_gae(T, N, nA, p(dev["reward"]), p(dev["value"]), p(dev["valid"]), p(dev["done"]), gamma, lam, p(adv), p(ret), st))
    else:
        L.check(L.lib().hh_gae_rllib(T, N, nA, p(dev["reward"]), p(dev["value"]), p(dev["done"]), gamma, lam, p(adv), p(ret), st))
    torch.cuda.synchronize()
    for b in big:
        g = torch.cat([b[:GUARD], b[-GUARD:]]).cpu()
        assert torch.equal(g, torch.full_like(g, SENT)), "a guard element was overwritten"
    for k, v in host.items():
        assert np.array_equal(dev[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), f"input {k} was modified"
    return adv.cpu().numpy().reshape(T, N, nA).copy(), ret.cpu().numpy().reshape(T, N, nA).copy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


CASES = G.cases()


@pytest.mark.parametrize("case", CASES, ids=[f"N{c[0]}x{c[1]}-T{c[2]}-{c[3]}-g{c[4]}-l{c[5]}" for c in CASES])
def test_both_kernels_on_the_shape_and_done_table(case):
    x, want, e32 = G.general_case(case)
    gamma, lam = case[4], case[5]
    # RLlib's semantics: nothing masked, reward 0.0 where there is no key; bit for bit
    r0 = np.where(x["valid"] > 0, x["reward"], np.float32(0.0)).astype(np.float32)
    a_ref, r_ref = gae_ref.rllib_stream(r0, x["valid"], x["value"], x["done"], gamma, lam)
    adv, ret = run("rllib", x, gamma, lam, reward=r0)
    assert same_bits(adv, a_ref) and same_bits(ret, r_ref)
    # the masked recursion: 4 x e32 of float64, invalid rows exactly zero
    assert min(e32) > 0.0
    adv, ret = run("masked", x, gamma, lam)
    err = G.errors((adv, ret), want)
    print(f"gae N={case[0]} nA={case[1]} T={case[2]} done={case[3]} gamma={gamma} lambda={lam}: e32 (adv, ret) = {e32[0]:.3e} {e32[1]:.3e}; "
          f"kernel = {err[0]:.3e} {err[1]:.3e}")
    off = x["valid"] == 0
    assert (adv[off] == 0).all() and (ret[off] == 0).all()
    for name, e, b in zip(("adv", "ret"), err, e32):
        assert e <= 4.0 * b, f"{name}: kernel error {e:.3e} above 4 x e32 = {4 * b:.3e}"


@pytest.mark.parametrize("case", G.EXACT_CASES)
def test_masked_recursion_is_exact_where_float32_is(case):
    x = G.exact_case(case)
    a64, r64 = G.masked(x["reward"], x["valid"], x["value"], x["done"], 0.5, 0.5, np.float64)
    adv, ret = run("masked", x, 0.5, 0.5)
    assert same_bits(adv, a64.astype(np.float32)) and same_bits(ret, r64.astype(np.float32))


@pytest.mark.parametrize("N,nA", [(129, 2), (86, 3)])
def test_invalid_rows_and_arena_order(N, nA):
    case = (N, nA, 97, "ragged", 0.99, 0.95)
    x, want, _ = G.general_case(case)
    off = x["valid"] == 0
    adv, ret = run("masked", x, 0.99, 0.95)
    assert off.any() and (adv[off] == 0).all() and (ret[off] == 0).all()
    # an invalid row's reward is not read (gae_ref.masked_stream agrees: tests/test_gae_edges_host.py)
    adv_n, ret_n = run("masked", x, 0.99, 0.95, reward=np.where(off, np.float32("nan"), x["reward"]))
    assert same_bits(adv_n, adv) and same_bits(ret_n, ret)
    # arenas are independent: permuting them permutes the outputs bit for bit, for both kernels
    perm = np.random.default_rng(5).permutation(N)
    xp = dict(reward=x["reward"][:, perm], value=x["value"][:, perm], valid=x["valid"][:, perm], done=x["done"][:, perm])
    adv_p, ret_p = run("masked", xp, 0.99, 0.95)
    assert same_bits(adv_p, np.ascontiguousarray(adv[:, perm])) and same_bits(ret_p, np.ascontiguousarray(ret[:, perm]))
    a, r = run("rllib", x, 0.99, 0.95)
    a_p, r_p = run("rllib", xp, 0.99, 0.95)
    assert same_bits(a_p, np.ascontiguousarray(a[:, perm])) and same_bits(r_p, np.ascontiguousarray(r[:, perm]))
