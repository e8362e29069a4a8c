"""The learners' fused shared layer (trunk="fused") without a GPU: dense_tanh_torch against autograd in float64, the float64 restatement
and its error bound (a float32 run of the restatement lies inside it, a run that loses the lo halves does not), a numpy emulation of
the kernels' scaled split-fp16 arithmetic on the input families of tests/dense_tanh_ref.py (inside the bound each family is held to;
with one scale table read one entry off it leaves the bound on "scales" and stays inside on the default inputs wherever that table is
uniform there), the `trunk` argument, and the ctypes struct against the header."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_tanh_ref as REF
from hhmarl_2d_amd import _lib
from hhmarl_2d_amd import learner as LR
from hhmarl_2d_amd import policy_nets as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, P = _lib.DENSE_ROW_TILE, _lib.DENSE_MAX_PARTS
SHAPES = [(K, N, R) for K, N in REF.DIMS for R in REF.row_counts(K, N, T, P)]
EDGE_SHAPES = [(K, N, R) for K, N in REF.EDGE_DIMS for R in REF.row_counts(K, N, T, P)]
GRID = REF.family_grid(T)
CAP_ROWS = ((1, P * T + 1), (T + 1, P * T - T))          # 500 x 500: a small block 0, then a block 1 past the partial-sum cap


def test_dense_tanh_torch_equals_autograd_and_the_restatement():
    """float64: dense_tanh_torch is tanh(F.linear) for one and for two inputs, and the restatement's backward is autograd's"""
    c = REF.case(33, 17, (5, 3), seed=1)
    w, b = (torch.from_numpy(c[k].copy()).double().requires_grad_() for k in ("w", "b"))
    xs = [torch.from_numpy(x.copy()).double().requires_grad_() for x in c["xs"]]
    ys = LR.dense_tanh_torch(xs, w, b)
    assert isinstance(ys, tuple) and len(ys) == 2
    for x, y in zip(xs, ys):
        assert torch.equal(y, torch.tanh(F.linear(x, w, b)))
    single = LR.dense_tanh_torch(xs[0].reshape(1, 5, 33), w, b)
    assert isinstance(single, torch.Tensor) and tuple(single.shape) == (1, 5, 17) and torch.equal(single[0], ys[0])
    dys = [torch.from_numpy(d.copy()).double() for d in c["dys"]]
    sum((y * d).sum() for y, d in zip(ys, dys)).backward()
    y64 = REF.forward(c["xs"], c["w"], c["b"])
    d_xs, d_w, d_b, _ = REF.backward(c["xs"], y64, c["dys"], c["w"])
    for y, want in zip(ys, y64):
        assert np.allclose(y.detach().numpy(), want, rtol=0, atol=1e-15)
    for x, want in zip(xs, d_xs):
        assert np.allclose(x.grad.numpy(), want, rtol=0, atol=1e-14)
    assert np.allclose(w.grad.numpy(), d_w, rtol=0, atol=1e-14) and np.allclose(b.grad.numpy(), d_b, rtol=0, atol=1e-14)


def _run(c, y_in, operand):
    """the restatement in float32 with every product's operands passed through `operand`; backward from y_in -> (ys, d_xs, d_w, d_b)"""
    f32 = np.float32
    w = operand(c["w"])
    ys = [np.tanh((operand(x) @ w.T).astype(f32) + c["b"]).astype(f32) for x in c["xs"]]
    d_pres = [(dy * (f32(1) - y * y)).astype(f32) for y, dy in zip(y_in, c["dys"])]
    d_xs = [(operand(dp) @ w).astype(f32) for dp in d_pres]
    d_w = sum((operand(dp).T @ operand(x)).astype(f32) for dp, x in zip(d_pres, c["xs"]))
    d_b = sum(dp.sum(axis=0, dtype=f32) for dp in d_pres)
    return ys, d_xs, d_w, d_b


def _ratios(c, got, y_in, ext=False, formed=False):
    """the largest error / bound of each of y, d_x, d_w, d_b (no assertion; nan where an output is not finite); ext: the extended bound;
    formed: with REF.formation_terms"""
    ys, d_xs, d_w, d_b = got
    y64 = REF.forward(c["xs"], c["w"], c["b"])
    x64, w64, b64, dp64 = REF.backward(c["xs"], y_in, c["dys"], c["w"])
    b_y = (REF.forward_bound_ext if ext else REF.forward_bound)(c["xs"], c["w"], c["b"])
    b_dx, b_dw, b_db = (REF.backward_bounds_ext if ext else REF.backward_bounds)(c["xs"], dp64, c["w"], (y_in, c["dys"]) if formed else None)

    def r(g, w_, b_):
        with np.errstate(invalid="ignore"):
            return float(np.max(np.abs(g.astype(np.float64) - w_) / np.maximum(b_, 1e-300))) if g.size else 0.0
    top = lambda gs, ws, bs: float(np.max([r(g, w_, b_) for g, w_, b_ in zip(gs, ws, bs)]))      # np.max: a nan stays a nan
    return dict(y=top(ys, y64, b_y), d_x=top(d_xs, x64, b_dx), d_w=r(d_w, w64, b_dw), d_b=r(d_b, b64, b_db))


def _inside(ratios):
    return all(v <= 1.0 for v in ratios.values())            # a nan is outside


def _y32(c):
    return [y.astype(np.float32) for y in REF.forward(c["xs"], c["w"], c["b"])]


def _split(v):
    """fp16 hi and fp16(v - hi) of float32 v, both as float32 (hhx_split2: round to nearest even, fp16 subnormals kept)"""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16).astype(np.float32)
        return hi, (v - hi).astype(np.float16).astype(np.float32)


def _product(a, sa, b, sb, ua, ub):
    """a [I, n] (row i times 2^sa[i]) against b [J, n] (row j times 2^sb[j]) as the kernels multiply: scaled, split, hi hi + lo hi + hi lo
    with float32 accumulation, then unscaled by 2^-ua[i] and 2^-ub[j] in that order -> [I, J] float32"""
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        ah, al = _split((a * np.ldexp(f32(1), sa)[:, None]).astype(f32))
        bh, bl = _split((b * np.ldexp(f32(1), sb)[:, None]).astype(f32))
        acc = ((al @ bh.T).astype(f32) + (ah @ bl.T).astype(f32)).astype(f32) + (ah @ bh.T).astype(f32)
        return ((acc * np.ldexp(f32(1), -ua)[:, None]).astype(f32) * np.ldexp(f32(1), -ub)[None, :]).astype(f32)


def emulate(c, y_in, tables=None, pre_out=None):
    """hh_dense_tanh_forward and _backward (from y_in) in numpy, operation for operation where the result depends on it: the scales by
    hdt_sf's rule (REF.scale_exp), the scaled (hi, lo) split, three products into float32, the unscale in the kernels' order, d_W per
    64-row tile onto float32 sums of min(P, tiles) walks that are then added in float64, d_b in float64 -> (ys, d_xs, d_w, d_b).
    tables = (name, "stage" | "undo"): the named table of REF.TABLES is read one entry further on (cyclically, within its block or
    tile) when the operand is staged ("stage": entry i + 1 scales, entry i unscales) or when the scale is undone ("undo").
    pre_out: a list that receives the blocks' unscaled sums x W^T, before the bias."""
    f32 = np.float32
    K, N = c["K"], c["N"]
    w, dps = c["w"], REF.d_pre32(y_in, c["dys"])
    tb = REF.scale_tables(c, y_in, T)

    def two(name, e):
        """-> (the exponents that stage, the exponents that are undone) of one table"""
        if tables is None or tables[0] != name:
            return e, e
        return (np.roll(e, -1), e) if tables[1] == "stage" else (e, np.roll(e, -1))

    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        wr_s, wr_u = two("w_rows", tb["w_rows"])
        ys = []
        for x, ex in zip(c["xs"], tb["x_rows"]):
            xs_, xu = two("x_rows", ex)
            acc = _product(x, xs_, w, wr_s, xu, wr_u)           # forward: acc * inv[q] * invw[n] + b
            ys.append(np.tanh((acc + c["b"][None, :]).astype(f32)).astype(f32))
            if pre_out is not None:
                pre_out.append(acc)
        wc_s, wc_u = two("w_cols", tb["w_cols"])
        d_xs = []
        for dp, ed in zip(dps, tb["dp_rows"]):
            ds, du = two("dp_rows", ed)
            d_xs.append(_product(dp, ds, np.ascontiguousarray(w.T), wc_s, du, wc_u))
        tiles = [(dp[r:r + T], x[r:r + T], en, ek) for dp, x, ens, eks in zip(dps, c["xs"], tb["dp_tile_cols"], tb["x_tile_cols"])
                 for (r, en, ek) in zip(range(0, x.shape[0], T), ens, eks)]
        parts = min(P, len(tiles))
        tot = np.zeros((parts, N, K), dtype=f32)
        bsum = np.zeros((parts, N), dtype=np.float64)
        for i, (dp, x, en, ek) in enumerate(tiles):
            ns, nu = two("dp_tile_cols", en)
            ks, ku = two("x_tile_cols", ek)
            # tot = fmaf(acc * un, uk, tot): the product with uk is exact, so one rounding of the sum
            tot[i % parts] = (tot[i % parts] + _product(np.ascontiguousarray(dp.T), ns, np.ascontiguousarray(x.T), ks, nu, ku)).astype(f32)
            bsum[i % parts] += dp.astype(np.float64).sum(axis=0)
        d_w = tot.astype(np.float64).sum(axis=0).astype(f32)
        d_b = bsum.astype(f32).astype(np.float64).sum(axis=0).astype(f32)
    return ys, d_xs, d_w, d_b


@pytest.mark.parametrize("K,N,R", SHAPES)
def test_float32_restatement_lies_inside_the_bound(K, N, R):
    """the reference alone satisfies the bound, with one block and with two blocks of (R, 1) rows"""
    for rows in ((R,), (R, 1)):
        c = REF.case(K, N, rows)
        y_in = [y.astype(np.float32) for y in REF.forward(c["xs"], c["w"], c["b"])]
        ratios = _ratios(c, _run(c, y_in, lambda a: a), y_in)
        print(K, N, rows, {k: round(v, 4) for k, v in ratios.items()})
        assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("K,N,R", SHAPES)
def test_losing_the_lo_halves_violates_the_bound(K, N, R):
    """both operands of every product rounded to fp16 (hi only): the run leaves the bound, in y and in d_x on every shape, and in d_w on
    every shape with more than one element whose sum over the rows is at most a tile + 1 long.  The two exceptions are printed, not
    asserted: d_w over P T + 1 = 2049 rows (0.36 of the bound: independent fp16 roundings of relative size 2^-12 add up like sqrt(n),
    the bound's accumulation term grows like n, and at n = 2049 the bound has overtaken them), and the single element of the 1 x 1
    d_w, where 64 roundings cancel or not by chance.  The lost lo pass still shows in y and d_x of the same runs."""
    c = REF.case(K, N, (R,))
    y_in = [y.astype(np.float32) for y in REF.forward(c["xs"], c["w"], c["b"])]
    ratios = _ratios(c, _run(c, y_in, lambda a: a.astype(np.float16).astype(np.float32)), y_in)
    print(K, N, R, {k: round(v, 2) for k, v in ratios.items()})
    assert ratios["y"] > 1.0 and ratios["d_x"] > 1.0, ratios
    assert ratios["d_w"] > 1.0 or R > T + 1 or K * N == 1, ratios


def test_families_start_from_the_default_draws():
    """every family is the default times exact powers of two (the same float32 mantissas) or exact zeros / ones where it says so; the
    "scales" case has at least 4 distinct exponents in each of the six scale tables (case() asserts it as well: it fails here first)"""
    mant = lambda a: np.frexp(a)[0]
    for K, N, rows in ((500, 500, (T + 1, 1)), (33, 17, (2 * T + 1, T - 1))):
        d = REF.case(K, N, rows)
        assert d["family"] == "default" and REF.same_bits(d["w"], REF.case(K, N, rows, family="default")["w"])
        for fam in ("scales", "range"):
            c = REF.case(K, N, rows, family=fam)
            for key in ("w", "b"):
                assert np.array_equal(mant(c[key]), mant(d[key]))
            for key in ("xs", "dys"):
                assert all(np.array_equal(mant(a), mant(b)) for a, b in zip(c[key], d[key]))
        counts = REF.distinct_scales(REF.case(K, N, rows, family="scales"))
        print(K, N, rows, counts)
        assert set(counts) == set(REF.TABLES) and min(counts.values()) >= 4, counts
        c = REF.case(K, N, rows, family="zeros")
        z = c["zeros"]
        assert not c["w"][z["w_row"]].any() and not c["w"][:, z["w_col"]].any()
        for x, dy, xr, dr, dt in zip(c["xs"], c["dys"], z["x_rows"], z["dy_rows"], z["dy_tiles"]):
            assert not x[xr].any() and not x[:, z["x_col"]].any() and not dy[:, z["dy_col"]].any()
            assert (dt is not None) == (x.shape[0] >= 2 * T) and (dt is None or (dt[1] - dt[0] == T and dt[0] % T == 0 and not dy[dt[0]:dt[1]].any()))
            assert dr is None or not dy[dr].any()
        changed = lambda a, b: (a != b)
        assert all(not (changed(a, b) & (a != 0)).any() for a, b in zip([c["w"]] + c["xs"] + c["dys"], [d["w"]] + d["xs"] + d["dys"]))
        c = REF.case(K, N, (T + 1,), family="picked")
        d1 = REF.case(K, N, (T + 1,))
        assert np.array_equal(c["xs"][0][:, 1], d1["xs"][0][:, 1] * np.float32(2.0 ** -30)) and np.array_equal(np.delete(c["xs"][0], 1, 1), np.delete(d1["xs"][0], 1, 1))
        assert (c["w"][:, 1] == 1).all() and not np.delete(c["w"], 1, 1).any()


def _both_inside(c, ext=False):
    """the float32 restatement and the emulation of one case against the bound -> their ratios.  REF.formation_terms join the extended
    bound, and the componentwise one at K = 1 only: there the bias is U(-1, 1), y^2 passes 1/2, and the float32 restatement itself
    is 1.3 x outside without them (d_b at 1 x 512, one row)"""
    y_in = _y32(c)
    formed = ext or c["K"] == 1
    plain, emu = _ratios(c, _run(c, y_in, lambda a: a), y_in, ext, formed), _ratios(c, emulate(c, y_in), y_in, ext, formed)
    print(c["family"], c["K"], c["N"], c["rows"], "float32", {k: round(v, 4) for k, v in plain.items()}, "emulation", {k: round(v, 4) for k, v in emu.items()})
    assert _inside(plain), plain
    assert _inside(emu), emu
    return plain, emu


@pytest.mark.parametrize("family,K,N,rows", GRID)
def test_families_lie_inside_the_bound_they_are_held_to(family, K, N, rows):
    """the reference alone (float32) and the emulation of the kernels' arithmetic: "scales" and "zeros" inside the componentwise bound,
    "range" and "picked" inside the extended one"""
    _both_inside(REF.case(K, N, rows, family=family), ext=family in REF.EXT_FAMILIES)


@pytest.mark.parametrize("K,N,R", SHAPES + EDGE_SHAPES)
def test_emulation_lies_inside_the_bound(K, N, R):
    """the default inputs on every shape of the GPU tests, the edge shapes included: float32 restatement and emulation"""
    for rows in ((R,), (R, 1)):
        _both_inside(REF.case(K, N, rows))


@pytest.mark.parametrize("rows", CAP_ROWS)
def test_walk_from_a_small_block_into_a_long_one(rows):
    """500 x 500 with more row tiles than partial sums, most of them in block 1"""
    _both_inside(REF.case(500, 500, rows))


FEEDS = dict(w_rows="y", x_rows="y", w_cols="d_x", dp_rows="d_x", dp_tile_cols="d_w", x_tile_cols="d_w")


def _uniform(tb, name):
    """every unit of the table that a damage rolls (the table, a block's rows, a tile's columns) holds one value"""
    units = [tb[name]] if name in ("w_rows", "w_cols") else tb[name] if name in ("x_rows", "dp_rows") else [t for blk in tb[name] for t in blk]
    return all(len(np.unique(u)) <= 1 for u in units)


@pytest.mark.parametrize("how", ("stage", "undo"))
@pytest.mark.parametrize("table", REF.TABLES)
def test_a_scale_table_read_one_entry_off(table, how):
    """The emulation with ONE table damaged: entry i + 1 scales what entry i unscales ("stage"), or entry i + 1 undoes what entry i
    scaled ("undo").  On "scales" the output that the table feeds leaves the bound, on all three shapes.  On the default inputs
    the same damage stays inside the bound wherever the table is uniform, which is why these families exist: at 500 x 500 and
    481 x 497 that is asserted for the row scales of W and of x and the column scales of W (the largest of >= 481 uniform draws
    lies in the top binade but for 2^-481).  The other three are NOT always uniform there (the largest of 500 normal draws passes
    4 in about 3 % of the rows, that of a tile's 64 stays below 2 in about 5 % of the columns, and a last tile of one row has as
    many x scales as its row has binades), so for them, and at 33 x 17, the assertion is the equivalence: the damage is invisible
    exactly where the table is uniform."""
    rows = (2 * T + 1, T - 1)
    for K, N in ((500, 500), (481, 497), (33, 17)):
        c = REF.case(K, N, rows, family="scales")
        y_in = _y32(c)
        ratios = _ratios(c, emulate(c, y_in, tables=(table, how)), y_in)
        print("scales", K, N, table, how, ratios)
        assert not ratios[FEEDS[table]] <= 1.0, (K, N, ratios)
        d = REF.case(K, N, rows)
        y_in = _y32(d)
        uniform = _uniform(REF.scale_tables(d, y_in, T), table)
        ratios = _ratios(d, emulate(d, y_in, tables=(table, how)), y_in)
        print("default", K, N, table, how, "uniform" if uniform else "not uniform", ratios)
        assert _inside(ratios) == uniform, (K, N, uniform, ratios)
        if K > 33 and table in ("w_rows", "x_rows", "w_cols"):
            assert uniform and _inside(ratios), (K, N, ratios)


@pytest.mark.parametrize("K,N", ((500, 500), (33, 17)))
def test_picked_column_leaves_the_componentwise_bound_and_keeps_the_extended_one(K, N):
    """W picks the one column of x that is 2^-30 of its row: the pre-activation's error is more than 100 times the componentwise term
    (4 * 2^-22 + (K + 2) * 2^-24) |x| |W|^T, and inside that term plus the derived floor"""
    c = REF.case(K, N, (T + 1,), family="picked")
    pre = []
    emulate(c, _y32(c), pre_out=pre)
    x64, w64 = c["xs"][0].astype(np.float64), c["w"].astype(np.float64)
    err = np.abs(pre[0].astype(np.float64) - x64 @ w64.T)
    comp = REF.factor(K) * (np.abs(x64) @ np.abs(w64).T)
    old, ext = float(np.max(err / comp)), float(np.max(err / (comp + REF.forward_floor(c["xs"], c["w"])[0])))
    print(K, N, "error / componentwise term", round(old, 1), "error / extended", round(ext, 5))
    assert old > 100.0 and ext <= 1.0, (old, ext)


@pytest.mark.parametrize("s", (30, -30))
@pytest.mark.parametrize("K,N", ((500, 500), (481, 497)))
def test_emulation_is_equivariant_under_powers_of_two(K, N, s):
    """REF.pow2_variants on the emulation, from a fixed y: the marked outputs are the baseline's times 2^s bit for bit, the outputs a
    change does not reach keep their bytes, the ones it does reach stay inside the bound (y, which sees a changed row maximum: the
    extended one).  The GPU test asks the kernels the same."""
    c = REF.case(K, N, (T + 1, T - 1))
    y_in = _y32(c)
    names = ("ys", "d_xs", "d_w", "d_b")
    base = dict(zip(names, emulate(c, y_in)))
    for name, c2, scaled, exact in REF.pow2_variants(c, s):
        got = emulate(c2, y_in)
        want = scaled(base)
        for key, g in zip(names, got):
            if key in exact:
                assert all(REF.same_bits(a, b) for a, b in zip(g, want[key])) if isinstance(g, list) else REF.same_bits(g, want[key]), (name, key)
        ratios = _ratios(c2, got, y_in, ext="ys" not in exact, formed="ys" not in exact)
        print(K, N, name, {k: round(v, 4) for k, v in ratios.items()})
        assert _inside(ratios), (name, ratios)


def test_trunk_argument():
    for make in (lambda **kw: LR.TrainableNet(PN.FIGHT1, **kw), lambda **kw: LR.TrainableNet(PN.ESC2, **kw), lambda **kw: LR.CommanderTrainable(**kw)):
        with pytest.raises(ValueError):
            make(trunk="bogus")
        plain, fused = make(), make(trunk="fused")
        assert plain.trunk == "torch" and fused.trunk == "fused"
        a, b = plain.state_dict(), fused.state_dict()
        assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    assert LR.TRUNK_MODES == ("torch", "fused")
    m = LR.TrainableNet(PN.FIGHT2, attention="fused", inputs="fused", trunk="fused")
    assert (m.attention, m.inputs, m.trunk) == ("fused", "fused", "fused")
    for cls in (LR.PPOLearner, LR.CommanderLearner, LR.TrainableNet, LR.CommanderTrainable):
        assert inspect.signature(cls.__init__).parameters["trunk"].default == "torch"


def test_fused_trunk_refuses_cpu_tensors():
    x, w, b = torch.rand((4, 12)), torch.rand((8, 12)), torch.rand((8,))
    with pytest.raises((ValueError, RuntimeError)):                 # host tensors: ValueError; RuntimeError where there is no GPU at all
        LR.dense_tanh(x, w, b)
    with pytest.raises((ValueError, RuntimeError)):
        LR.dense_tanh((x, x), w, b)
    m = LR.TrainableNet(PN.ESC1, trunk="fused")
    with pytest.raises((ValueError, RuntimeError)):
        m(torch.rand((3, PN.OBS_DIM[PN.ESC1])), torch.rand((3, sum(PN.CRITIC_DIMS[PN.ESC1]))))
    cm = LR.CommanderTrainable(trunk="fused")
    with pytest.raises((ValueError, RuntimeError)):
        cm(torch.rand((2, 4, 34)), torch.rand((2, 4, 105)), torch.zeros((2, 2, 200)), torch.full((2,), 4, dtype=torch.int32), fused_gru=False)


@pytest.mark.parametrize("kind", (PN.FIGHT1, PN.FIGHT2, PN.ESC1, PN.ESC2))
def test_default_trunk_is_bit_equal_to_a_module_built_without_the_argument(kind):
    torch.manual_seed(kind)
    a = LR.TrainableNet(kind)
    b = LR.TrainableNet(kind, trunk="torch")
    b.load_state_dict(a.state_dict())
    d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
    lead = (3, 20) if PN.HAS_ATT[kind] else (7,)
    obs, crit = torch.rand(lead + (PN.OBS_DIM[kind],)), torch.rand(lead + (d1 + a1 + d2 + a2,))
    with torch.no_grad():
        for u, v in zip(a(obs, crit), b(obs, crit)):
            assert torch.equal(u, v)


def test_default_commander_trunk_is_bit_equal():
    torch.manual_seed(5)
    a, b = LR.CommanderTrainable(), LR.CommanderTrainable(trunk="torch")
    b.load_state_dict(a.state_dict())
    args = (torch.rand((3, 6, 34)), torch.rand((3, 6, 105)), 0.1 * torch.randn((3, 2, 200)), torch.tensor([6, 2, 4], dtype=torch.int32))
    with torch.no_grad():
        for u, v in zip(a(*args, fused_gru=False), b(*args, fused_gru=False)):
            assert torch.equal(u, v)


def test_struct_and_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "hh_learner.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (HH_DENSE_[A-Z_]+)\s+(\d+)", txt)}
    assert (defs["HH_DENSE_MAX_SRC"], defs["HH_DENSE_MAX_DIM"], defs["HH_DENSE_ROW_TILE"], defs["HH_DENSE_MAX_PARTS"], defs["HH_DENSE_FWD_SCRATCH_BYTES"]) == (
        _lib.DENSE_MAX_SRC, _lib.DENSE_MAX_DIM, _lib.DENSE_ROW_TILE, _lib.DENSE_MAX_PARTS, _lib.DENSE_FWD_SCRATCH_BYTES)
    body = re.search(r"typedef struct hh_dense_src \{(.*?)\} hh_dense_src;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"[\*\s]", "", nm) for decl in body.split(";") if decl.strip() for nm in re.match(r"(?:const\s+)?\w+\s+(.*)", decl.strip()).group(1).split(",")]
    assert names == [f[0] for f in _lib.HHDenseSrc._fields_]
    assert C.sizeof(_lib.HHDenseSrc) == 8 * len(names) and all(getattr(_lib.HHDenseSrc, nm).offset == 8 * i for i, nm in enumerate(names))   # every field is 8 bytes wide
    for sym in ("hh_dense_tanh_scratch_bytes", "hh_dense_tanh_forward", "hh_dense_tanh_backward"):
        assert sym in _lib.LEARNER_EXPORTS and re.search(r"\b" + sym + r"\s*\(", txt)
        assert hasattr(C.CDLL(_lib.LIB_PATH), sym), f"libhh_world.so does not export {sym}"
