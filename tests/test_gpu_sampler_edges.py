"""The PPO sampler step (hh_policy_sample) in BOTH forms — hh_k_policy_ppo (32-row tiles) and hh_k_policy_w16_ppo (64-row tiles, 16 rows per
wave) — against the row-by-row restatement of tests/sampler_ref.py at ragged tiles, mixed row lists and the edges of the draw.

Every listed row of every case is compared, nothing is sub-sampled: logits and vf within TOL = 1e-5 (the documented bound, include/hh_policy.h) of
the fp32 restatement, the drawn action EQUAL to the float64 inverse CDF (tests/test_sampler_edges_host.py shows why no row needs excluding), logp
within TOL of TorchMultiCategorical.logp of the kernel's own logits at the kernel's own action.  Each check prints the distances it measured
(`pytest -s`); the bound does not follow them."""
import contextlib
import os

import numpy as np
import pytest
import torch

from hhmarl_2d_amd import policy_nets as PN
import policy_ref as PR
import sampler_ref as SR

pytestmark = pytest.mark.gpu
TOL = 1e-5
FORMS = {"tile-form": ("0", "hh_k_policy_ppo"), "weights-through-lds-16-rows": ("2", "hh_k_policy_w16_ppo")}   # HH_POLICY_W, read at hh_policy_create
MAX_ROWS = 1024
SENTINEL = -777.0
_banks = {}


@contextlib.contextmanager
def _env(**kv):
    """environment variables set (None: unset) for the block and restored after it"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _new_bank(form, kinds, W):
    """slot i = kinds[i] with its value branch; the selector bytes of sampler_ref.SEL"""
    from hhmarl_2d_amd.pilots import PolicyBank
    with _env(HH_POLICY_W=FORMS[form][0]):
        bank = PolicyBank(torch.device("cuda", 0), MAX_ROWS)
    for slot, kind in enumerate(kinds):
        bank.load_trainable(slot, kind, *W[kind])
    bank.set_lut({SR.SEL[kind]: slot for slot, kind in enumerate(kinds)})
    assert bank.kernel_name(2, sampler=True) == FORMS[form][1] and bank.kernel_name(MAX_ROWS, sampler=True) == FORMS[form][1]
    return bank


def _bank(form, mode, seed):
    """one bank per (form, weight set), shared by the cases"""
    key = (form, mode, seed)
    if key not in _banks:
        _banks[key] = _new_bank(form, SR.KINDS if mode == "four" else SR.MODE_KINDS[mode], SR.weights(seed))
    return _banks[key]


def _sample(bank, obs, sel, uniforms=None, crit_act=None, greedy=False):
    """one call on numpy inputs, every output pre-filled with SENTINEL (actions: 77) -> numpy (actions [R, 4], logp [R], vf [R], logits [R, 32])"""
    N = obs.shape[0]
    cu = lambda a, dt: None if a is None else torch.tensor(np.asarray(a), dtype=dt).cuda().contiguous()
    logits = torch.full((N, 2, 32), SENTINEL, dtype=torch.float32, device="cuda")
    logp = torch.full((N, 2), SENTINEL, dtype=torch.float32, device="cuda")
    vf = torch.full((N, 2), SENTINEL, dtype=torch.float32, device="cuda")
    act = torch.full((N, 2, 4), 77, dtype=torch.int8, device="cuda")
    bank.sample(cu(obs, torch.float32), cu(sel, torch.uint8), uniforms=cu(uniforms, torch.float64), crit_act=cu(crit_act, torch.float32), greedy=greedy,
                actions=act, logp=logp, vf=vf, logits=logits)
    torch.cuda.synchronize()
    return act.cpu().numpy().reshape(-1, 4), logp.cpu().numpy().reshape(-1), vf.cpu().numpy().reshape(-1), logits.cpu().numpy().reshape(-1, 32)


def _check(tag, kinds, got, ref, exact_actions=True):
    """every row of one call against the restatement `ref` (a sample_ref dict)"""
    act, logp, vf, logits = got
    flat = np.asarray(kinds).reshape(-1)
    live = flat >= 0
    assert np.isfinite(logits[live]).all() and np.isfinite(vf[live]).all() and np.isfinite(logp[live]).all()
    d_l = float(np.abs(logits[live] - ref["logits"][live]).max())
    d_v = float(np.abs(vf[live] - ref["vf"][live]).max())
    d_p = 0.0
    for kind in SR.KINDS:
        idx = np.flatnonzero(flat == kind)
        if len(idx):
            own = PR.multicategorical_logp(logits[idx], act[idx], PN.N_OUT[kind]).numpy()
            d_p = max(d_p, float(np.abs(logp[idx] - own).max()))
            assert (logits[idx, PN.N_OUT[kind]:] == 0).all(), f"{tag}: logit columns beyond N_OUT"
    print(f"sampler-edges {tag}: rows {int(live.sum())} max|dlogit| {d_l:.3e} max|dvf| {d_v:.3e} max|dlogp| {d_p:.3e}")
    assert d_l <= TOL, f"{tag}: logits {d_l}"
    assert d_v <= TOL, f"{tag}: vf {d_v}"
    assert d_p <= TOL, f"{tag}: logp {d_p}"
    if exact_actions:
        bad = np.flatnonzero((act != ref["actions"]).any(axis=1) & live)
        assert not len(bad), f"{tag}: drawn action differs on rows {bad[:8].tolist()} of {len(bad)}: {act[bad[:4]].tolist()} != {ref['actions'][bad[:4]].tolist()}"
    # rows in no list: a zero action, every other output untouched
    assert (act[~live] == 0).all() and (logp[~live] == SENTINEL).all() and (vf[~live] == SENTINEL).all() and (logits[~live] == SENTINEL).all(), f"{tag}: unlisted rows"
    return d_l, d_v


def _run_case(form, case, obs=None):
    inp = SR.build(case)
    bank = _bank(form, case["mode"], case["seed"])
    obs = np.ascontiguousarray(inp["obs30"][..., : inp["D"]]) if obs is None else obs
    assert bank.kernel_name(2 * case["n"], sampler=True) == FORMS[form][1]
    return inp, bank, obs, _sample(bank, obs, inp["sel"], uniforms=inp["uniforms"], crit_act=inp["crit_act"])


def _ids(group):
    return [c["name"] for c in SR.CASES if c["group"] == group]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", _ids("ragged"))
def test_ragged_uniform_lists(name, form):
    """(a) [N, 2] arenas of one mode, N around the 16-row wave and the 32- and 64-row tiles, non-zero critic actions, midpoint uniforms: every row;
    then greedy on the lists of that call (sel = None): the arg-max of policy_ref.decode and bit for bit the same vf.
    (b) the same data at observation stride 30 with NaN in every column neither the row's actor nor its partner's critic may read: bit for bit the
    same outputs"""
    case = SR.CASE_BY_NAME[name]
    inp, bank, obs, got = _run_case(form, case)
    _check(f"{form} {name}", inp["kinds"], got, inp["ref"])
    g = _sample(bank, obs, None, crit_act=inp["crit_act"], greedy=True)
    # the reference's arg-max is the kernel's wherever its winner leads by more than both sides' logit error; the rest is compared on the kernel's own logits
    for kind in SR.KINDS:
        idx = np.flatnonzero(inp["kinds"].reshape(-1) == kind)
        if len(idx):
            assert np.array_equal(g[0][idx], PR.decode(torch.from_numpy(g[3][idx]), PN.N_OUT[kind]).numpy())
            ref_l = torch.from_numpy(inp["greedy"]["logits"][idx, : PN.N_OUT[kind]])
            parts = ref_l.split(PN.ACTION_SPLIT[: SR.n_comp(kind)], dim=1)
            clear = torch.stack([p.topk(2, dim=1).values[:, 0] - p.topk(2, dim=1).values[:, 1] > 2 * TOL for p in parts], dim=1).all(dim=1).numpy()
            assert np.array_equal(g[0][idx][clear], inp["greedy"]["actions"][idx][clear])
    _check(f"{form} {name} greedy", inp["kinds"], g, inp["greedy"], exact_actions=False)
    assert np.array_equal(g[2], got[2]), "vf does not depend on how the action is chosen"
    assert np.array_equal(g[3], got[3])
    nan_obs = SR.with_garbage(inp)
    assert np.isnan(nan_obs).any() or case["mode"] == "escape"
    _, _, _, got30 = _run_case(form, case, obs=nan_obs)
    for a, b, what in zip(got, got30, ("actions", "logp", "vf", "logits")):
        assert np.isfinite(b).all() and np.array_equal(a, b), f"{name}: {what} at stride 30 with NaN beyond the rows' widths"


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", _ids("no-network") + _ids("four-nets"))
def test_mixed_lists(name, form):
    """(c) selector 0 on a third of the rows: arenas with one listed row (its critic still reads the unlisted partner's observation and critic action)
    and with none (NaN everywhere, nothing reads them); (d) Fight1, Fight2, Esc1 and Esc2 trainable in one bank, any pairing per arena: each row's critic
    takes the first d2 columns of row r ^ 1 whatever that row flies.  Unlisted rows: action 0, the other outputs keep their fill."""
    inp, bank, obs, got = _run_case(form, SR.CASE_BY_NAME[name])
    assert np.isnan(obs).any() and (inp["kinds"] < 0).any()
    _check(f"{form} {name}", inp["kinds"], got, inp["ref"])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", _ids("draw-edges"))
def test_draw_edges(name, form):
    """(e) u = 0 -> index 0, u = 1 - 2^-53 (1.0f once rounded to float) -> the last index of every component"""
    case = SR.CASE_BY_NAME[name]
    inp, bank, obs, got = _run_case(form, case)
    _check(f"{form} {name}", inp["kinds"], got, inp["ref"])
    for slot, kind in enumerate(SR.MODE_KINDS[case["mode"]]):
        last = np.array([12, 8, 1, 1 if PN.N_OUT[kind] == 26 else 0])
        assert (got[0].reshape(-1, 2, 4)[:, slot] == (0 if case["uniforms"] == "zero" else last)).all()


# ---------------------------------------------------------------------------------------------------------------- (f) controlled logits
def _bias_weights(bias_by_kind):
    """the fight networks of seed 5 with act_out = (0, bias): the logits are the bias, exactly, whatever the observation"""
    W = {}
    for kind in SR.MODE_KINDS["fight"]:
        sd, csd = SR.weights(5)[kind]
        sd = dict(sd)
        sd["act_out._model.0.weight"] = np.zeros_like(sd["act_out._model.0.weight"])
        sd["act_out._model.0.bias"] = np.asarray(bias_by_kind[kind], dtype=np.float32)
        W[kind] = (sd, csd)
    return W


def _bias(kind, base, peak=None, height=0.0):
    """per component the constant base[k]; peak[k] (an index, negative from the end) raised by `height`"""
    b, lo = np.zeros(PN.N_OUT[kind], dtype=np.float32), 0
    for k, w in enumerate(PN.ACTION_SPLIT[: SR.n_comp(kind)]):
        b[lo:lo + w] = base[k]
        if peak is not None:
            b[lo + peak[k] % w] += height
        lo += w
    return b


def _controlled(form, tag, bias_by_kind, uniforms, N=33):
    """load the bias networks into the form's spare bank, draw with `uniforms` ("midpoint" or an array [2 N, 4]) -> (kinds, got, ref, targets)"""
    key = (form, "controlled")
    W = _bias_weights(bias_by_kind)
    if key not in _banks:
        _banks[key] = _new_bank(form, SR.MODE_KINDS["fight"], W)
    bank = _banks[key]
    for slot, kind in enumerate(SR.MODE_KINDS["fight"]):
        bank.load_trainable(slot, kind, *W[kind])
    inp = SR.build("ragged-fight-33")     # its observations; the actor's output does not depend on them
    flat = inp["kinds"].reshape(-1)
    obs = np.ascontiguousarray(inp["obs30"][..., :26])
    targets = np.zeros((2 * N, 4), dtype=np.int64)
    if isinstance(uniforms, str):
        u = np.full((2 * N, 4), 0.5)
        for kind in SR.MODE_KINDS["fight"]:
            idx = np.flatnonzero(flat == kind)
            targets[idx] = SR.cycle_targets(len(idx), PN.N_OUT[kind])
            u[idx], _ = SR.midpoint_uniforms(np.tile(bias_by_kind[kind], (len(idx), 1)), PN.N_OUT[kind], targets[idx])
    else:
        u = uniforms
    got = _sample(bank, obs, inp["sel"], uniforms=u.reshape(N, 2, 4), crit_act=inp["crit_act"])
    ref = SR.sample_ref(flat, W, obs.reshape(2 * N, 26), inp["crit_act"], u, False)
    for kind in SR.MODE_KINDS["fight"]:
        idx = np.flatnonzero(flat == kind)
        assert np.array_equal(got[3][idx, : PN.N_OUT[kind]], np.tile(bias_by_kind[kind], (len(idx), 1))), f"{tag}: the logits are the bias, bit for bit"
        assert np.array_equal(ref["logits"][idx, : PN.N_OUT[kind]], np.tile(bias_by_kind[kind], (len(idx), 1)))
    _check(f"{form} {tag}", inp["kinds"], got, ref)
    return inp, bank, obs, got, ref, targets


@pytest.mark.parametrize("form", list(FORMS))
def test_tied_logits(form):
    """all logits of a component equal: greedy takes index 0 (torch.argmax's first maximum), a draw splits [0, 1) evenly"""
    bias = {k: _bias(k, (0.25, -0.5, 1.0, 0.0)) for k in SR.MODE_KINDS["fight"]}
    inp, bank, obs, got, ref, targets = _controlled(form, "tied", bias, "midpoint")
    assert np.array_equal(got[0], targets.astype(np.int8))
    g = _sample(bank, obs, None, crit_act=inp["crit_act"], greedy=True)
    assert (g[0] == 0).all()
    want = -(np.log(13.0) + np.log(9.0) + np.log(2.0))
    assert np.abs(g[1].reshape(-1, 2)[:, 0] - (want - np.log(2.0))).max() <= TOL and np.abs(g[1].reshape(-1, 2)[:, 1] - want).max() <= TOL


@pytest.mark.parametrize("form", list(FORMS))
def test_peaked_logits(form):
    """one logit 30 above the rest: the others share e^-30 = 9.4e-14 of the mass each.  The peak is the LAST index of its component, so that every
    other interval lies next to 0, where a float resolves it (the kernels draw with (float) u: next to 1 a float steps by 6e-8, and an interval 9.4e-14
    wide behind a peak cannot be addressed by any u the kernel can see).  A midpoint then sits half an interval = at least 1 / 26 of its own value away
    from both neighbours — against 1e-6 relative error of the device's exp and sum — so every index is hit exactly; logp of a -30 action against float64."""
    bias = {k: _bias(k, (0.0, 0.5, -0.25, 1.0), peak=(-1, -1, -1, -1), height=30.0) for k in SR.MODE_KINDS["fight"]}
    inp, bank, obs, got, ref, targets = _controlled(form, "peaked", bias, "midpoint")
    assert np.array_equal(ref["actions"], targets.astype(np.int8)) and np.array_equal(got[0], targets.astype(np.int8))
    assert np.abs(got[1] - ref["logp"]).max() <= TOL
    assert ref["logp"].min() < -85.0      # rows with three -30 actions (the two 2-wide components take turns at their peak)


@pytest.mark.parametrize("form", list(FORMS))
def test_saturated_logits(form):
    """one logit 200 above the rest, in the MIDDLE of its component: every other index has no mass a float can hold (e^-200).  Whatever the uniform —
    the midpoint of the peak's interval or 1 - 2^-53, which a float rounds to 1 — the draw is the peak, as the float64 inverse CDF gives, and logp is 0,
    not -200 per component"""
    peak = (5, 4, 0, 1)
    bias = {k: _bias(k, (0.0, 0.0, 0.0, 0.0), peak=peak, height=200.0) for k in SR.MODE_KINDS["fight"]}
    for tag, u in (("saturated-midpoint", np.full((66, 4), 0.5)), ("saturated-one", np.full((66, 4), SR.ONE_BELOW))):
        inp, bank, obs, got, ref, _ = _controlled(form, tag, bias, u)
        for slot, kind in enumerate(SR.MODE_KINDS["fight"]):
            want = np.array(peak[: SR.n_comp(kind)] + (0,) * (4 - SR.n_comp(kind)))
            assert (ref["actions"].reshape(-1, 2, 4)[:, slot] == want).all() and (got[0].reshape(-1, 2, 4)[:, slot] == want).all(), tag
        assert np.isfinite(got[1]).all() and np.abs(got[1] - ref["logp"]).max() <= TOL


# ------------------------------------------------------------------------------------------------------------------ (g) form selection
def test_form_selection_boundary():
    """left to itself (HH_POLICY_W, HH_POLICY_TILE unset) the sampler takes the streamed form for more than 40 rows per CU (hhp_sampler_is_w16)"""
    from hhmarl_2d_amd.pilots import PolicyBank
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    with _env(HH_POLICY_W=None, HH_POLICY_TILE=None):
        bank = PolicyBank(torch.device("cuda", 0), 64)
    for slot, kind in enumerate(SR.MODE_KINDS["escape"]):
        bank.load_trainable(slot, kind, *SR.weights(5)[kind])
    assert bank.kernel_name(40 * n_cu, sampler=True) == "hh_k_policy_ppo"
    assert bank.kernel_name(40 * n_cu + 2, sampler=True) == "hh_k_policy_w16_ppo"
    assert bank.kernel_name(2, sampler=True) == "hh_k_policy_ppo"
    bank.close()


# ------------------------------------------------------------------------------------------------------------- (h) the production path
@pytest.mark.parametrize("form", list(FORMS))
def test_ppo_rollout_at_a_ragged_size(form):
    """PPORollout (fight, level 3) at 97 arenas — one full tile and a ragged one per network in either form: what every tick stored (logits, vf, logp,
    actions) against the restatement of the observation it stored, zero critic actions"""
    from hhmarl_2d_amd.world import World, make_config
    from hhmarl_2d_amd.rollout import PPORollout
    N, T = 97, 4
    bank = _bank(form, "fight", 5)
    w = World(make_config(n_arenas=N, level=3, seed=31, auto_reset=True), device=0)
    ro = PPORollout(w, bank, T, record_logits=True)
    ro.collect()
    torch.cuda.synchronize()
    obs, logits, vf, logp, act = (x.cpu().numpy() for x in (ro.obs, ro.logits, ro.vf, ro.logp, ro.actions))
    kinds = np.tile(np.array(SR.MODE_KINDS["fight"]), (N, 1))
    for t in range(T + 1):
        ref = SR.sample_ref(kinds, SR.weights(5), obs[t].reshape(2 * N, -1), None, None, True)
        if t == T:   # the bootstrap value of the observation behind the last tick
            assert np.abs(vf[t].reshape(-1) - ref["vf"]).max() <= TOL
            break
        got = (act[t].reshape(-1, 4), logp[t].reshape(-1), vf[t].reshape(-1), logits[t].reshape(-1, 32))
        _check(f"{form} rollout-97 tick {t}", kinds, got, ref, exact_actions=False)
        assert (got[0] >= 0).all() and (got[0] <= np.array([12, 8, 1, 1])).all() and (got[0].reshape(N, 2, 4)[:, 1, 3] == 0).all()
    assert len(np.unique(act[..., 0])) > 6, "a draw, not the arg-max"
