"""The commander's device path — hh_k_commander behind CommanderNet.sample and hh_k_commander_chain behind CommanderNet.act_chain — against the
arena-by-arena restatement of tests/commander_sampler_ref.py at ragged tiles, fresh arenas and the edges of the draw.

Every row of every case is compared, nothing is sub-sampled: logits, vf and h_out (BOTH states) within TOL = 1e-5 of float64 — the bound
tests/test_gpu_commander.py and tests/test_gpu_commander_chain.py hold the commander to; it does not follow the measurements — the drawn action
EQUAL to the target and the greedy action EQUAL to the float64 arg-max (tests/test_commander_sampler_edges_host.py shows why no row needs
excluding), logp within TOL of log_softmax of the kernel's own logits at its own action.  h_out is compared on every row because the logits do
not pin the GRU stage: a lost lo plane of a GRU matrix moves them by about TOL itself and the state by 2e-4 (the host test's table; on the
device, with both W_hh packed without their lo plane, the 33- and 30-row cases stayed inside TOL in logits and vf — 6.9e-6 to 8.5e-6 and 4.3e-6 to
5.7e-6 — and left it in h_out only, at 1.7e-4 to 2.1e-4).
Each check prints the distances it measured and e32, the distance of the float32 torch restatement from float64 (`pytest -s`).

Every call goes through `_call`: all output buffers and h_in are allocated for two arenas more than the call has, pre-filled with a sentinel, and
the tail must still hold it afterwards — in every test of this file, not only in test_guard_rows."""
import numpy as np
import pytest
import torch

import commander_sampler_ref as SR

pytestmark = pytest.mark.gpu
TOL = SR.TOL
SENTINEL, SENTINEL_ACT = -777.0, 77
GUARD = 2                                   # arenas behind the call's own in every buffer
_nets = {}


def _net(which="case"):
    """one net per weight set, shared by the cases: "case" holds SR.weights(); "exact" is reloaded with a bias triple's weights by its tests"""
    from hhmarl_2d_amd.commander import CommanderNet
    if which not in _nets:
        _nets[which] = CommanderNet(0, SR.MAX_ROWS).set_weights(SR.weights())
    return _nets[which]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _call(net, obs, h_in, fresh=None, uniforms=None, crit_act=None, greedy=False, world=None, want_vf=True, want_logits=True):
    """one call of N arenas on numpy (or CUDA) inputs -> dict of numpy outputs (actions, logp, vf, logits, h_out, h_in afterwards), None where not
    asked for.  Guard rows: see the module's docstring"""
    N = int(obs.shape[0])
    M = N + GUARD
    cu = lambda a, dt: None if a is None else (a if torch.is_tensor(a) else torch.tensor(np.asarray(a))).to(device="cuda", dtype=dt).contiguous()
    full = lambda shape, v, dt=torch.float32: torch.full(shape, v, dtype=dt, device="cuda")
    buf = dict(h_in=full((M, 3, 2, 200), SENTINEL), h_out=full((M, 3, 2, 200), SENTINEL), actions=full((M, 3), SENTINEL_ACT, torch.int8),
               logp=full((M, 3), SENTINEL), vf=full((M, 3), SENTINEL), logits=full((M, 3, 4), SENTINEL))
    buf["h_in"][:N] = cu(h_in, torch.float32)
    net.sample(cu(obs, torch.float32), buf["h_in"][:N], buf["h_out"][:N], fresh=cu(fresh, torch.uint8), world=world, uniforms=cu(uniforms, torch.float64),
               crit_act=cu(crit_act, torch.float32), greedy=greedy, actions=buf["actions"][:N], logp=buf["logp"][:N],
               vf=buf["vf"][:N] if want_vf else None, logits=buf["logits"][:N] if want_logits else None, want_vf=want_vf)
    torch.cuda.synchronize()
    out = {}
    for k, t in buf.items():
        a = t.cpu().numpy()
        fill = SENTINEL_ACT if k == "actions" else np.float32(SENTINEL)
        assert (a[N:] == fill).all(), f"{k}: rows beyond 3 N were written"
        if (k == "vf" and not want_vf) or (k == "logits" and not want_logits):
            assert (a == fill).all(), f"{k}: written though not asked for"
            out[k] = None
        else:
            out[k] = a[:N]
    return out


def _run_case(name, **kw):
    inp = SR.build(name)
    args = dict(fresh=inp["fresh"], uniforms=inp["uniforms"], crit_act=inp["crit_act"])
    args.update(kw)
    return inp, _call(_net(), inp["obs"], inp["h_in"], **args)


def _own_logp(got):
    """float64 log_softmax of the kernel's own logits at its own action"""
    lg = got["logits"][..., :3].astype(np.float64)
    m = lg.max(-1, keepdims=True)
    lsm = (lg - m) - np.log(np.exp(lg - m).sum(-1, keepdims=True))
    return np.take_along_axis(lsm, got["actions"].astype(np.int64)[..., None], -1)[..., 0]


def _check(tag, inp, got, want_actions):
    """every row of one call against the float64 restatement"""
    ref, e32 = inp["ref"], inp["e32"]
    for k in ("logits", "vf", "h_out", "logp"):
        assert np.isfinite(got[k]).all(), f"{tag}: {k} not finite"
    d_l = float(np.abs(got["logits"][..., :3] - ref["logits"]).max())
    d_v = float(np.abs(got["vf"] - ref["vf"]).max())
    d_ha = float(np.abs(got["h_out"][:, :, 0] - ref["h_out"][:, :, 0]).max())
    d_hv = float(np.abs(got["h_out"][:, :, 1] - ref["h_out"][:, :, 1]).max())
    d_p = float(np.abs(got["logp"] - _own_logp(got)).max())
    print(f"commander-edges {tag}: rows {3 * inp['n']} max|dlogits| {d_l:.3e} (e32 {e32['logits']:.3e}) max|dvf| {d_v:.3e} (e32 {e32['vf']:.3e}) "
          f"max|dh_out| act {d_ha:.3e} val {d_hv:.3e} (e32 {e32['h_out']:.3e}) max|dlogp| {d_p:.3e}")
    assert d_l <= TOL, f"{tag}: logits {d_l}"
    assert d_v <= TOL, f"{tag}: vf {d_v}"
    assert d_ha <= TOL and d_hv <= TOL, f"{tag}: h_out {d_ha} {d_hv}"
    assert d_p <= TOL, f"{tag}: logp {d_p}"
    bad = np.argwhere(got["actions"] != want_actions)
    assert not len(bad), f"{tag}: action differs on (arena, slot) {bad[:8].tolist()} of {len(bad)}"
    assert _same(got["h_in"], inp["h_used"]), f"{tag}: h_in afterwards is not 0 in fresh arenas and what was given elsewhere"
    assert _same(got["logits"][..., 3], np.zeros_like(got["logits"][..., 3])), f"{tag}: logits column 3"


@pytest.mark.parametrize("name", SR.names("ragged") + SR.names("fresh"))
def test_ragged_and_fresh_cases(name):
    """3 N either side of one, two and three 32-row tiles with an arena split 2|1 and 1|2 across an edge (`ragged`); no arena, every arena, every
    other arena and only the straddling arenas fresh, with NaN in the state a fresh arena brings (`fresh`): every output of every row, the drawn
    action = the target (r + r // 3) % 3; then greedy: the float64 arg-max on every row, the forward's bytes unchanged"""
    inp, got = _run_case(name)
    assert np.array_equal(inp["ref"]["actions"], inp["targets"])
    _check(name, inp, got, inp["targets"])
    g = _call(_net(), inp["obs"], inp["h_in"], fresh=inp["fresh"], crit_act=inp["crit_act"], greedy=True)
    _check(f"{name} greedy", inp, g, inp["ref"]["greedy"])
    for k in ("logits", "vf", "h_out", "h_in"):
        assert _same(g[k], got[k]), f"{name}: {k} depends on how the action is chosen"


@pytest.mark.parametrize("name", SR.names("draw-edges"))
def test_draw_edges(name):
    """u = 0 -> action 0, u = 1 - 2^-53 (1.0f once rounded to float) -> action 2, on every row"""
    inp, got = _run_case(name)
    want = 0 if inp["case"]["uniforms"] == "zero" else 2
    assert (inp["ref"]["actions"] == want).all()
    _check(name, inp, got, np.full((inp["n"], 3), want))


def _exact_net(bias):
    net = _net("exact")
    net.set_weights(SR.exact_weights(bias))
    return net


def test_exact_logits():
    """act_out's weight zero: the logits are the bias triple bit for bit, so the draw's own float32 arithmetic is tested on logits without the MFMA
    path's error — ties, a component float32 cannot hold (e^-200) in each position, a gap of 80; u = 0, u = 1 - 2^-53 and 1e-3 either side of every CDF
    boundary; greedy = the FIRST arg-max.  33 rows per call (a tile edge), every row the same uniform."""
    inp = SR.build("ragged-11")
    N = inp["n"]
    for row in SR.exact_table():
        net = _exact_net(row["bias"])
        bias = np.tile(np.array(row["bias"] + (0.0,), dtype=np.float32), (N, 3, 1))
        lsm = None
        for u, want, logp64 in zip(row["uniforms"], row["expected"], row["logp64"]):
            got = _call(net, inp["obs"], inp["h_in"], fresh=inp["fresh"], uniforms=np.full((N, 3), u), crit_act=inp["crit_act"])
            assert _same(got["logits"], bias), f"bias {row['bias']}: the logits are not the bias, bit for bit"
            assert (got["actions"] == want).all(), f"bias {row['bias']} u {u!r}: drew {np.unique(got['actions']).tolist()}, the float32 inverse CDF gives {want}"
            assert np.isfinite(got["logp"]).all()
            d = float(np.abs(got["logp"].astype(np.float64) - logp64).max())
            assert d <= TOL, f"bias {row['bias']} u {u!r}: logp {d}"
            lsm = d if lsm is None else max(lsm, d)
        g = _call(net, inp["obs"], inp["h_in"], fresh=inp["fresh"], crit_act=inp["crit_act"], greedy=True)
        b = np.array(row["bias"])
        want_lp = (b - b.max() - np.log(np.exp(b - b.max()).sum()))[row["greedy"]]
        assert _same(g["logits"], bias) and (g["actions"] == row["greedy"]).all(), f"bias {row['bias']}: greedy is not the first arg-max"
        assert np.abs(g["logp"].astype(np.float64) - want_lp).max() <= TOL
        print(f"commander-edges exact-logits {row['bias']}: {len(row['uniforms'])} uniforms, max|dlogp| {lsm:.3e}")
        # the rest of the network does not see act_out: vf and both states as with the case's own weights
        ref = inp["ref"]
        assert np.abs(g["vf"] - ref["vf"]).max() <= TOL and np.abs(g["h_out"] - ref["h_out"]).max() <= TOL


@pytest.mark.parametrize("name", ["ragged-11", "ragged-32"])
def test_guard_rows(name):
    """a call of N arenas on buffers of N + 2: the last two arenas' worth of actions, logp, vf, logits, h_out and h_in keep their fill (asserted inside
    _call), with the arenas in front of them fresh or not"""
    inp = SR.build(name)
    for fresh in (inp["fresh"], np.ones_like(inp["fresh"]), None):
        got = _call(_net(), inp["obs"], inp["h_in"], fresh=fresh, uniforms=inp["uniforms"], crit_act=inp["crit_act"])
        assert all((got[k] != (SENTINEL_ACT if k == "actions" else np.float32(SENTINEL))).all() for k in ("actions", "logp", "vf", "h_out"))
        assert (got["logits"][..., :3] != np.float32(SENTINEL)).all()


def test_optional_outputs():
    """vf = NULL and logits = NULL leave everything else alone: the same bytes in actions, logp and h_out"""
    inp, both = _run_case("ragged-33")
    for kw in (dict(want_vf=False), dict(want_logits=False), dict(want_vf=False, want_logits=False)):
        _, got = _run_case("ragged-33", **kw)
        for k in ("actions", "logp", "h_out", "h_in"):
            assert _same(got[k], both[k]), (kw, k)
        for k in ("vf", "logits"):
            assert got[k] is None or _same(got[k], both[k]), (kw, k)


def _permuted(inp, perm):
    return dict(obs=inp["obs"][perm], h_in=inp["h_in"][perm], fresh=inp["fresh"][perm], crit_act=inp["crit_act"][perm], uniforms=inp["uniforms"][perm])


def test_position_independence():
    """what the chain's header relies on ("bit for bit what hh_commander_sample gives for the same row and h_in"): a row's result does not depend on
    where in the call it sits — each row's contraction runs the same instruction sequence whatever the tile and the lane.  43 arenas in a fixed random
    order return the permuted bytes of the call in the given order, and an arena alone returns the bytes of its rows in the large call"""
    inp, base = _run_case("ragged-43")
    N = inp["n"]
    perm = np.random.default_rng(43).permutation(N)
    assert (perm != np.arange(N)).sum() > N // 2 and ((3 * perm) // 32 != (3 * np.arange(N)) // 32).sum() > N // 2     # most arenas change tile
    p = _permuted(inp, perm)
    got = _call(_net(), p["obs"], p["h_in"], fresh=p["fresh"], uniforms=p["uniforms"], crit_act=p["crit_act"])
    for k in ("actions", "logp", "vf", "logits", "h_out", "h_in"):
        rows = np.argwhere((_bits(got[k]) != _bits(base[k][perm])).reshape(N, -1).any(axis=1)).reshape(-1)
        assert not len(rows), f"{k}: arenas {perm[rows][:8].tolist()} differ once moved to positions {rows[:8].tolist()}"
    alone = sorted(set(SR.straddlers(N).tolist()) | {0, 31, 32, N - 1})
    assert {10, 21, 42} <= set(alone)
    for n in alone:
        one = _permuted(inp, np.array([n]))
        got = _call(_net(), one["obs"], one["h_in"], fresh=one["fresh"], uniforms=one["uniforms"], crit_act=one["crit_act"])
        for k in ("actions", "logp", "vf", "logits", "h_out", "h_in"):
            assert _same(got[k], base[k][n:n + 1]), f"{k}: arena {n} alone differs from its rows in the call of {N}"


@pytest.mark.parametrize("arena", [3, 10])
def test_critic_gather_is_local(arena):
    """the value branch of a row gathers the other two slots of ITS arena (arena 10 of 11: across the tile edge).  Another observation and crit_act
    on slot 1 of one arena change vf and the value state of that arena's three rows, the logits and the actor state of its row 1, and no other byte"""
    inp, base = _run_case("ragged-11")
    obs, ca = inp["obs"].copy(), inp["crit_act"].copy()
    obs[arena, 1] = np.random.default_rng(arena).random(34, dtype=np.float32)
    ca[arena, 1] = (ca[arena, 1] + 0.5) % 1.5
    got = _call(_net(), obs, inp["h_in"], fresh=inp["fresh"], uniforms=inp["uniforms"], crit_act=ca)
    others = np.arange(inp["n"]) != arena
    for k in ("actions", "logp", "vf", "logits", "h_out", "h_in"):
        assert _same(got[k][others], base[k][others]), f"{k}: another arena changed"
    assert (got["vf"][arena] != base["vf"][arena]).all(), "vf of all three rows reads slot 1"
    assert all((got["h_out"][arena, s, 1] != base["h_out"][arena, s, 1]).any() for s in range(3))
    for s in (0, 2):                                        # the actor reads its own row only
        assert _same(got["logits"][arena, s], base["logits"][arena, s]) and _same(got["h_out"][arena, s, 0], base["h_out"][arena, s, 0])
        assert got["actions"][arena, s] == base["actions"][arena, s] and _same(got["logp"][arena, s], base["logp"][arena, s])
    assert (got["logits"][arena, 1, :3] != base["logits"][arena, 1, :3]).any() and (got["h_out"][arena, 1, 0] != base["h_out"][arena, 1, 0]).any()
    assert _same(got["h_in"], base["h_in"])
    # ... and each of the two inputs alone reaches all three rows' vf: slot 1 is "the other agent" of rows 0 and 2 in different input blocks
    only_act = _call(_net(), inp["obs"], inp["h_in"], fresh=inp["fresh"], uniforms=inp["uniforms"], crit_act=ca)
    assert (only_act["vf"][arena] != base["vf"][arena]).all() and _same(only_act["logits"], base["logits"])
    assert _same(only_act["vf"][others], base["vf"][others])


def test_two_runs_give_the_same_bytes():
    _, a = _run_case("ragged-97")
    _, b = _run_case("ragged-97")
    assert all(_same(a[k], b[k]) for k in a)


def test_keyed_draws_on_every_row(oracle):
    """the draws keyed by (seed, arena, episode, steps, agent, site 27, 0) on EVERY row of a 97-arena world whose arenas are in different episodes
    at different steps — with every episode counter still 0 a key that ignored it would pass"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.env_hier import macro_step
    from hhmarl_2d_amd.pilots import RandomPilot
    from hhmarl_2d_amd.world import World, make_config
    from test_gpu_commander import _check_draws
    N, seed, offset = 97, 13, 700
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=seed, arena_offset=offset, auto_reset=True, horizon=40), device=0)
    obs = w.reset()
    pilot = RandomPilot(w.device, seed=2)
    g = torch.Generator(device="cuda").manual_seed(1)
    for k in range(40):
        obs = macro_step(w, torch.randint(0, 3, (N, 3), device="cuda", dtype=torch.int8, generator=g), pilot)[0]
        st = w.get_state()["ar_i"]          # steps, ..., episode (column 5)
        if len(np.unique(st[:, 5])) >= 2 and len(np.unique(st[:, 0])) >= 2:
            break
    print(f"keyed draws: after {k + 1} commander steps episode counters {np.unique(st[:, 5]).tolist()} step counters {np.unique(st[:, 0]).tolist()}")
    assert len(np.unique(st[:, 5])) >= 2 and st[:, 5].max() > 0, "every arena in the same episode"
    assert len(np.unique(st[:, 0])) >= 2, "every arena at the same step"
    net = _net()
    h = torch.zeros((N, 3, 2, 200), device="cuda")
    got = _call(net, obs.contiguous(), h, world=w)
    lib = oracle.lib()
    u = np.array([[lib.hho_rng_u01(seed, offset + n, int(st[n, 5]), int(st[n, 0]), s + 1, 27, 0) for s in range(3)] for n in range(N)])
    t = lambda k: torch.from_numpy(got[k])
    _check_draws(t("logits"), u, t("actions"), t("logp"), need_clear=0.99)
    for s in range(3):
        assert len(np.unique(got["actions"][:, s])) == 3
    again = _call(net, obs.contiguous(), h, world=w)
    assert _same(again["actions"], got["actions"]) and _same(again["logp"], got["logp"])       # keyed, not a stream


# --------------------------------------------------------------------------------------------------------------------------- the chain
def _chain_obs(N, nA, seed):
    rng = np.random.default_rng([seed, N, nA])
    obs = rng.random((N, nA, 34), dtype=np.float32)
    obs[:, :, 4:24] *= rng.random((N, nA, 1)) > 0.2
    obs *= rng.random((N, nA, 1)) > 0.15
    return obs


def _chain(net, obs, want_h=True, want_logits=True):
    """act_chain on buffers of N + 2 arenas pre-filled with a sentinel; the tail must keep it -> numpy (actions, h_out, logits)"""
    N, nA = obs.shape[:2]
    M = N + GUARD
    act = torch.full((M, nA), SENTINEL_ACT, dtype=torch.int8, device="cuda")
    h = torch.full((M, nA, 200), SENTINEL, device="cuda")
    lg = torch.full((M, nA, 4), SENTINEL, device="cuda")
    net.act_chain(torch.from_numpy(obs).cuda().contiguous(), actions=act[:N], h_out=h[:N] if want_h else None, logits=lg[:N] if want_logits else None)
    torch.cuda.synchronize()
    act, h, lg = act.cpu().numpy(), h.cpu().numpy(), lg.cpu().numpy()
    assert (act[N:] == SENTINEL_ACT).all() and (h[N:] == np.float32(SENTINEL)).all() and (lg[N:] == np.float32(SENTINEL)).all(), "rows beyond N were written"
    assert want_h or (h == np.float32(SENTINEL)).all()
    assert want_logits or (lg == np.float32(SENTINEL)).all()
    return act[:N], h[:N] if want_h else None, lg[:N] if want_logits else None


def test_chain_takes_the_first_arg_max_of_tied_logits():
    N, nA = 33, 5
    obs = _chain_obs(N, nA, 1)
    for row in SR.exact_table():
        if row["bias"] not in [tuple(map(float, b)) for b in SR.TIES]:
            continue
        act, h, lg = _chain(_exact_net(row["bias"]), obs)
        assert _same(lg, np.tile(np.array(row["bias"] + (0.0,), dtype=np.float32), (N, nA, 1))), f"bias {row['bias']}: the logits are not the bias, bit for bit"
        assert (act == row["greedy"]).all(), f"bias {row['bias']}: links chose {np.unique(act).tolist()}, the first arg-max is {row['greedy']}"
        assert np.isfinite(h).all() and (np.abs(h) <= 1.0).all()


@pytest.mark.parametrize("N,nA", [(33, 5), (11, 1), (32, 3)])
def test_chain_guard_rows_and_optional_outputs(N, nA):
    obs = _chain_obs(N, nA, 2)
    act, h, lg = _chain(_net(), obs)
    assert (act >= 0).all() and (act <= 2).all() and (h != np.float32(SENTINEL)).all() and (lg[..., :3] != np.float32(SENTINEL)).all()
    assert _same(lg[..., 3], np.zeros_like(lg[..., 3]))
    assert np.array_equal(act, np.argmax(lg[..., :3], axis=-1))
    for kw in (dict(want_h=False), dict(want_logits=False), dict(want_h=False, want_logits=False)):
        a2, h2, lg2 = _chain(_net(), obs, **kw)
        assert np.array_equal(a2, act), kw
        assert (h2 is None or _same(h2, h)) and (lg2 is None or _same(lg2, lg)), kw


def test_chain_arena_permutation():
    """65 arenas (two tiles and one arena) x 3 agents in a fixed random order: the permuted bytes"""
    N, nA = 65, 3
    obs = _chain_obs(N, nA, 3)
    perm = np.random.default_rng(65).permutation(N)
    base = _chain(_net(), obs)
    got = _chain(_net(), np.ascontiguousarray(obs[perm]))
    for k, a, b in zip(("actions", "h_out", "logits"), got, base):
        assert _same(a, b[perm]), k
