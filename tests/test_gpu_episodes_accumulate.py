"""hh_episodes_emit_append / hh_commander_episodes_emit_append (train_batch_size) on the MI355X, on synthetic collects (no world) in
the style of tests/test_gpu_episodes_aux.py: keyed random rows with random done flags, episodes of at most carry_cap + 1 rows, K = 8
consecutive calls of T = 5 ticks with carry_cap = 11; N = 3, 300 and 1100 arenas (1100: the scan's threads sum runs of two arenas); the
2-vs-2 geometry (2 agents, D = 26, aux 32) and the commander's (3 x 34, L = 4, with states, aux 4), each with and without the aux column.
Everything is compared byte for byte with the host restatement (tests/episodes_ref.py per collect, tests/episodes_accumulate_ref.py for
the accumulation): every column, the tables, state_in, carried, the counts and the accumulator."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from episode_metrics_ref import EPS, bounds, restate_metrics
from episodes_accumulate_ref import accumulate, batch_keys
from episodes_ref import restate

pytestmark = pytest.mark.gpu
T, K, CAP, L_SEQ = 5, 8, 11, 4
GEOMETRY = {"2v2": dict(nA=2, D=26, aux_dim=32, act=(4,), commander=False), "commander": dict(nA=3, D=34, aux_dim=4, act=(), commander=True)}
CASES = [(g, N, aux) for g in GEOMETRY for N in (3, 300, 1100) for aux in (False, True)]
CASE_IDS = [f"{g}-N{N}-{'aux' if aux else 'plain'}" for g, N, aux in CASES]
SMALL = [(g, N, aux) for g, N, aux in CASES if N <= 300 and (aux or N == 300)]
SMALL_IDS = [f"{g}-N{N}-{'aux' if aux else 'plain'}" for g, N, aux in SMALL]
QUIET = 4       # the collect that ends no episode in the streams of the fourth test
MARK = 12345.0


def _stream(N, nA, D, aux_dim, act_shape, seed, with_state=False, quiet=None):
    """K T ticks of rows (numpy, [K T, N, ...]); an episode ends with probability 0.15 per tick and at the latest on its (CAP + 1)-th row.
    quiet = k: no arena ends an episode in collect k (every arena ends one on the tick before it, so that none outgrows the carry)"""
    rng = np.random.default_rng(seed)
    n = K * T
    s = {"obs": rng.standard_normal((n, N, nA, D), dtype=np.float32),
         "actions": rng.integers(0, 13, (n, N, nA) + act_shape).astype(np.int8),
         "logp": -rng.random((n, N, nA), dtype=np.float32), "vf": rng.standard_normal((n, N, nA), dtype=np.float32),
         "reward": rng.standard_normal((n, N, nA), dtype=np.float32), "valid": rng.integers(0, 2, (n, N, nA)).astype(np.uint8),
         "aux": rng.standard_normal((n, N, nA, aux_dim), dtype=np.float32)}
    done = (rng.random((n, N)) < 0.15).astype(np.uint8)
    run = np.zeros(N, dtype=np.int64)
    for t in range(n):
        run += 1
        done[t, run >= CAP + 1] = 1
        if quiet is not None:
            if t == quiet * T - 1:
                done[t] = 1
            elif t // T == quiet:
                done[t] = 0
        run[done[t] != 0] = 0
    s["done"] = done
    if with_state:
        s["state_in"] = rng.standard_normal((n, N, nA, 2, 200), dtype=np.float32)
    return s


@functools.lru_cache(maxsize=None)
def _reference(geometry, N, quiet=None):
    """-> (the stream, the per-collect restatement with the aux column as "aux", carried [K, N] after every collect): computed once per
    case, shared by the tests and never modified"""
    g = GEOMETRY[geometry]
    seq = L_SEQ if g["commander"] else None
    s = _stream(N, g["nA"], g["D"], g["aux_dim"], g["act"], seed=4000 * N + g["D"] + (0 if quiet is None else 17), with_state=g["commander"],
                quiet=quiet)
    cols = ("obs", "actions", "logp", "vf", "reward", "valid", "done") + (("state_in",) if seq else ())
    per = restate([{k: s[k][c * T:(c + 1) * T] for k in cols} for c in range(K)], seq, gamma=0.99, lam=0.95)[0]
    # the restatement with the aux rows in place of obs: its emitted obs is the expected aux column (tests/test_gpu_episodes_aux.py)
    aux = restate([{k: (s["aux"] if k == "obs" else s[k])[c * T:(c + 1) * T] for k in cols} for c in range(K)], seq, gamma=0.99, lam=0.95)[0]
    per = [dict(p, aux=a["obs"]) for p, a in zip(per, aux)]
    carried = np.zeros((K, N), dtype=np.int32)
    for k in range(K):
        d = s["done"][:(k + 1) * T]
        last = np.where(d.any(axis=0), d.shape[0] - 1 - np.argmax(d[::-1], axis=0), -1)
        carried[k] = (k + 1) * T - 1 - last
    for v in s.values():
        v.setflags(write=False)
    return s, per, carried


def _total(per):
    return sum(len(p["t"]) for p in per)


class _Emitter:
    """device buffers of one emitter fed from a host stream, T ticks per call; aux: record the column; B: train_batch_size"""

    def __init__(self, stream, aux, commander=False, B=None, metrics=False):
        from hhmarl_2d_amd.commander import CommanderEpisodeBatch
        from hhmarl_2d_amd.rollout import EpisodeBatch
        self.s = stream
        self.names = [k for k in stream if k != "aux"] + (["aux"] if aux else [])
        self.dev = {k: torch.zeros(stream[k][:T].shape, dtype=torch.from_numpy(stream[k][:1].copy()).dtype, device="cuda") for k in self.names}
        collect = {k: v for k, v in self.dev.items() if k != "aux"}
        a = ("aux", self.dev["aux"]) if aux else None
        kw = dict(aux=a, metrics=metrics, train_batch_size=B)
        self.eb = (CommanderEpisodeBatch(collect, L_SEQ, CAP, 0.99, 0.95, **kw) if commander else EpisodeBatch(collect, CAP, 0.99, 0.95, **kw))
        self.seq = commander

    def upload(self, k):
        for name in self.names:
            self.dev[name].copy_(torch.from_numpy(self.s[name][k * T:(k + 1) * T].copy()))   # the shared stream is read-only
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(self, k):
        """upload collect k, emit through the batch's own path -> the emitted parts as numpy"""
        self.eb.emit(self.upload(k))
        return {k2: v.cpu().numpy() for k2, v in self.eb.rows().items()}

    def state(self):
        """(acc i32 [8] or None, counts (rows, episodes, sequences of the last call), carried [N]) as numpy"""
        c = self.eb._counts.cpu().numpy()
        acc = None if self.eb._acc is None else self.eb._acc.cpu().numpy()
        return acc, (int(c[0]), int(c[1]), int(c[3]) if self.seq else 0), self.eb.carried.cpu().numpy()


def _emitter(geometry, N, aux, **kw):
    return _Emitter(_reference(geometry, N, kw.pop("quiet", None))[0], aux, commander=GEOMETRY[geometry]["commander"], **kw)


def _same(got, want, keys, what):
    for k in keys:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {k} is {g.dtype} {g.shape}, the restatement {w.dtype} {w.shape}"
        assert g.tobytes() == w.tobytes(), f"{what}: {k} differs from the restatement"


def _keys(geometry, aux):
    return batch_keys(GEOMETRY[geometry]["commander"]) + (("aux",) if aux else ())


def _check_call(e, got, ref_entry, carried, keys, what):
    batch, acc, counts = ref_entry
    assert set(got) == set(keys), what
    _same(got, batch, keys, what)
    d_acc, d_counts, d_carried = e.state()
    assert d_acc.tolist() == acc.tolist(), f"{what}: acc {d_acc.tolist()}, the restatement {acc.tolist()}"
    assert d_counts == counts, f"{what}: counts {d_counts}, the restatement {counts}"
    assert np.array_equal(d_carried, carried), f"{what}: carried"
    assert int(e.eb.n_rows) == acc[0] and int(e.eb.n_episodes) == acc[1]
    info = e.eb.batch_info()
    assert info == dict(rows=acc[0], episodes=acc[1], sequences=acc[3], collects=acc[5], batches=acc[6]) and e.eb.ready() == bool(acc[4])
    assert all(type(v) is int for v in info.values())


@pytest.mark.parametrize("geometry,N,aux", CASES, ids=CASE_IDS)
def test_a_batch_larger_than_the_stream_is_the_shifted_concatenation(geometry, N, aux):
    """B above everything the K collects emit: after every call the batch is the shifted concatenation of the per-collect batches.  Before
    each call adv / target beyond acc[0] are filled with NaN: the call must write its own episodes' there.  On a second emitter the adv
    / target of the rows already there are overwritten with a mark before each call: the call must leave them (the GAE of a call runs
    over the episodes it appended only)."""
    s, per, carried = _reference(geometry, N)
    B = _total(per) + 1
    ref = accumulate(per, B)
    assert ref[-1][1][4] == 0 and ref[-1][1][6] == 0 and ref[-1][1][5] == K
    e, marked = _emitter(geometry, N, aux, B=B), _emitter(geometry, N, aux, B=B)
    keys = _keys(geometry, aux)
    if N >= 300:
        assert max(int(p["t"].max()) for p in per if len(p["t"])) + 1 > T, "no episode spanning calls: the carry is not exercised"
    for k in range(K):
        n0 = int(ref[k - 1][1][0]) if k else 0
        for x in (e, marked):
            x.eb.adv[n0:] = float("nan")
            x.eb.target[n0:] = float("nan")
        marked.eb.adv[:n0] = MARK
        marked.eb.target[:n0] = MARK
        got = e.call(k)
        _check_call(e, got, ref[k], carried[k], keys, f"call {k}")
        m = marked.call(k)
        for name in ("adv", "target"):
            assert (m[name][:n0] == np.float32(MARK)).all(), f"call {k}: {name} of earlier episodes was rewritten"
            assert m[name][n0:].tobytes() == ref[k][0][name][n0:].tobytes(), f"call {k}: {name} of the appended episodes"
        _same(m, ref[k][0], [x for x in keys if x not in ("adv", "target")], f"call {k} (marked emitter)")


@pytest.mark.parametrize("geometry,N,aux", CASES, ids=CASE_IDS)
def test_batches_complete_and_start_over(geometry, N, aux):
    """B = a quarter of the stream's rows: the batch completes and the next call starts at 0, at least twice within the K calls (asserted
    on the restatement).  Contents, counts and acc — acc[4] complete, acc[5] collects, acc[6] batches — after every call."""
    s, per, carried = _reference(geometry, N)
    B = max(_total(per) // 4, 1)
    ref = accumulate(per, B)
    restarts = [k for k in range(1, K) if ref[k - 1][1][4]]
    assert len(restarts) >= 2 and ref[-1][1][6] == len(restarts), f"the batch restarts at calls {restarts}"
    assert any(ref[k][1][5] >= 2 for k in range(K)), "no batch of more than one collect"
    e = _emitter(geometry, N, aux, B=B)
    keys = _keys(geometry, aux)
    for k in range(K):
        _check_call(e, e.call(k), ref[k], carried[k], keys, f"call {k} (B = {B}, restarts at {restarts})")
        if k in restarts:
            assert ref[k][1][5] == 1 and ref[k][1][0] == len(per[k]["t"]), "a restarted batch holds this collect's rows only"


@pytest.mark.parametrize("geometry,N,aux", SMALL, ids=SMALL_IDS)
def test_b_1_is_the_existing_entry_point(geometry, N, aux):
    """train_batch_size = 1: a batch with any row is complete, every call starts at 0 and writes what a second emitter driven through
    hh_episodes_emit / _aux (hh_commander_episodes_emit / _aux) writes: rows(), the counts, the carry"""
    s, per, carried = _reference(geometry, N)
    one, old = _emitter(geometry, N, aux, B=1), _emitter(geometry, N, aux)
    assert old.eb._acc is None and old.eb.train_batch_size is None
    assert tuple(one.eb.obs.shape) == tuple(old.eb.obs.shape) and tuple(one.eb.ep_start.shape) == tuple(old.eb.ep_start.shape)
    keys = _keys(geometry, aux)
    for k in range(K):
        g, p = one.call(k), old.call(k)
        assert set(g) == set(p) == set(keys)
        _same(g, p, keys, f"call {k}")
        _same(g, dict(per[k], **{t: p[t] for t in ("ep_start", "ep_len", "ep_arena")}), keys, f"call {k} (restatement)")
        assert one.eb._counts.cpu().tolist() == old.eb._counts.cpu().tolist(), f"call {k}: counts"
        assert np.array_equal(one.eb.carried.cpu().numpy(), old.eb.carried.cpu().numpy()) and np.array_equal(one.state()[2], carried[k])
        for name, buf in one.eb._carry.items():
            assert torch.equal(buf, old.eb._carry[name]), f"call {k}: carry {name}"
        acc = one.state()[0]
        assert acc[0] == len(g["t"]) and acc[4] == (len(g["t"]) > 0) and acc[5] >= 1


@pytest.mark.parametrize("geometry,N,aux", SMALL, ids=SMALL_IDS)
def test_a_call_that_emits_nothing_leaves_the_partial_batch(geometry, N, aux):
    """collect QUIET ends no episode while the batch is partly filled (asserted on the restatement): acc[0..3] are unchanged, acc[5]
    goes up by one, and not a byte of the batch moves"""
    s, per, carried = _reference(geometry, N, QUIET)
    B = _total(per) + 1
    ref = accumulate(per, B)
    assert ref[QUIET][2] == (0, 0, 0) and ref[QUIET - 1][1][0] > 0 and ref[QUIET - 1][1][4] == 0, "the stream must have a quiet collect"
    assert ref[QUIET][1][:4].tolist() == ref[QUIET - 1][1][:4].tolist() and ref[QUIET][1][5] == ref[QUIET - 1][1][5] + 1
    e = _emitter(geometry, N, aux, B=B, quiet=QUIET)
    keys = _keys(geometry, aux)
    full = lambda: {k: getattr(e.eb, k).cpu().numpy().tobytes() for k in keys}
    before = None
    for k in range(K):
        if k == QUIET:
            before = full()
        _check_call(e, e.call(k), ref[k], carried[k], keys, f"call {k}")
        if k == QUIET:
            assert full() == before, "the quiet call wrote into the batch"
            assert (carried[k] == T).all()


@pytest.mark.parametrize("geometry,short", [("2v2", "row_cap"), ("commander", "row_cap"), ("commander", "seq_cap")])
def test_overflow_sets_the_flag_and_writes_nothing_behind_the_capacity(geometry, short):
    """through the C ABI directly, with row_cap (the commander also: seq_cap) one short of what the stream needs: acc[2] is set by the
    call that would pass it, the accumulator is clamped, the rows (sequences) behind the capacity keep their sentinel, rows() raises"""
    from hhmarl_2d_amd import _lib as L
    N = 300
    s, per, carried = _reference(geometry, N)
    B = _total(per) + 1
    full = accumulate(per, B)[-1][1]
    e = _emitter(geometry, N, True, B=B)
    b = e.eb._bufs
    caps = [int(b.row_cap), int(b.ep_cap), int(b.seq_cap) if e.seq else None]
    caps[0 if short == "row_cap" else 2] = int(full[0 if short == "row_cap" else 3]) - 1
    b.row_cap = caps[0]
    if e.seq:
        b.seq_cap = caps[2]
        assert b.row_cap >= N * (CAP + T) and b.seq_cap >= N * (T + CAP // L_SEQ), "the entry point's own floor"
    ref = accumulate(per, B, caps=caps)
    first = min(k for k in range(K) if ref[k][1][2])
    assert [r[1][2] for r in ref] == [0] * first + [1] * (K - first)
    guarded = (("obs", "actions", "logp", "vf", "reward", "valid", "adv", "target", "done", "arena", "episode", "t", "aux") if short == "row_cap"
               else ("seq_start", "seq_len", "seq_ep", "state_in"))
    cap = caps[0] if short == "row_cap" else caps[2]
    sentinel = {}
    for name in guarded:
        t = getattr(e.eb, name)
        t[cap:] = float("nan") if t.dtype.is_floating_point else 0x55
        sentinel[name] = t[cap:].cpu().numpy().tobytes()
        assert len(sentinel[name]) > 0
    f = getattr(L.lib(), "hh_commander_episodes_emit_append" if e.seq else "hh_episodes_emit_append")
    for k in range(K):
        st = e.upload(k)
        assert f(C.byref(b), C.byref(e.eb._aux), B, e.eb._acc.data_ptr(), None, st) == 0
        torch.cuda.synchronize()
        acc, counts, _ = e.state()
        assert acc.tolist() == ref[k][1].tolist() and counts == ref[k][2], f"call {k}: acc {acc.tolist()}, the restatement {ref[k][1].tolist()}"
        assert int(e.eb._counts[2]) == int(ref[k][1][2])
        for name in guarded:
            assert getattr(e.eb, name)[cap:].cpu().numpy().tobytes() == sentinel[name], f"call {k}: {name} written behind the capacity"
        if ref[k][1][2]:
            with pytest.raises(RuntimeError, match="outgrew"):
                e.eb.rows()
        else:
            _same({n: v.cpu().numpy() for n, v in e.eb.rows().items()}, ref[k][0], _keys(geometry, True), f"call {k}")


def _close(got, want, tol, what):
    assert abs(got - want) <= tol, f"{what}: {got!r} vs {want!r} (bound {tol:.3e})"


def _check_metrics(batch, own, m, keys, what):
    """metrics() of the accumulated batch against tests/episode_metrics_ref.restate_metrics of the accumulated restatement, under the
    rules of tests/test_gpu_episode_metrics.py / test_gpu_rollout_metrics.py: counts and lengths exact; ep_return within ep_len 2^-52
    sum|reward|; the means within n 2^-52 sum|x| of the sequential mean of the device's own values and within the derived bounds of the
    restatement's; min / max exactly those of the device's own values and within the per-episode bounds of the restatement's;
    vf_explained_var within 1e-9 relative where Var(target) >= 1e-2 mean(target^2)"""
    ref = restate_metrics(batch["reward"], batch["vf"], batch["target"], batch["ep_start"], batch["ep_len"])
    E, nA = ref["ep_return"].shape
    assert own.shape == (E, nA) and own.dtype == np.float64 and nA == len(keys)
    assert m["episodes_this_iter"] == E and m["timesteps_this_iter"] == len(batch["reward"]) == int(np.sum(batch["ep_len"]))
    per_agent = ("policy_reward_mean", "policy_reward_min", "policy_reward_max", "vf_explained_var")
    if E == 0:
        for k in ("episode_reward_mean", "episode_reward_min", "episode_reward_max", "episode_len_mean"):
            assert math.isnan(m[k]), (what, k)
        for k in per_agent:
            assert tuple(m[k]) == keys and all(math.isnan(v) for v in m[k].values()), (what, k)
        return 0
    b = bounds(batch["reward"], batch["ep_start"], batch["ep_len"], ref)
    assert (np.abs(own - ref["ep_return"]) <= b["ep_return"]).all(), what
    own_reward = own[:, 0].copy()
    for a in range(1, nA):
        own_reward += own[:, a]
    seq_mean = lambda x: float(np.add.accumulate(x)[-1] / E)
    _close(m["episode_reward_mean"], seq_mean(own_reward), E * EPS * np.abs(own_reward).sum(), f"{what} episode_reward_mean (own values)")
    _close(m["episode_reward_mean"], ref["episode_reward_mean"], b["episode_reward_mean"], f"{what} episode_reward_mean")
    assert m["episode_reward_min"] == own_reward.min() and m["episode_reward_max"] == own_reward.max(), what
    _close(m["episode_reward_min"], ref["episode_reward_min"], b["episode_reward"].max(), f"{what} episode_reward_min")
    _close(m["episode_reward_max"], ref["episode_reward_max"], b["episode_reward"].max(), f"{what} episode_reward_max")
    assert m["episode_len_mean"] == ref["episode_len_mean"] and m["episode_len_min"] == ref["episode_len_min"], what
    assert m["episode_len_max"] == ref["episode_len_max"], what
    checked = 0
    for a, key in enumerate(keys):
        _close(m["policy_reward_mean"][key], seq_mean(own[:, a]), E * EPS * np.abs(own[:, a]).sum(), f"{what} policy_reward_mean[{key}] (own values)")
        _close(m["policy_reward_mean"][key], ref["agent_return_mean"][a], b["agent_return_mean"][a], f"{what} policy_reward_mean[{key}]")
        assert m["policy_reward_min"][key] == own[:, a].min() and m["policy_reward_max"][key] == own[:, a].max(), what
        _close(m["policy_reward_min"][key], ref["agent_return_min"][a], b["ep_return"][:, a].max(), f"{what} policy_reward_min[{key}]")
        _close(m["policy_reward_max"][key], ref["agent_return_max"][a], b["ep_return"][:, a].max(), f"{what} policy_reward_max[{key}]")
        got, want = m["vf_explained_var"][key], ref["vf_explained_var"][a]
        t = batch["target"][:, a].astype(np.float64)
        if math.isnan(want) or t.var() < 1e-2 * (t ** 2).mean():
            assert math.isnan(got) == math.isnan(want) and (got == -1.0) == (want == -1.0), (what, key, got, want)
        else:
            _close(got, want, 1e-9 * abs(want), f"{what} vf_explained_var[{key}]")
            checked += 1
    return checked


@pytest.mark.parametrize("geometry", list(GEOMETRY))
def test_metrics_describe_the_accumulated_batch(geometry):
    """metrics=True with a B that restarts: after every call metrics() is the restatement over the accumulated batch, while
    episodes_total / timesteps_total are the sums of the per-call counts — every episode and row once"""
    N = 300
    s, per, carried = _reference(geometry, N)
    B = max(_total(per) // 4, 1)
    ref = accumulate(per, B)
    assert ref[-1][1][6] >= 2 and any(r[1][5] >= 2 for r in ref)
    e = _emitter(geometry, N, False, B=B, metrics=True)
    keys = e.eb.AGENT_KEYS
    m = e.eb.metrics()
    assert m["episodes_total"] == 0 and m["episodes_this_iter"] == 0 and math.isnan(m["episode_reward_mean"]), "before the first call"
    tot_e = tot_r = checked = 0
    for k in range(K):
        got = e.call(k)
        batch, acc, counts = ref[k]
        _same(got, batch, _keys(geometry, False), f"call {k}")
        m = e.eb.metrics()
        checked += _check_metrics(batch, got["ep_return"], m, keys, f"call {k}")
        tot_e, tot_r = tot_e + counts[1], tot_r + counts[0]
        assert (m["episodes_total"], m["timesteps_total"]) == (tot_e, tot_r), f"call {k}: running totals"
        assert e.eb.metrics_device()["totals"].tolist() == [tot_e, tot_r]
    assert tot_r == _total(per) and checked >= len(keys)
    # clear() discards the batch, not the totals or the carry; reset() zeroes all three
    e.eb.clear()
    assert e.eb.batch_info() == dict(rows=0, episodes=0, sequences=0, collects=0, batches=0) and not e.eb.ready()
    m = e.eb.metrics()
    assert m["episodes_this_iter"] == 0 and (m["episodes_total"], m["timesteps_total"]) == (tot_e, tot_r)
    assert np.array_equal(e.state()[2], carried[-1]) and len(e.eb.rows()["t"]) == 0
    e.eb.reset()
    assert e.eb.metrics()["episodes_total"] == 0 and not e.state()[2].any() and not e.state()[0].any()


def test_argument_errors_on_real_buffers_launch_nothing():
    from hhmarl_2d_amd import _lib as L
    e = _emitter("2v2", 3, True, B=64)
    e.upload(0)
    f, b, x = L.lib().hh_episodes_emit_append, e.eb._bufs, e.eb._aux
    acc = e.eb._acc.data_ptr()
    for args, msg in (((0, acc, None), b"train_rows"), ((64, None, None), b"null acc"), ((64, acc + 2, None), b"4-byte"),
                      ((64, acc, acc + 4), b"8-byte")):
        assert f(C.byref(b), C.byref(x), *args, None) == -1 and msg in L.lib().hh_last_error(), msg
    torch.cuda.synchronize()
    assert not e.eb._acc.any() and not e.eb._counts.any() and not e.eb.carried.any() and not e.eb.aux.any(), "a refused call launches nothing"
    with pytest.raises(RuntimeError, match="train_batch_size"):
        _emitter("2v2", 3, False).eb.ready()
