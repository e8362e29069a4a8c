"""The whole-episode emitters (csrc/hh_episodes.h) on the MI355X at production episode lengths, on the scripted streams of
tests/episodes_long_ref.py (no world): host streams uploaded T ticks per call into an EpisodeBatch / CommanderEpisodeBatch built from a
dict of device tensors, as in tests/test_gpu_episodes_accumulate.py.  What the short-episode tests never reach: hh_k_ep_gae's chunked
walk (episodes of up to three chunks of 512 // n_agents rows, the recursion carried in registers), its ACC instance on such episodes,
more than one ballot round of hh_ep_tick_tables (T = 96), a second trip of the sequence instance's 64-episode scan, a done on tick 0
behind a long carry and on tick T - 1, an episode of exactly carry_cap + 1 rows, sequence cuts with L = 1, 4 and 20 at those lengths,
and the instances for 1, 5 and 64 agents.  tests/test_episodes_long_host.py asserts on the restatement that the streams hold all that.
One real rollout at horizon 300 must emit an episode above 256 rows.

Everything is compared byte for byte with the host restatement (tests/episodes_ref.py per collect, tests/episodes_accumulate_ref.py
for the accumulation) after every call: every column, the tables, state_in, carried, the counts and the accumulator."""
import ctypes as C

import numpy as np
import pytest
import torch

from episodes_accumulate_ref import accumulate, batch_keys
from episodes_long_ref import COMMANDER, GAMMA, GEOMETRIES, LAM, SEQ_LENS, most_per_window, reference

pytestmark = pytest.mark.gpu
GEOMETRY_IDS = ["x".join(map(str, g)) for g in GEOMETRIES]
AUX_DIM = 32
MARK = 12345.0
INT_SENTINEL = 0x55


class _Emitter:
    """device buffers of one emitter fed from a scripted host stream, T ticks per call; aux: record the column; B: train_batch_size"""

    def __init__(self, ref, aux=False, B=None):
        from hhmarl_2d_amd.commander import CommanderEpisodeBatch
        from hhmarl_2d_amd.rollout import EpisodeBatch
        self.s, self.T, self.seq = ref["stream"], ref["T"], ref["L"] is not None
        self.names = [k for k in self.s if k != "aux"] + (["aux"] if aux else [])
        self.dev = {k: torch.zeros(self.s[k][:self.T].shape, dtype=torch.from_numpy(self.s[k][:1].copy()).dtype, device="cuda") for k in self.names}
        collect = {k: v for k, v in self.dev.items() if k != "aux"}
        kw = dict(aux=("aux", self.dev["aux"]) if aux else None, train_batch_size=B)
        self.eb = (CommanderEpisodeBatch(collect, ref["L"], ref["carry_cap"], GAMMA, LAM, **kw) if self.seq
                   else EpisodeBatch(collect, ref["carry_cap"], GAMMA, LAM, **kw))
        self.keys = batch_keys(self.seq) + (("aux",) if aux else ())

    def call(self, k):
        """upload collect k, emit through the batch's own path -> the emitted parts as numpy"""
        for name in self.names:
            self.dev[name].copy_(torch.from_numpy(self.s[name][k * self.T:(k + 1) * self.T].copy()))   # the shared stream is read-only
        self.eb.emit(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return {k2: v.cpu().numpy() for k2, v in self.eb.rows().items()}

    def counts(self):
        """(rows, episodes, sequences) of the last call"""
        c = self.eb._counts.cpu().numpy()
        return int(c[0]), int(c[1]), int(c[3]) if self.seq else 0

    def poison_gae(self, n0=0):
        """adv / target from row n0 on are NaN before a call: a row the GAE skipped shows"""
        self.eb.adv[n0:] = float("nan")
        self.eb.target[n0:] = float("nan")


def _same(got, want, keys, what):
    assert set(got) == set(keys), what
    for k in keys:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {k} is {g.dtype} {g.shape}, the restatement {w.dtype} {w.shape}"
        assert g.tobytes() == w.tobytes(), f"{what}: {k} differs from the restatement"


def _run_against_the_restatement(ref, what):
    """every call of one emitter (hh_episodes_emit / hh_commander_episodes_emit) against the per-collect restatement
    -> (longest episode, most episodes of one arena in one call) as the device wrote them"""
    e = _Emitter(ref)
    N = len(ref["arenas"])
    longest = most = 0
    for k in range(ref["K"]):
        e.poison_gae()
        got, want = e.call(k), ref["per"][k]
        _same(got, want, e.keys, f"{what} call {k}")
        assert int(e.eb._counts[2]) == 0, f"{what} call {k}: the overflow flag"
        assert e.counts() == (len(want["t"]), len(want["ep_start"]), len(want["seq_start"]) if e.seq else 0), f"{what} call {k}: counts"
        assert np.array_equal(e.eb.carried.cpu().numpy(), ref["carried"][k]), f"{what} call {k}: carried"
        if len(got["ep_len"]):
            longest = max(longest, int(got["ep_len"].max()))
            most = max(most, int(np.bincount(got["ep_arena"], minlength=N).max()))
    print(f"{what}: longest episode on the device {longest} rows, most episodes of one arena in one call {most}")
    assert longest == ref["carry_cap"] + 1 and most == most_per_window(ref["per"], N)
    return longest, most


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GEOMETRY_IDS)
def test_generic_emitter_against_the_restatement(geometry):
    """hh_episodes_emit through EpisodeBatch.emit: after every call everything byte for byte, the overflow flag 0; adv / target are NaN
    before each call.  Episodes of c - 1 .. 3 c rows walk hh_k_ep_gae's chunks; T = 96 takes two ballot rounds of the tick tables."""
    longest, most = _run_against_the_restatement(reference(*geometry), "x".join(map(str, geometry)))
    assert longest == 3 * (512 // geometry[0]) and most == min(geometry[2], longest)


@pytest.mark.parametrize("L", SEQ_LENS)
def test_commander_emitter_against_the_restatement(L):
    """hh_commander_episodes_emit with max_seq_len = L: as above, and seq_start / seq_len / seq_ep and state_in — 96 one-row episodes of
    one arena per call take a second trip of the 64-episode scan; the states come from the window, from the state carry (slots up to
    ceil(509 / L)) and, where a sequence starts on a window's first tick, from the window again"""
    ref = reference(*COMMANDER, L)
    _run_against_the_restatement(ref, f"commander L={L}")


def test_nothing_is_written_beyond_what_a_call_emits():
    """2 x 26, T = 96: every batch tensor is filled with sentinels before each call (NaN, 0x55 bytes); after it everything beyond the
    rows / episodes the call emitted still holds them"""
    ref = reference(*GEOMETRIES[0])
    e = _Emitter(ref)
    rows, tables = batch_keys(False)[:-3], batch_keys(False)[-3:]
    assert tables == ("ep_start", "ep_len", "ep_arena")
    for k in range(ref["K"]):
        for name in rows + tables:
            t = getattr(e.eb, name)
            t.fill_(float("nan") if t.dtype.is_floating_point else INT_SENTINEL)
        got = e.call(k)
        _same(got, ref["per"][k], e.keys, f"call {k}")
        n_rows, n_eps, _ = e.counts()
        assert (n_rows, n_eps) == (len(ref["per"][k]["t"]), len(ref["per"][k]["ep_start"]))
        for names, used in ((rows, n_rows), (tables, n_eps)):
            for name in names:
                t = getattr(e.eb, name)[used:]
                assert t.numel() > 0
                untouched = torch.isnan(t).all() if t.dtype.is_floating_point else (t == INT_SENTINEL).all()
                assert bool(untouched), f"call {k}: {name} written beyond the {used} entries emitted"


def _appended(acc_ref, k):
    """the rows the accumulated batch held before call k (0 where call k starts a batch)"""
    return int(acc_ref[k - 1][1][0]) if k and not acc_ref[k - 1][1][4] else 0


def test_append_with_aux_on_chunked_episodes():
    """hh_episodes_emit_append with an aux column of 32 floats and train_batch_size = half the stream's rows: the ACC instance of
    hh_k_ep_gae walks chunked episodes appended behind earlier rows, before and after the batch completes and starts over (asserted on
    the restatement).  On a second emitter the adv / target of the rows already there carry a mark before each call: the call leaves
    them (the marked-emitter check of test_a_batch_larger_than_the_stream_is_the_shifted_concatenation)."""
    nA, D, T = GEOMETRIES[0]
    ref = reference(nA, D, T, None, AUX_DIM)
    per, K, c = ref["per"], ref["K"], ref["c"]
    B = sum(len(p["t"]) for p in per) // 2
    acc_ref = accumulate(per, B)
    restarts = [k for k in range(1, K) if acc_ref[k - 1][1][4]]
    chunked_behind = [k for k in range(K) if _appended(acc_ref, k) > 0 and len(per[k]["ep_len"]) and per[k]["ep_len"].max() > c]
    assert restarts and acc_ref[-1][1][6] == len(restarts), f"the batch restarts at calls {restarts}"
    assert [k for k in chunked_behind if k < restarts[0]] and [k for k in chunked_behind if k > restarts[0]], \
        f"chunked episodes are appended behind earlier rows at calls {chunked_behind}, the batch restarts at {restarts}"
    e, marked = _Emitter(ref, aux=True, B=B), _Emitter(ref, aux=True, B=B)
    for k in range(K):
        n0 = _appended(acc_ref, k)
        e.poison_gae(n0)
        marked.poison_gae(n0)
        marked.eb.adv[:n0] = MARK
        marked.eb.target[:n0] = MARK
        batch, acc, counts = acc_ref[k]
        got = e.call(k)
        _same(got, batch, e.keys, f"call {k}")
        assert e.eb._acc.cpu().numpy().tolist() == acc.tolist(), f"call {k}: acc"
        assert e.counts() == counts and int(e.eb._counts[2]) == 0, f"call {k}: counts"
        assert np.array_equal(e.eb.carried.cpu().numpy(), ref["carried"][k]), f"call {k}: carried"
        assert e.eb.batch_info() == dict(rows=acc[0], episodes=acc[1], sequences=0, collects=acc[5], batches=acc[6]) and e.eb.ready() == bool(acc[4])
        m = marked.call(k)
        for name in ("adv", "target"):
            assert (m[name][:n0] == np.float32(MARK)).all(), f"call {k}: {name} of earlier episodes was rewritten"
            assert m[name][n0:].tobytes() == batch[name][n0:].tobytes(), f"call {k}: {name} of the appended episodes"
        _same({x: m[x] for x in e.keys if x not in ("adv", "target")}, batch, [x for x in e.keys if x not in ("adv", "target")],
              f"call {k} (marked emitter)")


def test_a_real_rollout_at_a_production_horizon():
    """PPORollout, 32 arenas of the level 1 fight world at horizon 300 (HORIZON_BY_LEVEL of level 3), T = 64, six collects against the
    restatement as tests/test_gpu_complete_episodes.py checks its rollouts.  With the untrained policy of that module's _rollout (seed
    23) the longest episode observed is 300 rows, first in the fifth collect: episodes that run to the horizon walk two chunks of
    hh_k_ep_gae.  (Level 3 escape reached 272 rows within 12 collects, the tenth being the first above 256.)"""
    import test_gpu_complete_episodes as ce
    ro = ce._rollout(32, 64, horizon=300, level=1, mode="fight", seed=23)
    collects, emitted, carried = ce._check_against_restatement(ro, 6)
    ce._check_bookkeeping(collects, emitted, carried, 64)
    lens = np.concatenate([b["ep_len"] for b in emitted])
    print(f"real rollout: {len(lens)} episodes, longest {int(lens.max())} rows")
    assert lens.max() > 256, "no episode beyond one chunk of the GAE walk: the case no longer covers it"
    assert lens.max() <= 300 and max(int(c.max()) for c in carried) <= 299


def test_two_runs_give_the_same_bytes():
    """2 x 26, T = 96: every part after every call, and the carry at the end"""
    ref = reference(*GEOMETRIES[0])

    def run():
        e = _Emitter(ref)
        out = []
        for k in range(ref["K"]):
            got = e.call(k)
            out.append({name: got[name].tobytes() for name in e.keys})
            out[-1]["carried"] = e.eb.carried.cpu().numpy().tobytes()
        out.append({name: buf.cpu().numpy().tobytes() for name, buf in e.eb._carry.items()})
        return out
    assert run() == run()
