"""CommanderRollout(batch_mode="complete_episodes") on the MI355X: the whole-episode GRU-sequence batch of hh_commander_episodes_emit
against the host restatement of tests/episodes_ref.py (the rollout's own [T, N] buffers, cloned after every collect), bit for
bit in every column, table and sequence-start state; its bookkeeping; a replay of the learner's forward from the emitted states; graph
against eager; the default mode unchanged; the overflow flag; and the default carry at 8192 arenas."""
import numpy as np
import pytest
import torch

from episodes_ref import IN_COLS, OUT_COLS, SEQ_TABLE, TABLE, pad_sequences, restate

pytestmark = pytest.mark.gpu
ALL = OUT_COLS + TABLE + SEQ_TABLE + ("state_in",)


def _rollout(N, T, horizon, max_seq_len=5, batch_mode="complete_episodes", use_graph=True, carry_cap=None, seed=21):
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=seed, arena_offset=500, auto_reset=True,
                          horizon=horizon), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    pilot = VariantNetPilot(w, seed=8)
    if batch_mode is None:
        return CommanderRollout(w, net, pilot, T, use_graph=use_graph)
    return CommanderRollout(w, net, pilot, T, use_graph=use_graph, batch_mode=batch_mode, max_seq_len=max_seq_len, carry_cap=carry_cap)


def _collect(ro, K):
    """K collects -> (the [T, N] buffers of each (numpy; obs / vf / state_in cut to T rows), the emitted batch of each, carried after each)"""
    T = ro.T
    collects, emitted, carried = [], [], []
    for _ in range(K):
        ro.collect()
        torch.cuda.synchronize()
        collects.append({k: getattr(ro, k)[:T].clone().cpu().numpy() for k in IN_COLS})
        emitted.append({k: v.cpu().numpy() for k, v in ro.episodes.rows().items()})
        carried.append(ro.episodes.carried.cpu().numpy())
    return collects, emitted, carried


def _assert_equal(got, want, what):
    for k in ALL:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, f"{what}: {k} {got[k].shape} {got[k].dtype} vs {want[k].shape} {want[k].dtype}"
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs"


def _check_against_restatement(ro, K):
    collects, emitted, carried = _collect(ro, K)
    want, want_carried = restate(collects, ro.max_seq_len, gamma=ro.gamma, lam=ro.lam)
    for i, (g, w) in enumerate(zip(emitted, want)):
        _assert_equal(g, w, f"collect {i}")
    assert np.array_equal(carried[-1], want_carried)
    return collects, emitted, carried


def _check_bookkeeping(collects, emitted, carried, T):
    K, N = len(collects), collects[0]["done"].shape[1]
    seen = set()
    for b in emitted:
        for e, (s, n) in enumerate(zip(b["ep_start"], b["ep_len"])):
            sl = slice(s, s + n)
            assert np.array_equal(b["t"][sl], np.arange(n)) and b["done"][s + n - 1] == 1 and not b["done"][s:s + n - 1].any()
            key = (int(b["arena"][s]), int(b["episode"][s]))
            assert key not in seen and (b["arena"][sl] == key[0]).all() and (b["episode"][sl] == key[1]).all()
            seen.add(key)
            sq = np.nonzero(b["seq_ep"] == e)[0]
            assert b["seq_start"][sq[0]] == s and not b["state_in"][sq[0]].any(), "an episode's first sequence starts at t = 0 from a zero state"
            assert b["seq_len"][sq].sum() == n and np.array_equal(b["seq_start"][sq], s + np.cumsum(np.r_[0, b["seq_len"][sq][:-1]]))
        assert len(b["done"]) == len(b["t"]) and b["done"].sum() == len(b["ep_start"])
    # per arena, the episodes are numbered 0, 1, ... from start(), and emitted plus carried rows equal collected rows
    for n in range(N):
        eps = sorted(e for a, e in seen if a == n)
        assert eps == list(range(len(eps)))
    emitted_rows = sum(len(b["t"]) for b in emitted)
    assert emitted_rows + int(carried[-1].sum()) == K * T * N


def test_device_batch_equals_the_restatement_and_keeps_its_books():
    """N = 64, T = 8, L = 5, horizon 300 ticks: episodes span several collects; then L = 20 at horizon 500"""
    ro = _rollout(64, 8, 300, max_seq_len=5)
    collects, emitted, carried = _check_against_restatement(ro, 6)
    _check_bookkeeping(collects, emitted, carried, 8)
    lens = np.concatenate([b["ep_len"] for b in emitted])
    assert len(lens) > 20 and (lens > 8).any(), "no episode spanning collects: the carry is not exercised"
    # sequences whose first step lies in an earlier collect than their episode's end (their state came from the state carry)
    back = [b["ep_len"][b["seq_ep"]] - (b["seq_start"] - b["ep_start"][b["seq_ep"]]) for b in emitted]
    assert max(int(x.max()) for x in back if len(x)) > 8
    ro20 = _rollout(64, 8, 500, max_seq_len=20, seed=22)
    collects, emitted, carried = _check_against_restatement(ro20, 6)
    _check_bookkeeping(collects, emitted, carried, 8)


def test_replay_of_the_learners_forward_from_the_emitted_states():
    """CommanderNet.sample stepped through every padded sequence from its emitted state_in (greedy, logits out) recomputes the recorded
    vf bit for bit and the recorded logp at the recorded action within 1e-6: the states are the ones the sampler's forward used.
    Bit-exact vf: hh_k_commander computes every agent row on its own, in the same operation order whatever the batch, with the same
    zero action inputs as while sampling; only the arrangement of rows in the launch differs."""
    from hhmarl_2d_amd.commander import CommanderNet, random_weights
    ro = _rollout(64, 8, 300, max_seq_len=5)
    net = CommanderNet(0, 3 * 4096).set_weights(random_weights(6))
    checked = 0
    for _ in range(5):
        ro.collect()
        p = ro.episodes.sequences()
        S, L = p["mask"].shape
        if S == 0:
            continue
        want = pad_sequences({k: v.cpu().numpy() for k, v in ro.episodes.rows().items()}, L)
        for k in ("obs", "actions", "logp", "vf", "adv", "target", "mask", "state_in"):
            assert np.array_equal(p[k].cpu().numpy(), want[k]), f"sequences(): {k}"
        h_in = p["state_in"].clone().contiguous()
        h_out = torch.empty_like(h_in)
        for s in range(L):
            logits = torch.zeros((S, 3, 4), dtype=torch.float32, device="cuda")
            _, _, vf = net.sample(p["obs"][:, s].contiguous(), h_in, h_out, greedy=True, logits=logits)
            m = p["mask"][:, s]
            assert torch.equal(vf[m], p["vf"][:, s][m]), f"step {s}: vf differs from the recorded one"
            lsm = torch.log_softmax(logits[..., :3].double(), dim=-1)
            lp = torch.gather(lsm, -1, p["actions"][:, s].long()[..., None])[..., 0]
            assert (lp[m] - p["logp"][:, s][m].double()).abs().max().item() <= 1e-6
            checked += int(m.sum())
            h_in, h_out = h_out, h_in
    assert checked > 500


def test_graph_and_eager_batches_are_identical_and_trace_enable_recaptures():
    g, e = _rollout(64, 8, 300, use_graph=True), _rollout(64, 8, 300, use_graph=False)
    for c in range(4):
        if c == 3:
            gen0 = g._graph_gen
            g.w.trace_enable(n_arenas=4, capacity=256)
        bg, be = g.collect().episodes.rows(), e.collect().episodes.rows()
        for k in ALL:
            assert torch.equal(bg[k], be[k]), (c, k)
    assert g._graph_gen != gen0 and len(bg["t"]) > 0


def test_default_mode_is_unchanged():
    """the [T, N] buffers of a rollout built without the new keywords, with batch_mode = "truncate_episodes" and with
    "complete_episodes" (the emission only reads them) are identical, from the same seed"""
    ros = [_rollout(64, 8, 300, batch_mode=None), _rollout(64, 8, 300, batch_mode="truncate_episodes"), _rollout(64, 8, 300)]
    assert ros[0].episodes is None and ros[1].episodes is None
    for _ in range(3):
        bufs = [{k: getattr(r.collect(), k).clone() for k in IN_COLS + ("adv", "target")} for r in ros]
        for b in bufs[1:]:
            for k in bufs[0]:
                assert torch.equal(b[k], bufs[0][k]), k


def test_a_too_small_carry_sets_the_overflow_flag():
    ro = _rollout(64, 8, 300, carry_cap=1)
    for _ in range(3):
        ro.collect()
    with pytest.raises(RuntimeError, match="outgrew"):
        ro.episodes.rows()


def test_default_carry_at_8192_arenas():
    from hhmarl_2d_amd.commander import default_carry_cap
    ro = _rollout(8192, 16, 500, max_seq_len=20)
    cap = default_carry_cap(500)
    assert ro.episodes.carry_cap == cap == 47
    longest, rows, K = 0, 0, 8
    for _ in range(K):
        ro.collect()
        b = ro.episodes.rows()                     # raises on an overflow
        if len(b["ep_len"]):
            longest = max(longest, int(b["ep_len"].max()))
        rows += len(b["t"])
        assert int(ro.episodes.carried.max()) <= cap
    assert 0 < longest <= cap + 1
    assert rows + int(ro.episodes.carried.sum()) == K * 16 * 8192
