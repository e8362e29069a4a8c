"""PPORollout / CommanderRollout with metrics=True on the MI355X: after every collect `episodes.metrics()` against the float64
restatement of tests/episode_metrics_ref.py applied to that collect's `episodes.rows()` (bounds as in tests/test_gpu_episode_metrics.py),
the running totals, graph against eager runs byte for byte, start() zeroing the totals, and metrics=False unchanged: no `ep_return`,
`metrics()` raises, every other column bit-identical to the metrics=True run of the same seed."""
import math

import numpy as np
import pytest
import torch

from episode_metrics_ref import EPS, bounds, restate_metrics

pytestmark = pytest.mark.gpu


def _ppo(metrics, use_graph=True, N=32, T=16, horizon=40, seed=23):
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, level=1, seed=seed, auto_reset=True, horizon=horizon), device=0)
    bank = PolicyBank.trainable_init(torch.device("cuda", 0), mode="fight", seed=5, max_rows=2 * N, tie_shared=False)
    return PPORollout(w, bank, T, use_graph=use_graph, batch_mode="complete_episodes", metrics=metrics)


def _commander(metrics, use_graph=True, N=16, T=8, horizon=300, seed=21):
    """the fixture of tests/test_gpu_commander_episodes.py: random CommanderGru weights (seed 6), VariantNetPilot (seed 8)"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd.commander import CommanderNet, CommanderRollout, random_weights
    from hhmarl_2d_amd.pilots import VariantNetPilot
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=N, env_kind=L.ENV_HIGHLEVEL, n_agents=3, n_opps=3, seed=seed, arena_offset=500, auto_reset=True,
                          horizon=horizon), device=0)
    net = CommanderNet(0, 3 * N).set_weights(random_weights(6))
    return CommanderRollout(w, net, VariantNetPilot(w, seed=8), T, use_graph=use_graph, batch_mode="complete_episodes", max_seq_len=5,
                            metrics=metrics)


def _run(ro, K):
    """K collects -> per collect (rows() as numpy, metrics() or None, the raw device tensors of metrics_device() as bytes or None)"""
    out = []
    for _ in range(K):
        ro.collect()
        rows = {k: v.cpu().numpy() for k, v in ro.episodes.rows().items()}
        if ro.episodes._metrics is None:
            out.append((rows, None, None))
            continue
        dev = ro.episodes.metrics_device()
        raw = (dev["summary"].cpu().numpy().tobytes(), dev["totals"].cpu().numpy().tobytes(),
               dev["ep_return"][:len(rows["ep_start"])].cpu().numpy().tobytes())
        out.append((rows, ro.episodes.metrics(), raw))
    return out


def _close(got, want, tol, what):
    assert abs(got - want) <= tol, f"{what}: {got!r} vs {want!r} (bound {tol:.3e})"


def _check_collect(rows, m, keys, what):
    """one collect's metrics() against the restatement of its rows(); ref["ev_checked"]: how many agents' vf_explained_var were compared
    numerically"""
    ref = restate_metrics(rows["reward"], rows["vf"], rows["target"], rows["ep_start"], rows["ep_len"])
    E, nA = ref["ep_return"].shape
    assert nA == len(keys) and rows["ep_return"].shape == (E, nA) and rows["ep_return"].dtype == np.float64
    assert m["episodes_this_iter"] == E and m["timesteps_this_iter"] == len(rows["reward"]) == int(np.sum(rows["ep_len"]))
    per_agent = ("policy_reward_mean", "policy_reward_min", "policy_reward_max", "vf_explained_var")
    for k in per_agent:
        assert tuple(m[k]) == keys, k
    if E == 0:
        for k in ("episode_reward_mean", "episode_reward_min", "episode_reward_max", "episode_len_mean"):
            assert math.isnan(m[k]), (what, k)
        for k in per_agent:
            assert all(math.isnan(v) for v in m[k].values()), (what, k)
        ref["ev_checked"] = 0
        return ref
    b = bounds(rows["reward"], rows["ep_start"], rows["ep_len"], ref)
    own = rows["ep_return"]
    assert (np.abs(own - ref["ep_return"]) <= b["ep_return"]).all(), what
    own_reward = own[:, 0].copy()
    for a in range(1, nA):
        own_reward += own[:, a]
    # the means: n 2^-52 sum|x| against the sequential mean of the device's own values, then against the restatement's
    seq_mean = lambda x: float(np.add.accumulate(x)[-1] / E)
    _close(m["episode_reward_mean"], seq_mean(own_reward), E * EPS * np.abs(own_reward).sum(), f"{what} episode_reward_mean (own values)")
    _close(m["episode_reward_mean"], ref["episode_reward_mean"], b["episode_reward_mean"], f"{what} episode_reward_mean")
    ref["ev_checked"] = 0
    assert m["episode_reward_min"] == own_reward.min() and m["episode_reward_max"] == own_reward.max(), what
    _close(m["episode_reward_min"], ref["episode_reward_min"], b["episode_reward"].max(), f"{what} episode_reward_min")
    _close(m["episode_reward_max"], ref["episode_reward_max"], b["episode_reward"].max(), f"{what} episode_reward_max")
    assert m["episode_len_mean"] == ref["episode_len_mean"] and m["episode_len_min"] == ref["episode_len_min"], what
    assert m["episode_len_max"] == ref["episode_len_max"], what
    for a, key in enumerate(keys):
        _close(m["policy_reward_mean"][key], seq_mean(own[:, a]), E * EPS * np.abs(own[:, a]).sum(), f"{what} policy_reward_mean[{key}] (own values)")
        _close(m["policy_reward_mean"][key], ref["agent_return_mean"][a], b["agent_return_mean"][a], f"{what} policy_reward_mean[{key}]")
        assert m["policy_reward_min"][key] == own[:, a].min() and m["policy_reward_max"][key] == own[:, a].max(), what
        _close(m["policy_reward_min"][key], ref["agent_return_min"][a], b["ep_return"][:, a].max(), f"{what} policy_reward_min[{key}]")
        _close(m["policy_reward_max"][key], ref["agent_return_max"][a], b["ep_return"][:, a].max(), f"{what} policy_reward_max[{key}]")
        got, want = m["vf_explained_var"][key], ref["vf_explained_var"][a]
        t = rows["target"][:, a].astype(np.float64)
        if math.isnan(want) or t.var() < 1e-2 * (t ** 2).mean():
            # outside the range the 1e-9 is stated for (too few rows, or a target with next to no variance): nan / clamp must still agree
            assert math.isnan(got) == math.isnan(want) and (got == -1.0) == (want == -1.0), (what, key, got, want)
        else:
            _close(got, want, 1e-9 * abs(want), f"{what} vf_explained_var[{key}]")
            ref["ev_checked"] += 1
    return ref


def _check_run(make, keys, K, label):
    ro = make(True)
    assert ro.episodes.metrics()["episodes_total"] == 0 and math.isnan(ro.episodes.metrics()["episode_reward_mean"]), "before the first collect"
    run = _run(ro, K)
    eps = [len(rows["ep_start"]) for rows, _, _ in run]
    print(f"{label}: episodes per collect {eps}")
    assert min(eps) == 0 and max(eps) >= 2, f"{label}: the collects must include one without an episode and one with several: {eps}"
    tot_e = tot_r = ev_checked = 0
    for i, (rows, m, _) in enumerate(run):
        ev_checked += _check_collect(rows, m, keys, f"{label} collect {i}")["ev_checked"]
        tot_e, tot_r = tot_e + len(rows["ep_start"]), tot_r + len(rows["reward"])
        assert (m["episodes_total"], m["timesteps_total"]) == (tot_e, tot_r), f"{label} collect {i}: running totals"
    print(f"{label}: vf_explained_var compared numerically {ev_checked} times")
    assert ev_checked >= len(keys), f"{label}: no collect whose targets vary enough for the 1e-9 comparison of vf_explained_var"
    # eager launches give the graph's bytes
    eager = _run(make(True, use_graph=False), K)
    for i, ((rows, m, raw), (rows_e, m_e, raw_e)) in enumerate(zip(run, eager)):
        assert raw == raw_e, f"{label} collect {i}: graph and eager metrics differ"
        assert rows["ep_return"].tobytes() == rows_e["ep_return"].tobytes()
    # start() zeroes the totals (and the next collect counts from there)
    assert tot_e > 0
    ro.start()
    assert ro.episodes.metrics_device()["totals"].tolist() == [0, 0]
    m = ro.episodes.metrics()      # and the summary is not the previous collect's
    assert m["episodes_this_iter"] == 0 and m["episodes_total"] == 0 and math.isnan(m["episode_reward_mean"])
    ro.collect()
    m = ro.episodes.metrics()
    assert (m["episodes_total"], m["timesteps_total"]) == (m["episodes_this_iter"], m["timesteps_this_iter"])
    # metrics=False: what it was — no ep_return, metrics() raises, the other columns bit-identical
    off = make(False)
    plain = _run(off, K)
    with pytest.raises(RuntimeError, match="metrics=True"):
        off.episodes.metrics()
    with pytest.raises(RuntimeError, match="metrics=True"):
        off.episodes.metrics_device()
    assert not hasattr(off.episodes, "ep_return")
    for i, ((rows, _, _), (rows_p, _, _)) in enumerate(zip(run, plain)):
        assert set(rows) == set(rows_p) | {"ep_return"} and "ep_return" not in rows_p
        for k, v in rows_p.items():
            assert v.dtype == rows[k].dtype and v.tobytes() == rows[k].tobytes(), f"{label} collect {i}: column {k} changes with metrics=True"


def test_ppo_rollout_metrics():
    """N = 32, T = 16, level 1, horizon 40, 5 collects: no episode can end in the first collect unless an aircraft is lost within 16
    ticks, and every arena's first episode has ended by tick 40, inside the third"""
    _check_run(_ppo, ("ac1_policy", "ac2_policy"), 5, "PPORollout")


def test_commander_rollout_metrics():
    """N = 16, T = 8 commander steps, horizon 300 ticks (at least 19 commander steps without a kill event), n_agents = 3, keys 1..3"""
    _check_run(_commander, (1, 2, 3), 6, "CommanderRollout")
