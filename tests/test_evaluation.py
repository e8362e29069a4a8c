"""evaluation.py on the device, the host side (no GPU): postprocess_eval against a line-by-line restatement of the reference's
evaluation.py:66-82, the metrics file's name and content, config.py:100-102's level override, and the arguments the Evaluator refuses."""
import json
import math

import numpy as np
import pytest

from hhmarl_2d_amd import evaluation as E
from hhmarl_2d_amd.commander import random_weights
from hhmarl_2d_amd.config import make_args


def _reference_postprocess(ev, N_EVALS):
    """evaluation.py:66-79, line by line (a ZeroDivisionError where the reference raises one)"""
    win = (ev["agents_win"] / N_EVALS) * 100
    lose = (ev["opps_win"] / N_EVALS) * 100
    draw = (ev["draw"] / N_EVALS) * 100
    fight = (ev["agent_fight"] / ev["agent_steps"]) * 100
    esc = (ev["agent_escape"] / ev["agent_steps"]) * 100
    fight_opp = (ev["opp_fight"] / ev["opp_steps"]) * 100
    esc_opp = (ev["opp_escape"] / ev["opp_steps"]) * 100
    opp1 = (ev["opp1"] / ev["agent_fight"]) * 100
    opp2 = (ev["opp2"] / ev["agent_fight"]) * 100
    opp3 = (ev["opp3"] / ev["agent_fight"]) * 100
    return {"win": win, "lose": lose, "draw": draw, "fight": fight, "esc": esc, "fight_opp": fight_opp, "esc_opp": esc_opp, "opp1": opp1,
            "opp2": opp2, "opp3": opp3}


def _stats(rng, n):
    """counters of n episodes as evaluation.py accumulates them (consistent: fight + escape = steps, opp1..3 sum to agent_fight)"""
    outcome = rng.integers(0, 3, n)
    d = {"agents_win": int((outcome == 0).sum()), "opps_win": int((outcome == 1).sum()), "draw": int((outcome == 2).sum())}
    d["agent_steps"], d["opp_steps"] = int(rng.integers(50, 5000)), int(rng.integers(50, 5000))
    d["agent_fight"] = int(rng.integers(1, d["agent_steps"]))
    d["agent_escape"] = d["agent_steps"] - d["agent_fight"]
    d["opp_fight"] = int(rng.integers(0, d["opp_steps"] + 1))
    d["opp_escape"] = d["opp_steps"] - d["opp_fight"]
    o1 = int(rng.integers(0, d["agent_fight"] + 1))
    o2 = int(rng.integers(0, d["agent_fight"] - o1 + 1))
    d["opp1"], d["opp2"], d["opp3"] = o1, o2, d["agent_fight"] - o1 - o2
    d["total_n_actions"] = int(rng.integers(n, 50 * n))
    return {k: d[k] for k in E.STAT_KEYS}


def test_stat_keys_are_evaluation_py_counters_in_order():
    assert E.STAT_KEYS == ("agents_win", "opps_win", "draw", "agent_fight", "agent_escape", "opp_fight", "opp_escape", "agent_steps",
                           "opp_steps", "total_n_actions", "opp1", "opp2", "opp3")


@pytest.mark.parametrize("n", [1, 24, 1000, 65536])
def test_postprocess_eval_equals_the_reference(n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        st = _stats(rng, n)
        got, want = E.postprocess_eval(st, n), _reference_postprocess(st, n)
        assert list(got) == list(want) == list(E.METRIC_KEYS)
        for k in want:
            assert got[k] == want[k], k        # the same float operations: bit for bit


@pytest.mark.parametrize("zero", [("agent_steps", "agent_fight", "agent_escape", "opp1", "opp2", "opp3"),
                                  ("opp_steps", "opp_fight", "opp_escape"), ("agent_fight", "opp1", "opp2", "opp3")])
def test_postprocess_eval_zero_denominator_is_nan(zero):
    """where the reference raises ZeroDivisionError, that entry is nan and the others are the reference's"""
    st = _stats(np.random.default_rng(7), 100)
    for k in zero:
        st[k] = 0
    if "agent_fight" in zero:
        st["agent_escape"] = st["agent_steps"]
    with pytest.raises(ZeroDivisionError):
        _reference_postprocess(st, 100)
    got = E.postprocess_eval(st, 100)
    den = {"fight": "agent_steps", "esc": "agent_steps", "fight_opp": "opp_steps", "esc_opp": "opp_steps", "opp1": "agent_fight",
           "opp2": "agent_fight", "opp3": "agent_fight"}
    for k in E.METRIC_KEYS:
        if k in den and st[den[k]] == 0:
            assert math.isnan(got[k]), k
        else:
            num = {"win": "agents_win", "lose": "opps_win", "draw": "draw", "fight": "agent_fight", "esc": "agent_escape",
                   "fight_opp": "opp_fight", "esc_opp": "opp_escape", "opp1": "opp1", "opp2": "opp2", "opp3": "opp3"}[k]
            want = (st[num] / (100 if k in ("win", "lose", "draw") else st[den[k]])) * 100
            assert got[k] == want, k


def test_postprocess_eval_refuses_no_episodes():
    with pytest.raises(ValueError):
        E.postprocess_eval(_stats(np.random.default_rng(0), 5), 0)


@pytest.mark.parametrize("eval_hl,n,m,name", [(True, 3, 3, "Metrics_Commander_3-vs-3.json"), (False, 3, 3, "Metrics_Low-Level_3-vs-3.json"),
                                              (True, 5, 4, "Metrics_Commander_5-vs-4.json"), (False, 2, 3, "Metrics_Low-Level_2-vs-3.json")])
def test_metrics_file_name_and_content(tmp_path, eval_hl, n, m, name):
    args = make_args(2, num_agents=n, num_opps=m, eval_hl=eval_hl)
    assert E.metrics_file_name(args) == name
    st = _stats(np.random.default_rng(n * 10 + m), 1000)
    st["opp_steps"] = st["opp_fight"] = st["opp_escape"] = 0                # a nan entry too
    metrics = E.postprocess_eval(st, 1000)
    ev = E.Evaluator(args, commander=random_weights(1) if eval_hl else None, policy_dir=str(tmp_path))
    ev.metrics = metrics
    path = ev.write_json(str(tmp_path))                                     # a directory: the reference's name inside it
    assert path == str(tmp_path / name)
    text = open(path).read()
    want = dict(metrics)
    import io
    buf = io.StringIO()
    json.dump(want, buf, indent=3)                                          # evaluation.py:80-81
    assert text == buf.getvalue()
    back = json.loads(text)
    assert list(back) == list(E.METRIC_KEYS) and math.isnan(back["fight_opp"]) and back["win"] == metrics["win"]
    assert ev.write_json(str(tmp_path / "x.json")) == str(tmp_path / "x.json")


def test_write_json_before_run_is_refused(tmp_path):
    ev = E.Evaluator(make_args(2), commander=random_weights(1), policy_dir=str(tmp_path))
    with pytest.raises(RuntimeError):
        ev.write_json(str(tmp_path))


def test_level_override_of_config_py_100_102(tmp_path):
    """Config(2) with eval_hl sets eval_level_ag = eval_level_opp = 5; make_args does not, the Evaluator does, on a copy"""
    args = make_args(2)
    assert (args.eval_level_ag, args.eval_level_opp) == (5, 4)
    ev = E.Evaluator(args, commander=random_weights(1), policy_dir=str(tmp_path))
    assert (ev.args.eval_level_ag, ev.args.eval_level_opp) == (5, 5)
    assert ev.args.env_config["args"] is ev.args
    assert (args.eval_level_ag, args.eval_level_opp) == (5, 4) and args.env_config["args"] is args      # the caller's args unchanged
    assert (ev.args.horizon, ev.args.map_size, ev.args.eval_info) == (500, 0.5, True)
    low = E.Evaluator(make_args(2, eval_hl=False, eval_level_ag=3), policy_dir=str(tmp_path))
    assert (low.args.eval_level_ag, low.args.eval_level_opp) == (3, 4)                               # no override without eval_hl


def test_bad_arguments_are_refused(tmp_path):
    pdir = str(tmp_path)
    sd = random_weights(1)
    ev = E.Evaluator(make_args(2), commander=sd, policy_dir=pdir)
    for n in (0, -3):
        with pytest.raises(ValueError):
            ev.run(n_episodes=n)
    with pytest.raises(ValueError):
        ev.run(n_episodes=4, arena_offset=-1)
    for side in ("num_agents", "num_opps"):
        for n in (0, 6):
            with pytest.raises(ValueError):
                E.Evaluator(make_args(2, **{side: n}), commander=sd, policy_dir=pdir)
    with pytest.raises(ValueError):
        E.Evaluator(make_args(2), commander=None, policy_dir=pdir)                         # eval_hl needs a commander
    with pytest.raises(ValueError):
        E.Evaluator(make_args(2, eval_hl=False), commander=sd, policy_dir=pdir)            # and without eval_hl none is used
    with pytest.raises(ValueError):
        E.Evaluator(make_args(2), commander=sd, policy_dir=None)
    with pytest.raises(ValueError):
        E.Evaluator(make_args(2), commander=sd, policy_dir=pdir, max_arenas=0)
    bad = dict(sd)
    del bad["rnn_act.weight_ih_l0"]
    with pytest.raises(ValueError):
        E.Evaluator(make_args(2), commander=bad, policy_dir=pdir)
