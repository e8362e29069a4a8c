"""evaluation.LowLevelEvaluator on the MI355X: every episode's return, length and outcome equal a plain eager loop over one world of the
same size (tests/lowlevel_eval_ref.py) at levels 3, 4 and 5 in fight mode and level 5 in escape mode, and for 96 episodes in two batches
of 64 and 32 with blocks of 5 ticks (blocks of 16 and of 7, which do not divide the horizon, run past it in the other cases); the
statistics are a float64 restatement of per_episode; arena_offset shifts the episodes;
a learner, its state dicts and its exported files evaluate alike; and what cannot be evaluated is refused.  64 arenas, horizon 40, on
a map of 0.22 degrees: the synthetic policies then end about a third of the episodes early, won and lost, at ticks 1 to 39, and fly
the rest out to the horizon (on the default map of 0.3 every episode of 40 ticks is a draw at the horizon, and the blocks' ticks
behind a finished episode would go untested)."""
import json
import os

import numpy as np
import pytest
import torch

from lowlevel_eval_ref import actor_weights, plain_loop

pytestmark = pytest.mark.gpu

N, HORIZON, MAP, SEED = 64, 40, 0.22, 11
LEARN = dict(num_sgd_iter=1, sgd_minibatch_size=128)
# (level, agent_mode, n_episodes, max_arenas, block)
CASES = {"L3-fight": (3, "fight", N, N, 16), "L4-fight": (4, "fight", N, N, 16), "L5-fight": (5, "fight", N, N, 16),
         "L5-escape": (5, "escape", N, N, 16), "L3-fight-two-batches": (3, "fight", 96, 64, 5), "L5-fight-two-batches": (5, "fight", 96, 64, 5)}


def _learner(mode, seed):
    from hhmarl_2d_amd import learner as LR
    return LR.PPOLearner.trainable_init(torch.device("cuda", 0), mode=mode, seed=seed, **LEARN)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """the policies under evaluation (one fight and one escape learner) and the directory of opponent policies levels 4-5 read by name:
    L3 / L4 / L5 fights and the L3 escapes as export_policies writes them, one learner (one seed) per export"""
    d = str(tmp_path_factory.mktemp("policies"))
    for level, mode, seed in ((3, "fight", 31), (4, "fight", 41), (5, "fight", 51), (3, "escape", 33)):
        _learner(mode, seed).export_policies(d, level)
    return {"dir": d, "fight": _learner("fight", 7), "escape": _learner("escape", 8)}


def _args(level, mode):
    from hhmarl_2d_amd.config import make_args
    return make_args(0, level=level, agent_mode=mode, horizon=HORIZON, map_size=MAP)


_runs = {}


def _case(setup, name):
    """one run of the evaluator and of the plain loop per case, shared by the tests and left unchanged"""
    if name not in _runs:
        from hhmarl_2d_amd.evaluation import LowLevelEvaluator
        level, mode, n, max_arenas, block = CASES[name]
        pdir = setup["dir"] if level >= 4 else None
        ev = LowLevelEvaluator(_args(level, mode), setup[mode], policy_dir=pdir, max_arenas=max_arenas, block=block)
        stats = ev.run(n_episodes=n, seed=SEED)
        want, ticks = plain_loop(_args(level, mode), actor_weights(setup[mode]), n, SEED, max_arenas=max_arenas, policy_dir=pdir)
        _runs[name] = (ev, stats, want, ticks)
    return _runs[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_episode_equals_the_plain_loop(setup, name):
    ev, stats, want, ticks = _case(setup, name)
    n = CASES[name][2]
    per = ev.per_episode
    assert set(per) == {"ret", "len", "outcome"}
    assert (per["ret"].dtype, per["len"].dtype, per["outcome"].dtype) == (np.float32, np.int32, np.int8)
    assert per["ret"].shape == per["len"].shape == per["outcome"].shape == (n,)
    print(f"{name}: ticks per batch {ticks}, win/lose/draw {stats['agents_win']}/{stats['opps_win']}/{stats['draw']}, "
          f"len {per['len'].min()}..{per['len'].max()}, reward mean {stats['episode_reward_mean']:.4f}")
    # the case has episodes that end early and episodes that last out the horizon, and more than one outcome (the plain loop's, not the evaluator's)
    assert (want["len"] < HORIZON).any() and (want["len"] == HORIZON).any() and len(np.unique(want["outcome"])) >= 2
    for k in ("outcome", "len"):
        assert np.array_equal(per[k], want[k]), f"{k}: episodes {np.nonzero(per[k] != want[k])[0][:8]} differ"
    assert np.array_equal(per["ret"].view(np.uint32), want["ret"].view(np.uint32)), f"ret: episodes {np.nonzero(per['ret'] != want['ret'])[0][:8]} differ"
    # the plain loop stopped at the tick its batch was done; the evaluator's blocks of 16 do not divide the horizon of 40 and ran past it
    assert all(1 <= t <= HORIZON for t in ticks) and len(ticks) == (n + CASES[name][3] - 1) // CASES[name][3]


@pytest.mark.parametrize("name", list(CASES))
def test_outcomes_lengths_and_statistics(setup, name):
    ev, stats, _, _ = _case(setup, name)
    n = CASES[name][2]
    ret, ln, oc = (ev.per_episode[k] for k in ("ret", "len", "outcome"))
    assert stats == ev.stats and list(stats) == ["episodes", "agents_win", "opps_win", "draw", "episode_reward_mean", "episode_reward_min",
                                                 "episode_reward_max", "episode_len_mean"]
    assert stats["episodes"] == n and stats["agents_win"] + stats["opps_win"] + stats["draw"] == n
    assert not (oc == 2).any() and np.isin(oc, (-1, 0, 1)).all()
    assert (stats["agents_win"], stats["opps_win"], stats["draw"]) == (int((oc == 1).sum()), int((oc == -1).sum()), int((oc == 0).sum()))
    assert (ln >= 1).all() and (ln <= HORIZON).all()
    assert (oc[ln == HORIZON] == 0).all()                    # an episode that lasts out the horizon is a draw
    assert np.isfinite(ret).all()
    # the means: float64 on the host, summed in index order
    tot_r = tot_l = 0.0
    for i in range(n):
        tot_r += float(ret[i])
        tot_l += float(ln[i])
    assert stats["episode_reward_mean"] == tot_r / n and stats["episode_len_mean"] == tot_l / n
    assert stats["episode_reward_min"] == float(ret.min()) and stats["episode_reward_max"] == float(ret.max())
    assert all(type(stats[k]) is int for k in ("episodes", "agents_win", "opps_win", "draw"))
    assert all(type(stats[k]) is float for k in ("episode_reward_mean", "episode_reward_min", "episode_reward_max", "episode_len_mean"))
    assert ev.metrics == {"win": stats["agents_win"] / n * 100, "lose": stats["opps_win"] / n * 100, "draw": stats["draw"] / n * 100}


def test_write_json_writes_the_metrics(setup, tmp_path):
    ev = _case(setup, "L4-fight")[0]
    path = ev.write_json(str(tmp_path))
    assert os.path.dirname(path) == str(tmp_path) and path.endswith(".json")
    with open(path) as f:
        assert json.load(f) == ev.metrics
    assert ev.write_json(str(tmp_path / "m.json")) == str(tmp_path / "m.json")
    from hhmarl_2d_amd.evaluation import LowLevelEvaluator
    with pytest.raises(RuntimeError, match=r"run\(\) first"):
        LowLevelEvaluator(_args(3, "fight"), setup["fight"]).write_json(str(tmp_path))


@pytest.mark.parametrize("level", [3, 5])
def test_arena_offset_shifts_the_episodes(setup, level):
    """episode i of a run at arena_offset 7 is global arena i + 7: episode i + 7 of a run at offset 0 with the same batch shapes"""
    from hhmarl_2d_amd.evaluation import LowLevelEvaluator
    pdir = setup["dir"] if level >= 4 else None
    ev = LowLevelEvaluator(_args(level, "fight"), setup["fight"], policy_dir=pdir, max_arenas=32, block=7)
    ev.run(n_episodes=64, seed=SEED)
    base = {k: v.copy() for k, v in ev.per_episode.items()}
    ev.run(n_episodes=64, seed=SEED, arena_offset=7)
    for k in base:
        assert np.array_equal(ev.per_episode[k][:57].view(np.uint8), base[k][7:].view(np.uint8)), k
    assert not all(np.array_equal(ev.per_episode[k], base[k]) for k in base)
    ev.run(n_episodes=64, seed=SEED + 1)                      # another seed: other episodes
    assert not all(np.array_equal(ev.per_episode[k], base[k]) for k in base)
    with pytest.raises(ValueError, match="arena_offset"):
        ev.run(n_episodes=4, arena_offset=-1)
    ev.close()


@pytest.mark.parametrize("mode, level", [("fight", 4), ("escape", 3)])
def test_learner_state_dicts_and_files_evaluate_alike(setup, tmp_path, mode, level):
    from hhmarl_2d_amd.evaluation import LowLevelEvaluator
    learner = _learner(mode, 7 if mode == "fight" else 8)
    pdir = setup["dir"] if level >= 4 else None
    kw = dict(policy_dir=pdir, max_arenas=N)
    ev = LowLevelEvaluator(_args(level, mode), learner, **kw)
    ev.run(n_episodes=N, seed=SEED)
    first = {k: v.copy() for k, v in ev.per_episode.items()}
    if (mode, level) == ("fight", 4):
        want = _case(setup, "L4-fight")[0].per_episode
        assert all(np.array_equal(first[k], want[k]) for k in want)
    # the learner's weights are read at run(): after a change of the weights the same evaluator gives what the new weights give
    with torch.no_grad():
        for m in learner.modules:
            m.act_out._model[0].bias.add_(torch.linspace(-0.5, 0.5, m.act_out._model[0].bias.numel(), device="cuda"))
    ev.run(n_episodes=N, seed=SEED)
    moved = {k: v.copy() for k, v in ev.per_episode.items()}
    assert not all(np.array_equal(moved[k], first[k]) for k in first)
    paths = learner.export_policies(str(tmp_path), level)
    for policies in ([m.state_dict() for m in learner.modules], paths, tuple(os.fspath(p) for p in paths),
                     [{k: v.detach().cpu().numpy() for k, v in m.state_dict().items()} for m in learner.modules]):
        other = LowLevelEvaluator(_args(level, mode), policies, **kw)
        other.run(n_episodes=N, seed=SEED)
        for k in moved:
            assert np.array_equal(other.per_episode[k].view(np.uint8), moved[k].view(np.uint8)), k
        other.close()
    ev.close()


def test_what_cannot_be_evaluated_is_refused(setup, tmp_path):
    from hhmarl_2d_amd.config import make_args
    from hhmarl_2d_amd.evaluation import LowLevelEvaluator
    fight, escape, d = setup["fight"], setup["escape"], setup["dir"]
    # kinds against agent_mode: a learner, files, state dicts
    with pytest.raises(ValueError, match="the learner trains kinds"):
        LowLevelEvaluator(_args(3, "escape"), fight)
    with pytest.raises(ValueError, match="the learner trains kinds"):
        LowLevelEvaluator(_args(3, "fight"), escape)
    files = [os.path.join(d, f"L3_AC{ac}_escape.pt") for ac in (1, 2)]
    with pytest.raises(ValueError, match="holds a Esc1 network"):
        LowLevelEvaluator(_args(3, "fight"), files)
    with pytest.raises(ValueError, match="holds a Fight2 network"):
        LowLevelEvaluator(_args(3, "fight"), [os.path.join(d, "L3_AC2_fight.pt"), os.path.join(d, "L3_AC1_fight.pt")])
    with pytest.raises(ValueError, match="not a Fight1 network|has shape"):
        LowLevelEvaluator(_args(3, "fight"), [m.state_dict() for m in escape.modules])
    with pytest.raises(ValueError, match="a pair"):
        LowLevelEvaluator(_args(3, "fight"), [fight.modules[0].state_dict()])
    with pytest.raises(FileNotFoundError):
        LowLevelEvaluator(_args(3, "fight"), [str(tmp_path / "L3_AC1_fight.pt"), str(tmp_path / "L3_AC2_fight.pt")])
    # the opponents' directory: required exactly at levels 4-5
    for level in (4, 5):
        with pytest.raises(ValueError, match="policy_dir"):
            LowLevelEvaluator(_args(level, "fight"), fight)
    with pytest.raises(ValueError, match="no policy_dir is read"):
        LowLevelEvaluator(_args(3, "fight"), fight, policy_dir=d)
    with pytest.raises(ValueError, match="escape mode flies frozen opponents at level 5 only"):
        LowLevelEvaluator(_args(4, "escape"), escape, policy_dir=d)
    with pytest.raises(ValueError, match="2-vs-2"):
        LowLevelEvaluator(make_args(0, level=3, horizon=HORIZON, map_size=MAP, num_opps=3), fight)
    with pytest.raises(ValueError, match="at least 1"):
        LowLevelEvaluator(_args(3, "fight"), fight, max_arenas=0)
    with pytest.raises(ValueError, match="at least 1"):
        LowLevelEvaluator(_args(3, "fight"), fight, block=0)
    ev = LowLevelEvaluator(_args(3, "fight"), fight)
    for n in (0, -3):
        with pytest.raises(ValueError, match="n_episodes must be at least 1"):
            ev.run(n_episodes=n)
    # a directory that lacks a file the level reads by name
    lone = tmp_path / "lone"
    fight.export_policies(str(lone), 3)
    ev5 = LowLevelEvaluator(_args(5, "fight"), fight, policy_dir=str(lone), max_arenas=N)
    with pytest.raises(FileNotFoundError):
        ev5.run(n_episodes=N)
    ev.close()
    ev5.close()


def test_a_batch_that_cannot_finish_raises(setup, monkeypatch):
    """the cap of a batch observed on an ordinary world: the evaluator is told a horizon shorter than the world's (5 of 40 ticks), and
    after the one block of 5 ticks that fits it arenas are still running"""
    from hhmarl_2d_amd.evaluation import LowLevelEvaluator
    ev = LowLevelEvaluator(_args(3, "fight"), setup["fight"], max_arenas=N, block=5)
    monkeypatch.setattr(ev, "horizon", 5)
    with pytest.raises(RuntimeError, match=r"still running after 5 ticks \(horizon 5\)"):
        ev.run(n_episodes=N, seed=SEED)
    assert ev.stats is None and ev.per_episode is None
    monkeypatch.undo()
    assert ev.run(n_episodes=N, seed=SEED) == _case(setup, "L3-fight")[1]      # the evaluator and its bank are usable afterwards
    ev.close()
