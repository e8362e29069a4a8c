"""What CommanderLearner(optimizer=..., step=...) and the GRU tile query need no GPU for: the constructor's validation, the C ABI's
declaration of hh_gru_seq_tile, and the schedule graph_prepare builds."""
import inspect
import os
import re

import numpy as np
import pytest

from hhmarl_2d_amd import _lib
from hhmarl_2d_amd import learner as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_arguments_are_ppo_learners():
    ours = inspect.signature(LR.CommanderLearner.__init__).parameters
    theirs = inspect.signature(LR.PPOLearner.__init__).parameters
    for name in ("optimizer", "step"):
        assert ours[name].default == theirs[name].default
    assert (ours["optimizer"].default, ours["step"].default) == ("torch", "eager")
    for name in ("graph_prepare", "graph_replay", "graph_stats"):
        assert callable(getattr(LR.CommanderLearner, name))
        assert "agent" not in inspect.signature(getattr(LR.CommanderLearner, name)).parameters


@pytest.mark.parametrize("learner,args", [(LR.CommanderLearner, (None, "cpu")), (LR.PPOLearner, ((0, 1), None, "cpu"))])
def test_validation_comes_before_any_gpu_use(learner, args):
    """the same values are refused with the same exception and message, before the device or the weights are looked at"""
    for kw, text in ((dict(optimizer="adam"), "optimizer is one of"), (dict(step="replay", optimizer="fused"), "step is one of"),
                     (dict(step="graph"), 'step="graph" needs optimizer="fused"'), (dict(step="graph", optimizer="torch"), 'needs optimizer="fused"')):
        with pytest.raises(ValueError, match=re.escape(text)):
            learner(*args, **kw)


def test_the_tile_query_is_declared():
    assert "hh_gru_seq_tile" in _lib.LEARNER_EXPORTS
    txt = open(os.path.join(ROOT, "include", "hh_learner.h")).read()
    assert re.search(r"^int hh_gru_seq_tile\(int64_t n_seq\);", txt, re.M)
    assert re.search(r"0 <= seq_len\[s\] <= max_len", txt) and "seq_len[0] >= 1" in txt
    assert _lib.GRU_TILES[0] == 16 and set(_lib.GRU_TILES[1:]) & {8, 4}
    src = open(os.path.join(ROOT, "hhmarl_2d_amd", "csrc", "hh_gru_seq.h")).read()
    assert re.search(r"template <int TILE>\s*__global__[^\n]*hh_k_gru_seq_fwd", src) and re.search(r"template <int TILE>\s*__global__[^\n]*hh_k_gru_seq_bwd", src)
    for tile in _lib.GRU_TILES:
        assert f"hhg_launch_fwd<{tile}>" in src and f"hhg_launch_bwd<{tile}>" in src


def test_the_staged_columns():
    assert LR.COMMANDER_STAGE_COLS == ("obs", "critic", "actions", "old_logp", "adv", "target", "mask", "old_logits", "state_in", "seq_len")
    assert _lib.STAGE_MAX_COLS == 8 and len(LR.COMMANDER_STAGE_COLS) - _lib.STAGE_MAX_COLS == 2


@pytest.mark.parametrize("size,passes", [(256, 3), (100000, 1), (1, 2)])
def test_the_schedule_visits_each_sequence_once_per_pass(size, passes):
    rng = np.random.default_rng(5)
    seq_len = rng.integers(1, 21, size=331)
    seed, update = 6, 2
    parts, sched = LR.sequence_schedule(seq_len, size, passes, seed, update, 0)
    assert parts == LR.minibatch_partition(seq_len, size)
    assert sched.dtype == np.int32 and sched.shape == (passes * len(parts), 4) and not sched[:, 3].any()
    for sgd_pass in range(passes):
        rows = sched[sgd_pass * len(parts):(sgd_pass + 1) * len(parts)]
        seen = np.concatenate([np.arange(s0, s1) for s0, s1, _, _ in rows])
        assert sorted(seen.tolist()) == list(range(len(seq_len))), "every sequence exactly once per pass"
        assert int(rows[:, 2].sum()) == int(seq_len.sum())
        assert all(int(nv) == int(seq_len[s0:s1].sum()) for s0, s1, nv, _ in rows)
        # the eager path's order: minibatch_order(..., policy=0, ...)
        order = LR.minibatch_order(len(parts), seed, update, 0, sgd_pass)
        assert [tuple(r[:2]) for r in rows.tolist()] == [parts[i] for i in order]
