"""The replayable minibatch step without a GPU: the float64 Adam restatement against torch.optim.Adam, the staging restatement
against pad_chunks and slicing, the schedule builder, flag validation, and the ctypes structs against include/hh_learner.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import train_step_ref as TR
from hhmarl_2d_amd import _lib
from hhmarl_2d_amd import learner as LR
from hhmarl_2d_amd import policy_nets as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR_, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-8


@pytest.mark.parametrize("fresh", (True, False))
def test_adam_restatement_equals_torch_adam_in_float64(fresh):
    """five steps; 1e-12 relative to max(|p|, lr): about ten float64 roundings with a thousandfold margin"""
    rng = np.random.default_rng(3 + fresh)
    sizes = (1, 3, 65, 26 * 50)
    ps = [0.1 * rng.standard_normal(n) for n in sizes]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = torch.optim.Adam(params, lr=LR_)
    ms, vs, t = [np.zeros(n) for n in sizes], [np.zeros(n) for n in sizes], 0
    if not fresh:      # non-zero state: three steps taken before the comparison starts, by both
        t = 3
        ms = [0.01 * rng.standard_normal(n) for n in sizes]
        vs = [1e-4 * rng.random(n) for n in sizes]
        for p_, m_, v_ in zip(params, ms, vs):
            opt.state[p_] = {"step": torch.tensor(3.0), "exp_avg": torch.from_numpy(m_.copy()), "exp_avg_sq": torch.from_numpy(v_.copy())}
    for step in range(5):
        gs = [10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1.0, 1.0], n) * (rng.random(n) > 0.1) for n in sizes]
        for p_, g_ in zip(params, gs):
            p_.grad = torch.from_numpy(g_.copy())
        opt.step()
        for i in range(len(sizes)):
            ps[i], ms[i], vs[i] = TR.adam_ref(ps[i], gs[i], ms[i], vs[i], t, LR_, B1, B2, EPS)
        t += 1
        for i, p_ in enumerate(params):
            st = opt.state[p_]
            assert np.all(np.abs(p_.detach().numpy() - ps[i]) <= 1e-12 * np.maximum(np.abs(ps[i]), LR_))
            # m and v: relative to the larger of the result and the term that was added (their sum may cancel)
            assert np.all(np.abs(st["exp_avg"].numpy() - ms[i]) <= 1e-12 * np.maximum(np.abs(ms[i]), np.abs(gs[i])))
            assert np.all(np.abs(st["exp_avg_sq"].numpy() - vs[i]) <= 1e-12 * np.maximum(np.abs(vs[i]), gs[i] ** 2))


def test_adam_step_torch_equals_the_restatement():
    rng = np.random.default_rng(9)
    p, m, v = 0.1 * rng.standard_normal(77), np.zeros(77), np.zeros(77)
    tp, tm, tv = (torch.from_numpy(x.copy()) for x in (p, m, v))
    for t in range(5):
        g = rng.standard_normal(77) * 10.0 ** rng.uniform(-6, 3, 77)
        LR.adam_step_torch([tp], [torch.from_numpy(g)], [tm], [tv], t, lr=LR_)
        p, m, v = TR.adam_ref(p, g, m, v, t, LR_)
        for got, want, floor in ((tp, p, LR_), (tm, m, np.abs(g)), (tv, v, g * g)):
            assert np.all(np.abs(got.numpy() - want) <= 1e-12 * np.maximum(np.abs(want), floor))


def _fight_columns(S, Lc, seed):
    g = torch.Generator().manual_seed(seed)
    seq_len = torch.randint(1, Lc + 1, (S,), generator=g)
    seq_start = torch.cumsum(seq_len, 0) - seq_len
    R = int(seq_len.sum())
    flat = {"obs": torch.rand((R, 7), generator=g), "actions": torch.randint(0, 9, (R, 4), generator=g).to(torch.int8), "adv": torch.randn((R,), generator=g)}
    cols = {k: LR.pad_chunks(v, seq_start, seq_len, Lc) for k, v in flat.items()}
    cols["mask"] = LR.chunk_mask(seq_len, Lc).to(torch.uint8)
    return cols, seq_len


def test_staging_restatement_against_pad_chunks_and_slicing():
    cols, seq_len = _fight_columns(37, 20, 1)
    bounds = [(0, 1), (1, 6), (6, 22), (22, 37)]
    for s0, s1 in bounds:
        row = (s0, s1, int(seq_len[s0:s1].sum()), 0)
        staged, nv = LR.minibatch_stage_torch(list(cols.values()), 16, row)
        assert nv == row[2]
        for (k, c), st in zip(cols.items(), staged):
            want = torch.zeros((16,) + tuple(c.shape[1:]), dtype=c.dtype)
            want[:s1 - s0] = c[s0:s1]
            assert st.dtype == c.dtype and torch.equal(st, want)
            assert np.array_equal(TR.stage_ref(c.numpy(), 16, row), want.numpy())
        assert int(staged[-1].sum()) == row[2]        # the staged mask counts exactly the unpadded rows
    with pytest.raises((RuntimeError, ValueError)):
        LR.minibatch_stage_torch(list(cols.values()), 15, (6, 22, 0, 0))      # a minibatch larger than the capacity


def test_schedule_visits_every_part_once_per_pass_in_minibatch_order():
    seq_len = np.random.default_rng(0).integers(1, 21, 200)
    parts = LR.minibatch_partition(seq_len, 256)
    csum = np.concatenate([[0], np.cumsum(seq_len)])
    nv = [csum[s1] - csum[s0] for s0, s1 in parts]
    assert len(parts) > 3
    sched = LR.minibatch_schedule(parts, nv, 3, seed=7, update=2, policy=1)
    assert sched.dtype == np.int32 and sched.shape == (3 * len(parts), 4) and not sched[:, 3].any()
    for sgd_pass in range(3):
        rows = sched[sgd_pass * len(parts):(sgd_pass + 1) * len(parts)]
        order = LR.minibatch_order(len(parts), 7, 2, 1, sgd_pass)
        assert [tuple(r[:2]) for r in rows] == [parts[i] for i in order]
        assert sorted(tuple(r[:2]) for r in rows) == sorted(parts)
        assert [int(r[2]) for r in rows] == [int(nv[i]) for i in order] and int(rows[:, 2].sum()) == int(seq_len.sum())
    assert LR.minibatch_schedule([], [], 3, 0, 0, 0).shape == (0, 4)


def test_flags_are_validated():
    assert LR.OPTIMIZER_MODES == ("torch", "fused") and LR.STEP_MODES == ("eager", "graph")
    sds = [dict(PN.random_weights(k, 0), **PN.random_critic_weights(k, 0)) for k in (PN.ESC1, PN.ESC2)]
    for kw in (dict(optimizer="adam"), dict(optimizer=None), dict(step="captured"), dict(optimizer="fused", step=1)):
        with pytest.raises(ValueError):
            LR.PPOLearner((PN.ESC1, PN.ESC2), sds, "cpu", **kw)
    with pytest.raises(ValueError, match="optimizer"):
        LR.PPOLearner((PN.ESC1, PN.ESC2), sds, "cpu", step="graph")                       # the graph needs the device-side Adam
    with pytest.raises(ValueError, match="optimizer"):
        LR.PPOLearner((PN.ESC1, PN.ESC2), sds, "cpu", optimizer="torch", step="graph")
    assert LR._step_mode("graph", "fused") == "graph" and LR._step_mode("eager", "torch") == "eager" and LR._optimizer_mode("fused") == "fused"


def test_structs_and_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "hh_learner.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (HH_(?:ADAM|STAGE)_[A-Z_]+)\s+(\d+)", txt)}
    assert (defs["HH_ADAM_MAX_TENSORS"], defs["HH_STAGE_MAX_COLS"]) == (_lib.ADAM_MAX_TENSORS, _lib.STAGE_MAX_COLS)
    assert 48 * defs["HH_ADAM_MAX_TENSORS"] + 64 <= 4096        # the kernel's descriptors (48 bytes each) and scalars fit the kernel-argument limit
    for cname, S in (("hh_adam_tensor", _lib.HHAdamTensor), ("hh_stage_col", _lib.HHStageCol)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.sub(r"[\*\s]", "", nm) for decl in body.split(";") if decl.strip()
                 for nm in re.match(r"(?:const\s+)?\w+\s+(.*)", decl.strip()).group(1).split(",")]
        assert names == [f[0] for f in S._fields_]
        assert C.sizeof(S) == 8 * len(names) and all(getattr(S, nm).offset == 8 * i for i, nm in enumerate(names))     # every field is 8 bytes wide
    assert C.sizeof(_lib.HHAdamTensor) == 40 and C.sizeof(_lib.HHStageCol) == 24
    for sym in ("hh_adam_step", "hh_minibatch_stage", "hh_train_commit"):
        assert sym in _lib.LEARNER_EXPORTS and re.search(r"\b" + sym + r"\s*\(", txt)
        assert hasattr(C.CDLL(_lib.LIB_PATH), sym), f"libhh_world.so does not export {sym}"
