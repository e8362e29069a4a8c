"""learner.adam_step (hh_adam_step) and learner.train_commit (hh_train_commit) on the MI355X against the float64 restatement of
tests/train_step_ref.py, with float32 torch.optim.Adam on the same inputs as the yardstick (the project's 4 x rule)."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_step_ref as TR

pytestmark = pytest.mark.gpu
LR_ = 1e-4
SENTINEL = -7.25e11
GUARD = 4            # floats in front of and behind every buffer: 16 bytes, so a guarded view keeps the allocation's 16-byte alignment
# the sizes the vector body, its tail and the tile edges meet, then enough small tensors to need a second launch (capacity 64 per launch)
SIZES = (1, 3, 63, 64, 65, 257, 26 * 500, 500 * 500, 4097, 1000) + tuple(1 + (7 * i) % 40 for i in range(60))
MISALIGNED = {8: ("p",), 9: ("p", "g", "m", "v")}     # tensor index -> the buffers that start at a 4-byte-aligned offset of their allocation


def _guarded(values, shift=0):
    """a CUDA float32 view of len(values) elements inside an allocation filled with SENTINEL, `shift` extra floats in (1: only 4-byte aligned)"""
    n = len(values)
    big = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=torch.float32, device="cuda")
    view = big[GUARD + shift:GUARD + shift + n]
    view.copy_(torch.from_numpy(np.asarray(values, dtype=np.float32)))
    return big, view


def _guards_intact(big, view):
    n = view.numel()
    off = (view.data_ptr() - big.data_ptr()) // 4
    return bool((big[:off] == SENTINEL).all() and (big[off + n:] == SENTINEL).all())


@pytest.fixture(scope="module")
def runs():
    """five steps of every tensor: the device kernel (twice), float32 torch.optim.Adam and the float64 restatement, computed once"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    assert len(SIZES) > L.ADAM_MAX_TENSORS
    inputs = TR.adam_inputs(SIZES, seed=11)

    def device_run():
        bufs = {k: [_guarded(p if k == "p" else np.zeros_like(p), 1 if k in MISALIGNED.get(i, ()) else 0) for i, (p, _) in enumerate(inputs)] for k in "pmv"}
        t = torch.zeros((1,), dtype=torch.int32, device="cuda")
        cursor = torch.zeros((1,), dtype=torch.int32, device="cuda")
        table = torch.zeros((5, 6), dtype=torch.float64, device="cuda")
        steps, t_seen = [], []
        for s in range(5):
            gb = [_guarded(gs[s], 1 if "g" in MISALIGNED.get(i, ()) else 0) for i, (_, gs) in enumerate(inputs)]
            LR.adam_step([b[1] for b in bufs["p"]], [b[1] for b in gb], [b[1] for b in bufs["m"]], [b[1] for b in bufs["v"]], t, lr=LR_)
            t_seen.append(int(t.item()))          # the Adam launch itself leaves t alone
            LR.train_commit(torch.full((6,), float(s), dtype=torch.float64, device="cuda"), table, cursor, t)
            t_seen.append(int(t.item()))
            assert all(_guards_intact(*b) for b in gb)
            steps.append({k: [b[1].cpu().numpy().copy() for b in bufs[k]] for k in "pmv"})
        guards = all(_guards_intact(*b) for k in "pmv" for b in bufs[k])
        aligned = [{k: bufs[k][i][1].data_ptr() % 16 for k in "pmv"} for i in range(len(inputs))]
        return steps, t_seen, guards, aligned, (int(cursor.item()), table.cpu().numpy())

    dev1, dev2 = device_run(), device_run()
    params = [torch.nn.Parameter(torch.from_numpy(p.copy()).cuda()) for p, _ in inputs]
    opt = torch.optim.Adam(params, lr=LR_)
    ref = [(p.astype(np.float64), np.zeros(len(p)), np.zeros(len(p))) for p, _ in inputs]
    torch_steps, ref_steps = [], []
    for s in range(5):
        for p_, (_, gs) in zip(params, inputs):
            p_.grad = torch.from_numpy(gs[s]).cuda()
        opt.step()
        torch_steps.append({"p": [p_.detach().cpu().numpy().copy() for p_ in params], "m": [opt.state[p_]["exp_avg"].cpu().numpy().copy() for p_ in params],
                            "v": [opt.state[p_]["exp_avg_sq"].cpu().numpy().copy() for p_ in params]})
        ref = [TR.adam_ref(p, gs[s], m, v, s, LR_) for (p, m, v), (_, gs) in zip(ref, inputs)]
        ref_steps.append({"p": [r[0] for r in ref], "m": [r[1] for r in ref], "v": [r[2] for r in ref]})
    return dict(dev=dev1, dev2=dev2, torch=torch_steps, ref=ref_steps, inputs=inputs)


def test_five_steps_against_float64_by_the_four_times_rule(runs):
    """per tensor, step and quantity (p, m, v): the largest error against float64 is at most 4 x float32 torch.optim.Adam's on the same
    inputs, or one float32 ulp of the tensor's largest value where torch's error is smaller than that"""
    worst = {k: 0.0 for k in "pmv"}
    for s in range(5):
        for k in "pmv":
            for i in range(len(SIZES)):
                want = runs["ref"][s][k][i]
                e_dev = np.abs(runs["dev"][0][s][k][i].astype(np.float64) - want).max()
                e_torch = np.abs(runs["torch"][s][k][i].astype(np.float64) - want).max()
                ulp = float(np.spacing(np.float32(np.abs(want).max())))
                worst[k] = max(worst[k], e_dev / max(e_torch, ulp / 4.0))
                assert np.isfinite(runs["dev"][0][s][k][i]).all()
                assert e_dev <= max(4.0 * e_torch, ulp), (s, k, i, SIZES[i], e_dev, e_torch, ulp)
    print("largest ratio of the kernel's error to max(torch's error, ulp / 4) per quantity:", {k: round(v, 3) for k, v in worst.items()})


def test_alignment_cases_are_what_they_claim(runs):
    aligned = runs["dev"][3]
    assert aligned[8]["p"] % 16 == 4 and aligned[8]["m"] % 16 == 0          # one pointer 4-byte aligned only: the whole tensor goes scalar
    assert all(a % 16 == 4 for a in aligned[9].values())
    assert all(a == 0 for i, d in enumerate(aligned) if i not in MISALIGNED for a in d.values())


def test_t_counts_the_commits_and_the_table_fills(runs):
    steps, t_seen, guards, _, (cursor, table) = runs["dev"]
    assert t_seen == [0, 1, 1, 2, 2, 3, 3, 4, 4, 5] and cursor == 5
    assert np.array_equal(table, np.repeat(np.arange(5.0)[:, None], 6, axis=1))
    assert guards


def test_same_bytes_on_two_runs(runs):
    for s in range(5):
        for k in "pmv":
            for a, b in zip(runs["dev"][0][s][k], runs["dev2"][0][s][k]):
                assert a.tobytes() == b.tobytes()
    assert runs["dev2"][2]


def test_zero_gradient_on_fresh_state_changes_nothing():
    from hhmarl_2d_amd import learner as LR
    sizes = (1, 65, 4099)
    rng = np.random.default_rng(2)
    ps = [_guarded(rng.standard_normal(n).astype(np.float32)) for n in sizes]
    before = [v.clone() for _, v in ps]
    zeros = lambda: [torch.zeros((n,), dtype=torch.float32, device="cuda") for n in sizes]
    g, m, v = zeros(), zeros(), zeros()
    t = torch.zeros((1,), dtype=torch.int32, device="cuda")
    LR.adam_step([b[1] for b in ps], g, m, v, t, lr=LR_)
    torch.cuda.synchronize()
    for (big, view), b0, m_, v_ in zip(ps, before, m, v):
        assert view.cpu().numpy().tobytes() == b0.cpu().numpy().tobytes() and _guards_intact(big, view)
        assert not m_.any() and not v_.any()


def test_refused_arguments_enqueue_nothing():
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    lib = L.lib()
    p = torch.full((40,), 1.5, dtype=torch.float32, device="cuda")
    g, m, v = torch.ones_like(p), torch.zeros_like(p), torch.zeros_like(p)
    t = torch.zeros((1,), dtype=torch.int32, device="cuda")
    cursor = torch.zeros((1,), dtype=torch.int32, device="cuda")
    table = torch.zeros((2, 6), dtype=torch.float64, device="cuda")
    stats = torch.ones((6,), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def desc(**kw):
        d = (L.HHAdamTensor * 1)()
        d[0].p, d[0].g, d[0].m, d[0].v, d[0].n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 40
        for k, val in kw.items():
            setattr(d[0], k, val)
        return d
    E = -1      # HH_E_ARG
    assert lib.hh_adam_step(1, desc(), None, LR_, 0.9, 0.999, 1e-8, st) == E
    assert lib.hh_adam_step(-1, desc(), ptr(t), LR_, 0.9, 0.999, 1e-8, st) == E
    assert lib.hh_adam_step(1, None, ptr(t), LR_, 0.9, 0.999, 1e-8, st) == E
    for field in "pgmv":
        assert lib.hh_adam_step(1, desc(**{field: None}), ptr(t), LR_, 0.9, 0.999, 1e-8, st) == E
    assert lib.hh_adam_step(1, desc(n=-4), ptr(t), LR_, 0.9, 0.999, 1e-8, st) == E
    assert lib.hh_adam_step(0, None, ptr(t), LR_, 0.9, 0.999, 1e-8, st) == 0             # an empty list: success, no launch
    assert lib.hh_adam_step(1, desc(n=0), ptr(t), LR_, 0.9, 0.999, 1e-8, st) == 0
    for args in ((None, ptr(table), 2, ptr(cursor), ptr(t)), (ptr(stats), None, 2, ptr(cursor), ptr(t)), (ptr(stats), ptr(table), 2, None, ptr(t)),
                 (ptr(stats), ptr(table), 2, ptr(cursor), None), (ptr(stats), ptr(table), -1, ptr(cursor), ptr(t))):
        assert lib.hh_train_commit(*args, st) == E
    torch.cuda.synchronize()
    assert bool((p == 1.5).all()) and not m.any() and not v.any() and int(t.item()) == 0 and int(cursor.item()) == 0 and not table.any()
    with pytest.raises(ValueError):
        LR.adam_step([p], [g.double()], [m], [v], t, lr=LR_)
    with pytest.raises(ValueError):
        LR.adam_step([p], [g], [m], [v], t.long(), lr=LR_)
    # a commit beyond the table's rows advances the counters and writes no row
    cursor.fill_(2)
    LR.train_commit(stats, table, cursor, t)
    assert int(cursor.item()) == 3 and int(t.item()) == 1 and not table.any()
