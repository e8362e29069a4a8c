"""The window batch without a GPU: the cut rule (tests/window_batch_ref.py) against the project's own cut_chunks on the window's
fragments, its invariants, the torch-op twins on the CPU, the C ABI as _lib.py binds it, and the Python layer's refusals."""
import ctypes as C
import re
import types

import numpy as np
import pytest
import torch

import window_batch_ref as WR

TS, NS, LS, RATES = (1, 5, 20, 21, 64), (1, 63, 65), (1, 4, 20, 32), (0.0, 0.1, 0.5, 1.0)


def _done(T, N, rate, seed=0):
    rng = np.random.default_rng([T, N, int(rate * 10), seed])
    return (rng.random((T, N)) < rate).astype(np.uint8)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
def test_cut_rule_is_cut_chunks_on_the_fragments(T, N):
    from hhmarl_2d_amd import learner as LR
    for L in LS:
        for rate in RATES:
            done = _done(T, N, rate)
            t0, arena, ln = WR.window_cut_ref(done, L)
            start, length = WR.window_fragments(done)
            assert length.sum() == T * N
            seq_start, seq_len = LR.cut_chunks(torch.from_numpy(start), torch.from_numpy(length), L)
            assert np.array_equal(arena.astype(np.int64) * T + t0, seq_start.numpy()) and np.array_equal(ln, seq_len.numpy())
            # every (t, n) exactly once
            seen = np.zeros((T, N), dtype=np.int32)
            for a, n, k in zip(t0, arena, ln):
                seen[a:a + k, n] += 1
                assert not done[a:a + k - 1, n].any(), "a done row is the last row of its sequence"
            assert (seen == 1).all()
            assert ln.min() >= 1 and ln.max() <= L
            S = len(ln)
            assert S <= N * -(-T // L) + int((done[:T - 1] != 0).sum()) and S <= T * N
            # arena-major, then time
            key = arena.astype(np.int64) * T + t0
            assert (np.diff(key) > 0).all()
            # the torch-op twin, on the CPU
            got = LR.window_cut_torch(torch.from_numpy(done), L)
            assert all(g.dtype == torch.int32 and np.array_equal(g.numpy(), w) for g, w in zip(got, (t0, arena, ln)))


def test_any_non_zero_byte_is_a_done():
    from hhmarl_2d_amd import learner as LR
    done = _done(21, 5, 0.3)
    for a, b in zip(WR.window_cut_ref(done, 4), WR.window_cut_ref(done * 255, 4)):
        assert np.array_equal(a, b)
    for a, b in zip(WR.window_cut_ref(done, 4), LR.window_cut_torch(torch.from_numpy(done * 7), 4)):
        assert np.array_equal(a, b.numpy())


def test_gather_twin_on_the_cpu():
    from hhmarl_2d_amd import learner as LR
    T, N, L = 21, 5, 4
    rng = np.random.default_rng(3)
    done = _done(T, N, 0.2)
    tabs = [x.copy() for x in WR.window_cut_ref(done, L)]
    tabs[0][1], tabs[2][2], tabs[1][3], tabs[0][4] = -1, L + 1, N, T - 1         # entries that name no rows of the window (T - 1 + len > T)
    tabs[2][4] = 2
    obs = rng.standard_normal((T + 1, N, 2, 26)).astype(np.float32)
    act = rng.integers(-3, 9, (T, N, 2)).astype(np.int8)                        # T rows: the call's T_src is T
    state = rng.standard_normal((T + 1, N, 3, 8)).astype(np.float32)
    cols = [(torch.from_numpy(obs), (24,), 104, False), (torch.from_numpy(act), (), 1, False), (torch.from_numpy(state), (3, 8), 0, True)]
    got = LR.window_gather_torch(cols, [torch.from_numpy(x) for x in tabs], L)
    for g, (src, tail, off, per_seq) in zip(got, cols):
        width = int(np.prod(tail, dtype=np.int64)) * src.element_size()
        want = WR.gather_ref(src.numpy(), *tabs, L, off, width, per_seq, T_src=T)
        assert g.dtype == src.dtype and tuple(g.shape) == ((len(tabs[0]),) if per_seq else (len(tabs[0]), L)) + tuple(tail)
        assert np.array_equal(g.contiguous().numpy().reshape(want.shape[:-1] + (-1,)).view(np.uint8), want)
    assert not got[0][1].any() and not got[0][2].any() and not got[0][3].any() and not got[0][4].any() and got[0][0].any()


def test_abi_as_bound():
    from hhmarl_2d_amd import _lib
    import os
    txt = open(os.path.join(os.path.dirname(_lib.HERE), "include", "hh_learner.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (HH_\w+)\s+(\d+)", txt, re.M)}
    assert defs["HH_WINDOW_MAX_LEN"] == 32 == _lib.WINDOW_MAX_LEN and defs["HH_STAGE_MAX_COLS"] == _lib.STAGE_MAX_COLS
    m = re.search(r"typedef struct hh_window_col \{(.*?)\} hh_window_col;", txt, re.S)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert names == [f[0] for f in _lib.HHWindowCol._fields_] and C.sizeof(_lib.HHWindowCol) == 48
    for name, n_args in (("hh_window_cut", 10), ("hh_window_gather", 10)):
        m = re.search(r"^int " + name + r"\((.*?)\);", txt, re.M | re.S)
        assert m and len(m.group(1).split(",")) == n_args and name in _lib.LEARNER_EXPORTS
        if os.path.exists(_lib.LIB_PATH):
            assert hasattr(C.CDLL(_lib.LIB_PATH), name) and len(getattr(_lib.lib(), name).argtypes) == n_args
    src = open(os.path.join(_lib.HERE, "csrc", "hh_world.hip")).read()
    assert '#include "hh_window_batch.h"' in src


def test_refusals_that_need_no_gpu():
    from hhmarl_2d_amd import _lib
    from hhmarl_2d_amd import learner as LR
    done = torch.zeros((4, 3), dtype=torch.uint8)
    for fn in (LR.window_cut, LR.window_cut_torch):
        for L in (0, 33, -1, 2.5, True):
            with pytest.raises(ValueError, match="max_seq_len"):
                fn(done, L)
        for bad in (done.bool(), done[0], torch.zeros((0, 3), dtype=torch.uint8), done.numpy()):
            with pytest.raises(ValueError, match="done is a uint8 tensor"):
                fn(bad, 4)
    tabs = [torch.zeros(2, dtype=torch.int32)] * 3
    src = torch.zeros((4, 3, 2, 5))
    for fn in (LR.window_gather, LR.window_gather_torch):
        with pytest.raises(ValueError, match="columns per call"):
            fn([], tabs, 4)
        with pytest.raises(ValueError, match="columns per call"):
            fn([(src, (5,), 0, False)] * 9, tabs, 4)
        with pytest.raises(ValueError, match="max_seq_len"):
            fn([(src, (5,), 0, False)], tabs, 33)
        with pytest.raises(ValueError, match="tables is"):
            fn([(src, (5,), 0, False)], [t.long() for t in tabs], 4)
        with pytest.raises(ValueError, match="inside its 40-byte step-row"):
            fn([(src, (5,), 24, False)], tabs, 4)                          # 24 + 20 > 40
        with pytest.raises(ValueError, match="inside its 40-byte step-row"):
            fn([(src, (5,), 2, False)], tabs, 4)                           # not element-aligned
        with pytest.raises(ValueError, match="inside its 40-byte step-row"):
            fn([(src, (0,), 0, False)], tabs, 4)
        with pytest.raises(ValueError, match="same N"):
            fn([(src, (5,), 0, False), (torch.zeros((4, 2, 1)), (1,), 0, False)], tabs, 4)
        with pytest.raises(ValueError, match="contiguous tensor"):
            fn([(src.transpose(0, 1), (5,), 0, False)], tabs, 4)
    # the learners' refusals: the checks run before anything touches the device
    world = types.SimpleNamespace(cfg=types.SimpleNamespace(agent_mode=_lib.MODE_FIGHT), N=3)
    z = torch.zeros
    ro = types.SimpleNamespace(semantics="rllib", obs=z((5, 3, 2, 26)), actions=z((4, 3, 2, 4)), logp=z((4, 3, 2)), adv=z((4, 3, 2)),
                               target=z((4, 3, 2)), done=done, T=4, w=world, collects=0)
    from hhmarl_2d_amd import policy_nets as PN
    fight = types.SimpleNamespace(kinds=(PN.FIGHT1, PN.FIGHT2), recurrent=True)
    escape = types.SimpleNamespace(kinds=(PN.ESC1, PN.ESC2), recurrent=False)
    with pytest.raises(RuntimeError, match="has not collected yet"):
        LR.PPOLearner._check_window(fight, ro)
    ro.collects = 1
    assert LR.PPOLearner._check_window(fight, ro) == (4, 3)
    with pytest.raises(ValueError, match="fight mode"):
        LR.PPOLearner._check_window(escape, ro)
    ro.semantics = "masked"
    with pytest.raises(ValueError, match="unmasked view"):
        LR.PPOLearner._check_window(fight, ro)
    with pytest.raises(ValueError, match="takes a PPORollout"):
        LR.PPOLearner._check_window(fight, types.SimpleNamespace())
    cmd = types.SimpleNamespace(max_seq_len=20)
    with pytest.raises(ValueError, match="takes a CommanderRollout"):
        LR.CommanderLearner.window_sequences(cmd, ro)
    cro = types.SimpleNamespace(obs=z((5, 3, 3, 34)), actions=z((4, 3, 3)), logp=z((4, 3, 3)), vf=z((5, 3, 3)), adv=z((4, 3, 3)), target=z((4, 3, 3)),
                                done=done, state_in=z((5, 3, 3, 2, 200)), T=4, collects=0)
    with pytest.raises(RuntimeError, match="has not collected yet"):
        LR.CommanderLearner.window_sequences(cmd, cro)
    cro.obs = z((5, 3, 2, 26))
    with pytest.raises(ValueError, match="3-agent commander"):
        LR.CommanderLearner.window_sequences(cmd, cro)
