"""Host side of the aux column of the whole-episode emitters (hh_episodes_emit_aux / hh_commander_episodes_emit_aux) and of
record_logits: the ctypes mirror of hh_episode_aux against the header, the bindings, the entry points' argument checks (they fail before
any launch, so no GPU is needed) and the Python argument validation."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from hhmarl_2d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_aux_struct_layout_matches_header():
    _l = _lib()
    txt = open(os.path.join(ROOT, "include", "hh_abi.h")).read()
    body = re.search(r"typedef struct hh_episode_aux \{(.*?)\} hh_episode_aux;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(int32_t|float)\s*(\*?)\s*([A-Za-z_0-9]+)\s*;", body)
    want = [(name, C.c_void_p if star else C.c_int32) for t, star, name in fields]
    assert [n for n, _ in want] == ["aux_dim", "reserved0", "aux", "c_aux", "o_aux"]
    assert want == list(_l.HHEpisodeAux._fields_)
    assert C.sizeof(_l.HHEpisodeAux) == 2 * 4 + 3 * 8
    offs = {n: getattr(_l.HHEpisodeAux, n).offset for n, _ in want}
    assert offs == {"aux_dim": 0, "reserved0": 4, "aux": 8, "c_aux": 16, "o_aux": 24}
    assert int(re.search(r"#define HH_EP_AUX_MAX_DIM (\d+)", txt).group(1)) == _l.EP_AUX_MAX_DIM == 32
    pol = open(os.path.join(ROOT, "include", "hh_policy.h")).read()
    cmd = open(os.path.join(ROOT, "include", "hh_commander.h")).read()
    assert int(re.search(r"#define HH_POLICY_LOGITS (\d+)", pol).group(1)) == _l.POLICY_LOGITS
    assert int(re.search(r"#define HH_CMD_LOGITS (\d+)", cmd).group(1)) == _l.CMD_LOGITS


def test_entry_points_are_declared_exported_and_bound():
    _l = _lib()
    so = C.CDLL(_l.LIB_PATH)
    abi = open(os.path.join(ROOT, "include", "hh_abi.h")).read()
    cmd = open(os.path.join(ROOT, "include", "hh_commander.h")).read()
    assert re.search(r"\bint hh_episodes_emit_aux\(const hh_episode_bufs \*b, const hh_episode_aux \*x, void \*stream\);", abi)
    assert re.search(r"\bint hh_commander_episodes_emit_aux\(const hh_commander_episode_bufs \*b, const struct hh_episode_aux \*x, void \*stream\);", cmd)
    assert hasattr(so, "hh_episodes_emit_aux") and hasattr(so, "hh_commander_episodes_emit_aux")
    assert "hh_episodes_emit_aux" in _l.EXPORTS and "hh_commander_episodes_emit_aux" in _l.COMMANDER_EXPORTS
    lib = _l.lib()
    assert lib.hh_episodes_emit_aux.argtypes == [C.POINTER(_l.HHEpisodeBufs), C.POINTER(_l.HHEpisodeAux), C.c_void_p]
    assert lib.hh_commander_episodes_emit_aux.argtypes == [C.POINTER(_l.HHCommanderEpisodeBufs), C.POINTER(_l.HHEpisodeAux), C.c_void_p]


def _fill_pointers(b, value=0x10000):
    """every pointer field a non-null, 16-byte aligned dummy: the checks under test all fail before any launch reads them"""
    for name, ct in b._fields_:
        if ct is C.c_void_p:
            setattr(b, name, value)


def _aux_errors(_l, call):
    """the aux checks of one entry point; call(x) -> rc with x an HHEpisodeAux"""
    err = lambda: _l.lib().hh_last_error()
    x = _l.HHEpisodeAux(aux_dim=4, reserved0=0, aux=0x10000, c_aux=0x10000, o_aux=0x10000)
    for bad in (0, -1, 33, 1 << 20):
        x.aux_dim = bad
        assert call(x) == -1 and b"aux_dim" in err(), bad
    x.aux_dim, x.reserved0 = 4, 1
    assert call(x) == -1 and b"reserved0" in err()
    x.reserved0 = 0
    for k in ("aux", "c_aux", "o_aux"):
        setattr(x, k, None)
        assert call(x) == -1 and b"null aux buffer" in err(), k
        setattr(x, k, 0x10002)
        assert call(x) == -1 and b"4-byte aligned" in err(), k
        setattr(x, k, 0x10000)


def test_aux_argument_checks_fail_before_any_launch():
    _l = _lib()
    f = _l.lib().hh_episodes_emit_aux
    b = _l.HHEpisodeBufs()
    x = _l.HHEpisodeAux(aux_dim=4, reserved0=0, aux=0x10000, c_aux=0x10000, o_aux=0x10000)
    assert f(None, C.byref(x), None) == -1
    assert f(C.byref(b), C.byref(x), None) == -1 and b"hh_episodes_emit_aux: bad sizes" in _l.lib().hh_last_error()
    b.T, b.N, b.n_agents, b.obs_dim, b.carry_cap, b.row_cap, b.ep_cap = 5, 3, 3, 34, 11, 3 * 16, 3 * 5
    assert f(C.byref(b), C.byref(x), None) == -1 and b"null buffer" in _l.lib().hh_last_error()     # the struct's own checks come first
    assert f(C.byref(b), None, None) == -1 and b"null buffer" in _l.lib().hh_last_error()            # x = NULL: hh_episodes_emit's checks
    _fill_pointers(b)
    _aux_errors(_l, lambda x: f(C.byref(b), C.byref(x), None))


def test_commander_aux_argument_checks_fail_before_any_launch():
    _l = _lib()
    f = _l.lib().hh_commander_episodes_emit_aux
    b = _l.HHCommanderEpisodeBufs()
    x = _l.HHEpisodeAux(aux_dim=4, reserved0=0, aux=0x10000, c_aux=0x10000, o_aux=0x10000)
    assert f(C.byref(b), C.byref(x), None) == -1 and b"hh_commander_episodes_emit_aux: bad sizes" in _l.lib().hh_last_error()
    b.T, b.N, b.max_seq_len, b.carry_cap = 5, 3, 4, 11
    b.row_cap, b.ep_cap, b.seq_cap = 3 * 16, 3 * 5, 3 * (5 + 2)
    assert f(C.byref(b), C.byref(x), None) == -1 and b"null buffer" in _l.lib().hh_last_error()
    _fill_pointers(b)
    _aux_errors(_l, lambda x: f(C.byref(b), C.byref(x), None))


def test_check_aux_validates_the_python_argument():
    from hhmarl_2d_amd.commander import CommanderEpisodeBatch
    from hhmarl_2d_amd.rollout import EpisodeBatch
    cpu = torch.device("cpu")
    T, N, nA = 5, 3, 2
    ok = torch.zeros((T, N, nA, 32))
    assert EpisodeBatch.check_aux(("logits", ok), T, N, nA, cpu) == ("logits", ok)
    assert EpisodeBatch.check_aux(("x", torch.zeros((T, N, nA, 1))), T, N, nA, cpu)[0] == "x"
    bad = [ok, ("logits",), ("logits", ok, 1), (1, ok), ("logits", ok.numpy()),            # not a (name, tensor) pair
           ("obs", ok), ("t", ok), ("ep_len", ok), ("rows", ok), ("_x", ok), ("a b", ok),  # a taken or unusable name
           ("logits", ok.double()), ("logits", ok.transpose(0, 1)),                        # dtype, contiguity
           ("logits", torch.zeros((T, N, nA))), ("logits", torch.zeros((T + 1, N, nA, 32))), ("logits", torch.zeros((T, N, nA + 1, 32))),
           ("logits", torch.zeros((T, N, nA, 33))), ("logits", torch.zeros((T, N, nA, 0))),
           ("logits", ok.to("meta"))]                                                     # another device
    for a in bad:
        with pytest.raises(ValueError, match="aux"):
            EpisodeBatch.check_aux(a, T, N, nA, cpu)
    for name in ("seq_start", "state_in", "sequences"):
        with pytest.raises(ValueError, match="aux"):
            CommanderEpisodeBatch.check_aux((name, torch.zeros((T, N, 3, 4))), T, N, 3, cpu)
    assert CommanderEpisodeBatch.check_aux(("logits", torch.zeros((T, N, 3, 4))), T, N, 3, cpu)[0] == "logits"


def test_record_logits_is_a_keyword_of_both_rollouts_and_off_by_default():
    import inspect
    from hhmarl_2d_amd.commander import CommanderRollout
    from hhmarl_2d_amd.rollout import PPORollout
    for cls in (PPORollout, CommanderRollout):
        p = inspect.signature(cls.__init__).parameters
        assert p["record_logits"].default is False and list(p)[-1] == "record_logits"   # appended: positional callers are unaffected
    with pytest.raises(ValueError, match="batch_mode"):           # the earlier checks still come first
        PPORollout(None, None, 8, batch_mode="whole", record_logits=True)
    with pytest.raises(ValueError, match="max_seq_len"):
        CommanderRollout(None, None, None, 8, batch_mode="complete_episodes", max_seq_len=0, record_logits=True)


def test_learners_take_the_column_and_refuse_a_malformed_one():
    """batch_old_logits on host tensors: the column is returned as it stands (PPO: the very tensor; commander: agent-major), no sampler
    or module is touched (none exists here), and a column of the wrong shape is an error, not a silent recompute"""
    from hhmarl_2d_amd.learner import CommanderLearner, PPOLearner
    ppo = PPOLearner.__new__(PPOLearner)           # no device: the method reads only its arguments on this path
    rows = {"obs": torch.zeros((7, 2, 26)), "logits": torch.randn((7, 2, 32))}
    assert ppo.batch_old_logits(rows, None) is rows["logits"]
    with pytest.raises(ValueError, match="logits"):
        ppo.batch_old_logits({"obs": rows["obs"], "logits": torch.zeros((7, 2, 26))}, None)
    with pytest.raises(ValueError, match="record_logits"):
        ppo.batch_old_logits({"obs": rows["obs"]}, None)
    cmd = CommanderLearner.__new__(CommanderLearner)
    seqs = {"obs": torch.zeros((5, 4, 3, 34)), "logits": torch.randn((5, 4, 3, 4))}
    got = cmd.batch_old_logits(seqs)
    assert got.shape == (15, 4, 4) and got.is_contiguous()
    for a in range(3):
        assert torch.equal(got[5 * a:5 * (a + 1)], seqs["logits"][:, :, a])
    with pytest.raises(ValueError, match="logits"):
        cmd.batch_old_logits({"obs": seqs["obs"], "logits": torch.zeros((5, 4, 3, 3))})
