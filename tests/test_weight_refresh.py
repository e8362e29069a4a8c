"""The device weight refresh without a GPU: every new entry point is declared in its header, exported by libhh_world.so, listed in _lib
and bound with argtypes; the argument checks that need no device; PolicyBank.refresh / CommanderNet.refresh_weights refuse bad input
before anything reaches the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICY = ("hh_policy_refresh", "hh_policy_copy_packed")
COMMANDER = ("hh_commander_refresh_weights", "hh_commander_copy_packed")


def _lib():
    from hhmarl_2d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_entry_points_are_declared_exported_and_listed():
    _l = _lib()
    so = C.CDLL(_l.LIB_PATH)
    pol = open(os.path.join(ROOT, "include", "hh_policy.h")).read()
    cmd = open(os.path.join(ROOT, "include", "hh_commander.h")).read()
    for s in POLICY:
        assert re.search(r"\bint " + s + r"\(", pol) and hasattr(so, s) and s in _l.EXPORTS
    for s in COMMANDER:
        assert re.search(r"\bint " + s + r"\(", cmd) and hasattr(so, s) and s in _l.COMMANDER_EXPORTS and s not in _l.EXPORTS


def test_argtypes_are_bound():
    _l = _lib()
    L, vp = _l.lib(), C.c_void_p
    assert L.hh_policy_refresh.argtypes == [vp, C.c_int32, C.POINTER(_l.HHNetWeights), C.POINTER(_l.HHCriticWeights), vp]
    assert L.hh_policy_copy_packed.argtypes == [vp, C.c_int32, C.c_int32, vp, C.c_int64, C.POINTER(C.c_int64), vp]
    assert L.hh_commander_refresh_weights.argtypes == [vp, C.POINTER(_l.HHCommanderWeights), vp]
    assert L.hh_commander_copy_packed.argtypes == [vp, C.c_int32, vp, C.c_int64, C.POINTER(C.c_int64), vp]


def test_argument_checks_without_a_gpu():
    L = _lib().lib()
    n = C.c_int64(-7)
    assert L.hh_policy_refresh(None, 0, None, None, None) == -1
    assert L.hh_policy_copy_packed(None, 0, 0, None, 0, C.byref(n), None) == -1
    assert L.hh_commander_refresh_weights(None, None, None) == -1
    assert L.hh_commander_copy_packed(None, 0, None, 0, C.byref(n), None) == -1
    assert n.value == -7


def test_device_weights_refuses_bad_tensors_before_the_library():
    import torch
    from hhmarl_2d_amd import policy_nets as PN
    keys = {"a": (2, 3), "b": (3,)}
    dev = torch.device("cuda", 0)
    good = {"a": torch.zeros((2, 3)), "b": torch.zeros((3,))}
    with pytest.raises(ValueError, match="missing"):
        PN.device_weights(keys, {"b": good["b"]}, dev, "t")
    with pytest.raises(ValueError, match="not a torch tensor"):
        PN.device_weights(keys, {"a": np.zeros((2, 3), np.float32), "b": good["b"]}, dev, "t")
    with pytest.raises(ValueError, match="shape"):
        PN.device_weights(keys, {"a": torch.zeros((3, 2)), "b": good["b"]}, dev, "t")
    with pytest.raises(ValueError, match="float32"):
        PN.device_weights(keys, {"a": torch.zeros((2, 3), dtype=torch.float64), "b": good["b"]}, dev, "t")
    with pytest.raises(ValueError, match="lives on cpu"):
        PN.device_weights(keys, good, dev, "t")


def test_policy_bank_refresh_refuses_an_empty_slot_before_the_library():
    import torch
    from hhmarl_2d_amd.pilots import PolicyBank
    bank = PolicyBank.__new__(PolicyBank)          # no device needed: the check comes first
    bank.h, bank.device, bank.kinds, bank._critics = None, torch.device("cuda", 0), {}, set()
    with pytest.raises(ValueError, match="empty"):
        bank.refresh(3, {})
