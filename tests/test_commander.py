"""The trainable commander (train_hier.py's CommanderGru) without a GPU: the PyTorch restatement against the golden vectors recorded from
the reference's own class (tools/gen_commander_golden.py), the draw's definition, the weight table and the C ABI surface."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import commander_ref as CR
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(GOLDEN, "commander_gru.npz"))
META = json.loads(str(G["meta"]))


def _weights(dtype=torch.float64):
    from hhmarl_2d_amd import commander as CM
    return CR.to_torch(CM.random_weights(META["seed"]), dtype)


def _ck(t):
    return int(np.nonzero(G["ck_steps"] == t)[0][0])


def test_random_weights_match_the_reference_state_dict():
    from hhmarl_2d_amd import commander as CM
    keys = CM.state_keys()
    assert {k: list(v) for k, v in keys.items()} == META["ref_keys"]
    sd = CM.random_weights(META["seed"])
    assert all(sd[k].shape == tuple(s) and sd[k].dtype == np.float32 for k, s in keys.items())
    assert sum(int(np.prod(s)) for s in keys.values()) == 778904
    assert all(np.array_equal(sd[k], v) for k, v in CM.random_weights(META["seed"]).items())   # deterministic


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-5), (torch.float32, 1e-5)])
def test_restatement_reproduces_the_reference_chain(dtype, tol):
    """state fed back step by step from zero (reset where `fresh`): logits and value at every step, both states at the stored steps"""
    sd = _weights(dtype)
    obs = torch.from_numpy(G["obs"]).to(dtype)
    h = torch.zeros((META["n_arenas"], 3, 2, 200), dtype=dtype)
    for t in range(META["K"]):
        h = torch.where(torch.from_numpy(G["fresh"][t]).bool()[:, None, None, None], torch.zeros_like(h), h)
        lg, v, h = CR.arena_forward(sd, obs[t], h)
        assert np.abs(lg.numpy() - G["logits"][t]).max() <= tol, t
        assert np.abs(v.numpy() - G["value"][t]).max() <= tol, t
        if t in G["ck_steps"]:
            assert np.abs(h.numpy() - G["h_out_ck"][_ck(t)]).max() <= tol, t


def test_restatement_value_branch_with_action_inputs():
    sd = _weights()
    t = META["b_step"]
    h = torch.from_numpy(G["h_out_ck"][_ck(t - 1)]).double()
    h = torch.where(torch.from_numpy(G["fresh"][t]).bool()[:, None, None, None], torch.zeros_like(h), h)
    lg, v, ho = CR.arena_forward(sd, torch.from_numpy(G["obs"][t]).double(), h, torch.from_numpy(G["b_act"]).double())
    assert np.abs(v.numpy() - G["b_value"]).max() <= 1e-5 and np.abs(ho.numpy() - G["b_hout"]).max() <= 1e-5
    assert np.abs(lg.numpy() - G["b_logits"]).max() <= 1e-5
    assert np.abs(G["b_value"] - G["value"][t]).max() > 1e-3          # the action columns do matter
    assert np.array_equal(G["b_logits"], G["logits"][t])              # ... to the value branch only


def test_multi_step_call_equals_the_stepwise_chain():
    L = META["L_multi"]
    assert np.abs(G["m_logits"] - G["logits"][:L, 0, 0]).max() <= 1e-6
    assert np.abs(G["m_value"] - G["value"][:L, 0, 0]).max() <= 1e-6
    h = G["h_out_ck"][_ck(L - 1)][0, 0]
    assert np.abs(G["m_hact"] - h[0]).max() <= 1e-6 and np.abs(G["m_hval"] - h[1]).max() <= 1e-6


def test_inverse_cdf_reproduces_the_recorded_draws():
    a, lp = CR.inverse_cdf(G["logits"].astype(np.float64), G["uniforms"])
    assert np.array_equal(a, G["action"].astype(np.int64)) and np.array_equal(lp, G["logp"])
    assert set(np.unique(a)) == {0, 1, 2}
    # the draw's logp is Categorical(logits).log_prob
    lt = torch.from_numpy(G["logits"].astype(np.float64))
    want = torch.distributions.Categorical(logits=lt).log_prob(torch.from_numpy(a)).numpy()
    assert np.abs(want - lp).max() <= 1e-12


def test_library_exports_the_commander_abi():
    from hhmarl_2d_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, s) for s in _lib.COMMANDER_EXPORTS)


def test_weights_struct_matches_the_header():
    from hhmarl_2d_amd import _lib
    src = open(os.path.join(ROOT, "include", "hh_commander.h")).read()
    body = re.search(r"typedef struct hh_commander_weights \{(.*?)\} hh_commander_weights;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n = 0
    for m in re.finditer(r"\*\s*(\w+)(?:\[(\d+)\])?", body):
        n += int(m.group(2) or 1)
    assert n == 30
    assert C.sizeof(_lib.HHCommanderWeights) == n * C.sizeof(C.c_void_p)


def test_argument_checks_without_a_gpu():
    from hhmarl_2d_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.hh_commander_create(0, 0, C.byref(h)) == -1             # max_rows <= 0
    assert lib.hh_commander_create(0, 16, None) == -1
    assert lib.hh_commander_destroy(None) == -1
    assert lib.hh_commander_set_weights(None, None) == -1
    assert lib.hh_commander_sample(None, None, 1, None, None, None, None, None, None, 0, None, None, None, None, None) == -1
    assert lib.hh_commander_kernel_name(None, 1, C.create_string_buffer(8), 8) == -1
