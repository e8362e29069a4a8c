"""hhmarl_2d_amd.learner without a GPU: the batch geometry (chunk cut, minibatch partition and order), the KL rule, the trainable
modules against the policy restatement (L = 1) and against the reference's own training-form forward (golden), the C ABI of
include/hh_learner.h, and the loss test's input generator."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import episodes_ref
import policy_ref
import ppo_loss_ref
from hhmarl_2d_amd import _lib
from hhmarl_2d_amd import learner as LR
from hhmarl_2d_amd import policy_nets as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (PN.FIGHT1, PN.FIGHT2, PN.ESC1, PN.ESC2)


def _weights(kind, seed):
    return dict(PN.random_weights(kind, seed), **PN.random_critic_weights(kind, seed))


# ---------------------------------------------------------------------------------------------------------------- geometry
def _synthetic_collects(rng, n_collects, T, N):
    out = []
    for _ in range(n_collects):
        out.append({"obs": rng.random((T, N, 3, 2), dtype=np.float32), "actions": rng.integers(0, 2, (T, N, 3, 1)).astype(np.int8),
                    "logp": rng.random((T, N, 3), dtype=np.float32), "vf": rng.random((T, N, 3), dtype=np.float32),
                    "reward": rng.random((T, N, 3), dtype=np.float32), "valid": np.ones((T, N, 3), np.uint8),
                    "done": (rng.random((T, N)) < 0.04).astype(np.uint8), "state_in": np.zeros((T, N, 3, 2, 200), np.float32)})
    return out


@pytest.mark.parametrize("max_seq_len", [20, 7, 1])
def test_chunk_cut_equals_episodes_ref(max_seq_len):
    rng = np.random.default_rng(5)
    batches, _ = episodes_ref.restate(_synthetic_collects(rng, 3, 48, 6), max_seq_len)
    assert sum(len(b["ep_len"]) for b in batches) > 10
    for b in batches:
        seq_start, seq_len = LR.cut_chunks(torch.from_numpy(b["ep_start"]), torch.from_numpy(b["ep_len"]), max_seq_len)
        assert np.array_equal(seq_start.numpy(), b["seq_start"]) and np.array_equal(seq_len.numpy(), b["seq_len"])
        pad = episodes_ref.pad_sequences(b, max_seq_len)
        assert np.array_equal(LR.chunk_mask(seq_len, max_seq_len).numpy(), pad["mask"])
        for k in ("obs", "actions", "logp", "adv"):
            got = LR.pad_chunks(torch.from_numpy(b[k]), seq_start, seq_len, max_seq_len).numpy()
            assert got.dtype == pad[k].dtype and np.array_equal(got, pad[k]), k


@pytest.mark.parametrize("size", [1, 64, 256, 10 ** 6])
def test_minibatch_partition(size):
    rng = np.random.default_rng(size)
    seq_len = rng.integers(1, 21, 977)
    parts = LR.minibatch_partition(seq_len, size)
    assert parts[0][0] == 0 and parts[-1][1] == len(seq_len)
    assert all(a[1] == b[0] for a, b in zip(parts, parts[1:])) and all(s1 > s0 for s0, s1 in parts)   # every chunk once, in order
    rows = [int(seq_len[s0:s1].sum()) for s0, s1 in parts]
    assert all(r >= size for r in rows[:-1])
    assert all(int(seq_len[s0:s1 - 1].sum()) < size for s0, s1 in parts)      # and no chunk more than needed
    ones = LR.minibatch_partition(np.ones(1000, np.int64), 256)               # escape: plain rows
    assert ones == [(0, 256), (256, 512), (512, 768), (768, 1000)]


def test_minibatch_order_is_keyed():
    a = LR.minibatch_order(200, 3, 1, 0, 2)
    assert np.array_equal(a, LR.minibatch_order(200, 3, 1, 0, 2)) and sorted(a.tolist()) == list(range(200))
    for other in ((4, 1, 0, 2), (3, 2, 0, 2), (3, 1, 1, 2), (3, 1, 0, 3)):
        assert not np.array_equal(a, LR.minibatch_order(200, *other))


def test_kl_rule_branches():
    assert LR.kl_coeff_update(0.2, 0.051, 0.025) == pytest.approx(0.3)      # above 2 x target
    assert LR.kl_coeff_update(0.2, 0.012, 0.025) == pytest.approx(0.1)      # below 0.5 x target
    assert LR.kl_coeff_update(0.2, 0.03, 0.025) == 0.2
    assert LR.kl_coeff_update(0.2, 0.05, 0.025) == 0.2 and LR.kl_coeff_update(0.2, 0.0125, 0.025) == 0.2   # the bounds are strict


def test_standardize_is_rllibs():
    x = torch.tensor([1.0, 2.0, 4.0, 9.0])
    want = (x.numpy() - x.numpy().mean()) / max(1e-4, x.numpy().std())
    assert np.allclose(LR.standardize(x).numpy(), want, rtol=1e-6)
    assert torch.equal(LR.standardize(torch.full((5,), 3.0)), torch.zeros(5))


# ---------------------------------------------------------------------------------------------------------------- modules
@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_keys_and_shapes(kind):
    want = dict(PN.actor_keys(kind), **PN.critic_keys(kind))
    got = {k: tuple(v.shape) for k, v in LR.TrainableNet(kind).state_dict().items()}
    assert got == {k: tuple(v) for k, v in want.items()}


def test_tie_leaves_one_parameter_object():
    mods = LR.tie([LR.TrainableNet(k) for k in KINDS])
    for m in mods[1:]:
        assert m.shared_layer._model[0].weight is mods[0].shared_layer._model[0].weight
        assert m.shared_layer._model[0].bias is mods[0].shared_layer._model[0].bias
    assert len({id(p) for m in mods for n, p in m.named_parameters() if n.startswith("shared_layer")}) == 2
    assert mods[1].state_dict()["shared_layer._model.0.weight"].data_ptr() == mods[0].state_dict()["shared_layer._model.0.weight"].data_ptr()


@pytest.mark.parametrize("kind", KINDS)
def test_length_one_forward_equals_policy_ref(kind):
    """L = 1 is the sampler's forward: oracle/policy_ref.py's logits and value, to float32 round-off (both are the same few float32
    GEMVs in another association; 2e-6 is ~16 ulp of the O(1) outputs)"""
    g = torch.Generator().manual_seed(11 + kind)
    d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
    R = 257
    own, other = torch.rand((R, d1), generator=g), torch.rand((R, d2), generator=g)
    act_own, act_2 = torch.rand((R, a1), generator=g), torch.rand((R, a2), generator=g)
    crit = torch.cat([act_own, act_2, own, other], dim=1)
    sd, csd = PN.random_weights(kind, 3), PN.random_critic_weights(kind, 3)
    m = LR.TrainableNet(kind).load_numpy(dict(sd, **csd)).eval()
    with torch.no_grad():
        logits, value = m(own, crit)
        if PN.HAS_ATT[kind]:
            l3, v3 = m(own[:, None], crit[:, None])
            assert torch.equal(l3[:, 0], logits) and torch.equal(v3[:, 0], value)
    want_l = policy_ref.torch_forward(kind, sd, own)
    want_v = policy_ref.torch_value(kind, sd, csd, own, act_own, other, act_2)
    assert logits.shape == (R, PN.N_OUT[kind]) and value.shape == (R,)
    assert (logits - want_l).abs().max().item() < 2e-6 and (value - want_v).abs().max().item() < 2e-6


@pytest.mark.parametrize("kind", [PN.FIGHT1, PN.FIGHT2])
def test_training_form_equals_reference_forward(kind):
    """tests/golden/fight_sequence_forward.npz: the reference's own Fight1 / Fight2 forward + value_function on padded chunks
    (tools/gen_fight_sequence_golden.py), zero rows as attention keys included.  Measured on the CPU in float32: largest difference
    3.85e-5 (Fight1 logits; 0.0 for Fight1's values and for Fight2's logits and values).  The 3.85e-5 sits in ten rows of one chunk,
    where the recorded float32 output of the reference is itself 3.8e-5 away from a float64 evaluation of the same network (the module
    is 6e-7 away from it, everywhere): the CPU GEMM kernels the recording ran through, not the architecture.  Bound: 4 x the measured
    difference, 1.5e-4; a wrong attention (no padded keys, or the sampler's length-1 form) is off by more than 1e-3, which the last
    assertion shows.  The padded rows are compared too: they are real outputs (tanh(bias) through the attention), not zeros."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "fight_sequence_forward.npz"))
    name = PN.KIND_NAMES[kind]
    seed = __import__("json").loads(str(g["meta"]))["seed"]
    m = LR.TrainableNet(kind).load_numpy(_weights(kind, seed)).eval()
    with torch.no_grad():
        logits, value = m(torch.from_numpy(g[f"{name}_obs"]), torch.from_numpy(g[f"{name}_critic"]))
    dl = np.abs(logits.numpy() - g[f"{name}_logits"]).max()
    dv = np.abs(value.numpy() - g[f"{name}_value"]).max()
    print(f"{name}: max |logits - reference| = {dl:.3e}, max |value - reference| = {dv:.3e}")
    assert dl <= 1.5e-4 and dv <= 1.5e-4
    # the chunk matters: the same rows one by one (the sampler's forward) give other numbers
    with torch.no_grad():
        l1, _ = m(torch.from_numpy(g[f"{name}_obs"]).reshape(-1, 1, PN.OBS_DIM[kind]),
                  torch.from_numpy(g[f"{name}_critic"]).reshape(-1, 1, g[f"{name}_critic"].shape[-1]))
    assert np.abs(l1.numpy().reshape(logits.shape) - g[f"{name}_logits"]).max() > 1e-3


def test_torch_loss_equals_restatement():
    """learner.ppo_loss_torch (the fused = False path) against the restatement, float64, masked and not"""
    for n_comp, masked in ((4, True), (3, False)):
        kw = dict(n_comp=n_comp, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)
        inp = ppo_loss_ref.make_inputs(4096, n_comp, 32, masked, 0)
        want, dl, dv, _ = ppo_loss_ref.reference(inp, torch.float64, **kw)
        logits, vf = inp["logits"].double().requires_grad_(True), inp["vf"].double().requires_grad_(True)
        batch = {k: inp[k] for k in ("old_logits", "actions", "old_logp", "adv", "target")}
        if masked:
            batch["mask"] = inp["mask"]
        total, stats = LR.ppo_loss_torch(logits, vf, batch, **kw)
        total.backward()
        assert np.allclose(stats.numpy(), want, rtol=1e-12, atol=1e-13)
        assert (logits.grad[:, :sum(ppo_loss_ref.SPLITS[n_comp])] - dl[:, :sum(ppo_loss_ref.SPLITS[n_comp])]).abs().max() < 1e-15
        assert (vf.grad - dv).abs().max() < 1e-15


# ---------------------------------------------------------------------------------------------------------------- the loss test's inputs
CASES = [(R, n_comp, masked) for R in (1, 63, 4096, 100003) for n_comp in (4, 3) for masked in (False, True)]


@pytest.mark.parametrize("R,n_comp,masked", CASES)
def test_loss_inputs_reach_every_branch_and_avoid_the_kinks(R, n_comp, masked):
    """the generator of tests/test_gpu_ppo_loss.py, checked with the float64 restatement alone: at most 1 % of a case's rows lie in
    the issue's exclusion bands, and the large cases reach every branch of min / clamp"""
    clip, vclip = 0.25, 10.0
    ld = {4: 26, 3: 24}[n_comp] if R % 2 else 32
    inp = ppo_loss_ref.make_inputs(R, n_comp, ld, masked, 0)
    _, _, _, aux = ppo_loss_ref.reference(inp, torch.float64, n_comp=n_comp, clip_param=clip, vf_clip_param=vclip, vf_loss_coeff=1.0,
                                          entropy_coeff=0.01, kl_coeff=0.2)
    near = ppo_loss_ref.near_kink(aux, clip, vclip)
    assert near.sum().item() <= 0.01 * R
    if R >= 4096:
        on = inp["mask"] if masked else torch.ones(R, dtype=torch.bool)
        r, a = aux["ratio"][on], inp["adv"][on]
        for sel in (r < 1 - clip, r > 1 + clip, (r > 1 - clip) & (r < 1 + clip)):
            assert (sel & (a > 0)).sum() > 50 and (sel & (a < 0)).sum() > 50
        assert (aux["vf_sq"][on] > vclip).sum() > 50 and (aux["vf_sq"][on] < vclip).sum() > 50


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_learner_header_symbols_exported_and_prototyped():
    txt = open(os.path.join(ROOT, "include", "hh_learner.h")).read()
    syms = sorted(set(re.findall(r"\b(hh_[a-z_]+)\s*\(", txt)))
    assert syms == sorted(_lib.LEARNER_EXPORTS)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"libhh_world.so does not export {s}"
    # the struct: field names, order and types as the header declares them
    body = re.search(r"typedef struct hh_ppo_loss_params \{(.*?)\} hh_ppo_loss_params;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"int32_t": C.c_int32, "float": C.c_float}[ctype]) for n in names.split(",")]
    assert fields == list(_lib.HHPpoLossParams._fields_) and C.sizeof(_lib.HHPpoLossParams) == 32
    assert int(re.search(r"#define HH_PPO_STATS (\d+)", txt).group(1)) == len(_lib.PPO_STATS)
    # the prototypes: one ctypes argument per declared parameter
    L = _lib.lib()
    for s in syms:
        params = re.search(r"\bint " + s + r"\s*\((.*?)\);", txt, re.S).group(1)
        assert len(getattr(L, s).argtypes) == len(params.split(",")), s
    want = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    params = [p.strip() for p in re.search(r"\bint hh_ppo_loss\s*\((.*?)\);", txt, re.S).group(1).split(",")]
    for p, at in zip(params, L.hh_ppo_loss.argtypes):
        if "*" in p:
            assert at in (C.c_void_p, C.POINTER(_lib.HHPpoLossParams)), p
        else:
            assert at is want[p.split()[0]], p
