"""The curriculum's policy files on the MI355X: what PPOLearner.export_policies writes, PolicyBank.from_reference_dir loads into the same
packed bytes as set_net from the learner's modules and flies to the same actions and logits; a directory may mix these files with the
reference's pickled modules; PPOLearner.from_policy_files gives the exporter's weights back; and evaluation.Evaluator takes the file
CommanderLearner.export_commander writes."""
import os

import numpy as np
import pytest
import torch

from helpers import stub_reference_module
from lowlevel_eval_ref import actor_weights
from resume_harness import same

pytestmark = pytest.mark.gpu

LEARN = dict(num_sgd_iter=1, sgd_minibatch_size=128)


def _dev():
    return torch.device("cuda", 0)


def _learner(mode, seed=3, **kw):
    from hhmarl_2d_amd import learner as LR
    return LR.PPOLearner.trainable_init(_dev(), mode=mode, seed=seed, **dict(LEARN, **kw))


def _train_a_little(learner):
    """move every parameter off its synthetic initial value, the tied shared layer once: an export must hold the CURRENT weights"""
    g = torch.Generator().manual_seed(1)
    seen = set()
    with torch.no_grad():
        for m in learner.modules:
            for p in m.parameters():
                if id(p) not in seen:
                    seen.add(id(p))
                    p.add_((0.01 * torch.randn(p.shape, generator=g)).cuda())
    return learner


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """trainable_init(seed=3) for fight and for escape, each exported as level 3 into one directory"""
    d = str(tmp_path_factory.mktemp("policies"))
    learners = {mode: _train_a_little(_learner(mode)) for mode in ("fight", "escape")}
    paths = {mode: lr.export_policies(d, 3) for mode, lr in learners.items()}
    return d, learners, paths


def _hand_bank(weights, lut, max_rows=4096):
    """a bank filled by set_net: weights [(kind, actor state dict)] into slots 0.., lut {selector: slot}"""
    from hhmarl_2d_amd.pilots import PolicyBank
    b = PolicyBank(_dev(), max_rows)
    for slot, (kind, sd) in enumerate(weights):
        b.set_net(slot, kind, sd)
    b.set_lut(lut)
    return b


def _same_banks(got, want, n_slots):
    assert got.kinds == want.kinds and sorted(got.kinds) == list(range(n_slots))
    assert np.array_equal(got._lut, want._lut)
    for slot in range(n_slots):
        for part in (0, 1, 2):
            a, b = got.packed(slot, part), want.packed(slot, part)
            assert a.numel() == b.numel() > 0 and torch.equal(a, b), (slot, part)


def _same_actions(got, want, selectors, n=4096):
    rng = np.random.default_rng(2)
    obs = torch.from_numpy(rng.random((n, 30)).astype(np.float32)).cuda()
    sel = torch.from_numpy(np.asarray(selectors, dtype=np.uint8)[rng.integers(0, len(selectors), n)]).cuda()
    out = []
    for bank in (got, want):
        logits = torch.zeros((n, 32), device="cuda")
        act = bank.act(obs, sel, logits=logits)
        out.append((act.clone(), logits))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))
    assert len(torch.unique(out[0][0].reshape(n, 4), dim=0)) > 4      # not one constant action


def test_exported_files_load_into_the_bytes_set_net_writes(exported):
    from hhmarl_2d_amd import pilots as P
    from hhmarl_2d_amd.config import make_args
    d, learners, paths = exported
    assert [os.path.basename(p) for p in paths["fight"]] == ["L3_AC1_fight.pt", "L3_AC2_fight.pt"]
    assert [os.path.basename(p) for p in paths["escape"]] == ["L3_AC1_escape.pt", "L3_AC2_escape.pt"]
    assert sorted(os.listdir(d)) == sorted(os.path.basename(p) for m in paths for p in paths[m])          # no temporary files
    fight, esc = actor_weights(learners["fight"]), actor_weights(learners["escape"])
    # LowLevelEnv level 4: the L3 fights
    got = P.PolicyBank.from_reference_dir(_dev(), d, "LowLevel", make_args(0, level=4), max_rows=4096)
    want = _hand_bank(fight, {P.SEL_FIGHT1: 0, P.SEL_FIGHT2: 1})
    _same_banks(got, want, 2)
    _same_actions(got, want, (P.SEL_FIGHT1, P.SEL_FIGHT2))
    # HighLevelEnv flying level 3: the L3 fights and, with no L5 escapes there, the L3 escapes
    got = P.PolicyBank.from_reference_dir(_dev(), d, "HighLevel", make_args(1, eval_level_ag=3), max_rows=4096)
    want = _hand_bank(fight + esc, {P.SEL_FIGHT1: 0, P.SEL_FIGHT2: 1, P.SEL_ESC1: 2, P.SEL_ESC2: 3})
    _same_banks(got, want, 4)
    _same_actions(got, want, (P.SEL_FIGHT1, P.SEL_FIGHT2, P.SEL_ESC1, P.SEL_ESC2))


def test_both_files_carry_the_one_shared_layer(exported):
    from hhmarl_2d_amd import policy_files as PF
    from hhmarl_2d_amd import policy_nets as PN
    d, learners, paths = exported
    for mode, kinds in (("fight", (PN.FIGHT1, PN.FIGHT2)), ("escape", (PN.ESC1, PN.ESC2))):
        docs = [torch.load(p, weights_only=True) for p in paths[mode]]
        assert [x["kind"] for x in docs] == list(kinds) and all(x["level"] == 3 and x["agent_mode"] == mode for x in docs)
        loaded = [PF.load_policy(p) for p in paths[mode]]
        live = learners[mode].modules[0].state_dict()
        for k in ("shared_layer._model.0.weight", "shared_layer._model.0.bias"):
            assert torch.equal(loaded[0][1][k], loaded[1][1][k]) and torch.equal(loaded[0][1][k], live[k].cpu())


def test_a_directory_may_mix_plain_files_and_pickled_modules(exported, tmp_path):
    """LowLevelEnv level 5 reads six files by name: here the L3 fights are plain exports, the L4 fights and the L3 escapes the pickled
    modules the reference writes (synthetic stand-ins of its classes)"""
    import shutil
    from hhmarl_2d_amd import pilots as P
    from hhmarl_2d_amd import policy_nets as PN
    from hhmarl_2d_amd.config import make_args
    d, learners, paths = exported
    for p in paths["fight"]:
        shutil.copy(p, str(tmp_path))
    stubs = {"L4_AC1_fight.pt": (PN.FIGHT1, 41), "L4_AC2_fight.pt": (PN.FIGHT2, 42), "L3_AC1_escape.pt": (PN.ESC1, 33), "L3_AC2_escape.pt": (PN.ESC2, 34)}
    for name, (kind, seed) in stubs.items():
        torch.save(stub_reference_module(kind, seed)[0], os.path.join(str(tmp_path), name))
    got = P.PolicyBank.from_reference_dir(_dev(), str(tmp_path), "LowLevel", make_args(0, level=5), max_rows=4096)
    lut = {P.SEL_FIGHT1: 0, P.SEL_FIGHT2: 1, P.SEL_FIGHT1 + 16: 2, P.SEL_FIGHT2 + 16: 3, P.SEL_ESC1 + 32: 4, P.SEL_ESC2 + 32: 5}
    want = _hand_bank(actor_weights(learners["fight"]) + [(kind, PN.random_weights(kind, seed)) for kind, seed in stubs.values()], lut)
    _same_banks(got, want, 6)
    _same_actions(got, want, tuple(lut))
    # a caller's own loader is used as before, and its result goes the same way
    calls = []

    def load(path):
        calls.append(os.path.basename(path))
        return torch.load(path, weights_only=False)
    hooked = P.PolicyBank.from_reference_dir(_dev(), str(tmp_path), "LowLevel", make_args(0, level=5), max_rows=4096, load=load)
    assert calls == ["L3_AC1_fight.pt", "L3_AC2_fight.pt", "L4_AC1_fight.pt", "L4_AC2_fight.pt", "L3_AC1_escape.pt", "L3_AC2_escape.pt"]
    _same_banks(hooked, want, 6)
    # a missing file is still FileNotFoundError
    os.remove(os.path.join(str(tmp_path), "L4_AC2_fight.pt"))
    with pytest.raises(FileNotFoundError):
        P.PolicyBank.from_reference_dir(_dev(), str(tmp_path), "LowLevel", make_args(0, level=5), max_rows=4096)


def test_highlevel_takes_both_l5_escapes_or_both_l3_ones(exported, tmp_path):
    """env_base.py:336-342 with plain files: one L5 escape alone is not used"""
    import shutil
    from hhmarl_2d_amd import pilots as P
    from hhmarl_2d_amd.config import make_args
    d, learners, paths = exported
    for p in paths["fight"] + paths["escape"]:
        shutil.copy(p, str(tmp_path))
    other = _learner("escape", seed=9)
    l5 = other.export_policies(str(tmp_path), 5)
    args = make_args(1, eval_level_ag=3)
    sels = {P.SEL_FIGHT1: 0, P.SEL_FIGHT2: 1, P.SEL_ESC1: 2, P.SEL_ESC2: 3}
    got = P.PolicyBank.from_reference_dir(_dev(), str(tmp_path), "HighLevel", args, max_rows=4096)
    _same_banks(got, _hand_bank(actor_weights(learners["fight"]) + actor_weights(other), sels), 4)
    os.remove(l5[1])
    got = P.PolicyBank.from_reference_dir(_dev(), str(tmp_path), "HighLevel", args, max_rows=4096)
    _same_banks(got, _hand_bank(actor_weights(learners["fight"]) + actor_weights(learners["escape"]), sels), 4)


@pytest.mark.parametrize("mode", ["fight", "escape"])
def test_from_policy_files_gives_the_exporters_modules(exported, mode):
    from hhmarl_2d_amd import learner as LR
    d, learners, _ = exported
    src = learners[mode]
    got = LR.PPOLearner.from_policy_files(_dev(), d, 3, mode, seed=3, **LEARN)
    assert got.kinds == src.kinds
    assert same(got.state_dict()["modules"], src.state_dict()["modules"]) is None
    assert got.modules[0].shared_layer is got.modules[1].shared_layer                 # tied, as every learner's
    # the weights only: Adam state, kl_coeff and the update count are a fresh learner's
    fresh = _learner(mode)
    assert same(got.state_dict()["policies"], fresh.state_dict()["policies"]) is None and got.updates == 0 and got.kl_coeff == fresh.kl_coeff
    assert same(got.state_dict()["modules"], fresh.state_dict()["modules"]) is not None


def test_export_and_from_policy_files_refusals(exported, tmp_path):
    import shutil
    from hhmarl_2d_amd import learner as LR
    d, learners, paths = exported
    fight = learners["fight"]
    with pytest.raises(ValueError, match="trains the fight policies"):
        fight.export_policies(str(tmp_path), 3, agent_mode="escape")
    with pytest.raises(ValueError, match="level"):
        fight.export_policies(str(tmp_path / "none"), 6)
    assert os.listdir(tmp_path) == []
    made = fight.export_policies(str(tmp_path / "a" / "b"), 1, agent_mode="fight")      # any level; the directory is created
    assert made == [str(tmp_path / "a" / "b" / f"L1_AC{ac}_fight.pt") for ac in (1, 2)] and all(os.path.isfile(p) for p in made)
    # two files of two different exports: their shared layers differ
    other = _train_a_little(_train_a_little(_learner("fight")))
    mixed = tmp_path / "mixed"
    other.export_policies(str(mixed), 3)
    shutil.copy(paths["fight"][0], str(mixed))
    with pytest.raises(ValueError, match=r"`shared_layer._model.0.weight` differs"):
        LR.PPOLearner.from_policy_files(_dev(), str(mixed), 3, "fight", **LEARN)
    with pytest.raises(FileNotFoundError):
        LR.PPOLearner.from_policy_files(_dev(), d, 4, "fight", **LEARN)
    with pytest.raises(ValueError, match="agent_mode"):
        LR.PPOLearner.from_policy_files(_dev(), d, 3, "both", **LEARN)
    # a file under another policy's name
    swapped = tmp_path / "swapped"
    os.makedirs(swapped)
    shutil.copy(paths["escape"][0], str(swapped / "L3_AC1_fight.pt"))
    shutil.copy(paths["fight"][1], str(swapped / "L3_AC2_fight.pt"))
    with pytest.raises(ValueError, match="holds a Esc1 network"):
        LR.PPOLearner.from_policy_files(_dev(), str(swapped), 3, "fight", **LEARN)


def test_evaluator_takes_the_exported_commander_file(tmp_path):
    from test_gpu_evaluation import _policy_dir
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_files as PF
    from hhmarl_2d_amd.config import make_args
    from hhmarl_2d_amd.evaluation import Evaluator
    pol = tmp_path / "policies"
    os.makedirs(pol)
    learner = LR.CommanderLearner.trainable_init(_dev(), seed=17, **LEARN)
    with torch.no_grad():
        learner.module.act_out._model[0].bias.add_(torch.tensor([0.05, -0.05, 0.02], device="cuda"))
    path = learner.export_commander(str(tmp_path / "commander.pt"))
    assert path == str(tmp_path / "commander.pt")
    sd = {k: v.detach().cpu() for k, v in learner.module.state_dict().items()}
    assert same(PF.load_commander(path), dict(sd)) is None
    assert torch.load(path, weights_only=True)["format"] == "hhmarl_2d_amd.commander"
    args = make_args(2, horizon=30)
    runs = []
    for commander in (sd, path, tmp_path / "commander.pt"):
        ev = Evaluator(args, commander=commander, policy_dir=_policy_dir(pol), max_arenas=32)
        runs.append((ev.run(n_episodes=32, seed=3), ev.per_episode.copy()))
        ev.close()
    assert runs[0][0] == runs[1][0] == runs[2][0] and runs[0][0]["agent_steps"] > 0
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][1], runs[2][1])
    with pytest.raises(FileNotFoundError):
        Evaluator(args, commander=str(tmp_path / "none.pt"), policy_dir=str(pol))
    with pytest.raises(ValueError, match="is not a hhmarl_2d_amd.commander file"):
        Evaluator(args, commander=_plain_policy(tmp_path), policy_dir=str(pol))      # a policy file is no commander file


def _plain_policy(tmp_path):
    from hhmarl_2d_amd import policy_files as PF
    from hhmarl_2d_amd import policy_nets as PN
    return PF.save_policy(str(tmp_path / "p.pt"), PN.ESC1, dict(PN.random_weights(PN.ESC1, 1), **PN.random_critic_weights(PN.ESC1, 1)))
