"""hhmarl_2d_amd/policy_files.py without a GPU: the curriculum's file names, the plain policy-file format round-trips bit for bit for all
four architectures and reads under the restricted loader, the write is atomic, every refusal names the key and leaves the previous
file as it was, and from_policy_object takes a document or a loaded reference module.  The banks, learners and evaluators that read
and write these files are tested on the device (tests/test_gpu_policy_files.py)."""
import os

import numpy as np
import pytest
import torch

from hhmarl_2d_amd import policy_files as PF
from hhmarl_2d_amd import policy_nets as PN
from test_policy_nets import _stub_reference_module

KINDS = [PN.FIGHT1, PN.FIGHT2, PN.ESC1, PN.ESC2]
kind_ids = lambda k: PN.KIND_NAMES[k]


def _state(kind, seed=4):
    return dict(PN.random_weights(kind, seed), **PN.random_critic_weights(kind, seed))


def _bits(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------- names
def test_names_for_every_level_aircraft_and_mode():
    for level in range(1, 6):
        for ac in (1, 2):
            for mode in ("fight", "escape"):
                assert PF.policy_file_name(level, ac, mode) == f"L{level}_AC{ac}_{mode}.pt"
    # the names PolicyBank.from_reference_dir looks for (env_base.py:312-347)
    assert PF.policy_file_name(3, 1, "fight") == "L3_AC1_fight.pt" and PF.policy_file_name(5, 2, "escape") == "L5_AC2_escape.pt"


@pytest.mark.parametrize("level, ac, mode, match", [
    (0, 1, "fight", "level"), (6, 1, "fight", "level"), ("3", 1, "fight", "level"), (3.0, 1, "fight", "level"), (True, 1, "fight", "level"),
    (3, 0, "fight", "ac"), (3, 3, "fight", "ac"), (3, "1", "fight", "ac"),
    (3, 1, "Fight", "agent_mode"), (3, 1, "esc", "agent_mode"), (3, 1, None, "agent_mode"),
])
def test_names_outside_the_curriculum_are_refused(level, ac, mode, match):
    with pytest.raises(ValueError, match=match):
        PF.policy_file_name(level, ac, mode)


# ---------------------------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("kind", KINDS, ids=kind_ids)
def test_round_trip_is_bit_for_bit(tmp_path, kind):
    sd = _state(kind)
    mode = "fight" if PN.HAS_ATT[kind] else "escape"
    path = tmp_path / PF.policy_file_name(3, 1 if kind in (PN.FIGHT1, PN.ESC1) else 2, mode)
    assert PF.save_policy(path, kind, sd, level=3, agent_mode=mode) == str(path)
    got_kind, got = PF.load_policy(path)
    assert got_kind == kind and set(got) == set(PN.actor_keys(kind)) | set(PN.critic_keys(kind)) == set(sd)
    for k, v in sd.items():
        assert got[k].dtype == torch.float32 and got[k].device.type == "cpu" and tuple(got[k].shape) == v.shape
        assert np.array_equal(_bits(got[k]), _bits(v)), k


@pytest.mark.parametrize("kind", KINDS, ids=kind_ids)
def test_file_is_a_plain_dict_the_restricted_loader_reads(tmp_path, kind):
    path = tmp_path / "p.pt"
    # torch tensors (a module's state_dict()) are taken as numpy arrays are
    PF.save_policy(path, kind, {k: torch.from_numpy(v) for k, v in _state(kind).items()})
    doc = torch.load(path, weights_only=True)               # no pickled classes
    assert set(doc) == {"format", "version", "kind", "level", "agent_mode", "state"}
    assert doc["format"] == PF.FORMAT == "hhmarl_2d_amd.policy" and doc["version"] == PF.FORMAT_VERSION == 1
    assert doc["kind"] == kind and type(doc["kind"]) is int and doc["level"] is None and doc["agent_mode"] is None
    assert all(isinstance(v, torch.Tensor) and v.dtype == torch.float32 for v in doc["state"].values())
    want = dict(PN.actor_keys(kind), **PN.critic_keys(kind))
    assert {k: tuple(v.shape) for k, v in doc["state"].items()} == want


def test_level_and_mode_are_recorded_and_checked(tmp_path):
    path = tmp_path / "p.pt"
    PF.save_policy(path, PN.ESC2, _state(PN.ESC2), level=5, agent_mode="escape")
    doc = torch.load(path, weights_only=True)
    assert doc["level"] == 5 and doc["agent_mode"] == "escape"
    before = path.read_bytes()
    with pytest.raises(ValueError, match="no fight policy"):
        PF.save_policy(path, PN.ESC2, _state(PN.ESC2), level=5, agent_mode="fight")
    with pytest.raises(ValueError, match="level"):
        PF.save_policy(path, PN.ESC2, _state(PN.ESC2), level=7)
    assert path.read_bytes() == before


def test_save_replaces_atomically_through_a_temporary_in_the_same_directory(tmp_path, monkeypatch):
    path = tmp_path / "p.pt"
    seen = []
    real = os.replace

    def spy(src, dst):
        seen.append((os.path.dirname(os.path.abspath(src)), os.path.abspath(dst), os.path.exists(src)))
        real(src, dst)
    monkeypatch.setattr(os, "replace", spy)
    PF.save_policy(path, PN.FIGHT1, _state(PN.FIGHT1))
    assert seen == [(str(tmp_path), str(path), True)]
    assert os.listdir(tmp_path) == ["p.pt"]


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def _drop(sd, k):
    sd.pop(k)


def _extra(sd, k):
    sd["att_extra.weight"] = np.zeros((3, 3), dtype=np.float32)


def _reshape(sd, k):
    sd[k] = np.zeros(tuple(s + 1 for s in sd[k].shape), dtype=np.float32)


def _nan(sd, k):
    sd[k] = sd[k].copy()
    sd[k].reshape(-1)[3] = np.nan


def _inf(sd, k):
    sd[k] = sd[k].copy()
    sd[k].reshape(-1)[0] = -np.inf


BAD_STATES = [(_drop, "act_out._model.0.bias", "has no `act_out._model.0.bias`"), (_drop, "val_out._model.0.weight", "has no `val_out._model.0.weight`"),
              (_extra, "att_extra.weight", "unexpected `att_extra.weight`"), (_reshape, "inp2._model.0.weight", "`inp2._model.0.weight` has shape"),
              (_reshape, "shared_layer._model.0.bias", "`shared_layer._model.0.bias` has shape"),
              (_nan, "shared_layer._model.0.weight", "`shared_layer._model.0.weight` holds a non-finite"), (_inf, "inp1._model.0.bias", "`inp1._model.0.bias` holds a non-finite")]


@pytest.mark.parametrize("kind", [PN.FIGHT2, PN.ESC1], ids=kind_ids)
@pytest.mark.parametrize("edit, key, match", BAD_STATES, ids=[f"{e.__name__[1:]}-{k.split('.')[0]}" for e, k, _ in BAD_STATES])
def test_save_refuses_a_bad_state_and_leaves_the_previous_file(tmp_path, kind, edit, key, match):
    path = tmp_path / "p.pt"
    PF.save_policy(path, kind, _state(kind, 1))
    before = path.read_bytes()
    sd = _state(kind, 2)
    edit(sd, key)
    with pytest.raises(ValueError, match=match):
        PF.save_policy(path, kind, sd)
    assert path.read_bytes() == before
    assert os.listdir(tmp_path) == ["p.pt"]                  # no temporary file left behind
    assert PF.load_policy(path)[0] == kind


def test_save_refuses_an_unknown_kind(tmp_path):
    path = tmp_path / "p.pt"
    for kind in (4, -1, "Fight1", None, True):
        with pytest.raises(ValueError, match="kind"):
            PF.save_policy(path, kind, _state(PN.FIGHT1))
    with pytest.raises(ValueError, match="has no `inp1_val._model.0.weight`"):     # another kind's tensors
        PF.save_policy(path, PN.ESC1, _state(PN.FIGHT1))
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("edit, key, match", BAD_STATES, ids=[f"{e.__name__[1:]}-{k.split('.')[0]}" for e, k, _ in BAD_STATES])
def test_load_refuses_a_bad_state(tmp_path, edit, key, match):
    path = tmp_path / "p.pt"
    PF.save_policy(path, PN.FIGHT1, _state(PN.FIGHT1))
    doc = torch.load(path, weights_only=True)
    sd = {k: v.numpy() for k, v in doc["state"].items()}
    edit(sd, key)
    doc["state"] = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    torch.save(doc, path)
    with pytest.raises(ValueError, match=match):
        PF.load_policy(path)
    with pytest.raises(ValueError, match=match):
        PF.from_policy_object(torch.load(path, weights_only=True))


@pytest.mark.parametrize("edit, match", [
    (lambda d: d.update(version=PF.FORMAT_VERSION + 1), "format version 2"),
    (lambda d: d.update(format="hhmarl_2d_amd.checkpoint"), "is not a hhmarl_2d_amd.policy file"),
    (lambda d: d.update(format=PF.COMMANDER_FORMAT), "is not a hhmarl_2d_amd.policy file"),
    (lambda d: d.update(kind=7), "kind"),
    (lambda d: d.pop("state"), "state"),
])
def test_load_refuses_another_format_or_version(tmp_path, edit, match):
    path = tmp_path / "p.pt"
    PF.save_policy(path, PN.ESC1, _state(PN.ESC1))
    doc = torch.load(path, weights_only=True)
    edit(doc)
    torch.save(doc, path)
    with pytest.raises(ValueError, match=match):
        PF.load_policy(path)


def test_load_of_a_missing_file_is_file_not_found(tmp_path):
    with pytest.raises(FileNotFoundError):
        PF.load_policy(tmp_path / "L3_AC1_fight.pt")
    with pytest.raises(FileNotFoundError):
        PF.load_policy_file(str(tmp_path / "L3_AC1_fight.pt"))
    with pytest.raises(FileNotFoundError):
        PF.load_commander(tmp_path / "commander.pt")


# ---------------------------------------------------------------------------------------------------------------------------- objects
@pytest.mark.parametrize("kind", KINDS, ids=kind_ids)
def test_from_policy_object_on_a_document_gives_the_saved_actor(tmp_path, kind):
    path = tmp_path / "p.pt"
    sd = _state(kind)
    PF.save_policy(path, kind, sd)
    got_kind, got = PF.from_policy_object(PF.load_policy_file(str(path)))
    assert got_kind == kind and list(got) == list(PN.actor_keys(kind))
    for k in PN.actor_keys(kind):
        assert isinstance(got[k], np.ndarray) and got[k].dtype == np.float32 and np.array_equal(_bits(got[k]), _bits(sd[k])), k


@pytest.mark.parametrize("kind", KINDS, ids=kind_ids)
def test_from_policy_object_on_a_module_is_from_torch_module(tmp_path, kind):
    net, _ = _stub_reference_module(kind, 5)
    want_kind, want = PN.from_torch_module(net)
    got_kind, got = PF.from_policy_object(net)
    assert got_kind == want_kind == kind and list(got) == list(want)
    for k in want:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    # ... and through a file: the restricted loader refuses the pickled module, the default loader falls back to unpickling it
    path = str(tmp_path / "L3_AC1_fight.pt")
    torch.save(net, path)
    with pytest.raises(Exception):
        torch.load(path, weights_only=True)
    got_kind, got = PF.from_policy_object(PF.load_policy_file(path))
    assert got_kind == kind and all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in want)


def test_from_policy_object_refuses_other_dicts():
    with pytest.raises(ValueError, match="not a hhmarl_2d_amd.policy document"):
        PF.from_policy_object({"format": "hhmarl_2d_amd.checkpoint"})
    with pytest.raises(ValueError, match="not a hhmarl_2d_amd.policy document"):
        PF.from_policy_object(_state(PN.FIGHT1))              # a bare state dict carries no kind


# ---------------------------------------------------------------------------------------------------------------------------- the commander
def test_commander_file_round_trips_and_refuses(tmp_path):
    from hhmarl_2d_amd.commander import random_weights, state_keys
    path = tmp_path / "commander.pt"
    sd = random_weights(6)
    PF.save_commander(path, sd)
    doc = torch.load(path, weights_only=True)
    assert doc["format"] == "hhmarl_2d_amd.commander" and doc["version"] == 1 and set(doc) == {"format", "version", "state"}
    got = PF.load_commander(path)
    assert list(got) == list(state_keys())
    for k, v in sd.items():
        assert np.array_equal(_bits(got[k]), _bits(v)), k
    before = path.read_bytes()
    bad = dict(sd)
    bad.pop("rnn_val.bias_hh_l0")
    with pytest.raises(ValueError, match="has no `rnn_val.bias_hh_l0`"):
        PF.save_commander(path, bad)
    bad = dict(sd, **{"v4._model.0.weight": np.full((200, 105), np.nan, dtype=np.float32)})
    with pytest.raises(ValueError, match="`v4._model.0.weight` holds a non-finite"):
        PF.save_commander(path, bad)
    assert path.read_bytes() == before
    with pytest.raises(ValueError, match="is not a hhmarl_2d_amd.policy file"):
        PF.load_policy(path)
    policy = tmp_path / "p.pt"
    PF.save_policy(policy, PN.FIGHT1, _state(PN.FIGHT1))
    with pytest.raises(ValueError, match="is not a hhmarl_2d_amd.commander file"):
        PF.load_commander(policy)
