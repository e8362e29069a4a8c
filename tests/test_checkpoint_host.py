"""hhmarl_2d_amd/checkpoint.py without a GPU: the file format round-trips, the write is atomic, and wrong names, types and versions are
refused with the objects untouched.  Plain stand-in objects with state_dict / load_state_dict; the real objects of the loop are
tested on the device (tests/test_gpu_resume.py)."""
import os

import pytest
import torch

from hhmarl_2d_amd import checkpoint as ck


class Box:
    """a stand-in with the two methods and nothing else"""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.w = torch.randn((3, 5), generator=g)
        self.n = torch.randint(0, 100, (7,), generator=g, dtype=torch.int32)
        self.count, self.name, self.loads = seed, f"box{seed}", 0

    def state_dict(self):
        return {"w": self.w.clone(), "nested": {"n": self.n.clone(), "list": [self.count, 2.5, None, True]}, "count": self.count, "name": self.name}

    def load_state_dict(self, sd):
        self.w.copy_(sd["w"])
        self.n.copy_(sd["nested"]["n"])
        self.count, self.name = sd["count"], sd["name"]
        self.loads += 1

    def same(self, other):
        return torch.equal(self.w, other.w) and torch.equal(self.n, other.n) and (self.count, self.name) == (other.count, other.name)


class Crate(Box):
    """another type with the same state"""


class Planned(Box):
    """a stand-in that validates in _load_plan, as the objects of the loop do"""

    def _load_plan(self, sd):
        ck.need_keys("Planned", sd, ("w", "nested", "count", "name"))
        ck.check_tensor("Planned", "w", sd["w"], self.w)
        return lambda: self.load_state_dict(sd)


class Failing(Box):
    def state_dict(self):
        raise RuntimeError("serializer failed midway")


def test_round_trip_of_tensors_scalars_and_nesting(tmp_path):
    path = tmp_path / "a.ckpt"
    a, b = Box(1), Crate(2)
    size = ck.save(path, first=a, second=b)
    assert size == os.path.getsize(path) > 0
    a2, b2 = Box(10), Crate(20)
    assert not a2.same(a)
    ck.load(path, first=a2, second=b2)
    assert a2.same(a) and b2.same(b) and a2.loads == b2.loads == 1


def test_file_is_a_plain_dict_with_a_header(tmp_path):
    path = tmp_path / "a.ckpt"
    ck.save(path, first=Box(1), second=Crate(2))
    doc = torch.load(path, weights_only=True)          # no pickled classes: the restricted loader reads it
    assert doc["format"] == ck.FORMAT and doc["version"] == ck.FORMAT_VERSION
    assert doc["objects"] == {"first": "Box", "second": "Crate"}
    assert set(doc["state"]) == {"first", "second"}
    st = doc["state"]["first"]
    assert st["nested"]["list"] == [1, 2.5, None, True] and st["name"] == "box1" and st["w"].device.type == "cpu"


def test_failed_save_leaves_the_old_file_byte_identical(tmp_path):
    path = tmp_path / "a.ckpt"
    ck.save(path, first=Box(1), second=Box(2))
    before = path.read_bytes()
    with pytest.raises(RuntimeError, match="serializer failed midway"):
        ck.save(path, first=Box(3), second=Failing(4))      # the first object serialises, the second raises
    assert path.read_bytes() == before
    assert sorted(os.listdir(tmp_path)) == ["a.ckpt"]         # no temporary file left behind
    b = Box(9)
    ck.load(path, first=b, second=Box(8))
    assert b.same(Box(1))


def test_failed_first_save_leaves_no_file(tmp_path):
    path = tmp_path / "a.ckpt"
    with pytest.raises(RuntimeError):
        ck.save(path, only=Failing(1))
    assert os.listdir(tmp_path) == []


def test_save_replaces_atomically_through_a_temporary_in_the_same_directory(tmp_path, monkeypatch):
    path = tmp_path / "a.ckpt"
    seen = []
    real = os.replace

    def spy(src, dst):
        seen.append((os.path.dirname(os.path.abspath(src)), os.path.abspath(dst), os.path.exists(src)))
        real(src, dst)
    monkeypatch.setattr(os, "replace", spy)
    ck.save(path, only=Box(1))
    assert seen == [(str(tmp_path), str(path), True)]


@pytest.mark.parametrize("objects, match", [
    (lambda: dict(first=Box(5)), "the file holds"),                              # a name missing
    (lambda: dict(first=Box(5), second=Box(6), third=Box(7)), "the file holds"),  # a name too many
    (lambda: dict(first=Box(5), other=Box(6)), "the file holds"),                 # another name
    (lambda: dict(first=Crate(5), second=Box(6)), "was saved as a Box"),          # another type
])
def test_wrong_names_and_types_are_refused_before_any_object_is_touched(tmp_path, objects, match):
    path = tmp_path / "a.ckpt"
    ck.save(path, first=Box(1), second=Box(2))
    objs = objects()
    twins = {k: type(v)(v.count) for k, v in objs.items()}
    with pytest.raises(ValueError, match=match):
        ck.load(path, **objs)
    assert all(v.loads == 0 and v.same(twins[k]) for k, v in objs.items())


@pytest.mark.parametrize("edit, match", [
    (lambda d: d.update(version=ck.FORMAT_VERSION + 1), "format version"),
    (lambda d: d.update(format="something else"), "is not a"),
    (lambda d: d["state"].pop("second"), "no consistent object table"),
])
def test_wrong_versions_and_formats_are_refused(tmp_path, edit, match):
    path = tmp_path / "a.ckpt"
    ck.save(path, first=Box(1), second=Box(2))
    doc = torch.load(path, weights_only=True)
    edit(doc)
    torch.save(doc, path)
    a, b = Box(5), Box(6)
    with pytest.raises(ValueError, match=match):
        ck.load(path, first=a, second=b)
    assert a.loads == b.loads == 0 and a.same(Box(5)) and b.same(Box(6))


def test_every_object_is_validated_before_the_first_is_loaded(tmp_path):
    path = tmp_path / "a.ckpt"
    ck.save(path, first=Planned(1), second=Planned(2))
    doc = torch.load(path, weights_only=True)
    doc["state"]["second"]["w"] = torch.zeros((4, 4))        # the SECOND object's state no longer fits
    torch.save(doc, path)
    a, b = Planned(5), Planned(6)
    with pytest.raises(ValueError, match="`w` was saved with shape"):
        ck.load(path, first=a, second=b)
    assert a.loads == b.loads == 0 and a.same(Planned(5))


def test_objects_without_the_two_methods_are_refused(tmp_path):
    with pytest.raises(ValueError, match="has no state_dict"):
        ck.save(tmp_path / "a.ckpt", thing=object())
    with pytest.raises(ValueError, match="no objects given"):
        ck.save(tmp_path / "a.ckpt")
    assert os.listdir(tmp_path) == []


def test_helpers_name_the_field():
    with pytest.raises(ValueError, match="`lr` was 0.1 when saved, the live object has 0.2"):
        ck.check_options("X", {"lr": 0.1, "n": 2}, {"lr": 0.2, "n": 2})
    ck.check_options("X", {"betas": [0.9, 0.999], "clip": None}, {"betas": (0.9, 0.999), "clip": None})   # a list is the tuple it was saved from
    with pytest.raises(ValueError, match="has no `n`"):
        ck.check_options("X", {"lr": 0.1}, {"lr": 0.1, "n": 2})
    with pytest.raises(ValueError, match="`m` was saved as torch.float64"):
        ck.check_tensor("X", "m", torch.zeros(3, dtype=torch.float64), torch.zeros(3))
    with pytest.raises(ValueError, match="`m` was saved with shape"):
        ck.check_tensor("X", "m", torch.zeros(4), torch.zeros(3))
    ck.check_tensor("X", "rows", torch.zeros((2, 5)), torch.zeros((8, 5)), lead=2)                        # a cut buffer
    with pytest.raises(ValueError, match="`rows`"):
        ck.check_tensor("X", "rows", torch.zeros((9, 5)), torch.zeros((8, 5)), lead=9)
    blob = torch.zeros(32, dtype=torch.uint8)
    blob[:8] = torch.tensor(list(b"HHSW") + [1, 0, 0, 0], dtype=torch.uint8)
    ck.check_blob("X", blob, 32, b"HHSW")
    with pytest.raises(ValueError, match="truncated"):
        ck.check_blob("X", blob[:16], 32, b"HHSW")
    with pytest.raises(ValueError, match="magic"):
        ck.check_blob("X", blob, 32, b"HHSP")
    blob[4] = 2
    with pytest.raises(ValueError, match="format version 2"):
        ck.check_blob("X", blob, 32, b"HHSW")
