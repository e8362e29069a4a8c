"""checkpoint.load_subset / checkpoint.contents without a GPU: a subset of a file's objects loads alone and leaves the others as they
are, everything `load` validates is validated before anything is touched, and `load` itself keeps refusing a partial set.  Plain
stand-in objects, as tests/test_checkpoint_host.py uses them (imported from there); the learner's hand-over from one level of the
curriculum to the next is tested on the device (tests/test_gpu_curriculum_handover.py)."""
import pytest
import torch

from hhmarl_2d_amd import checkpoint as ck
from test_checkpoint_host import Box, Crate, Planned


class Refusing(Box):
    """a stand-in whose own validation refuses every state"""

    def _load_plan(self, sd):
        raise ValueError("Refusing: `lr` was 0.1 when saved, the live object has 0.2")


def _file(tmp_path):
    path = tmp_path / "a.ckpt"
    ck.save(path, world=Box(1), bank=Crate(2), learner=Planned(3))
    return path


def _untouched(objs, seeds):
    return all(o.loads == 0 and o.same(type(o)(s)) for o, s in zip(objs, seeds))


def test_one_name_out_of_three_loads_alone(tmp_path):
    path = _file(tmp_path)
    world, bank, learner = Box(10), Crate(20), Planned(30)
    ck.load_subset(path, learner=learner)
    assert learner.same(Planned(3)) and learner.loads == 1
    assert _untouched((world, bank), (10, 20))
    ck.load_subset(path, bank=bank, world=world)             # two of three, in another order than saved
    assert world.same(Box(1)) and bank.same(Crate(2)) and world.loads == bank.loads == 1 and learner.loads == 1


def test_all_names_load_as_load_does(tmp_path):
    path = _file(tmp_path)
    a, b = (Box(10), Crate(20), Planned(30)), (Box(10), Crate(20), Planned(30))
    ck.load_subset(path, world=a[0], bank=a[1], learner=a[2])
    ck.load(path, world=b[0], bank=b[1], learner=b[2])
    assert all(x.same(y) and x.loads == y.loads == 1 for x, y in zip(a, b))


@pytest.mark.parametrize("objects, match", [
    (lambda: dict(learner=Planned(30), rollout=Box(40)), r"the file holds \['bank', 'learner', 'world'\], not \['rollout'\]"),   # a name that is not in the file
    (lambda: dict(rollout=Box(40)), "not \\['rollout'\\]"),
    (lambda: dict(world=Box(10), learner=Box(30)), "`learner` was saved as a Planned, the object given is a Box"),               # another type
    (lambda: dict(world=Box(10), learner=Refusing(30)), "`learner` was saved as a Planned"),
])
def test_wrong_names_and_types_are_refused_with_nothing_touched(tmp_path, objects, match):
    path = _file(tmp_path)
    objs = objects()
    twins = {k: type(v)(v.count) for k, v in objs.items()}
    with pytest.raises(ValueError, match=match):
        ck.load_subset(path, **objs)
    assert all(v.loads == 0 and v.same(twins[k]) for k, v in objs.items())


def test_a_refusing_load_plan_stops_the_whole_subset(tmp_path):
    path = tmp_path / "a.ckpt"
    ck.save(path, world=Box(1), bank=Crate(2), learner=Refusing(3))
    world, learner = Box(10), Refusing(30)
    with pytest.raises(ValueError, match="`lr` was 0.1 when saved"):
        ck.load_subset(path, world=world, learner=learner)    # the world is given first and is valid: it must not be loaded
    assert _untouched((world, learner), (10, 30))
    # ... and a state that an object's validation refuses, as load's own test has it
    ck.save(path, world=Box(1), learner=Planned(3), other=Planned(4))
    doc = torch.load(path, weights_only=True)
    doc["state"]["learner"]["w"] = torch.zeros((4, 4))
    torch.save(doc, path)
    world, learner = Box(10), Planned(30)
    with pytest.raises(ValueError, match="`w` was saved with shape"):
        ck.load_subset(path, world=world, learner=learner)
    assert _untouched((world, learner), (10, 30))
    ck.load_subset(path, world=world)                         # the object whose state is damaged is not named: the rest loads
    assert world.same(Box(1))


@pytest.mark.parametrize("edit, match", [
    (lambda d: d.update(version=ck.FORMAT_VERSION + 1), "format version"),
    (lambda d: d.update(format="something else"), "is not a"),
    (lambda d: d["state"].pop("bank"), "no consistent object table"),
])
def test_wrong_versions_and_formats_are_refused(tmp_path, edit, match):
    path = _file(tmp_path)
    doc = torch.load(path, weights_only=True)
    edit(doc)
    torch.save(doc, path)
    learner = Planned(30)
    with pytest.raises(ValueError, match=match):
        ck.load_subset(path, learner=learner)
    with pytest.raises(ValueError, match=match):
        ck.contents(path)
    assert _untouched((learner,), (30,))


def test_objects_must_be_given_and_have_the_two_methods(tmp_path):
    path = _file(tmp_path)
    with pytest.raises(ValueError, match="no objects given"):
        ck.load_subset(path)
    with pytest.raises(ValueError, match="has no state_dict"):
        ck.load_subset(path, learner=object())


def test_contents_lists_names_and_types(tmp_path):
    path = _file(tmp_path)
    assert ck.contents(path) == {"world": "Box", "bank": "Crate", "learner": "Planned"}
    assert ck.contents(str(path)) == ck.contents(path)
    with pytest.raises(FileNotFoundError):
        ck.contents(tmp_path / "none.ckpt")


def test_load_itself_still_refuses_a_strict_subset(tmp_path):
    path = _file(tmp_path)
    learner, world = Planned(30), Box(10)
    with pytest.raises(ValueError, match="the file holds"):
        ck.load(path, learner=learner)
    with pytest.raises(ValueError, match="the file holds"):
        ck.load(path, learner=learner, world=world)
    assert _untouched((learner, world), (30, 10))
