"""Save and resume on the MI355X, end to end: run A does PROLOGUE + K1 + K2 iterations of collect -> update -> publish uninterrupted;
run B does PROLOGUE + K1, checkpoint.save, builds FRESH objects from the same constructor arguments, checkpoint.load, then K2.  Every
later collect's window buffers, every emitted batch (rows, tables, metrics), every statistics dict of update, the final module weights
and Adam state and the samplers' outputs are the same bit for bit (tests/resume_harness.py has the configurations, the iteration, the
records and the comparison; N = 64, T = 8, num_sgd_iter = 2, sgd_minibatch_size = 64, K1 = K2 = 2).

Each test asserts at its save point that the state it saves is not a trivial one: an arena mid-episode with a non-empty carry, a rocket
in flight and a dead aircraft somewhere, kl_coeff moved off its initial value and, with train_batch_size, the accumulator partly filled
and not ready()."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resume_harness as H

pytestmark = pytest.mark.gpu
CONFIGS = ("fight_torch", "escape_graph", "level5_fused", "commander_graph")


def _preconditions(name, objs):
    ro, learner, w = objs["rollout"], objs["learner"], objs["world"]
    torch.cuda.synchronize()
    st = w.get_state()
    n_units = w.cfg.n_agents + w.cfg.n_opps
    running = (st["ar_i"][:, 0] > 0) & (st["ar_i"][:, 1] > 0) & (st["ar_i"][:, 2] > 0)
    assert running.any(), "an arena is mid-episode"
    assert (st["rk_i"][:, :, 0] > 0).any(), "a rocket is in flight"
    assert (st["ac_i"][:, :n_units, 0] == 0).any(), "an aircraft is dead"
    if ro.episodes is not None:
        carried = ro.episodes.carried.cpu().numpy()
        assert (carried[running] > 0).any(), "a running arena has a non-empty carry"
        if ro.episodes.train_batch_size is not None:
            info = ro.episodes.batch_info()
            assert 0 < info["rows"] < ro.episodes.train_batch_size and not ro.episodes.ready(), "the accumulator is partly filled and not ready"
    kl = learner.kl_coeff if isinstance(learner.kl_coeff, list) else [learner.kl_coeff]
    assert all(k != 0.2 for k in kl), "kl_coeff has moved off its initial value"
    assert learner.updates > 0


_A = {}


def _run_a(name):
    """the uninterrupted run, once per configuration -> (records of the K2 iterations, final, its objects — still alive, graphs captured)"""
    if name not in _A:
        objs = H.build(name)
        H.iterate(name, objs, H.PROLOGUE[name] + H.K1)
        recs = H.iterate(name, objs, H.K2)
        _A[name] = (recs, H.final(name, objs), objs)
    return _A[name]


_B = {}


@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("resume")


def _run_b_to_save(name, folder, between=False):
    """run B up to its save, once per configuration: PROLOGUE + K1 iterations and checkpoint.save (between: after the last update,
    before its publish); its objects are dropped -> (the file, the bank's fp32 blobs at the save)"""
    from hhmarl_2d_amd import checkpoint
    if (name, between) not in _B:
        path = folder / f"{name}{'_between' if between else ''}.ckpt"
        objs = H.build(name)
        H.iterate(name, objs, H.PROLOGUE[name] + H.K1 - 1)
        H.update(name, objs, H.collect(name, objs))
        if not between:
            H.publish(name, objs)
        _preconditions(name, objs)
        size = checkpoint.save(path, **H.saved(objs))
        assert size == os.path.getsize(path)
        _B[(name, between)] = (path, [objs["bank"].packed(s, 0).cpu() for s in (0, 1)] if "bank" in objs else None)
    return _B[(name, between)]


def _assert_same(got, want, what):
    d = H.same(got, want, what)
    assert d is None, d


def _learned_something(recs):
    stats = [r["stats"] for r in recs if r["stats"] is not None]
    flat = [s for x in stats for s in (x if isinstance(x, list) else [x])]
    assert any(s["steps"] > 0 for s in flat), "an update with minibatch steps happens after the resume as well"


@pytest.mark.parametrize("name", CONFIGS)
def test_resume_into_fresh_objects(name, ckpt_dir):
    from hhmarl_2d_amd import checkpoint
    want, want_final, _ = _run_a(name)
    _learned_something(want)
    path, _ = _run_b_to_save(name, ckpt_dir)
    fresh = H.build(name)
    checkpoint.load(path, **H.saved(fresh))
    _assert_same(H.iterate(name, fresh, H.K2), want, name)
    _assert_same(H.final(name, fresh), want_final, name + " final")


def test_save_between_update_and_publish(ckpt_dir):
    """the sampler still holds the weights the update started from, the learner the new ones: both are in the file as they are"""
    from hhmarl_2d_amd import checkpoint
    name = "escape_graph"          # its window updates take steps in every iteration: the publish after the save changes the bank
    want, want_final, _ = _run_a(name)
    path, stale = _run_b_to_save(name, ckpt_dir, between=True)
    fresh = H.build(name)
    checkpoint.load(path, **H.saved(fresh))
    assert all(torch.equal(fresh["bank"].packed(s, 0).cpu(), x) for s, x in enumerate(stale)), "the bank came back with its pre-publish bytes"
    H.publish(name, fresh)
    assert not all(torch.equal(fresh["bank"].packed(s, 0).cpu(), x) for s, x in enumerate(stale)), "the publish was still to come"
    _assert_same(H.iterate(name, fresh, H.K2), want, name)
    _assert_same(H.final(name, fresh), want_final, name + " final")


@pytest.mark.parametrize("name", ["escape_graph", "commander_graph"])
def test_load_into_live_objects_that_have_captured_their_graphs(name, ckpt_dir):
    """run A's own objects — K2 iterations further on, collect and step graphs captured — are loaded into and replay"""
    from hhmarl_2d_amd import checkpoint
    want, want_final, live = _run_a(name)
    path, _ = _run_b_to_save(name, ckpt_dir)
    ro, learner = live["rollout"], live["learner"]
    books = learner._books if name == "escape_graph" else [learner._book]
    collect_graph = ro._graph
    assert collect_graph is not None and all(b.graph is not None and b.captures > 0 for b in books)
    checkpoint.load(path, **H.saved(live))
    _assert_same(H.iterate(name, live, H.K2), want, name)
    _assert_same(H.final(name, live), want_final, name + " final")
    # (the step graphs hold kl_coeff by value and are captured again whenever it has moved: graph_prepare's key)
    assert ro._graph is collect_graph, "the collect replayed from the graph it had captured"


def test_resume_in_a_fresh_process(ckpt_dir, tmp_path):
    name = "fight_torch"
    want, want_final, _ = _run_a(name)
    path, out = _run_b_to_save(name, ckpt_dir)[0], tmp_path / "child.pt"
    child = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "resume_harness.py"), name, str(path), str(H.K2), str(out)],
                           capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    got = torch.load(out, weights_only=True)
    _assert_same(got["records"], want, name)
    _assert_same(got["final"], want_final, name + " final")


def test_mismatched_objects_are_refused_before_anything_changes(tmp_path):
    """load_state_dict validates everything first: recorded options, shapes, dtypes — ValueError names the field, the object is untouched"""
    from hhmarl_2d_amd import checkpoint
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd.rollout import PPORollout
    name = "escape_graph"
    _, _, live = _run_a(name)
    path = tmp_path / "run.ckpt"
    checkpoint.save(path, **H.saved(live))
    before = H.final(name, live)
    dev = torch.device("cuda", 0)
    other = LR.PPOLearner.trainable_init(dev, mode="escape", seed=5, optimizer="fused", step="graph", shuffle_sequences=True, grad_clip=0.5, num_sgd_iter=3,
                                         sgd_minibatch_size=64)
    with pytest.raises(ValueError, match="`num_sgd_iter` was 2 when saved, the live object has 3"):
        other.load_state_dict(live["learner"].state_dict())
    torch_mode = LR.PPOLearner.trainable_init(dev, mode="escape", seed=5, optimizer="torch", **H.LEARN)
    with pytest.raises(ValueError, match="`shuffle_sequences`|`grad_clip`|`step`|`optimizer`"):
        torch_mode.load_state_dict(live["learner"].state_dict())
    sd = live["learner"].state_dict()
    sd["policies"][1]["adam"]["m"][0] = sd["policies"][1]["adam"]["m"][0].double()
    with pytest.raises(ValueError, match=r"`m\[0\]` was saved as torch.float64"):
        live["learner"].load_state_dict(sd)
    ro_sd = live["rollout"].state_dict()
    longer = PPORollout(live["world"], live["bank"], H.T + 1)
    with pytest.raises(ValueError, match="`T` was 8 when saved, the live object has 9"):
        longer.load_state_dict(ro_sd)
    ro_sd["window"]["obs"] = ro_sd["window"]["obs"][:-1]
    with pytest.raises(ValueError, match="`obs` was saved with shape"):
        live["rollout"].load_state_dict(ro_sd)
    # a file whose rollout does not fit is refused as a whole: the world, the bank and the learner in front of it stay as they are
    doc = torch.load(path, weights_only=True)
    doc["state"]["rollout"]["window"]["done"] = doc["state"]["rollout"]["window"]["done"].to(torch.int32)
    torch.save(doc, path)
    H.iterate(name, live, 1)
    moved = H.final(name, live)
    assert H.same(moved, before) is not None
    with pytest.raises(ValueError, match="`done` was saved as torch.int32"):
        checkpoint.load(path, **H.saved(live))
    _assert_same(H.final(name, live), moved, "nothing was loaded")
    shared = [m.shared_layer for m in live["learner"].modules]
    assert shared[0] is shared[1], "the shared layer is still one module"


def test_tied_shared_layer_is_saved_once_and_stays_tied():
    name = "fight_torch"
    _, _, live = _run_a(name)
    sd = live["learner"].state_dict()
    keys = [set(m) for m in sd["modules"]]
    assert "shared_layer._model.0.weight" in keys[0] and not any(k.startswith("shared_layer") for k in keys[1])
    fresh = H.build(name)["learner"]
    fresh.load_state_dict(sd)
    a, b = (m.shared_layer._model[0].weight for m in fresh.modules)
    assert a is b and torch.equal(a.cpu(), sd["modules"][0]["shared_layer._model.0.weight"])
    assert fresh.updates == live["learner"].updates and fresh.kl_coeff == live["learner"].kl_coeff
    _assert_same(fresh.state_dict(), sd, "learner")
