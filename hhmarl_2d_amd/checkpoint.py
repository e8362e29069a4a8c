"""Save and resume a training run bit for bit: `save(path, **objects)` / `load(path, **objects)` over the `state_dict()` /
`load_state_dict()` of every object of the loop (World, PolicyBank, CommanderNet, the rollouts with their episode batches, the learners
with their Adam state), and the helpers those methods share.

The reference's trainers save every 50 iterations and restore on request (train_hetero.py:98-107 `algo.save()`, 253-257
`algo.restore(...)`).  RLlib's own checkpoint format is not reproduced: a checkpoint here is ONE file, `torch.save` of a plain dict of
CPU tensors and scalars (no pickled project classes: `torch.load(..., weights_only=True)` reads it), whose header carries a format
version and the objects' names and types.  One file per process: a multi-rank run saves one file per rank under names of its own.

Why a resume is exact: every random draw of the loop is keyed by counters that are part of the saved state — the sampler's by the world's
(seed, arena, episode, step) (include/hh_policy.h: hh_policy_sample), the learners' minibatch and sequence orders by (seed, update count,
policy, pass) — and everything else is copied back byte for byte.  Loads copy IN PLACE (`copy_` into the existing tensors, the native
restores into the existing device arrays), so every address a captured HIP graph holds stays valid: an object that has already captured
its collect or step graph can be loaded into and replayed; the graphs themselves are never saved.

A `load_state_dict` validates everything (names, shapes, dtypes, the recorded options against the live object's) before it changes
anything and raises ValueError naming the field.  Objects split that into `_load_plan(sd) -> commit`, so that `load` can validate every
object of a file before the first one is touched."""
import os
import tempfile

import torch

FORMAT = "hhmarl_2d_amd.checkpoint"
FORMAT_VERSION = 1


# ------------------------------------------------------------------------------------------------------------------ shared helpers
def cpu(t):
    """a tensor as a checkpoint holds it: a detached, contiguous CPU copy (synchronises with the device that owns it)"""
    return t.detach().to("cpu", copy=True).contiguous()


def need_keys(who, sd, keys):
    """sd is a dict with exactly these keys, or ValueError naming the first one missing / unexpected"""
    if not isinstance(sd, dict):
        raise ValueError(f"{who}: a state dict is a dict, got {type(sd).__name__}")
    for k in keys:
        if k not in sd:
            raise ValueError(f"{who}: the state dict has no `{k}`")
    for k in sd:
        if k not in keys:
            raise ValueError(f"{who}: the state dict has an unexpected `{k}`")


def check_options(who, saved, live):
    """the recorded options against the live object's (two flat dicts of scalars / tuples / None), or ValueError naming the field"""
    need_keys(f"{who} options", saved, tuple(live))
    for k, v in live.items():
        s = saved[k]
        s = tuple(s) if isinstance(s, (list, tuple)) else s
        v = tuple(v) if isinstance(v, (list, tuple)) else v
        if s != v or isinstance(s, bool) != isinstance(v, bool):
            raise ValueError(f"{who}: `{k}` was {s!r} when saved, the live object has {v!r}")


def check_tensor(who, name, src, dst, lead=None):
    """src (from the file) can be copied into dst: a tensor of dst's dtype and shape — with `lead`, of dst's trailing shape and `lead`
    leading entries (a cut buffer), at most dst's — or ValueError naming the field"""
    if not isinstance(src, torch.Tensor):
        raise ValueError(f"{who}: `{name}` is not a tensor")
    if src.dtype != dst.dtype:
        raise ValueError(f"{who}: `{name}` was saved as {src.dtype}, the live tensor is {dst.dtype}")
    want = tuple(dst.shape) if lead is None else (int(lead),) + tuple(dst.shape[1:])
    if tuple(src.shape) != want or (lead is not None and int(lead) > dst.shape[0]):
        raise ValueError(f"{who}: `{name}` was saved with shape {tuple(src.shape)}, the live object takes {want}"
                         + ("" if lead is None else f" of at most {dst.shape[0]} entries"))


def plan_tensors(who, saved, live):
    """every tensor of `live` (name -> tensor) from `saved`, whole: validated now -> the list of (dst, src) pairs to copy"""
    need_keys(who, saved, tuple(live))
    for k, dst in live.items():
        check_tensor(who, k, saved[k], dst)
    return [(dst, saved[k]) for k, dst in live.items()]


def copy_pairs(pairs):
    """the in-place copies of a validated plan (dst keeps its address)"""
    with torch.no_grad():
        for dst, src in pairs:
            dst.copy_(src)


def check_blob(who, blob, n_bytes, magic):
    """a native snapshot as the state dicts hold it: a 1-D uint8 CPU tensor of the live object's snapshot size, magic and format version;
    the native restore checks the rest of the header (before it writes anything)"""
    if not isinstance(blob, torch.Tensor) or blob.dtype != torch.uint8 or blob.dim() != 1 or blob.device.type != "cpu":
        raise ValueError(f"{who}: `blob` is a 1-D uint8 CPU tensor")
    if blob.numel() != int(n_bytes):
        raise ValueError(f"{who}: `blob` holds {blob.numel()} bytes, a snapshot of the live object {int(n_bytes)} (another geometry, or a truncated blob)")
    head = bytes(blob[:8].tolist())
    if head[:4] != magic:
        raise ValueError(f"{who}: `blob` is not a snapshot of this kind of object (magic {head[:4]!r}, expected {magic!r})")
    if int.from_bytes(head[4:8], "little") != SNAPSHOT_VERSION:
        raise ValueError(f"{who}: `blob` has snapshot format version {int.from_bytes(head[4:8], 'little')}, this library reads {SNAPSHOT_VERSION}")


SNAPSHOT_VERSION = 1          # HH_SNAP_VERSION (csrc/hh_snapshot.h)


def load_plan(obj, sd):
    """obj's validated load as a callable: its `_load_plan(sd)` where it has one (validation now, the change when called), else its
    `load_state_dict` deferred as it is"""
    plan = getattr(obj, "_load_plan", None)
    if plan is not None:
        return plan(sd)
    return lambda: obj.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------------------------ the file
def _type_name(obj):
    return type(obj).__name__


def _check_objects(who, objects):
    if not objects:
        raise ValueError(f"{who}: no objects given (pass them by keyword: world=w, bank=b, ...)")
    for name, obj in objects.items():
        if not (callable(getattr(obj, "state_dict", None)) and callable(getattr(obj, "load_state_dict", None))):
            raise ValueError(f"{who}: `{name}` ({_type_name(obj)}) has no state_dict() / load_state_dict()")


def save(path, **objects):
    """One checkpoint file of the objects given by keyword: {format, version, objects: {name: type name}, state: {name: state_dict()}}
    through torch.save.  Atomic: written to a temporary name in the same directory, flushed to disk, then os.replace — a save that raises
    midway (a state_dict that fails, a full disk) leaves the previous file as it was.  -> the file's size in bytes"""
    _check_objects("checkpoint.save", objects)
    path = os.fspath(path)
    folder = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=folder)
    try:
        with os.fdopen(fd, "wb") as f:
            doc = {"format": FORMAT, "version": FORMAT_VERSION, "objects": {k: _type_name(v) for k, v in objects.items()},
                   "state": {k: v.state_dict() for k, v in objects.items()}}
            torch.save(doc, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return os.path.getsize(path)


def _read(who, path):
    """the document at `path`: format, version and object table checked -> (doc, {name: type name})"""
    doc = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    if not isinstance(doc, dict) or doc.get("format") != FORMAT:
        raise ValueError(f"{who}: {path} is not a {FORMAT} file")
    if doc.get("version") != FORMAT_VERSION:
        raise ValueError(f"{who}: {path} has format version {doc.get('version')!r}, this library reads {FORMAT_VERSION}")
    saved = doc.get("objects")
    if not isinstance(saved, dict) or not isinstance(doc.get("state"), dict) or set(doc["state"]) != set(saved):
        raise ValueError(f"{who}: {path} has no consistent object table")
    return doc, saved


def _load(who, path, objects, whole):
    """load (whole: the names given are the file's) and load_subset (they are among the file's)"""
    _check_objects(who, objects)
    doc, saved = _read(who, path)
    if whole and set(saved) != set(objects):
        raise ValueError(f"{who}: the file holds {sorted(saved)}, the objects given are {sorted(objects)}")
    absent = sorted(set(objects) - set(saved))
    if absent:
        raise ValueError(f"{who}: the file holds {sorted(saved)}, not {absent}")
    for name, obj in objects.items():
        if saved[name] != _type_name(obj):
            raise ValueError(f"{who}: `{name}` was saved as a {saved[name]}, the object given is a {_type_name(obj)}")
    plans = [load_plan(obj, doc["state"][name]) for name, obj in objects.items()]
    for commit in plans:
        commit()


def load(path, **objects):
    """The checkpoint at `path` into the objects given by keyword (built from the constructor arguments of the saved run).  Refused with
    ValueError, before any object is touched: another format or version, names that are not exactly the file's, an object of another
    type than was saved under its name, and whatever an object's own validation refuses (`_load_plan`).  Then every object is loaded in
    place, in the order given."""
    _load("checkpoint.load", path, objects, True)


def load_subset(path, **objects):
    """`load` with one rule relaxed: the names given must all be IN the file, they need not be all of it.  What a resume must not do — a
    run continued with half of its state is no longer the run that was saved, which is why `load` refuses it — is what the curriculum
    does at every level change (the reference's `restore` of the previous level's checkpoint, config.py:65-80, train_hetero.py:253-257):
    the learner goes on, with its weights, Adam state, KL coefficients and update count, in a world of the next level that no saved
    world, bank or rollout fits:

        checkpoint.load_subset(prev, learner=learner);  learner.publish(bank);  ro.start()

    Everything else is `load`'s: format and version, the type per name, every object's own validation before the first is touched,
    copies in place.  The objects of the file that are not named are not read."""
    _load("checkpoint.load_subset", path, objects, False)


def contents(path):
    """{name: type name} of the objects a checkpoint file holds (the file is read whole; format and version checked as `load` does)"""
    return dict(_read("checkpoint.contents", path)[1])
