"""The exported policy files of the curriculum, `policies/L{level}_AC{i}_{mode}.pt` (train_hetero.py:101-105, policy_export.py), in a
plain format of this project's own, and the commander's file in the same form.

The reference writes each policy as a pickled RLlib model object; reading one back needs ray and the reference's models/ importable.
A file written here is `torch.save` of a plain dict of float32 CPU tensors and scalars — `torch.load(..., weights_only=True)` reads
it, no class of either project is unpickled:

    {"format": "hhmarl_2d_amd.policy", "version": 1, "kind": int, "level": int | None, "agent_mode": str | None,
     "state": {key: float32 CPU tensor}}

`state` holds every key of policy_nets.actor_keys(kind) and policy_nets.critic_keys(kind) — what the reference's model.pt holds: the
actor for flying the policy as a frozen pilot or opponent, the value branch so that a learner can be started from the file
(PPOLearner.from_policy_files).  The commander's file ("format": "hhmarl_2d_amd.commander") holds commander.state_keys().

Everywhere a policy file is read by name (PolicyBank.from_reference_dir: LowLevelEnv levels 4-5, HighLevelEnv, the vector envs, the
evaluators) both kinds of file are taken, also mixed in one directory: `load_policy_file` tries the plain format first and falls back
to unpickling a reference module only when the restricted loader refuses the file; `from_policy_object` turns either into the
(kind, actor tensors) a PolicyBank slot takes."""
import os
import pickle
import tempfile

import numpy as np
import torch

from . import policy_nets as PN

FORMAT = "hhmarl_2d_amd.policy"
COMMANDER_FORMAT = "hhmarl_2d_amd.commander"
FORMAT_VERSION = 1
AGENT_MODES = ("fight", "escape")
MODE_KINDS = {"fight": (PN.FIGHT1, PN.FIGHT2), "escape": (PN.ESC1, PN.ESC2)}


def policy_file_name(level, ac, agent_mode):
    """train_hetero.py:104: L{level}_AC{ac}_{agent_mode}.pt; level 1..5, ac 1 | 2, agent_mode "fight" | "escape", else ValueError"""
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 1 <= int(level) <= 5:
        raise ValueError(f"policy_file_name: level is 1..5, got {level!r}")
    if isinstance(ac, bool) or not isinstance(ac, (int, np.integer)) or int(ac) not in (1, 2):
        raise ValueError(f"policy_file_name: ac is 1 or 2 (the aircraft type), got {ac!r}")
    if agent_mode not in AGENT_MODES:
        raise ValueError(f"policy_file_name: agent_mode is one of {AGENT_MODES}, got {agent_mode!r}")
    return f"L{int(level)}_AC{int(ac)}_{agent_mode}.pt"


def mode_of_kinds(kinds):
    """the agent_mode a pair of kinds (ac1_policy, ac2_policy) trains: "fight" | "escape", else ValueError"""
    kinds = tuple(int(k) for k in kinds)
    for mode, want in MODE_KINDS.items():
        if kinds == want:
            return mode
    raise ValueError(f"kinds {kinds} are neither the fight pair {MODE_KINDS['fight']} nor the escape pair {MODE_KINDS['escape']}")


def policy_keys(kind):
    """every key of a policy file's state -> shape: the actor's and the value branch's"""
    if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or int(kind) not in PN.KIND_NAMES:
        raise ValueError(f"kind is one of {sorted(PN.KIND_NAMES)} (policy_nets.FIGHT1 .. ESC2), got {kind!r}")
    return dict(PN.actor_keys(int(kind)), **PN.critic_keys(int(kind)))


def _checked_state(who, keys, state, finite=True):
    """`state` (key -> numpy array or tensor, any device) as a file holds it: exactly the keys of `keys` (-> shape), each a detached
    contiguous float32 CPU tensor of that shape, finite; or ValueError naming the key"""
    if not isinstance(state, dict):
        raise ValueError(f"{who}: the state is a dict of tensors, got {type(state).__name__}")
    for k in keys:
        if k not in state:
            raise ValueError(f"{who}: the state has no `{k}`")
    for k in state:
        if k not in keys:
            raise ValueError(f"{who}: the state has an unexpected `{k}`")
    out = {}
    for k, shp in keys.items():
        v = state[k]
        if isinstance(v, torch.Tensor):
            t = v.detach().to("cpu", copy=True)
        else:
            try:
                t = torch.from_numpy(np.array(v, copy=True))
            except (TypeError, ValueError) as e:
                raise ValueError(f"{who}: `{k}` is not a tensor or an array ({type(v).__name__})") from e
        if not t.is_floating_point():
            raise ValueError(f"{who}: `{k}` is {t.dtype}, not a floating-point tensor")
        if tuple(t.shape) != tuple(shp):
            raise ValueError(f"{who}: `{k}` has shape {tuple(t.shape)}, the network has {tuple(shp)}")
        t = t.to(torch.float32).contiguous()
        if finite and not bool(torch.isfinite(t).all()):
            raise ValueError(f"{who}: `{k}` holds a non-finite value")
        out[k] = t
    return out


def _write(path, doc):
    """torch.save(doc) at `path`, atomically, as checkpoint.save does it: a temporary name in the same directory, flush, fsync,
    os.replace — a write that fails leaves the previous file as it was -> the path"""
    path = os.fspath(path)
    folder = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=folder)
    try:
        with os.fdopen(fd, "wb") as f:
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
    return path


def _read(who, path, fmt):
    """the document at `path` through the restricted loader, its format and version checked"""
    doc = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    if not isinstance(doc, dict) or doc.get("format") != fmt:
        raise ValueError(f"{who}: {path} is not a {fmt} file")
    if doc.get("version") != FORMAT_VERSION:
        raise ValueError(f"{who}: {path} has format version {doc.get('version')!r}, this library reads {FORMAT_VERSION}")
    return doc


def save_policy(path, kind, state, level=None, agent_mode=None):
    """One policy file: `state` holds every key of actor_keys(kind) and critic_keys(kind) (numpy arrays or tensors; a module's
    state_dict() as it is).  ValueError — before anything is written, so the previous file stays as it was — for an unknown kind, a
    missing or unexpected key, a wrong shape, a non-finite value, a level outside 1..5 or an agent_mode that is not the kind's.
    level / agent_mode are recorded for the reader (the file name carries them too); None leaves them open.  -> the path"""
    keys = policy_keys(kind)
    kind = int(kind)
    if level is not None:
        policy_file_name(level, 1, "fight")
        level = int(level)
    if agent_mode is not None:
        if agent_mode not in AGENT_MODES:
            raise ValueError(f"save_policy: agent_mode is one of {AGENT_MODES}, got {agent_mode!r}")
        if kind not in MODE_KINDS[agent_mode]:
            raise ValueError(f"save_policy: a {PN.KIND_NAMES[kind]} network is no {agent_mode} policy")
    st = _checked_state(f"save_policy({PN.KIND_NAMES[kind]})", keys, state)
    return _write(path, {"format": FORMAT, "version": FORMAT_VERSION, "kind": kind, "level": level, "agent_mode": agent_mode, "state": st})


def _document_state(who, doc):
    """a policy document's (kind, validated state)"""
    try:
        keys = policy_keys(doc.get("kind"))
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None
    kind = int(doc["kind"])
    return kind, _checked_state(f"{who} ({PN.KIND_NAMES[kind]})", keys, doc.get("state"))


def load_policy(path):
    """-> (kind, state: {key: float32 CPU tensor}) of a file save_policy wrote, read with torch.load(weights_only=True).  ValueError for
    another format or version, a missing or unexpected key, a wrong shape or a non-finite value; FileNotFoundError for a missing file"""
    return _document_state("load_policy", _read("load_policy", path, FORMAT))


def is_policy_document(obj):
    return isinstance(obj, dict) and obj.get("format") == FORMAT


def load_policy_file(path):
    """What PolicyBank.from_reference_dir loads a file with when no loader is given: the plain format through the restricted loader;
    a file that loader refuses to unpickle — the reference's own export, a pickled module — through torch.load(weights_only=False), which
    needs the reference's model classes importable.  -> a document or a module, for from_policy_object"""
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        return torch.load(path, weights_only=False)


def from_policy_object(obj):
    """a loaded policy file -> (kind, the actor tensors as numpy float32, keyed by actor_keys(kind)): a document of the plain format
    (validated as load_policy does), or a loaded reference module (policy_nets.from_torch_module)"""
    if isinstance(obj, dict):
        if obj.get("format") != FORMAT:
            raise ValueError(f"from_policy_object: a dict that is not a {FORMAT} document")
        if obj.get("version") != FORMAT_VERSION:
            raise ValueError(f"from_policy_object: format version {obj.get('version')!r}, this library reads {FORMAT_VERSION}")
        kind, st = _document_state("from_policy_object", obj)
        return kind, {k: st[k].numpy() for k in PN.actor_keys(kind)}
    return PN.from_torch_module(obj)


# ------------------------------------------------------------------------------------------------------------------ the commander
def save_commander(path, state):
    """The commander's file: `state` holds every key of commander.state_keys() (CommanderGru's state_dict(), numpy or torch); the
    checks and the atomic write of save_policy.  -> the path"""
    from .commander import state_keys
    st = _checked_state("save_commander", dict(state_keys()), dict(state))
    return _write(path, {"format": COMMANDER_FORMAT, "version": FORMAT_VERSION, "state": st})


def load_commander(path):
    """-> {key: float32 CPU tensor} of a file save_commander wrote (torch.load(weights_only=True)); ValueError / FileNotFoundError as
    load_policy raises them"""
    from .commander import state_keys
    doc = _read("load_commander", path, COMMANDER_FORMAT)
    return _checked_state("load_commander", dict(state_keys()), doc.get("state"))
