"""The frozen low-level pilot / opponent policies the reference runs inside its environments
(envs/env_base.py:312-398): `PolicyBank` evaluates the reference's own architectures (Fight1/Fight2/Esc1/Esc2 actors,
models/ac_models_hetero.py) in the fused HIP kernel of csrc/hh_policy_kernel.h (C ABI include/hh_policy.h) and writes
int8 actions for every unit of every arena in one launch sequence; `NetPilot` / `OpponentNets` plug it into
HighLevelEnv / LowLevelEnv levels 4-5.  The reference torch.load()s `policies/L*_AC*_{fight,escape}.pt`, which are not
shipped (.gitignore:5): a deployment loads its own files with `PolicyBank.from_modules`, or by name with
`PolicyBank.from_reference_dir` (the reference's pickled modules, or the plain files PPOLearner.export_policies writes:
hhmarl_2d_amd/policy_files.py); benchmarks and tests use
deterministic synthetic weights of the same shapes (`PolicyBank.random_init`).

A pilot is `callable(pilot_obs f32 [N,A,30], pilot_mode u8 [N,A]) -> int8 actions [N,A,4]`
(MultiDiscrete([13,9,2,2]); rows with mode 0 are ignored; pilot_mode = policy type | aircraft type << 2).  Greedy
arg-max per action component is what the reference does (env_base.py:373-382).  The uniform / tape / MLP pilots below
are stand-ins for env-only measurements."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import policy_nets as PN

# selector byte the world kernels emit as pilot_mode: (1 fight | 2 escape) | (aircraft type << 2)
SEL_FIGHT1, SEL_ESC1, SEL_FIGHT2, SEL_ESC2 = 5, 6, 9, 10
SEL_OPP_SIDE = 64   # HH_SEL_OPP_SIDE: an opponent's fight row of a world created with opp_side_selector (eval_hl = False)


def tie_shared_layer(sds):
    """make every state dict of `sds` carry the FIRST one's shared_layer tensors (models/ac_models_hetero.py:21: one module-level
    SHARED_LAYER serves Fight1, Fight2, Esc1 and Esc2, so every policy of a trainer holds the same 500 x 500 layer)"""
    for sd in sds[1:]:
        for k in ("shared_layer._model.0.weight", "shared_layer._model.0.bias"):
            sd[k] = sds[0][k]
    return sds


def _net_struct(kind, p):
    """hh_net_weights of `kind`; p(state_dict key) -> pointer (None for the keys the kind does not have)"""
    w = L.HHNetWeights()
    w.kind = kind
    for i in range(3):
        w.inp_w[i] = p(f"inp{i + 1}._model.0.weight")
        w.inp_b[i] = p(f"inp{i + 1}._model.0.bias")
    w.att_in_proj_w, w.att_in_proj_b = p("att_act.in_proj_weight"), p("att_act.in_proj_bias")
    w.att_out_w, w.att_out_b = p("att_act.out_proj.weight"), p("att_act.out_proj.bias")
    w.shared_w, w.shared_b = p("shared_layer._model.0.weight"), p("shared_layer._model.0.bias")
    w.out_w, w.out_b = p("act_out._model.0.weight"), p("act_out._model.0.bias")
    return w


def _critic_struct(kind, p):
    """hh_critic_weights of `kind`; p(key) -> pointer, the shared layer under the actor's keys"""
    w = L.HHCriticWeights()
    w.kind = kind
    names = ("v1", "v2", "v3") if PN.HAS_ATT[kind] else ("inp1_val",)
    for i, n in enumerate(names):
        w.v_w[i] = p(f"{n}._model.0.weight")
        w.v_b[i] = p(f"{n}._model.0.bias")
    w.att_in_proj_w, w.att_in_proj_b = p("att_val.in_proj_weight"), p("att_val.in_proj_bias")
    w.att_out_w, w.att_out_b = p("att_val.out_proj.weight"), p("att_val.out_proj.bias")
    w.shared_w, w.shared_b = p("shared_layer._model.0.weight"), p("shared_layer._model.0.bias")
    w.val_w, w.val_b = p("val_out._model.0.weight"), p("val_out._model.0.bias")
    return w


class PolicyBank:
    """Up to 8 frozen actor networks resident on one GPU (hh_policy_* of include/hh_policy.h)."""
    FIGHT1, FIGHT2, ESC1, ESC2 = PN.FIGHT1, PN.FIGHT2, PN.ESC1, PN.ESC2

    def __init__(self, device, max_rows):
        if not torch.cuda.is_available():
            raise RuntimeError("hhmarl_2d_amd.PolicyBank needs a ROCm GPU (no CPU fallback)")
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.max_rows = int(max_rows)
        self.h = C.c_void_p()
        L.check(L.lib().hh_policy_create(self.device.index or 0, self.max_rows, C.byref(self.h)))
        self.kinds = {}
        self._critics = set()   # slots whose value branch is loaded (set_critic since the last set_net)
        self._lut = np.zeros(256, dtype=np.uint8)
        self.generation = 0   # bumped by every call that (re)allocates or rewrites what a captured HIP graph holds by value: weight blobs, the selector table

    def close(self):
        if getattr(self, "h", None):
            L.lib().hh_policy_destroy(self.h)
            self.h = None
            self.generation += 1

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_net(self, slot, kind, sd):
        """sd: the actor tensors keyed like the reference's state_dict() (policy_nets.actor_keys), numpy float32"""
        a = {k: np.ascontiguousarray(sd[k], dtype=np.float32) for k in PN.actor_keys(kind)}
        for k, shp in PN.actor_keys(kind).items():
            assert a[k].shape == shp, (k, a[k].shape, shp)
        w = _net_struct(kind, lambda k: a[k].ctypes.data_as(C.c_void_p) if k in a else None)
        L.check(L.lib().hh_policy_set_net(self.h, int(slot), C.byref(w)))
        self.kinds[int(slot)] = kind
        self._critics.discard(int(slot))   # hh_policy_set_net invalidates the slot's value branch
        self.generation += 1

    def set_critic(self, slot, kind, sd, csd):
        """the value branch of the network in `slot` (hh_policy_set_critic): sd = its actor tensors (for the shared layer), csd = the value
        branch keyed like the reference's state_dict() (policy_nets.critic_keys)"""
        a = {k: np.ascontiguousarray(csd[k], dtype=np.float32) for k in PN.critic_keys(kind)}
        for k, shp in PN.critic_keys(kind).items():
            assert a[k].shape == shp, (k, a[k].shape, shp)
        for k in ("shared_layer._model.0.weight", "shared_layer._model.0.bias"):
            a[k] = np.ascontiguousarray(sd[k], dtype=np.float32)
        w = _critic_struct(kind, lambda k: a[k].ctypes.data_as(C.c_void_p) if k in a else None)
        L.check(L.lib().hh_policy_set_critic(self.h, int(slot), C.byref(w)))
        self._critics.add(int(slot))
        self.generation += 1

    def sample(self, obs, sel, world=None, uniforms=None, crit_act=None, greedy=False, actions=None, logp=None, vf=None, logits=None,
               want_vf=True):
        """one sampler step of the trainable policies (hh_policy_sample): obs f32 [N, 2, D] rows of LowLevelEnv agents -> (actions int8
        [N, 2, 4], logp f32 [N, 2], vf f32 [N, 2] or None).  world: keyed draws from its episode / step counters; uniforms f64 [N, 2, 4]
        overrides them; crit_act f32 [N, 2, 4] = the critic's scaled action inputs (None = zeros, as while sampling)."""
        assert obs.dtype == torch.float32 and obs.is_contiguous()
        stride = obs.shape[-1]
        n_rows = obs.numel() // stride
        lead = tuple(obs.shape[:-1])
        if sel is not None:
            assert sel.dtype == torch.uint8 and sel.is_contiguous() and sel.numel() == n_rows
        if actions is None:
            actions = torch.empty(lead + (4,), dtype=torch.int8, device=obs.device)
        if logp is None:
            logp = torch.empty(lead, dtype=torch.float32, device=obs.device)
        if vf is None and want_vf:
            vf = torch.empty(lead, dtype=torch.float32, device=obs.device)
        assert actions.dtype == torch.int8 and actions.is_contiguous() and actions.numel() == n_rows * 4
        assert logp.dtype == torch.float32 and logp.numel() == n_rows and (vf is None or (vf.dtype == torch.float32 and vf.numel() == n_rows))
        if uniforms is not None:
            assert uniforms.dtype == torch.float64 and uniforms.is_contiguous() and uniforms.numel() == n_rows * 4
        if crit_act is not None:
            assert crit_act.dtype == torch.float32 and crit_act.is_contiguous() and crit_act.numel() == n_rows * 4
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        L.check(L.lib().hh_policy_sample(self.h, ptr(obs), n_rows, stride, ptr(sel), None if world is None else world.h, ptr(uniforms), ptr(crit_act),
                                         1 if greedy else 0, ptr(actions), ptr(logp), ptr(vf), ptr(logits), st))
        return actions, logp, vf

    @classmethod
    def trainable_init(cls, device, mode="fight", seed=0, max_rows=1 << 20, tie_shared=True):
        """the two trainable policies of train_hetero.py (ac1_policy = Fight1 | Esc1 in slot 0, ac2_policy = Fight2 | Esc2 in slot 1) with
        synthetic actor AND value-branch weights; selector bytes as the agents' aircraft types: SEL_FIGHT1 / SEL_FIGHT2 (| SEL_ESC*).
        tie_shared (default): both slots carry ONE shared_layer tensor — in the reference `SHARED_LAYER` is one module-level SlimFC used by
        Fight1, Fight2, Esc1 and Esc2 (models/ac_models_hetero.py:21), so ac1_policy and ac2_policy train the same 500 x 500 layer.
        tie_shared = False draws one per slot (what the committed policy_value.npz vectors were recorded with)."""
        b = cls(device, max_rows)
        kinds = (PN.FIGHT1, PN.FIGHT2) if mode == "fight" else (PN.ESC1, PN.ESC2)
        sds = [PN.random_weights(kind, seed) for kind in kinds]
        if tie_shared:
            tie_shared_layer(sds)
        for slot, (kind, sd) in enumerate(zip(kinds, sds)):
            b.set_net(slot, kind, sd)
            b.set_critic(slot, kind, sd, PN.random_critic_weights(kind, seed))
        b.set_lut({(SEL_FIGHT1 if mode == "fight" else SEL_ESC1): 0, (SEL_FIGHT2 if mode == "fight" else SEL_ESC2): 1})
        return b

    def load_trainable(self, slot, kind, sd, csd):
        """one policy of a PPO iteration into `slot`: actor and value branch TOGETHER (hh_policy_set_net invalidates the slot's value branch,
        whose private copy of the shared layer would otherwise go stale).  When syncing weights back from a learner, pass the same
        shared_layer tensors for every slot (tie_shared_layer): the reference has one SHARED_LAYER for all four architectures."""
        self.set_net(slot, kind, sd)
        self.set_critic(slot, kind, sd, csd)

    def refresh(self, slot, sd, csd=None):
        """The learner's new weights for a LOADED slot, from float32 CUDA tensors keyed like the reference's state_dict()
        (policy_nets.actor_keys; csd: critic_keys, required exactly when the slot's value branch is loaded, its shared layer taken from
        sd): repacked on the device into the same bytes set_net + set_critic write, in place, ordered on the current torch stream
        (hh_policy_refresh).  No host synchronisation; capturable into a CUDA graph.  The device addresses stay, so `generation` is not
        bumped and graphs captured before keep replaying, with the new weights.  A sampler on another stream must wait for an event
        recorded after this call; the tensors must stay unchanged until the stream has run it.  Tied shared layers
        (tie_shared_layer): pass the same tensor to both slots."""
        slot = int(slot)
        if slot not in self.kinds:
            raise ValueError(f"PolicyBank.refresh: slot {slot} is empty (load it once with set_net / load_trainable)")
        kind = self.kinds[slot]
        a = PN.device_weights(PN.actor_keys(kind), sd, self.device, "PolicyBank.refresh actor")
        w = _net_struct(kind, lambda k: a[k].data_ptr() if k in a else None)
        cw = None
        if csd is not None:
            c = PN.device_weights(PN.critic_keys(kind), csd, self.device, "PolicyBank.refresh critic")
            c.update({k: a[k] for k in ("shared_layer._model.0.weight", "shared_layer._model.0.bias")})
            cw = _critic_struct(kind, lambda k: c[k].data_ptr() if k in c else None)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(L.lib().hh_policy_refresh(self.h, slot, C.byref(w), None if cw is None else C.byref(cw), st))

    def refresh_trainable(self, modules_or_dicts):
        """refresh() for the slots of trainable_init (0: ac1_policy, 1: ac2_policy) from the learner's modules or their state dicts (actor
        and value-branch keys in one dict, as the reference's state_dict() holds them); the value branch goes along wherever it is loaded"""
        for slot, m in enumerate(modules_or_dicts):
            sd = m.state_dict() if hasattr(m, "state_dict") else m
            self.refresh(slot, sd, sd if slot in self._critics else None)

    def packed(self, slot, part):
        """test hook: one packed part of a slot as the forward kernels read it (hh_policy_copy_packed; 0 fp32 blob, 1 fp16 planes, 2 fragment
        stream, 3 value-branch planes + biases, 4 value-branch stream) -> uint8 CUDA tensor, copied on the current stream"""
        n = C.c_int64()
        L.check(L.lib().hh_policy_copy_packed(self.h, int(slot), int(part), None, 0, C.byref(n), None))
        out = torch.empty((n.value,), dtype=torch.uint8, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(L.lib().hh_policy_copy_packed(self.h, int(slot), int(part), C.c_void_p(out.data_ptr()), n.value, C.byref(n), st))
        return out

    # ---- complete snapshots (checkpointing: hh_policy_snapshot / hh_policy_restore, include/hh_policy.h) ----
    def snapshot(self):
        """the packed weights of every loaded slot exactly as the kernels read them, the selector table and the row lists, as an opaque
        blob (uint8 CPU tensor); synchronises the current stream"""
        return L.snapshot("policy", self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def restore(self, blob):
        """a snapshot() blob back into the device arrays in place (addresses, kinds and loaded flags stay: `generation` is not bumped and
        captured graphs replay with the restored weights).  ValueError, the bank untouched: another max_rows or slot layout, another
        format version, a truncated blob."""
        if not isinstance(blob, torch.Tensor) or blob.dtype != torch.uint8 or blob.dim() != 1 or blob.device.type != "cpu":
            raise ValueError("blob: a 1-D uint8 CPU tensor (PolicyBank.snapshot())")
        L.restore("policy", self.h, blob.contiguous(), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def _layout(self):
        return {"max_rows": self.max_rows, "slots": tuple(sorted(self.kinds)), "kinds": tuple(self.kinds[k] for k in sorted(self.kinds)),
                "critics": tuple(sorted(self._critics))}

    def state_dict(self):
        """the blob, the slot layout it was taken with and the host copy of the selector table"""
        return {"blob": self.snapshot(), "options": self._layout(), "lut": torch.from_numpy(self._lut.copy())}

    def _load_plan(self, sd):
        from . import checkpoint as ck
        ck.need_keys("PolicyBank", sd, ("blob", "options", "lut"))
        ck.check_options("PolicyBank", sd["options"], self._layout())
        ck.check_tensor("PolicyBank", "lut", sd["lut"], torch.from_numpy(self._lut))
        ck.check_blob("PolicyBank", sd["blob"], L.snapshot_bytes("policy", self.h), L.SNAPSHOT_MAGIC["policy"])

        def commit():
            self.restore(sd["blob"])
            self._lut = sd["lut"].numpy().copy()
        return commit

    def load_state_dict(self, sd):
        self._load_plan(sd)()

    def kernel_name(self, n_rows, sampler=False):
        """the forward kernel instance a call of n_rows rows launches (hh_policy_kernel_name)"""
        buf = C.create_string_buffer(64)
        L.check(L.lib().hh_policy_kernel_name(self.h, int(n_rows), 1 if sampler else 0, buf, 64))
        return buf.value.decode()

    def set_tile_rows(self, rows):
        """rows per workgroup tile of the forward kernel: 0 = by row count (default), 32 or 64 (hh_policy_set_tile_rows)"""
        L.check(L.lib().hh_policy_set_tile_rows(self.h, int(rows)))
        self.generation += 1   # another kernel instance: a captured graph would keep launching the old one

    def set_lut(self, mapping):
        """mapping: selector byte -> network slot (everything else: no action)"""
        lut = np.zeros(256, dtype=np.uint8)
        for sel, slot in mapping.items():
            lut[int(sel)] = int(slot) + 1
        L.check(L.lib().hh_policy_set_lut(self.h, lut.ctypes.data_as(C.c_void_p)))
        self._lut = lut
        self.generation += 1

    @classmethod
    def random_init(cls, device, seed=0, max_rows=1 << 20):
        """one synthetic network per architecture in slots FIGHT1..ESC2, selected by the world's pilot_mode bytes"""
        b = cls(device, max_rows)
        for kind in (PN.FIGHT1, PN.FIGHT2, PN.ESC1, PN.ESC2):
            b.set_net(kind, kind, PN.random_weights(kind, seed))
        lut = {SEL_FIGHT1: PN.FIGHT1, SEL_FIGHT2: PN.FIGHT2, SEL_ESC1: PN.ESC1, SEL_ESC2: PN.ESC2}
        # level-5 opponents: selector + 16 (k - 3) names the policy set of the arena's draw (OpponentNets); one synthetic set serves all
        lut.update({SEL_FIGHT1 + 16: PN.FIGHT1, SEL_FIGHT2 + 16: PN.FIGHT2, SEL_ESC1 + 32: PN.ESC1, SEL_ESC2 + 32: PN.ESC2})
        b.set_lut(lut)
        return b

    @classmethod
    def from_modules(cls, device, modules, max_rows=1 << 20):
        """modules: {slot: loaded reference policy (torch.load('policies/L3_AC1_fight.pt'))}"""
        b = cls(device, max_rows)
        for slot, m in modules.items():
            kind, sd = PN.from_torch_module(m)
            b.set_net(slot, kind, sd)
        return b

    @classmethod
    def from_reference_dir(cls, device, policy_dir, env, args, max_rows=1 << 20, load=None):
        """The reference's `_get_policies` (envs/env_base.py:312-347): which exported policies an environment flies, by file name
        in `policy_dir` (the reference keeps them in <repo>/policies).  A file is either this project's plain export
        (policy_files.save_policy, PPOLearner.export_policies: read with torch.load(weights_only=True), nothing else needed) or the
        reference's own, a pickled model object (torch.load(weights_only=False): needs the reference's model classes importable); a
        directory may mix both.  load: a caller's own `path -> loaded object` in place of that default; whatever it returns goes
        through policy_files.from_policy_object.
        env = "LowLevel" | "HighLevel".  Selector bytes as the world kernels emit them (policy type | aircraft type << 2, + 16 (k - 3)
        for the policy set k of a level-5 arena):
          LowLevel level 4 (fight):   L3_AC{1,2}_fight                                              -> 5, 9
          LowLevel level 5 (fight):   policies[3] = L3 fights, [4] = L4 fights, [5] = L3 escapes    -> 5, 9 | 21, 25 | 38, 42
          LowLevel level 5 (escape):  L5_AC{1,2}_fight                                              -> 5, 9
          HighLevel:                  L{eval_level_ag}_AC{1,2}_fight, L5 escapes (L3 escapes when EITHER is absent)  -> 5, 9, 6, 10
          HighLevel, eval_hl = False: additionally "fight_{1,2}_opp" = L{eval_level_opp}_AC{1,2}_fight for the opponents' fight rows, whose
                                      selector carries the side bit (hh_config.opp_side_selector)                      -> 69, 73
        LowLevel escape mode below level 5 loads nothing in the reference (env_base.py:328-330) and its _policy_actions would fail
        on the empty dict: refused here with a clear error."""
        import os
        from .policy_files import from_policy_object, load_policy_file
        if load is None:
            load = load_policy_file
        f = lambda name: load(os.path.join(policy_dir, name))
        plan = []   # (selector byte, file)
        if env == "LowLevel":
            if args.agent_mode == "fight" and args.level == 4:
                plan = [(SEL_FIGHT1, "L3_AC1_fight.pt"), (SEL_FIGHT2, "L3_AC2_fight.pt")]
            elif args.agent_mode == "fight":
                plan = [(SEL_FIGHT1, "L3_AC1_fight.pt"), (SEL_FIGHT2, "L3_AC2_fight.pt"), (SEL_FIGHT1 + 16, "L4_AC1_fight.pt"),
                        (SEL_FIGHT2 + 16, "L4_AC2_fight.pt"), (SEL_ESC1 + 32, "L3_AC1_escape.pt"), (SEL_ESC2 + 32, "L3_AC2_escape.pt")]
            elif args.level == 5:
                plan = [(SEL_FIGHT1, "L5_AC1_fight.pt"), (SEL_FIGHT2, "L5_AC2_fight.pt")]
            else:
                raise ValueError("LowLevelEnv in escape mode flies frozen opponents at level 5 only (the reference loads no policy for "
                                 f"escape mode at level {args.level}: envs/env_base.py:328-330)")
        else:
            lv = int(getattr(args, "eval_level_ag", 5))
            plan = [(SEL_FIGHT1, f"L{lv}_AC1_fight.pt"), (SEL_FIGHT2, f"L{lv}_AC2_fight.pt")]
            try:   # env_base.py:336-342: BOTH L5 escape policies, or (if either load fails) both L3 ones
                loaded = {n: f(n) for n in ("L5_AC1_escape.pt", "L5_AC2_escape.pt")}
                plan += [(SEL_ESC1, "L5_AC1_escape.pt"), (SEL_ESC2, "L5_AC2_escape.pt")]
            except Exception:   # noqa: BLE001 — the reference's bare except
                loaded = {}
                plan += [(SEL_ESC1, "L3_AC1_escape.pt"), (SEL_ESC2, "L3_AC2_escape.pt")]
            if not getattr(args, "eval_hl", True):   # env_base.py:343-346
                lo = int(getattr(args, "eval_level_opp", 4))
                plan += [(SEL_FIGHT1 + SEL_OPP_SIDE, f"L{lo}_AC1_fight.pt"), (SEL_FIGHT2 + SEL_OPP_SIDE, f"L{lo}_AC2_fight.pt")]
        b = cls(device, max_rows)
        lut = {}
        loaded = locals().get("loaded", {})
        for slot, (byte, name) in enumerate(plan):
            kind, sd = from_policy_object(loaded[name] if name in loaded else f(name))
            b.set_net(slot, kind, sd)
            lut[byte] = slot
        b.set_lut(lut)
        return b

    def act(self, obs, sel, actions=None, logits=None):
        """obs f32 [..., D] (rows = all leading dims), sel u8 [...] selector bytes -> int8 actions [..., 4]"""
        assert obs.dtype == torch.float32 and obs.is_contiguous()
        stride = obs.shape[-1]
        n_rows = obs.numel() // stride
        if sel is not None:   # None: same selectors as the previous call, the kernel re-uses its row lists
            assert sel.dtype == torch.uint8 and sel.is_contiguous() and sel.numel() == n_rows
        if actions is None:
            actions = torch.empty(tuple(obs.shape[:-1]) + (4,), dtype=torch.int8, device=obs.device)
        assert actions.dtype == torch.int8 and actions.is_contiguous() and actions.numel() == n_rows * 4
        st = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        lp = None if logits is None else C.c_void_p(logits.data_ptr())
        L.check(L.lib().hh_policy_act(self.h, C.c_void_p(obs.data_ptr()), n_rows, stride, None if sel is None else C.c_void_p(sel.data_ptr()),
                                      C.c_void_p(actions.data_ptr()), lp, st))
        return actions

    def act_binned(self, obs, actions, logits=None):
        """the forward over row lists a bound world's kernels wrote (World.bind_policy): no binning pass, the kernel clears the
        row counters behind itself"""
        assert obs.dtype == torch.float32 and obs.is_contiguous() and actions.dtype == torch.int8 and actions.is_contiguous()
        stride = obs.shape[-1]
        n_rows = obs.numel() // stride
        assert actions.numel() == n_rows * 4
        st = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        lp = None if logits is None else C.c_void_p(logits.data_ptr())
        L.check(L.lib().hh_policy_act_binned(self.h, C.c_void_p(obs.data_ptr()), n_rows, stride, C.c_void_p(actions.data_ptr()), lp, st))
        return actions

    def act_binned_live(self, obs, actions, live_rows, logits=None):
        """act_binned with the caller's estimate of the listed rows (the variant-row phases list ~0.3 of their [N, 15] slots): it picks the kernel form"""
        assert obs.dtype == torch.float32 and obs.is_contiguous() and actions.dtype == torch.int8 and actions.is_contiguous()
        stride = obs.shape[-1]
        n_rows = obs.numel() // stride
        assert actions.numel() == n_rows * 4
        st = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        lp = None if logits is None else C.c_void_p(logits.data_ptr())
        L.check(L.lib().hh_policy_act_binned_live(self.h, C.c_void_p(obs.data_ptr()), n_rows, stride, C.c_void_p(actions.data_ptr()), lp, int(live_rows), st))
        return actions

    @staticmethod
    def flops_per_row(kind):
        return PN.flops_per_row(kind)


class NetPilot:
    """HighLevelEnv pilots (env_base.py:349-398): every live unit's lowlevel_state row through the network its selector
    byte names (fight / escape policy of its aircraft type), actions written into one static [N, A, 4] buffer."""

    def __init__(self, world, bank=None, seed=0, bind=True):
        self.bank = bank if bank is not None else PolicyBank.random_init(world.device, seed=seed, max_rows=world.N * world.A)
        self.act = torch.zeros((world.N, world.A, 4), dtype=torch.int8, device=world.device)
        # bound: the world's phase kernels write the bank's row lists themselves (hh_bind_policy), every call is the forward only.
        # The pilot must then be called exactly once after every hl_begin / hl_agents_act / hl_tick whose rows are wanted, which is
        # what macro_step does; bind=False keeps the self-contained form (binning pass per call from pilot_mode).
        self.world = world if bind else None
        if bind:
            world.bind_policy(self.bank)

    def __call__(self, pilot_obs, pilot_mode):
        if self.world is not None:
            return self.bank.act_binned(pilot_obs, self.act)
        return self.bank.act(pilot_obs, pilot_mode, self.act)

    def close(self):
        if self.world is not None:
            self.world.bind_policy(None)
            self.world = None


def own_pilot(world, policy_dir, args, pilot_rows="variants"):
    """the pilot the facades fly when they load the reference's exported policies themselves (_get_policies("HighLevel"), env_base.py:333-343):
    the variant-row form (one launch + one policy call per sub-step) for worlds of up to three aircraft per side, the two-call form otherwise or on request
    (pilot_rows = "sides"); both fly the same trajectories bit for bit when the policy kernel runs the same forward form in both (the two paths issue calls of
    different sizes, which hhp_choose_form may hand to different forms — tile / weights-through-LDS, last-bit differences in the logits: HH_POLICY_W pins one)"""
    variants = pilot_rows == "variants" and world.A == 6
    bank = PolicyBank.from_reference_dir(world.device, policy_dir, "HighLevel", args, max_rows=world.N * (world.V_ROWS if variants else world.A))
    return VariantNetPilot(world, bank=bank) if variants else NetPilot(world, bank=bank)


class VariantNetPilot:
    """NetPilot for the variant-row form (World.hl_begin_variants / hl_act_tick: one launch and one policy call per sub-step): every listed row of
    the [N, 15, 30] buffer — the agents' rows and each opponent's row in its up-to-four variants — through the network its selector byte names."""

    variants = True

    def __init__(self, world, bank=None, seed=0, bind=True, live_fraction=0.3):
        rows = world.N * world.V_ROWS
        self.bank = bank if bank is not None else PolicyBank.random_init(world.device, seed=seed, max_rows=rows)
        self.act = torch.zeros((world.N, world.V_ROWS, 4), dtype=torch.int8, device=world.device)
        self.live = max(1, int(rows * live_fraction))
        self.world = world if bind else None
        if bind:
            world.bind_policy(self.bank)

    def __call__(self, pilot_obs, pilot_mode):
        if self.world is not None:
            return self.bank.act_binned_live(pilot_obs, self.act, self.live)
        return self.bank.act(pilot_obs, pilot_mode, self.act)

    def close(self):
        if self.world is not None:
            self.world.bind_policy(None)
            self.world = None


class OpponentNets:
    """LowLevelEnv levels 4-5 `opponent_policy` callable: opponents 3 / 4 are type-1 / type-2 aircraft (env_base.py:560-561
    fixes the first two slots of a side).  Level 4 flies the level-3 fight policies (selectors 5 / 9).  Level 5 draws k per
    arena and episode (env_hetero.py:55-59): selector = fight selector + 16 (k - 3), + 1 when k == 5 (escape), so a bank
    loaded with policies[3], policies[4] (fight sets) and policies[5] (escape set) maps 5/9, 21/25 and 38/42 to them."""

    def __init__(self, world, bank=None, seed=0, bind=None, skip_first=True):
        """skip_first: the binding is made AFTER a hh_step_begin already produced the opp_obs of the first call (a callable built
        lazily inside its first invocation): that call bins the rows itself.  A facade that binds before any step passes False —
        its first step_begin already filled the row lists, and binning them a second time would list every row twice."""
        self.world = world
        n_opp = world.A - world.n_agents
        # bound (default for a bank nobody else uses): hh_step_begin bins the opponents' rows into the bank's lists itself
        self._private = (bank is None) if bind is None else bool(bind)
        self.bank = bank if bank is not None else PolicyBank.random_init(world.device, seed=seed, max_rows=world.N * n_opp)
        self._skip = 0
        if self._private:
            world.bind_policy(self.bank)
            self._skip = 1 if skip_first else 0
        self.act = torch.zeros((world.N, n_opp, 4), dtype=torch.int8, device=world.device)
        self.sel_fight = torch.tensor([SEL_FIGHT1, SEL_FIGHT2], dtype=torch.uint8, device=world.device).repeat(world.N, 1).contiguous()
        self.k = torch.zeros((world.N,), dtype=torch.int8, device=world.device)

    def __call__(self, opp_obs, env=None):
        if self._private and not self._skip:   # the rows of the step_begin that wrote opp_obs are already in the bank's lists
            return self.bank.act_binned(opp_obs.contiguous(), self.act)
        self._skip = 0
        sel = self.sel_fight
        if self.world.cfg.level == 5 and self.world.cfg.agent_mode == L.MODE_FIGHT:
            k = self.world.opp_policy(self.k)
            sel = (self.sel_fight + (16 * (k - 3) + (k == 5)).to(torch.uint8)[:, None]).contiguous()
        return self.bank.act(opp_obs.contiguous(), sel, self.act)


class RandomPilot:
    """uniform actions from a device generator (env-only throughput measurements)"""

    def __init__(self, device, seed=0):
        torch.manual_seed(seed)  # default generator: usable inside a captured HIP graph
        self.hi = torch.tensor([13, 9, 2, 2], device=device)

    def __call__(self, pilot_obs, pilot_mode):
        n, a = pilot_mode.shape
        return (torch.rand((n, a, 4), device=pilot_obs.device) * self.hi).to(torch.int8)


class TapePilot:
    """uniform actions from a tape that is resident in HBM before the step starts (the way bench.py feeds LowLevelEnv):
    `bank` holds `chunks` x `depth` sub-steps of int8 actions [N, A, 4]; `load(k)` copies chunk k into the static buffer the
    calls hand out, one slice per sub-step (the agents' call and the opponents' call of a sub-step get the same tensor —
    each side's rows are read by its own launch).  No kernel runs inside the macro step."""

    def __init__(self, device, n_arenas, n_units, seed=0, depth=16, chunks=4, bank=None):
        """bank: a ready int8 tape [chunks, depth, n_arenas, n_units, 4] (e.g. world.action_tape_uniform: the keyed synthetic actions); else torch.rand"""
        if bank is not None:
            assert bank.dtype == torch.int8 and bank.is_contiguous() and tuple(bank.shape[1:]) == (depth, n_arenas, n_units, 4)
            self.bank = bank
        else:
            g = torch.Generator(device=device)
            g.manual_seed(seed)
            hi = torch.tensor([13, 9, 2, 2], device=device)
            self.bank = (torch.rand((chunks, depth, n_arenas, n_units, 4), device=device, generator=g) * hi).to(torch.int8).contiguous()
        self.static = self.bank[0].clone()
        self.depth, self.calls = depth, 0

    def load(self, k):
        self.static.copy_(self.bank[k % self.bank.shape[0]])
        self.calls = 0

    def __call__(self, pilot_obs, pilot_mode):
        act = self.static[(self.calls // 2) % self.depth]
        self.calls += 1
        return act


class MLPPilot(torch.nn.Module):
    """randomly initialised fight / escape networks with the reference's I/O shapes (obs 30 padded ->
    logits 13+9+2+2, models/ac_models_hetero.py), greedy arg-max decode; batched over all units"""

    def __init__(self, device, hidden=200, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)

        def net():
            m = torch.nn.Sequential(torch.nn.Linear(30, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, hidden), torch.nn.Tanh(),
                                    torch.nn.Linear(hidden, 26))
            for p in m.parameters():
                with torch.no_grad():
                    p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            return m
        self.fight, self.esc = net(), net()
        self.to(device)

    @torch.no_grad()
    def forward(self, pilot_obs, pilot_mode):
        n, a, _ = pilot_obs.shape
        x = pilot_obs.reshape(n * a, 30)
        lf, le = self.fight(x), self.esc(x)
        logits = torch.where(((pilot_mode.reshape(-1, 1) & 3) == 2), le, lf)
        parts = logits.split((13, 9, 2, 2), dim=1)
        act = torch.stack([p.argmax(dim=1) for p in parts], dim=1)
        return act.to(torch.int8).reshape(n, a, 4)
