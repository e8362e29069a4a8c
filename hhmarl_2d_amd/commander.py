"""The trainable commander of train_hier.py (commander side) on the device: `CommanderNet` evaluates
models/ac_models_hier.py:CommanderGru the way RLlib's sampler does (actor, value branch, both GRU cells, Categorical draw and
log-probability) for every agent row of every arena in one fused gfx950 kernel (include/hh_commander.h), and `CommanderRollout`
does for train_hier.py what `rollout.PPORollout` does for train_hetero.py."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from . import policy_nets as PN
from .rollout import (EpisodeBatch, central_critic_rows_hl, collect_until_ready, outcomes_keyword, rollout_load_plan, rollout_outcome_names,
                      rollout_state_dict, window_metrics_keyword)

OBS, HIDDEN, N_ACTIONS, N_AGENTS = 34, 200, 3, 3


def state_keys():
    """the reference's CommanderGru state_dict keys -> shapes (nn.Linear [out, in]; nn.GRU gate rows r | z | n)"""
    k = OrderedDict()
    k["shared_layer._model.0.weight"], k["shared_layer._model.0.bias"] = (500, 500), (500,)
    for rnn in ("rnn_act", "rnn_val"):
        k[f"{rnn}.weight_ih_l0"], k[f"{rnn}.weight_hh_l0"] = (600, 200), (600, 200)
        k[f"{rnn}.bias_ih_l0"], k[f"{rnn}.bias_hh_l0"] = (600,), (600,)
    for name, shp in (("inp1", (50, 4)), ("inp2", (200, 20)), ("inp3", (50, 10)), ("inp4", (200, 34)), ("act_out", (3, 500)),
                      ("v1", (100, 35)), ("v2", (100, 35)), ("v3", (100, 35)), ("v4", (200, 105)), ("val_out", (1, 500))):
        k[f"{name}._model.0.weight"], k[f"{name}._model.0.bias"] = shp, shp[:1]
    return k


def random_weights(seed):
    """Deterministic synthetic CommanderGru weights (policy_nets.random_weights' convention): numpy PCG64, N(0, 1/fan_in) weights,
    N(0, 0.1^2) biases — fixtures store the seed, not the matrices."""
    rng = np.random.default_rng([int(seed), 0xC0])
    sd = OrderedDict()
    for k, shp in state_keys().items():
        if len(shp) == 2:
            sd[k] = (rng.standard_normal(shp) / np.sqrt(shp[-1])).astype(np.float32)
        else:
            sd[k] = (0.1 * rng.standard_normal(shp)).astype(np.float32)
    return sd


def from_torch_module(module):
    """weights of a real CommanderGru (e.g. restored from a train_hier.py checkpoint) -> dict of numpy arrays"""
    sd = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in module.state_dict().items()}
    return OrderedDict((k, sd[k]) for k in state_keys())


def _weights_struct(p):
    """hh_commander_weights; p(state_dict key) -> pointer"""
    w = L.HHCommanderWeights()
    for i in range(4):
        w.inp_w[i], w.inp_b[i] = p(f"inp{i + 1}._model.0.weight"), p(f"inp{i + 1}._model.0.bias")
        w.v_w[i], w.v_b[i] = p(f"v{i + 1}._model.0.weight"), p(f"v{i + 1}._model.0.bias")
    w.act_w_ih, w.act_w_hh, w.act_b_ih, w.act_b_hh = (p(f"rnn_act.{n}_l0") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    w.val_w_ih, w.val_w_hh, w.val_b_ih, w.val_b_hh = (p(f"rnn_val.{n}_l0") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    w.shared_w, w.shared_b = p("shared_layer._model.0.weight"), p("shared_layer._model.0.bias")
    w.act_out_w, w.act_out_b = p("act_out._model.0.weight"), p("act_out._model.0.bias")
    w.val_out_w, w.val_out_b = p("val_out._model.0.weight"), p("val_out._model.0.bias")
    return w


class CommanderNet:
    """CommanderGru on one GPU: `set_weights(sd)` (the reference's state_dict, numpy or torch), `refresh_weights(sd)` (the same from CUDA
    tensors, on the device), `sample(...)` = one sampler step of [N, 3] agent rows (hh_commander_sample), `act_chain(obs)` = one greedy
    commander step as evaluation.py takes it, the actor's state chained through the agent slots (hh_commander_act_chain)."""

    def __init__(self, device, max_rows):
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.max_rows = int(max_rows)
        self.h = C.c_void_p()
        L.check(L.lib().hh_commander_create(self.device.index or 0, self.max_rows, C.byref(self.h)))
        self._w = None

    def close(self):
        if getattr(self, "h", None):
            L.lib().hh_commander_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_weights(self, sd):
        """load (or replace) the weights; synchronous.  The device copy keeps its addresses, so a captured rollout graph sees the new weights."""
        keys = state_keys()
        arr = {}
        for k, shp in keys.items():
            v = sd[k]
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            v = np.ascontiguousarray(v, dtype=np.float32)
            if v.shape != shp:
                raise ValueError(f"{k}: shape {v.shape}, CommanderGru has {shp}")
            arr[k] = v
        w = _weights_struct(lambda k: arr[k].ctypes.data)
        L.check(L.lib().hh_commander_set_weights(self.h, C.byref(w)))
        self._w = arr
        return self

    def refresh_weights(self, sd):
        """The learner's new weights from float32 CUDA tensors keyed like the reference's state_dict() (state_keys), repacked on the device
        into the same bytes set_weights writes, in place, ordered on the current torch stream (hh_commander_refresh_weights): no host
        synchronisation, capturable into a CUDA graph, and a captured CommanderRollout keeps replaying (same addresses, no re-capture).
        The commander must have been loaded once with set_weights."""
        arr = PN.device_weights(state_keys(), sd, self.device, "CommanderNet.refresh_weights")
        w = _weights_struct(lambda k: arr[k].data_ptr())
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(L.lib().hh_commander_refresh_weights(self.h, C.byref(w), st))
        self._w = None   # the host copy of set_weights is stale now
        return self

    def packed(self, part):
        """test hook: one packed part as the kernel reads it (hh_commander_copy_packed; 0 fp16 planes, 1 fp32 section) -> uint8 CUDA tensor"""
        n = C.c_int64()
        L.check(L.lib().hh_commander_copy_packed(self.h, int(part), None, 0, C.byref(n), None))
        out = torch.empty((n.value,), dtype=torch.uint8, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(L.lib().hh_commander_copy_packed(self.h, int(part), C.c_void_p(out.data_ptr()), n.value, C.byref(n), st))
        return out

    # ---- complete snapshots (checkpointing: hh_commander_snapshot / hh_commander_restore, include/hh_commander.h) ----
    def snapshot(self):
        """the packed weights exactly as the kernels read them, as an opaque blob (uint8 CPU tensor); synchronises the current stream"""
        return L.snapshot("commander", self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def restore(self, blob):
        """a snapshot() blob back in place (same addresses: a captured CommanderRollout keeps replaying).  ValueError, the net untouched:
        another geometry or format version, a net without weights on one side only, a truncated blob."""
        if not isinstance(blob, torch.Tensor) or blob.dtype != torch.uint8 or blob.dim() != 1 or blob.device.type != "cpu":
            raise ValueError("blob: a 1-D uint8 CPU tensor (CommanderNet.snapshot())")
        L.restore("commander", self.h, blob.contiguous(), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        self._w = None   # the host copy of set_weights is stale now

    def state_dict(self):
        return {"blob": self.snapshot()}

    def _load_plan(self, sd):
        from . import checkpoint as ck
        ck.need_keys("CommanderNet", sd, ("blob",))
        ck.check_blob("CommanderNet", sd["blob"], L.snapshot_bytes("commander", self.h), L.SNAPSHOT_MAGIC["commander"])
        return lambda: self.restore(sd["blob"])

    def load_state_dict(self, sd):
        self._load_plan(sd)()

    def sample(self, obs, h_in, h_out, fresh=None, world=None, uniforms=None, crit_act=None, greedy=False, actions=None, logp=None,
               vf=None, logits=None, want_vf=True):
        """obs f32 [N, 3, 34]; h_in / h_out f32 [N, 3, 2, 200] (state_in / state_out: 0 = rnn_act, 1 = rnn_val; rows of `fresh` arenas of
        h_in are overwritten with zeros); fresh u8 [N] or None; world (keyed draws) or uniforms f64 [N, 3]; crit_act f32 [N, 3] = the value
        branch's act inputs (None = zeros, as while sampling) -> (actions i8 [N, 3], logp f32 [N, 3], vf f32 [N, 3] or None)"""
        N = obs.shape[0]
        dev = obs.device
        assert obs.dtype == torch.float32 and obs.is_contiguous() and tuple(obs.shape) == (N, N_AGENTS, OBS)
        for t in (h_in, h_out):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == N * N_AGENTS * 2 * HIDDEN
        if actions is None:
            actions = torch.empty((N, N_AGENTS), dtype=torch.int8, device=dev)
        if logp is None:
            logp = torch.empty((N, N_AGENTS), dtype=torch.float32, device=dev)
        if vf is None and want_vf:
            vf = torch.empty((N, N_AGENTS), dtype=torch.float32, device=dev)
        assert actions.dtype == torch.int8 and actions.is_contiguous() and actions.numel() == N * N_AGENTS
        assert logp.dtype == torch.float32 and logp.is_contiguous() and logp.numel() == N * N_AGENTS
        assert vf is None or (vf.dtype == torch.float32 and vf.is_contiguous() and vf.numel() == N * N_AGENTS)
        if fresh is not None:
            assert fresh.dtype == torch.uint8 and fresh.is_contiguous() and fresh.numel() == N
        if uniforms is not None:
            assert uniforms.dtype == torch.float64 and uniforms.is_contiguous() and uniforms.numel() == N * N_AGENTS
        if crit_act is not None:
            assert crit_act.dtype == torch.float32 and crit_act.is_contiguous() and crit_act.numel() == N * N_AGENTS
        if logits is not None:
            assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() == N * N_AGENTS * 4
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(L.lib().hh_commander_sample(self.h, ptr(obs), N, ptr(h_in), ptr(h_out), ptr(fresh), None if world is None else world.h,
                                            ptr(uniforms), ptr(crit_act), 1 if greedy else 0, ptr(actions), ptr(logp), ptr(vf), ptr(logits), st))
        return actions, logp, vf

    def kernel_name(self, n_arenas):
        buf = C.create_string_buffer(64)
        L.check(L.lib().hh_commander_kernel_name(self.h, int(n_arenas), buf, 64))
        return buf.value.decode()

    def act_chain(self, obs, actions=None, h_out=None, logits=None):
        """The commander as evaluation.py:40-48 runs it (hh_commander_act_chain): per arena the actor over agent slots 0..n-1 in order,
        slot 0 from zero rnn_act state, slot k from slot k-1's state_out, greedy first arg-max; no value branch.
        obs f32 [N, n, 34] (1 <= n <= 5); h_out f32 [N, n, 200] / logits f32 [N, n, 4] optional outputs -> actions i8 [N, n].
        Ordered on the current torch stream; no host synchronisation (graph-capturable)."""
        if obs.dim() != 3 or tuple(obs.shape[2:]) != (OBS,):
            raise ValueError(f"act_chain: obs must be [N, n_agents, {OBS}], got {tuple(obs.shape)}")
        N, nA = int(obs.shape[0]), int(obs.shape[1])
        if not 1 <= nA <= 5:
            raise ValueError(f"act_chain: n_agents must be 1..5, got {nA}")
        if N < 1:
            raise ValueError("act_chain: no arenas")
        dev = obs.device
        if actions is None:
            actions = torch.empty((N, nA), dtype=torch.int8, device=dev)
        for name, t, dt, n in (("obs", obs, torch.float32, N * nA * OBS), ("actions", actions, torch.int8, N * nA),
                               ("h_out", h_out, torch.float32, N * nA * HIDDEN), ("logits", logits, torch.float32, N * nA * 4)):
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.numel() != n or t.device != dev):
                raise ValueError(f"act_chain: {name} must be a contiguous {dt} tensor of {n} elements on {dev}")
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(L.lib().hh_commander_act_chain(self.h, ptr(obs), N, nA, ptr(actions), ptr(h_out), ptr(logits), st))
        return actions

    def chain_kernel_name(self, n_arenas, n_agents):
        buf = C.create_string_buffer(64)
        L.check(L.lib().hh_commander_chain_kernel_name(self.h, int(n_arenas), int(n_agents), buf, 64))
        return buf.value.decode()


def default_carry_cap(horizon, n_agents=N_AGENTS, n_opps=3):
    """rows an unfinished commander episode can hold, with `horizon` H ticks (the carry of CommanderEpisodeBatch): ceil(H / 12) + n_agents
    + n_opps - 1 (47 at H = 500, 3 vs 3).

    The world's sub-step loop (env_hier.py:114-140; hh_kernels_hier.h / hh_kernels_oct.h, hl_run after every tick): a commander step
    runs ticks until hl_s > 15 (16 ticks), a kill event (an aircraft removed in the tick) or the surrounding event, which is looked for
    only while hl_s > 10 before the tick's increment, i.e. from the 12th tick on.  So a step without a kill event lasts at least 12 ticks,
    a step with one at least 1.  The episode ends (done) after the step in which `steps` reaches H or one side has no aircraft left.
    An episode still running after r steps therefore has fewer than H ticks behind it and both sides alive: at most
    (n_agents - 1) + (n_opps - 1) deaths, so at most that many kill-event steps, and the others fit 12 ticks each into H - 1:
    r <= floor((H - 1) / 12) + n_agents + n_opps - 2.  The rounder ceil(H / 12) + n_agents + n_opps - 1 is at least one more than that
    for every H.  (horizon - 1 rows, one per tick, would be 10 times as much carry: 1.7 GB of observations at N = 8192.)"""
    return -(-int(horizon) // 12) + int(n_agents) + int(n_opps) - 1


class CommanderEpisodeBatch(EpisodeBatch):
    """The whole-episode GRU-sequence batch of a `CommanderRollout(..., batch_mode="complete_episodes")` (train_hier.py:182 with the
    recurrent CommanderGru, RLlib's max_seq_len = 20): after every collect, the rows of every episode that ENDED in it, from its reset
    row to its done row, in one flat batch; GAE over each whole episode (hh_gae_rllib's float64 recursion, last_r = 0.0:
    oracle/gae_ref.compute_advantages per episode and agent); every episode cut into sequences of at most L = max_seq_len steps
    (ceil(E / L) per episode of E rows: L, ..., L, then the remainder; a sequence never crosses a done), and the GRU states of each
    sequence's first step, bit-identical to the state_in the sampler's forward used there — also when that step lies in an earlier
    collect: the device carry keeps, besides the running episode's rows, the states at its sequence starts.  Written by
    hh_commander_episodes_emit (include/hh_commander.h) inside the collect's graph; no host synchronisation until `rows()`.

    Device buffers of fixed capacity, overwritten by every collect, in the order arena-major, then episode, then time:
      obs f32 [R, 3, 34], actions i8 [R, 3], logp / vf / reward f32 [R, 3], valid u8 [R, 3], adv / target f32 [R, 3], done u8 [R] (1 on
      an episode's last row only), arena / episode / t i32 [R] (`episode` counts per arena from `start()`, `t` the step within the
      episode from 0); episode table ep_start / ep_len / ep_arena i32 [E]; sequence table seq_start (row in the batch) / seq_len /
      seq_ep (episode entry) i32 [S]; state_in f32 [S, 3, 2, 200] ([:, :, 0] = state_in_0 = rnn_act, [:, :, 1] = state_in_1 = rnn_val);
      carried i32 [N] (rows of each arena's running episode held for a later collect).
    vf stays VF_PREDS as sampled (zero action inputs); `critic_rows` gives the learner's action-filled CUR_OBS rows.

    Capacity, with C = carry_cap (default_carry_cap: the rows an unfinished episode can have) and L: the carry holds N C rows and
    N ceil(C / L) states; the batch R = N (C + T) rows, E = N T episodes and S = N (T + C // L) sequences (an arena emits at most
    C + T rows in at most T episodes, and sum ceil(E_k / L) <= n_eps + (rows - n_eps) / L).  Bytes per arena:
      450 C + 4800 ceil(C / L) (carry) + 487 (C + T) (rows) + 12 T (episode table) + 4812 (T + C // L) (sequences and their states).
    N = 8192, T = 16, H = 500 (C = 47), L = 20: 173 MB of row carry, 118 MB of state carry, 251 MB of rows, 2 MB of episode table
    and 710 MB of sequences: 1.25 GB in all.  Nothing overflows under that rule; if something did anyway (a carry_cap below it), a
    sticky device flag is set and `rows()` raises.

    aux = (name, f32 [T, N, 3, d]): EpisodeBatch's optional column (hh_commander_episodes_emit_aux) — `name` f32 [R, 3, d] in `rows()`
    and, zero padded like the other columns, [S, L, 3, d] in `sequences()`.  CommanderRollout(record_logits=True) puts the sampler's
    logits there (d = 4): 48 B per row on top of 450 (carry) / 487 (batch) — at N = 8192, T = 16, C = 47: 18 MB more carry, 25 MB more
    batch.

    train_batch_size = B: EpisodeBatch's accumulation (hh_commander_episodes_emit_append) — the collects are appended on the device
    until the batch holds at least B rows; ep_start, seq_start and seq_ep are positions in the accumulated batch, `sequences()` and
    `n_sequences` describe it.  Capacities: R = B - 1 + N (C + T) rows, E = B - 1 + N T episodes and by default S = B - 1 +
    N (T + C // L) sequences, all below 2^31.  That S is safe for one-row episodes (a sequence each), and a sequence costs 4812 B:
    seq_cap = S overrides it (at least N (T + C // L); with fewer than the batch needs the sticky flag is set and `rows()` raises).
    Bytes: 487 per row, 12 per episode, 4812 per sequence — B = 4 collects' worth of rows at N = 8192, T = 16 (B = 524288) is 255 MB
    of rows, 6 MB of episode table and 2.52 GB of sequences more than without; seq_cap = B // 4 + N (T + C // L) (enough while a batch
    averages four rows or more per sequence) brings the sequences to 0.63 GB."""

    SEQ_TABLE = ("seq_start", "seq_len", "seq_ep")
    _EMIT, _SCRATCH, _N_COUNTS = "hh_commander_episodes_emit", (10, 4), 4
    _critic_rows = staticmethod(central_critic_rows_hl)
    AGENT_KEYS = (1, 2, 3)   # metrics(): the three agents of the one commander policy, by agent id

    @classmethod
    def capacities(cls, N, T, carry_cap, train_batch_size=None, max_seq_len=None, seq_cap=None):
        """-> EpisodeBatch.capacities' (R, E), and with max_seq_len = L (R, E, S sequences): N (T + carry_cap // L), with
        train_batch_size = B another B - 1, or seq_cap where given (an int of at least N (T + carry_cap // L), train_batch_size only);
        ValueError for capacities that reach 2^31"""
        R, E = super().capacities(N, T, carry_cap, train_batch_size)
        if max_seq_len is None:
            return R, E
        floor = int(N) * (int(T) + int(carry_cap) // int(max_seq_len))
        S = floor + (0 if train_batch_size is None else train_batch_size - 1)
        if seq_cap is not None:
            if train_batch_size is None:
                raise ValueError("seq_cap: only with train_batch_size (without it the sequence table is N (T + carry_cap // max_seq_len))")
            if isinstance(seq_cap, bool) or not isinstance(seq_cap, int) or seq_cap < floor:
                raise ValueError(f"seq_cap: an int of at least N (T + carry_cap // max_seq_len) = {floor}, got {seq_cap!r}")
            S = seq_cap
        if train_batch_size is not None and S >= 2 ** 31:
            raise ValueError(f"train_batch_size = {train_batch_size}: the sequence capacity ({S}) must stay below 2^31")
        return R, E, S

    def __init__(self, collect, max_seq_len, carry_cap, gamma, lam, aux=None, metrics=False, train_batch_size=None, seq_cap=None):
        """collect: the rollout's [T(+1), N, ...] buffers (ROW_INPUTS, done and state_in) that every emission reads; aux: None or
        (name, f32 [T, N, 3, d]) as EpisodeBatch takes it; metrics: EpisodeBatch's episode metrics (per-agent entries keyed 1..3);
        train_batch_size / seq_cap: accumulate to at least that many rows, with that many sequence entries (see the class)"""
        self.L, self._seq_cap = int(max_seq_len), seq_cap
        super().__init__(collect, carry_cap, gamma, lam, aux=aux, metrics=metrics, train_batch_size=train_batch_size)
        S, sc = self._bufs.seq_cap, max(-(-self.carry_cap // self.L), 1)
        z = lambda shape: torch.zeros(shape, dtype=torch.int32, device=self._device)
        self.seq_start, self.seq_len, self.seq_ep = z((S,)), z((S,)), z((S,))
        state = tuple(collect["state_in"].shape[2:])
        self.state_in = torch.zeros((S,) + state, dtype=torch.float32, device=self._device)
        self._carry["state"] = torch.zeros((self.N, sc) + state, dtype=torch.float32, device=self._device)
        self.n_sequences = self._size[3]
        self._bind(collect, {"state": self._carry["state"]}, ("state_in",), ("state_in",), self.SEQ_TABLE)

    def _capacities(self):
        R, E, self._S = self.capacities(self.N, self.T, self.carry_cap, self.train_batch_size, self.L, self._seq_cap)
        return R, E

    def _struct(self, R, E, gamma, lam):
        return L.HHCommanderEpisodeBufs(T=self.T, N=self.N, max_seq_len=self.L, carry_cap=self.carry_cap, row_cap=R, ep_cap=E,
                                        seq_cap=self._S, gamma=gamma, lam=lam)

    def _parts(self):
        return super()._parts() + ((self.SEQ_TABLE + ("state_in",), 3),)   # rows() also holds the sequence table and state_in [S, 3, 2, 200]

    def _options(self):
        return dict(super()._options(), max_seq_len=self.L, seq_cap=int(self._bufs.seq_cap))

    def _carry_lead(self, k, m):
        """the state carry holds one entry per sequence start (within-episode steps 0, L, 2 L, ...) of the running episode"""
        return m if k != "state" else min(-(-m // self.L) + 1, self._carry["state"].shape[1])

    def sequences(self):
        """the learner's padded form (RLlib's chop_into_sequences, all three agents of an arena row side by side; per agent it is the slice
        [..., a, ...]), gathered on the device through the sequence table: obs f32 [S, L, 3, 34], actions i8 / logp / vf / adv / target
        [S, L, 3] (zero past seq_len), seq_lens i32 [S], mask bool [S, L], state_in f32 [S, 3, 2, 200]; with an aux column also that one,
        f32 [S, L, 3, d]"""
        r = self.rows()
        S, sl = r["seq_start"].shape[0], self.L
        steps = torch.arange(sl, dtype=torch.int64, device=self._device)
        mask = steps[None, :] < r["seq_len"].long()[:, None]
        idx = torch.where(mask, r["seq_start"].long()[:, None] + steps[None, :], torch.zeros((), dtype=torch.int64, device=self._device))
        out = {}
        for k in ("obs", "actions", "logp", "vf", "adv", "target") + ((self.aux_name,) if self.aux_name else ()):
            col = r[k]
            g = col[idx] if col.shape[0] > 0 else torch.zeros((S, sl) + tuple(col.shape[1:]), dtype=col.dtype, device=self._device)
            m = mask.view(S, sl, *([1] * (g.dim() - 2)))
            out[k] = torch.where(m, g, torch.zeros((), dtype=g.dtype, device=self._device))
        out["seq_lens"], out["mask"], out["state_in"] = r["seq_len"], mask, r["state_in"]
        return out


class CommanderRollout:
    """What RLlib's rollout workers produce for train_hier.py's commander PPO (train_hier.py:100-199), for every arena of a 3-vs-3
    HighLevelEnv `World` at once and without leaving the device: per commander step `CommanderNet.sample` (actor + value branch of
    CommanderGru on central_critic_observer's rows with zero action inputs, both GRU states carried per agent and zeroed at every
    episode start, the Categorical draw from the keyed RNG: HH_SITE_COMMANDER_SAMPLE) and one `env_hier.macro_step` with the frozen
    pilots; after T commander steps a greedy bootstrap evaluation of obs[T] and hh_gae_rllib (gamma 0.99, RLlib's default lambda 1.0:
    train_hier.py:186).  With the library's own NetPilot / VariantNetPilot a collect is ONE HIP graph; any other pilot runs eagerly.

    Buffers (device, overwritten by every collect): obs f32 [T+1, N, 3, 34], actions i8 [T, N, 3], logp f32 [T, N, 3], vf f32
    [T+1, N, 3], reward f32 [T, N, 3], valid u8 [T, N, 3], done u8 [T, N], adv / target f32 [T, N, 3], state_in f32 [T+1, N, 3, 2, 200]
    (row t = the state step t's forward used — zero at an episode's first step; row T carries into the next collect).
    Rewards: HighLevelEnv gives every agent id a reward key every step, dead agents included (env_hier.py:154,188); hh_hl_end writes
    0.0 wherever it reports valid = 0, and in an auto-resetting world valid is 1 on every row — RLlib's rewards.get(agent_id, 0.0) is the
    world's reward as it stands, nothing is masked.

    batch_mode = "truncate_episodes" (default): the buffers above are the result, and `CommanderLearner.update_window(rollout)` trains on
    them as they stand.  batch_mode = "complete_episodes" (train_hier.py:182):
    every collect still fills them exactly the same way, and then also `episodes`, a `CommanderEpisodeBatch` of every episode that ended
    in it, whole and cut into GRU sequences of at most `max_seq_len` steps; its launches join the collect's graph after the GAE.

    record_logits = True: every step's sampler call also writes its logits — the split-fp16 MFMA forward's own, the rows the actions were
    drawn from and `logp` was taken of: RLlib's ACTION_DIST_INPUTS — into `logits` f32 [T, N, 3, 4] (column 3 zero), and with
    batch_mode = "complete_episodes" the column travels with the rows (`episodes.rows()["logits"]` [R, 3, 4], `sequences()["logits"]`
    [S, L, 3, 4]): every emitted row carries the logits of the forward that sampled it, whatever weights the sampler held then, and
    `CommanderLearner.update` uses them.  The bootstrap evaluation keeps discarding its logits.  Cost: 48 T N bytes of collect buffer and
    48 B per row of carry and batch (on top of 450 / 487).  With the default False nothing is allocated and the launches, the graph and
    the results are what they were.

    metrics = True (batch_mode = "complete_episodes" only): `episodes.metrics()` gives the collect's line of RLlib's training result
    (`episode_reward_mean` and the rest, train_hier.py's print) from three more launches behind the emitter; the per-agent entries are
    keyed by agent id 1..3 (the three agents share the one commander policy); see EpisodeBatch.

    train_batch_size = B (batch_mode = "complete_episodes" only; train_hier.py's `train_batch_size=args.batch_size`): `episodes`
    accumulates the collects on the device until it holds at least B rows (commander steps of an arena) — whole collects, nothing
    trimmed — with the same launches per collect.  `collect_batch()` collects until `episodes.ready()`; the collect after a complete
    batch starts the next one.  See CommanderEpisodeBatch for the capacities (its seq_cap is a keyword of the batch, not of the
    rollout: the rollout takes the safe default).

    window_metrics = True (keyword-only; batch_mode = "truncate_episodes" only): the same result line for a run that trains from the
    windows — `window_metrics`, a `rollout.WindowMetrics` with the per-agent entries keyed 1..3, carries every arena's running return and
    length across collects and reports the episodes that finish inside each window: five more launches in the collect's graph right
    behind the GAE.  With the default False it is None and nothing changes.

    outcomes = True (keyword-only; needs metrics = True with batch_mode = "complete_episodes", or window_metrics = True): `outcome` i8
    [T, N], overwritten by every collect — row [t, n] is the outcome of the episode whose done row it is (1 agents win, -1 opponents win,
    0 draw: `World.episode_stats()`' codes) and 2 elsewhere, tapped right behind every commander step (`World.outcome_tap`: T more
    launches) — and `episodes` / `window_metrics` own `ep_outcome` and the outcome keys of `metrics()` (two more launches; see
    rollout.EpisodeBatch).  With the default False `outcome` is None and nothing changes."""

    @outcomes_keyword
    @window_metrics_keyword(CommanderEpisodeBatch.AGENT_KEYS)
    def __init__(self, world, commander, pilot, T, gamma=0.99, lam=1.0, use_graph=True, batch_mode="truncate_episodes", max_seq_len=20,
                 carry_cap=None, metrics=False, train_batch_size=None, record_logits=False):
        """batch_mode / max_seq_len / carry_cap: see CommanderEpisodeBatch (carry_cap None = default_carry_cap of the world); metrics /
        train_batch_size / record_logits: pass them by keyword (record_logits stays the last parameter); window_metrics is keyword-only
        (rollout.window_metrics_keyword)"""
        if batch_mode not in ("truncate_episodes", "complete_episodes"):
            raise ValueError("batch_mode: 'truncate_episodes' (fixed [T, N] windows) or 'complete_episodes' (whole episodes cut into GRU "
                             "sequences: CommanderEpisodeBatch)")
        if metrics and batch_mode != "complete_episodes":
            raise ValueError("metrics=True needs batch_mode='complete_episodes': the episode metrics are those of the whole-episode batch")
        if train_batch_size is not None and batch_mode != "complete_episodes":
            raise ValueError("train_batch_size needs batch_mode='complete_episodes': it is the whole-episode batch that accumulates")
        train_batch_size = EpisodeBatch.check_train_batch_size(train_batch_size)
        if int(max_seq_len) < 1:
            raise ValueError("max_seq_len must be at least 1")
        if carry_cap is not None and int(carry_cap) < 0:
            raise ValueError("carry_cap must not be negative")
        assert world.cfg.env_kind == L.ENV_HIGHLEVEL and world.n_agents == N_AGENTS and world.cfg.auto_reset, \
            "CommanderRollout drives an auto-resetting 3-agent HighLevelEnv world (central_critic_observer hard-codes three agents)"
        assert commander.max_rows >= N_AGENTS * world.N, "the commander's max_rows must cover 3 x n_arenas rows"
        self.w, self.net, self.pilot, self.T, self.gamma, self.lam = world, commander, pilot, int(T), float(gamma), float(lam)
        N, dev, T = world.N, world.device, self.T
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.obs = z((T + 1, N, N_AGENTS, OBS), torch.float32)
        self.actions = z((T, N, N_AGENTS), torch.int8)
        self.logp = z((T, N, N_AGENTS), torch.float32)
        self.vf = z((T + 1, N, N_AGENTS), torch.float32)
        self.reward = z((T, N, N_AGENTS), torch.float32)
        self.valid = z((T, N, N_AGENTS), torch.uint8)
        self.done = z((T, N), torch.uint8)
        self.adv = z((T, N, N_AGENTS), torch.float32)
        self.target = z((T, N, N_AGENTS), torch.float32)
        self.state_in = z((T + 1, N, N_AGENTS, 2, HIDDEN), torch.float32)
        self._fresh = z((N,), torch.uint8)                     # episode starts at the next collect's first step
        self._h_scratch = z((N, N_AGENTS, 2, HIDDEN), torch.float32)
        self._tmp_act, self._tmp_logp = z((N, N_AGENTS), torch.int8), z((N, N_AGENTS), torch.float32)
        self._pbuf = world.alloc_pilot_variants() if getattr(pilot, "variants", False) else world.alloc_pilot()
        self.batch_mode, self.max_seq_len = batch_mode, int(max_seq_len)
        self.record_logits = bool(record_logits)
        if self.record_logits:
            self.logits = z((T, N, N_AGENTS, L.CMD_LOGITS), torch.float32)
        self.episodes = None
        if batch_mode == "complete_episodes":
            cap = default_carry_cap(world.cfg.horizon, world.cfg.n_agents, world.cfg.n_opps) if carry_cap is None else int(carry_cap)
            self.episodes = CommanderEpisodeBatch({k: getattr(self, k) for k in EpisodeBatch.ROW_INPUTS + ("done", "state_in")},
                                                  self.max_seq_len, cap, self.gamma, self.lam,
                                                  aux=("logits", self.logits) if self.record_logits else None, metrics=bool(metrics),
                                                  train_batch_size=train_batch_size)
        self.window_metrics = None          # window_metrics_keyword puts a rollout.WindowMetrics here
        self.outcome = None                 # outcomes_keyword puts the tapped window here
        self.use_graph = use_graph
        self._graph = None
        self._started = False
        self.collects = 0                   # collects so far: the window buffers hold a batch once it is non-zero

    def _own_pilot(self):
        from .pilots import NetPilot, VariantNetPilot
        return isinstance(self.pilot, (NetPilot, VariantNetPilot))

    def start(self):
        """reset every arena (the first observation becomes row 0 of the next collect) and mark every arena fresh"""
        self.w.reset(obs=self.obs[self.T])
        self._fresh.fill_(1)
        self.state_in[self.T].zero_()
        if self.episodes is not None:
            self.episodes.reset()
        if self.window_metrics is not None:
            self.window_metrics.reset()
        self._started = True

    def _run(self):
        from .env_hier import macro_step
        T, w = self.T, self.w
        self.obs[0].copy_(self.obs[T])           # where the previous collect (or start) left every arena
        self.state_in[0].copy_(self.state_in[T])
        for t in range(T):
            fresh = self._fresh if t == 0 else self.done[t - 1]
            self.net.sample(self.obs[t], self.state_in[t], self.state_in[t + 1], fresh=fresh, world=w, actions=self.actions[t],
                            logp=self.logp[t], vf=self.vf[t], logits=self.logits[t] if self.record_logits else None)
            macro_step(w, self.actions[t], self.pilot, out=(self.obs[t + 1], self.reward[t], self.valid[t], self.done[t]),
                       pilot_buf=self._pbuf, early_exit=False)
            if self.outcome is not None:
                w.outcome_tap(self.done[t], self.outcome[t])
        # the bootstrap value of every arena's unfinished tail; its state_out goes to scratch (the carried state does not advance), arenas
        # that just finished are evaluated from zero state (their value is cut by the recursion and never read)
        self.net.sample(self.obs[T], self.state_in[T], self._h_scratch, fresh=self.done[T - 1], greedy=True, actions=self._tmp_act,
                        logp=self._tmp_logp, vf=self.vf[T])
        self._fresh.copy_(self.done[T - 1])
        st = C.c_void_p(torch.cuda.current_stream(w.device).cuda_stream)
        L.check(L.lib().hh_gae_rllib(T, w.N, N_AGENTS, C.c_void_p(self.reward.data_ptr()), C.c_void_p(self.vf.data_ptr()),
                                     C.c_void_p(self.done.data_ptr()), self.gamma, self.lam, C.c_void_p(self.adv.data_ptr()),
                                     C.c_void_p(self.target.data_ptr()), st))
        if self.window_metrics is not None:
            self.window_metrics.enqueue(st)
        if self.episodes is not None:
            self.episodes.emit(st)

    def _warm(self):
        """first launches of every kernel outside a capture"""
        dev = self.w.device
        nw = min(64, self.pilot.bank.max_rows)
        self.pilot.bank.act(torch.zeros((nw, 30), device=dev), torch.zeros((nw,), dtype=torch.uint8, device=dev))
        h = torch.zeros_like(self._h_scratch)
        self.net.sample(self.obs[self.T], h, self._h_scratch, greedy=True, actions=self._tmp_act, logp=self._tmp_logp)

    def collect(self):
        """T commander steps of every arena -> self (the buffers above); no host synchronisation"""
        if not self._started:
            self.start()
        if not (self.use_graph and self._own_pilot()):
            self._run()
            self.collects += 1
            return self
        # the captured graph holds device pointers by value: the world's (trace ring, bound bank's row lists), the pilot bank's (weight blobs,
        # selector table, the kernel instance its tile width picks) and the commander's — re-capture whenever World.trace_enable / bind_policy or
        # PolicyBank.set_net / set_critic / set_lut / set_tile_rows / close changed them since (CommanderNet.set_weights rewrites its weights
        # in place: the same addresses)
        gen = (getattr(self.w, "ptr_generation", 0), id(self.pilot.bank), getattr(self.pilot.bank, "generation", 0), id(self.net), self.net.h.value)
        if self._graph is not None and self._graph_gen != gen:
            self._graph = None
        if self._graph is None:
            dev = self.w.device
            self._warm()
            torch.cuda.synchronize(dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    self._run()
            torch.cuda.current_stream(dev).wait_stream(side)
            self._graph, self._graph_gen = graph, gen
        self._graph.replay()
        self.collects += 1
        return self

    def collect_batch(self, max_collects=None):
        """train_batch_size only: collect() until `episodes.ready()` (one small synchronising read per collect), at most max_collects
        times (None: no limit; `episodes.ready()` tells afterwards whether the batch is complete) -> self"""
        collect_until_ready(self, max_collects)
        return self

    # ---- checkpointing (hhmarl_2d_amd/checkpoint.py)
    def _window_names(self):
        return (("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target", "state_in", "_fresh")
                + (("logits",) if self.record_logits else ()) + rollout_outcome_names(self)[0])

    def _options(self):
        return dict({"T": self.T, "N": self.w.N, "gamma": self.gamma, "lam": self.lam, "batch_mode": self.batch_mode,
                     "max_seq_len": self.max_seq_len, "record_logits": self.record_logits}, **rollout_outcome_names(self)[1])

    def state_dict(self):
        """the window buffers of the last collect with the GRU states (state_in[T] and obs[T] / vf[T] are the hand-over of the next one),
        the episode-start flags, `collects`, `_started` and the CommanderEpisodeBatch; the world, the commander and the pilots' bank are
        saved by themselves.  The captured graph is not saved.  Synchronises the device."""
        return rollout_state_dict(self, self._window_names(), self._options())

    def _load_plan(self, sd):
        return rollout_load_plan(self, sd, self._window_names(), self._options())

    def load_state_dict(self, sd):
        """state_dict()'s dict back in place; validated first (ValueError names the field, nothing changed)"""
        self._load_plan(sd)()

    def critic_rows(self, agent):
        """the flattened CUR_OBS rows of `agent` (1..3) for the T collected steps with the actions filled in (central_critic_rows_hl)"""
        return central_critic_rows_hl(self.obs[: self.T], self.actions, agent)
