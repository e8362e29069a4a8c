"""Rollout post-processing next to the environment: the centralised-critic input
packing of train_hetero.py:113-181 and GAE (train_hetero.py:216) on device tensors."""
import ctypes as C
import functools
import inspect
import numbers

import torch

from . import _lib as L
from . import checkpoint as ck

ACTION_DIM_AC1, ACTION_DIM_AC2 = 4, 3


def _p(t):
    return C.c_void_p(t.data_ptr())


def gae(reward, value, valid, done, gamma=0.99, lam=0.95):
    """reward, valid [T,N,nA]; value [T+1,N,nA]; done [T,N] (device tensors) -> (advantages, returns)"""
    T, N, nA = reward.shape
    assert value.shape == (T + 1, N, nA) and valid.shape == reward.shape and done.shape == (T, N)
    reward, value = reward.contiguous().float(), value.contiguous().float()
    valid, done = valid.contiguous().to(torch.uint8), done.contiguous().to(torch.uint8)
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    st = C.c_void_p(torch.cuda.current_stream(reward.device).cuda_stream)
    L.check(L.lib().hh_gae(T, N, nA, _p(reward), _p(value), _p(valid), _p(done), float(gamma), float(lam), _p(adv), _p(ret), st))
    return adv, ret


def gae_rllib(reward, value, done, gamma=0.99, lam=0.95):
    """Advantages / value targets the way RLlib 2.4 computes them for the reference's step stream (hh_gae_rllib): rows of agents
    without a reward key stay in with reward 0.0 (nothing is masked), last_r = 0.0 at every episode end, float64 discounted sum.
    train_hetero.py:216 uses lam = 0.95, train_hier.py:186 RLlib's default lam = 1.0.
    reward [T,N,nA] (0.0 where the world reported reward_valid = 0); value [T+1,N,nA]; done [T,N] -> (advantages, value targets)"""
    T, N, nA = reward.shape
    assert value.shape == (T + 1, N, nA) and done.shape == (T, N)
    reward, value = reward.contiguous().float(), value.contiguous().float()
    done = done.contiguous().to(torch.uint8)
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    st = C.c_void_p(torch.cuda.current_stream(reward.device).cuda_stream)
    L.check(L.lib().hh_gae_rllib(T, N, nA, _p(reward), _p(value), _p(done), float(gamma), float(lam), _p(adv), _p(ret), st))
    return adv, ret


def central_critic_inputs(obs, actions):
    """The four blocks the reference's centralised critic sees per agent (central_critic_observer +
    on_postprocess_trajectory, train_hetero.py:113-181), for the 2-vs-2 low-level setting:
      agent 1: obs_1_own = obs[1] (26|30), obs_2 = obs[2] (24|29), act_1_own = own action (4), act_2 = friend's (3)
      agent 2: obs_1_own = obs[2],         obs_2 = obs[1],          act_1_own = own (3),        act_2 = friend's (4)
    with the heading / speed components scaled by 1/12 and 1/8 (train_hetero.py:143-160).
    obs [..., 2, D] (zero padded rows as the world emits them), actions int8 [..., 2, 4].
    Returns a dict per agent of float32 tensors with the reference's widths."""
    d1 = obs.shape[-1]
    d2 = d1 - 2 if d1 == 26 else d1 - 1          # 26/24 fight, 30/29 escape
    # the reference divides the integer actions in float64 and stores into the float32 batch (train_hetero.py:143-160): the same here
    # on any device (a float32 division on the GPU is not correctly rounded in every PyTorch build, the float64 one is)
    a = actions.double()
    scaled = torch.stack([a[..., 0] / 12.0, a[..., 1] / 8.0, a[..., 2], a[..., 3]], dim=-1).float()
    o1, o2 = obs[..., 0, :d1], obs[..., 1, :d2]
    a1, a2 = scaled[..., 0, :ACTION_DIM_AC1], scaled[..., 1, :ACTION_DIM_AC2]
    return {1: {"obs_1_own": o1, "obs_2": o2, "act_1_own": a1, "act_2": a2},
            2: {"obs_1_own": o2, "obs_2": o1, "act_1_own": a2, "act_2": a1}}


def central_critic_rows(obs, actions, agent):
    """The flattened CUR_OBS rows the reference's critic is trained on, for the 2-vs-2 low-level setting: RLlib flattens the
    observer's Dict in sorted key order (act_1_own, act_2, obs_1_own, obs_2) and `on_postprocess_trajectory`
    (train_hetero.py:120-160) then writes the own and the friend's actions into the first 7 columns, heading / speed components
    scaled by 1/12 and 1/8.  Agent 1 (type 1): [own act 4 | friend act 3 | own obs 26|30 | friend obs 24|29]; agent 2 (type 2):
    [own act 3 | friend act 4 | own obs 24|29 | friend obs 26|30].  obs [..., 2, D] as the world emits it (zero padded), actions
    int8 [..., 2, 4] -> float32 [..., 57] (fight) / [..., 66] (escape).  Pinned by tests/golden/critic_packing.npz (recorded
    from the reference's own callbacks)."""
    c = central_critic_inputs(obs, actions)[agent]
    return torch.cat([c["act_1_own"], c["act_2"], c["obs_1_own"], c["obs_2"]], dim=-1).float()


def central_critic_rows_hl(obs, actions, agent):
    """train_hier.py:100-165 for the 3-vs-3 commander: sorted keys (act_1_own, act_2, act_3, obs_1_own, obs_2, obs_3); the own
    action and the other two agents' actions (ascending id) divided by N_OPP_HL = 2 in columns 0..2.  obs [..., 3, 34],
    actions int8 [..., 3] -> float32 [..., 105]."""
    others = [i for i in (1, 2, 3) if i != agent]
    order = [agent] + others
    a = torch.stack([actions[..., i - 1].double() / 2.0 for i in order], dim=-1).float()
    return torch.cat([a] + [obs[..., i - 1, :].float() for i in order], dim=-1)


def episode_segments(done):
    """batch_mode="complete_episodes" (train_hetero.py:212) on the [T, N] done flags of a rollout with auto-reset:
    -> (segment id per row [T, N], starting at 0 per arena and increasing after every done row;
        complete [T, N] bool: the row belongs to an episode that also ENDS inside this rollout — the rows RLlib would train on;
        the trailing fragment of every arena is carried into the next rollout instead)"""
    d = done.to(torch.int64)
    seg = torch.cumsum(d, dim=0) - d                     # episodes finished strictly before this row
    n_done = d.sum(dim=0, keepdim=True)                  # episodes that end inside the rollout, per arena
    return seg, seg < n_done


def collect_until_ready(rollout, max_collects=None):
    """what the rollouts' collect_batch() does: rollout.collect() until rollout.episodes.ready(), at most max_collects times"""
    if rollout.episodes is None or rollout.episodes.train_batch_size is None:
        raise RuntimeError(f"{type(rollout).__name__}.collect_batch(): built without train_batch_size")
    if max_collects is not None and int(max_collects) < 1:
        raise ValueError("max_collects: None or at least 1")
    n = 0
    while True:
        rollout.collect()
        n += 1
        if rollout.episodes.ready() or (max_collects is not None and n >= int(max_collects)):
            return n


def metrics_dict(s, totals, agent_keys):
    """a summary block (list of len(_lib.EP_METRICS) floats: hh_episodes_metrics' / hh_window_metrics' slots) and the totals [2] under
    RLlib's result names: what EpisodeBatch.metrics() and WindowMetrics.metrics() return"""
    slot = L.EP_METRICS_SLOT
    per_agent = lambda name: {k: s[slot[name + "_0"] + a] for a, k in enumerate(agent_keys)}
    out = {k: s[slot[k]] for k in ("episode_reward_mean", "episode_reward_min", "episode_reward_max", "episode_len_mean", "episode_len_min",
                                   "episode_len_max")}
    out.update(episodes_this_iter=int(s[slot["episodes"]]), timesteps_this_iter=int(s[slot["rows"]]),
               policy_reward_mean=per_agent("agent_return_mean"), policy_reward_min=per_agent("agent_return_min"),
               policy_reward_max=per_agent("agent_return_max"), vf_explained_var=per_agent("vf_explained_var"),
               episodes_total=int(totals[0]), timesteps_total=int(totals[1]))
    return out


OUTCOME_CLASSES = ("win", "lose", "draw")   # hh_episode_outcomes' classes in slot order: codes 1, -1, 0


def outcome_metrics(s):
    """hh_episode_outcomes' summary (list of len(_lib.EO_SUMMARY) floats) under the names of evaluation.LOWLEVEL_STAT_KEYS /
    LowLevelEvaluator.metrics: what `metrics()` gains with outcomes=True"""
    n, counts = int(s[0]), [int(c) for c in s[1:4]]
    return {"agents_win": counts[0], "opps_win": counts[1], "draw": counts[2],
            "outcome_pct": {k: (c / n) * 100 if n else float("nan") for k, c in zip(OUTCOME_CLASSES, counts)},
            "episode_reward_mean_by_outcome": dict(zip(OUTCOME_CLASSES, s[4:7])),
            "episode_len_mean_by_outcome": dict(zip(OUTCOME_CLASSES, s[7:10]))}


class EpisodeOutcomes:
    """Win / lose / draw of an episode table (hh_episode_outcomes, include/hh_abi.h: two launches right behind the table's own, no
    host synchronisation): what `EpisodeBatch` and `WindowMetrics` own when their rollout was built with outcomes=True.
    `ep_outcome` i8 [ep_cap] (1 agents win, -1 opponents win, 0 draw: entry e is the outcome of the table's episode e; the call writes
    the window's segment only, the table's last), `summary` f64 [len(_lib.EO_SUMMARY)] over every entry of the table so far, `flags` i32
    [2] (the table did not hold this window's episodes; the window's done rows)."""

    def __init__(self, done, outcome, n_episodes, ep_arena, ep_len, ep_return):
        """done u8 / outcome i8 [T, N]: the rollout's window; n_episodes: a 0-d i32 view of the table's device count; ep_arena / ep_len
        i32 [E], ep_return f64 [E, n_agents]: the table"""
        T, N = done.shape
        E, nA = ep_return.shape
        dev = done.device
        if tuple(outcome.shape) != (T, N) or outcome.dtype != torch.int8 or not outcome.is_contiguous():
            raise ValueError(f"outcomes: outcome must be a contiguous int8 tensor of shape {(T, N)}")
        nbytes = C.c_int64(0)
        L.check(L.lib().hh_episode_outcomes_scratch_bytes(T, N, E, C.byref(nbytes)))
        self.ep_outcome = torch.full((E,), L.OUTCOME_NONE, dtype=torch.int8, device=dev)
        self.summary = torch.zeros((len(L.EO_SUMMARY),), dtype=torch.float64, device=dev)
        self.flags = torch.zeros((2,), dtype=torch.int32, device=dev)
        self._scratch = torch.zeros((nbytes.value // 8,), dtype=torch.float64, device=dev)
        self._keep = (done, outcome, n_episodes, ep_arena, ep_len, ep_return)   # the struct holds raw pointers: keep the tensors alive
        self._bufs = L.HHEpisodeOutcomeBufs(
            T=T, N=N, n_agents=nA, reserved0=0, ep_cap=E, done=done.data_ptr(), outcome=outcome.data_ptr(), n_episodes=n_episodes.data_ptr(),
            ep_arena=ep_arena.data_ptr(), ep_len=ep_len.data_ptr(), ep_return=ep_return.data_ptr(), ep_outcome=self.ep_outcome.data_ptr(),
            summary=self.summary.data_ptr(), flags=self.flags.data_ptr(), scratch=self._scratch.data_ptr(), scratch_bytes=nbytes.value)
        self.reset()

    def reset(self):
        """the summary of an empty table (0 episodes, counts 0, nan means) and clear flags, until the next collect"""
        self.summary.zero_()
        self.summary[4:10] = float("nan")
        self.flags.zero_()

    def enqueue(self, stream):
        L.check(L.lib().hh_episode_outcomes(C.byref(self._bufs), stream))

    def whole(self):
        """the small tensors a state_dict saves whole (ep_outcome is saved with the table, cut to its count)"""
        return {"outcome_summary": self.summary, "outcome_flags": self.flags}

    @staticmethod
    def failed(summary, flags):
        """host copies -> did the table not hold a window's episodes, or does an entry carry no outcome?"""
        return bool(flags[0]) or summary[L.EO_SUMMARY.index("other_codes")] != 0


class EpisodeBatch:
    """The whole-episode batch of a `PPORollout(..., batch_mode="complete_episodes")` (train_hetero.py:212): after every collect, the rows
    of every episode that ENDED in it, from its reset row to its done row, in one flat batch — the episode's earlier rows come from a
    per-arena carry that holds the running episode on the device across collects — with advantages / value targets computed over the
    whole episode (hh_gae_rllib's float64 recursion with last_r = 0.0 after the done row: oracle/gae_ref.compute_advantages on each
    episode).  Written by hh_episodes_emit (include/hh_abi.h) inside the collect's graph; no host synchronisation until `rows()`.

    Device buffers of fixed capacity, overwritten by every collect (the first n_rows rows / n_episodes episodes are valid), in the order
    arena-major, then episode, then time:
      obs f32 [R, 2, D], actions i8 [R, 2, 4], logp / vf / reward f32 [R, 2], valid u8 [R, 2], adv / target f32 [R, 2],
      done u8 [R] (1 on an episode's last row only), arena / episode / t i32 [R] (`episode` counts per arena from `start()`, `t` is the
      step within the episode from 0); episode table ep_start / ep_len / ep_arena i32 [E]; n_rows / n_episodes (0-d i32 views of the
      device counts); carried i32 [N] (rows of each arena's running episode held for a later collect).
    Capacity, with H = world.cfg.horizon (an episode has at most H rows): the carry holds N (H - 1) rows, the batch R = N (H - 1 + T)
    rows and E = N T episodes — for two agents about (H - 1) (8 D + 26) + (H - 1 + T) (8 D + 47) + 12 T bytes per arena (N = 16384,
    H = 300, T = 64, fight D = 26: 1.17 GB of carry, 1.60 GB of batch).  Nothing overflows under that rule; if something did anyway, a
    sticky device flag is set and `rows()` raises.

    aux = (name, tensor): one more per-agent float column of the collect, f32 [T, N, n_agents, d] with 1 <= d <= 32, that travels with the
    rows (hh_episodes_emit_aux): through the carry, into the batch `name` f32 [R, n_agents, d] in the same row order, bit for bit, and
    into `rows()` under that name.  PPORollout(record_logits=True) puts the sampler's logits there (name "logits", d = 32: RLlib's
    ACTION_DIST_INPUTS).  It costs 4 n_agents d bytes per row of the carry and of the batch: 256 B for the logits, next to the 8 D + 47
    of the other columns (N = 16384, H = 300, T = 64: 1.25 GB more carry, 1.52 GB more batch).

    metrics = True: RLlib's per-iteration episode metrics of every emitted batch, computed on the device right behind the emitter
    (hh_episodes_metrics, include/hh_abi.h: three more launches in the collect's graph, float64, fixed summation order): `ep_return` f64
    [E, n_agents] (every episode's per-agent reward sum; also in `rows()`), a summary block and running totals.  `metrics()` copies the
    summary and the totals to the host (a few hundred bytes, one synchronisation) and names them as RLlib's result dict does;
    `metrics_device()` hands out the device tensors without synchronising.  `reset()` zeroes the totals.  Two differences from RLlib:
    the means / min / max are over the episodes emitted by THIS collect (RLlib smooths over the last 100 episodes; here a collect
    without a finished episode reports nan), and `vf_explained_var` is that of the sampler's VF_PREDS (the `vf` column: zero action
    inputs) against the value targets, not of the learner's re-evaluation with the actions filled in.  `timesteps_total` counts
    environment steps (rows), not agent steps.  With the default False nothing is allocated and the launches, the graph and `rows()`
    are what they were.

    train_batch_size = B (an int >= 1; RLlib's knob of that name, train_hetero.py:216 `args.batch_size`): the collects are no longer
    overwritten but ACCUMULATED on the device until the batch holds at least B rows (environment steps) — whole collects, nothing
    trimmed, as RLlib's training_step concatenates whole sample batches.  hh_episodes_emit_append (include/hh_abi.h) appends in place:
    the same four launches in the collect's graph, no copy, no second batch, no host synchronisation; the order is collect-major, then
    arena, episode, time, and ep_start (the commander's seq_start / seq_ep too) are positions in the accumulated batch.  `rows()`,
    `critic_rows()`, `n_rows`, `n_episodes` describe the batch so far; `ready()` tells whether it has reached B, `batch_info()` its
    counts; the collect after a complete batch starts the next one by itself (read `rows()` before it), `clear()` discards a partial
    one.  With metrics=True, `metrics()` is RLlib's line for the iteration's batch so far (episodes_this_iter and the means over
    every episode accumulated), while episodes_total / timesteps_total count every episode and row once.
    Capacity: a batch was below B before its last collect, so R = B - 1 + N (H - 1 + T) rows and E = B - 1 + N T episodes (both must
    stay below 2^31); the carry is unchanged.  For two agents 8 D + 47 bytes per row and 12 per episode (with the logits 256 more per
    row): B = 4 collects' worth of rows at N = 16384, T = 64, fight D = 26 (B = 4194304) is 1.07 GB of rows and 50 MB of episode table
    more than without.  With the default None everything is what it was: the same entry point, allocations and graph.

    outcomes (the rollouts' keyword-only outcomes=True, with metrics=True; `attach_outcomes`): the batch also owns an `EpisodeOutcomes`
    over its episode table — `ep_outcome` i8 [E], entry e the outcome of episode e (1 agents win, -1 opponents win, 0 draw), in `rows()`
    and `metrics_device()` — filled by hh_episode_outcomes right behind the metrics (two more launches), and `metrics()` gains
    agents_win / opps_win / draw (ints: evaluation.LOWLEVEL_STAT_KEYS' names), outcome_pct = {win, lose, draw} ((count / episodes) *
    100 as LowLevelEvaluator.metrics computes it; nan with 0 episodes), episode_reward_mean_by_outcome and episode_len_mean_by_outcome
    (dicts over win / lose / draw; nan for a class without an episode) — over the batch so far, as the other keys.  The caller adds the
    counts across iterations and ranks.  Without it, nothing is allocated and every key set is what it was."""

    COLUMNS = ("obs", "actions", "logp", "vf", "reward", "valid", "adv", "target", "done", "arena", "episode", "t")
    TABLES = ("ep_start", "ep_len", "ep_arena")
    ROW_INPUTS = ("obs", "actions", "logp", "vf", "reward", "valid")   # the collect's columns the rows carry (and the carry holds)
    _EMIT, _SCRATCH, _N_COUNTS = "hh_episodes_emit", (5, 0), 3       # entry point; scratch i32 [5 N + 0]; counts
    _critic_rows = staticmethod(central_critic_rows)
    AGENT_KEYS = ("ac1_policy", "ac2_policy")   # metrics(): the keys of the per-agent entries (RLlib's policy ids in train_hetero.py)

    @classmethod
    def check_aux(cls, aux, T, N, n_agents, device):
        """aux = (name, tensor) as the constructor takes it -> (name, tensor), or ValueError"""
        if not (isinstance(aux, (tuple, list)) and len(aux) == 2 and isinstance(aux[0], str) and isinstance(aux[1], torch.Tensor)):
            raise ValueError("aux: a (name, tensor) pair, e.g. ('logits', f32 [T, N, n_agents, 32])")
        name, t = aux
        taken = set(cls.COLUMNS) | set(cls.TABLES) | set(getattr(cls, "SEQ_TABLE", ())) | {"state_in", "carried", "n_rows", "n_episodes", "n_sequences", "ep_return"}
        if not name.isidentifier() or name.startswith("_") or name in taken or hasattr(cls, name):
            raise ValueError(f"aux: the name {name!r} is not a free column name")
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise ValueError(f"aux: {name} must be a contiguous float32 tensor on {device}")
        if t.dim() != 4 or tuple(t.shape[:3]) != (T, N, n_agents) or not 1 <= t.shape[3] <= L.EP_AUX_MAX_DIM:
            raise ValueError(f"aux: {name} must be [T, N, n_agents, d] = [{T}, {N}, {n_agents}, 1 .. {L.EP_AUX_MAX_DIM}], got {tuple(t.shape)}")
        return name, t

    @staticmethod
    def check_train_batch_size(train_batch_size):
        """train_batch_size as the constructors take it -> None or the int, or ValueError"""
        B = train_batch_size
        if B is None:
            return None
        if isinstance(B, bool) or not isinstance(B, numbers.Integral) or B < 1:
            raise ValueError(f"train_batch_size: None (every collect is its own batch) or an int >= 1 (rows to accumulate), got {B!r}")
        return int(B)

    @classmethod
    def capacities(cls, N, T, carry_cap, train_batch_size=None):
        """-> (R rows, E episodes) of the batch buffers: N (carry_cap + T) and N T, with train_batch_size = B each B - 1 more (a batch was
        below B before its last collect); ValueError for a B whose capacities reach 2^31"""
        B = cls.check_train_batch_size(train_batch_size)
        more = 0 if B is None else B - 1
        R, E = more + int(N) * (int(carry_cap) + int(T)), more + int(N) * int(T)
        if B is not None and max(R, E) >= 2 ** 31:
            raise ValueError(f"train_batch_size = {B}: the capacities ({R} rows, {E} episodes) must stay below 2^31")
        return R, E

    def __init__(self, collect, carry_cap, gamma, lam, aux=None, metrics=False, train_batch_size=None):
        """collect: the rollout's [T(+1), N, ...] buffers (ROW_INPUTS and done) that every emission reads; every row column of the batch and
        of the carry takes its per-row shape and dtype from the collect's.  carry_cap: rows the carry holds per arena (horizon - 1).
        aux: None, or (name, f32 [T, N, n_agents, d]) — one more column that travels with the rows (see the class).
        metrics: also compute the episode metrics of every emitted batch on the device (see the class).
        train_batch_size: None, or the rows to accumulate before a batch is complete (see the class)."""
        T, N = collect["done"].shape
        self.N, self.T, self.carry_cap = int(N), int(T), int(carry_cap)
        self.n_agents, self.D = int(collect["obs"].shape[2]), int(collect["obs"].shape[-1])
        self._device = collect["done"].device
        self.aux_name, self._aux = None, None
        if aux is not None:
            self.aux_name, aux_t = self.check_aux(aux, self.T, self.N, self.n_agents, self._device)
        self.train_batch_size = self.check_train_batch_size(train_batch_size)
        N, T, cap = self.N, self.T, max(self.carry_cap, 1)
        R, E = self._capacities()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self._device)
        i32 = torch.int32
        self._carry = {}
        for k in self.ROW_INPUTS:
            row, dt = tuple(collect[k].shape[2:]), collect[k].dtype
            setattr(self, k, z((R,) + row, dt))
            self._carry[k] = z((N, cap) + row, dt)
        self.adv, self.target = z(self.reward.shape, torch.float32), z(self.reward.shape, torch.float32)
        self.done, self.arena, self.episode, self.t = z((R,), torch.uint8), z((R,), i32), z((R,), i32), z((R,), i32)
        for k in self.TABLES:
            setattr(self, k, z((E,), i32))
        self.carried = z((N,), i32)
        self._finished = z((N,), i32)            # episodes finished per arena since start()
        self._scratch = z((self._SCRATCH[0] * N + self._SCRATCH[1],), i32)
        self._counts = z((self._N_COUNTS,), i32)  # rows, episodes of the last collect; overflow flag (sticky)[; sequences of the last collect]
        # train_batch_size: the accumulator of hh_episodes_emit_append (_lib.EP_ACC: the counts' slots describe the batch so far)
        self._acc = z((len(L.EP_ACC),), i32) if self.train_batch_size is not None else None
        self._size = self._counts if self._acc is None else self._acc   # what rows() is cut to
        self.n_rows, self.n_episodes = self._size[0], self._size[1]
        b = self._struct(R, E, float(gamma), float(lam))
        self._bufs, self._collect = b, collect   # the struct holds raw pointers: keep the tensors alive
        self._bind(collect, self._carry, ("done",) + self.ROW_INPUTS, self.COLUMNS, self.TABLES)
        b.carried, b.episode, b.scratch, b.counts = (x.data_ptr() for x in (self.carried, self._finished, self._scratch, self._counts))
        if self.aux_name is not None:
            row = tuple(aux_t.shape[2:])
            setattr(self, self.aux_name, z((R,) + row, torch.float32))
            self._carry[self.aux_name] = z((N, cap) + row, torch.float32)
            self._aux_collect = aux_t            # the struct holds raw pointers: keep the tensor alive
            self._aux = L.HHEpisodeAux(aux_dim=row[1], reserved0=0, aux=aux_t.data_ptr(), c_aux=self._carry[self.aux_name].data_ptr(),
                                       o_aux=getattr(self, self.aux_name).data_ptr())
        self._metrics = None
        if metrics:
            if not 1 <= self.n_agents <= L.EP_METRICS_MAX_AGENTS or len(self.AGENT_KEYS) != self.n_agents:
                raise ValueError(f"metrics: {type(self).__name__} names {len(self.AGENT_KEYS)} agents, the collect has {self.n_agents}")
            nbytes = C.c_int64(0)
            L.check(L.lib().hh_episodes_metrics_scratch_bytes(E, R, self.n_agents, C.byref(nbytes)))
            self.ep_return = z((E, self.n_agents), torch.float64)
            self._summary = torch.full((len(L.EP_METRICS),), float("nan"), dtype=torch.float64, device=self._device)
            self._summary[:2] = 0.0                  # no collect yet: what a collect without a finished episode leaves
            self._totals = z((2,), torch.int64)      # episodes_total, timesteps_total since start() / reset()
            self._m_scratch = z((nbytes.value // 8,), torch.float64)
            self._m_host = None                      # pinned host copies (summary, totals, counts[, acc]), made by the first metrics()
            # accumulating: the metrics are taken over the batch so far (acc in place of the counts) and would count its earlier collects
            # again — their totals go to a throwaway, the real ones come from the emitter, every episode and row once
            self._m_totals = self._totals if self._acc is None else z((2,), torch.int64)
            self._metrics = L.HHEpisodeMetricsBufs(
                n_agents=self.n_agents, reserved0=0, row_cap=R, ep_cap=E, reward=self.reward.data_ptr(), vf=self.vf.data_ptr(),
                target=self.target.data_ptr(), ep_start=self.ep_start.data_ptr(), ep_len=self.ep_len.data_ptr(), counts=self._size.data_ptr(),
                ep_return=self.ep_return.data_ptr(), summary=self._summary.data_ptr(), totals=self._m_totals.data_ptr(),
                scratch=self._m_scratch.data_ptr(), scratch_bytes=nbytes.value)
        self._outcomes = None                    # attach_outcomes puts an EpisodeOutcomes here

    def attach_outcomes(self, outcome):
        """outcome i8 [T, N]: the rollout's tapped window (World.outcome_tap behind every tick).  From now on every emission also fills
        `ep_outcome` and the outcomes' summary (see the class); needs metrics=True (the summary reads ep_return)."""
        if self._metrics is None:
            raise ValueError(f"{type(self).__name__}: outcomes need metrics=True (their summary reads the episodes' returns)")
        self._outcomes = EpisodeOutcomes(self._collect["done"], outcome, self.n_episodes, self.ep_arena, self.ep_len, self.ep_return)
        self.ep_outcome = self._outcomes.ep_outcome
        self._m_host = None

    def _capacities(self):
        """(R, E) of this batch; a subclass checks its own capacities here as well"""
        return self.capacities(self.N, self.T, self.carry_cap, self.train_batch_size)

    def _struct(self, R, E, gamma, lam):
        return L.HHEpisodeBufs(T=self.T, N=self.N, n_agents=self.n_agents, obs_dim=self.D, carry_cap=self.carry_cap, reserved0=0, row_cap=R,
                               ep_cap=E, gamma=gamma, lam=lam)

    def _bind(self, collect, carry, inputs, columns, tables):
        """the device pointers of the struct: collect inputs, carry columns (c_), batch columns (o_), tables"""
        b = self._bufs
        for k in inputs:
            assert collect[k].is_contiguous() and collect[k].shape[1] == self.N
            setattr(b, k, collect[k].data_ptr())
        for k, v in carry.items():
            setattr(b, "c_" + k, v.data_ptr())
        for k in columns:
            setattr(b, "o_" + k, getattr(self, k).data_ptr())
        for k in tables:
            setattr(b, k, getattr(self, k).data_ptr())

    def _parts(self):
        """(names, index in the counts of the length they are cut to) for rows()"""
        return ((self.COLUMNS + ((self.aux_name,) if self.aux_name else ()), 0),
                (self.TABLES + (("ep_return",) if self._metrics else ()) + (("ep_outcome",) if self._outcomes else ()), 1))

    def reset(self):
        """no episode spans a reset: the carry and the per-arena episode counters start again (the overflow flag stays); with metrics, the
        running totals start
        again and the summary is that of a collect without a finished episode (0 episodes, 0 rows, nan) until the next collect; with
        train_batch_size, the batch accumulated so far is discarded as well (the accumulator is zeroed)"""
        if self._metrics is not None:
            self._totals.zero_()
            self._summary.fill_(float("nan"))    # no collect since the reset: what a collect without a finished episode leaves
            self._summary[:2] = 0.0
        if self._outcomes is not None:
            self._outcomes.reset()
        self.carried.zero_()
        self._finished.zero_()
        self._counts[:2].zero_()
        self._counts[3:].zero_()
        if self._acc is not None:
            self._acc.zero_()

    def _accumulating(self, what):
        if self._acc is None:
            raise RuntimeError(f"{type(self).__name__}.{what}: built without train_batch_size")

    def ready(self):
        """train_batch_size only: has the batch reached train_batch_size rows?  One small synchronising read.  The next collect after a
        True starts the next batch: take `rows()` before it."""
        self._accumulating("ready()")
        return bool(self._acc[4].item())

    def batch_info(self):
        """train_batch_size only; synchronises -> dict of ints: rows, episodes, sequences (0 without a sequence table) of the batch so far,
        collects accumulated in it, batches completed before it (since reset() / clear())"""
        self._accumulating("batch_info()")
        a = dict(zip(L.EP_ACC, self._acc.tolist()))
        return {k: a[k] for k in ("rows", "episodes", "sequences", "collects", "batches")}

    def clear(self):
        """train_batch_size only: discard the batch so far, complete or not (a zeroing of the accumulator in the order of the current
        stream, no synchronisation): the next collect starts a batch at row 0.  The carry, the per-arena episode counters and the
        running totals are untouched — the running episodes go on, none of their rows is lost."""
        self._accumulating("clear()")
        self._acc.zero_()
        if self._metrics is not None:
            self._summary.fill_(float("nan"))    # an empty batch: what a collect without a finished episode leaves
            self._summary[:2] = 0.0
        if self._outcomes is not None:
            self._outcomes.reset()

    def emit(self, stream):
        aux = None if self._aux is None else C.byref(self._aux)
        if self._acc is not None:
            totals = self._totals.data_ptr() if self._metrics is not None else None
            L.check(getattr(L.lib(), self._EMIT + "_append")(C.byref(self._bufs), aux, self.train_batch_size, self._acc.data_ptr(), totals, stream))
        elif aux is None:
            L.check(getattr(L.lib(), self._EMIT)(C.byref(self._bufs), stream))
        else:
            L.check(getattr(L.lib(), self._EMIT + "_aux")(C.byref(self._bufs), aux, stream))
        if self._metrics is not None:
            self.enqueue_metrics(stream)
        if self._outcomes is not None:
            self._outcomes.enqueue(stream)

    def enqueue_metrics(self, stream):
        """hh_episodes_metrics over the batch as it stands, on `stream` (what emit() does right behind the emitter; a second call adds the
        batch to the totals again: tools/episode_metrics_timing.py times the launches with it and puts the totals back).  With
        train_batch_size the batch is the accumulated one and the totals are the emitter's: this call leaves them alone."""
        if self._metrics is None:
            raise RuntimeError(f"{type(self).__name__}: built without metrics=True")
        L.check(L.lib().hh_episodes_metrics(C.byref(self._metrics), stream))

    def _overflow(self):
        return RuntimeError(f"{type(self).__name__}: an episode outgrew the carry or a batch capacity (more rows than carry_cap + 1?): "
                            "the batches since that collect are incomplete")

    def metrics_device(self):
        """the device tensors of the last collect's metrics, without synchronising (for a loop that logs asynchronously): `summary` f64
        [len(_lib.EP_METRICS)] (slots: _lib.EP_METRICS_SLOT), `totals` i64 [2] (episodes_total, timesteps_total), `ep_return` f64 [E,
        n_agents] (the first n_episodes entries are valid).  Overwritten by the next collect."""
        if self._metrics is None:
            raise RuntimeError(f"{type(self).__name__}: built without metrics=True")
        out = {"summary": self._summary, "totals": self._totals, "ep_return": self.ep_return}
        if self._outcomes is not None:   # ep_outcome [E] like ep_return; outcome_summary: _lib.EO_SUMMARY's slots; outcome_flags i32 [2]
            out.update(ep_outcome=self.ep_outcome, **self._outcomes.whole())
        return out

    def metrics(self):
        """-> the last collect's metrics (with train_batch_size: the accumulated batch's so far) under RLlib's result names (see the class
        for the two differences); copies the summary, the totals and the counts to the host: one synchronisation of the current stream.
        Raises like `rows()` after an overflow.
        Keys: episode_reward_mean / _min / _max, episode_len_mean, episodes_this_iter, policy_reward_mean / _min / _max, vf_explained_var,
        episodes_total, timesteps_total (RLlib's), and from the same summary episode_len_min / _max and timesteps_this_iter (the batch's
        rows).  The per-agent entries (policy_reward_*, vf_explained_var) are dicts keyed by AGENT_KEYS.  After reset() / start() and
        before the next collect: 0 episodes, nan, totals 0.  With outcomes: also outcome_metrics' keys (see the class); a table that did not
        hold a window's episodes, or an entry without an outcome, raises the overflow error."""
        if self._metrics is None:
            raise RuntimeError(f"{type(self).__name__}: built without metrics=True")
        eo = () if self._outcomes is None else (self._outcomes.summary, self._outcomes.flags)
        src = eo + (self._summary, self._totals, self._counts) + (() if self._acc is None else (self._acc,))
        if self._m_host is None:
            self._m_host = tuple(torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in src)
        for h, d in zip(self._m_host, src):
            h.copy_(d, non_blocking=True)
        torch.cuda.current_stream(self._device).synchronize()
        host = [h.tolist() for h in self._m_host]
        s, totals, *flags = host[len(eo):]
        if any(f[2] for f in flags) or (eo and EpisodeOutcomes.failed(*host[:2])):
            raise self._overflow()
        out = metrics_dict(s, totals, self.AGENT_KEYS)
        if eo:
            out.update(outcome_metrics(host[0]))
        return out

    def rows(self):
        """synchronises; -> dict of views cut to the last collect (with train_batch_size: to the accumulated batch so far): the columns
        (COLUMNS), the episode table (TABLES) and a subclass's own parts (_parts)"""
        torch.cuda.synchronize(self._device)
        counts = self._size.tolist()
        if counts[2] or (self._acc is not None and int(self._counts[2])):
            raise self._overflow()
        return {k: getattr(self, k)[:counts[i]] for names, i in self._parts() for k in names}

    def critic_rows(self, agent):
        """the CUR_OBS rows of `agent` for the emitted rows with the actions filled in (central_critic_rows: agent 1 | 2)"""
        r = self.rows()
        return self._critic_rows(r["obs"], r["actions"], agent)

    # ---- checkpointing (hhmarl_2d_amd/checkpoint.py)
    def _options(self):
        """what a saved batch must share with the one it is loaded into"""
        o = {"N": self.N, "T": self.T, "carry_cap": self.carry_cap, "n_agents": self.n_agents, "D": self.D, "aux_name": self.aux_name,
             "train_batch_size": self.train_batch_size, "metrics": self._metrics is not None, "row_cap": int(self._bufs.row_cap),
             "ep_cap": int(self._bufs.ep_cap), "gamma": float(self._bufs.gamma), "lam": float(self._bufs.lam)}
        if self._outcomes is not None:
            o["outcomes"] = True
        return o

    def _whole(self):
        """the small tensors saved whole: per-arena counts, the emitter's counts, the accumulator, the metrics' summary and totals"""
        t = {"carried": self.carried, "finished": self._finished, "counts": self._counts}
        if self._acc is not None:
            t["acc"] = self._acc
        if self._metrics is not None:
            t.update(summary=self._summary, totals=self._totals)
            if self._m_totals is not self._totals:
                t["m_totals"] = self._m_totals
        if self._outcomes is not None:
            t.update(self._outcomes.whole())
        return t

    def _carry_lead(self, k, m):
        """entries per arena of carry column k that a carry of at most m rows uses"""
        return m

    def state_dict(self):
        """The carry (cut to the longest running episode: rows beyond an arena's `carried` are never read), the per-arena counts, the
        emitter's counts and the accumulator, the batch's columns and tables cut to what they hold (`rows()`'s cut: with
        train_batch_size the batch accumulated so far), the metrics' summary and running totals, the aux column with the rest.  Scratch
        is not saved.  Synchronises the device."""
        torch.cuda.synchronize(self._device)
        size = self._size.tolist()
        m = int(self.carried.max().item()) if self.N else 0
        return {"options": self._options(), "state": {k: ck.cpu(v) for k, v in self._whole().items()}, "carry_rows": m,
                "carry": {k: ck.cpu(v[:, :self._carry_lead(k, m)]) for k, v in self._carry.items()},
                "batch": {k: ck.cpu(getattr(self, k)[:size[i]]) for names, i in self._parts() for k in names}}

    def _load_plan(self, sd):
        who = type(self).__name__
        ck.need_keys(who, sd, ("options", "state", "carry_rows", "carry", "batch"))
        ck.check_options(who, sd["options"], self._options())
        pairs = ck.plan_tensors(who, sd["state"], self._whole())
        m = sd["carry_rows"]
        if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= max(self.carry_cap, 1):
            raise ValueError(f"{who}: `carry_rows` is {m!r}, the carry holds 0 .. {max(self.carry_cap, 1)} rows per arena")
        ck.need_keys(who + " carry", sd["carry"], tuple(self._carry))
        for k, dst in self._carry.items():
            view = dst[:, :self._carry_lead(k, m)]      # [N, the entries in use, ...]
            ck.check_tensor(who, "carry." + k, sd["carry"][k], view)
            pairs.append((view, sd["carry"][k]))
        size = sd["state"]["acc" if self._acc is not None else "counts"].tolist()
        parts = self._parts()
        ck.need_keys(who + " batch", sd["batch"], tuple(k for names, _ in parts for k in names))
        for names, i in parts:
            for k in names:
                ck.check_tensor(who, "batch." + k, sd["batch"][k], getattr(self, k), lead=size[i])
                pairs.append((getattr(self, k)[:size[i]], sd["batch"][k]))
        return lambda: ck.copy_pairs(pairs)

    def load_state_dict(self, sd):
        """state_dict()'s dict back, in place (every device address stays): everything is validated first — the recorded capacities and
        options against this batch's, every tensor's dtype and shape — ValueError names the field and nothing was changed"""
        self._load_plan(sd)()


class WindowMetrics:
    """RLlib's per-iteration episode metrics of a rollout in batch_mode = "truncate_episodes" (`PPORollout(..., window_metrics=True)`,
    `CommanderRollout(..., window_metrics=True)`): the training curve of a run that trains from fixed [T, N] windows
    (`update_window`), without the carry and the second batch of "complete_episodes".  A window cuts episodes, so a small per-arena
    state lives on the device across collects — `run_return` f64 [N, n_agents] and `run_len` i32 [N], the return and the rows so far of
    every arena's running episode — and hh_window_metrics (include/hh_abi.h: five launches in the collect's graph right behind the GAE,
    float64, one sequential addition per row, no atomics, no host synchronisation) tabulates the episodes that finish inside each
    window, their rows of earlier windows included, and summarises them under the names of `EpisodeBatch.metrics()`.

    Device buffers, overwritten by every collect (the first n_episodes entries are valid; arena-major, then t): `ep_return` f64 [T N,
    n_agents], `ep_len` / `ep_arena` / `ep_end` i32 [T N] (the whole episode's rows, its arena, the t of its done row in this window),
    `counts` i32 [2] (episodes, rows = T N), `summary` f64 [len(_lib.EP_METRICS)], `totals` i64 [2] (episodes_total, timesteps_total
    since start() / reset()).  12 + 8 n_agents bytes per window row and 8 + 8 n_agents per arena: 29.8 MB for N = 16384, T = 64 and two
    agents (the table has room for an episode at every row, so it cannot overflow).

    The two differences from RLlib of EpisodeBatch's metrics hold here too (the means are over the episodes finished in THIS window, no
    smoothing over the last 100; `vf_explained_var` is the sampler's VF_PREDS against the value targets), and `vf_explained_var` is
    taken over the window's T N rows, whose targets bootstrap at the window's end.  A window without a finished episode reports
    episodes_this_iter = 0 and nan for the episode entries, but its timesteps and vf_explained_var as always.

    outcomes (the rollouts' keyword-only outcomes=True; `attach_outcomes`): also an `EpisodeOutcomes` over the table — `ep_outcome` i8
    [T N], entry e the outcome of the window's episode e (1 agents win, -1 opponents win, 0 draw), in `episodes()` and
    `metrics_device()`; two more launches right behind hh_window_metrics; `metrics()` gains the keys EpisodeBatch.metrics() gains
    (outcome_metrics), over the episodes finished in this window.  Without it, nothing is allocated and every key set is what it was."""

    TABLES = ("ep_return", "ep_len", "ep_arena", "ep_end")

    def __init__(self, collect, agent_keys):
        """collect: the rollout's window buffers every call reads — reward f32 [T, N, n_agents], vf f32 [T+1, N, n_agents], target f32
        [T, N, n_agents], done u8 [T, N]; agent_keys: the keys of metrics()' per-agent entries (the matching episode batch's AGENT_KEYS)"""
        T, N = collect["done"].shape
        self.T, self.N, self.n_agents = int(T), int(N), int(collect["reward"].shape[2])
        self.AGENT_KEYS = tuple(agent_keys)
        if not 1 <= self.n_agents <= L.EP_METRICS_MAX_AGENTS or len(self.AGENT_KEYS) != self.n_agents:
            raise ValueError(f"window_metrics: {len(self.AGENT_KEYS)} agent keys, the collect has {self.n_agents} agents")
        T, N, nA = self.T, self.N, self.n_agents
        for k, shape, dt in (("reward", (T, N, nA), torch.float32), ("vf", (T + 1, N, nA), torch.float32), ("target", (T, N, nA), torch.float32),
                             ("done", (T, N), torch.uint8)):
            t = collect[k]
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"window_metrics: {k} must be a contiguous {dt} tensor of shape {shape}")
        self._device = dev = collect["done"].device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        nbytes = C.c_int64(0)
        L.check(L.lib().hh_window_metrics_scratch_bytes(T, N, nA, C.byref(nbytes)))
        self.run_return, self.run_len = z((N, nA), torch.float64), z((N,), torch.int32)
        self.ep_return = z((T * N, nA), torch.float64)
        self.ep_len, self.ep_arena, self.ep_end = (z((T * N,), torch.int32) for _ in range(3))
        self.counts = z((2,), torch.int32)
        self.n_episodes = self.counts[0]
        self._summary = z((len(L.EP_METRICS),), torch.float64)
        self._totals = z((2,), torch.int64)
        self._scratch = z((nbytes.value // 8,), torch.float64)
        self._host = None                        # pinned host copies (summary, totals), made by the first metrics()
        self._collect = collect                  # the struct holds raw pointers: keep the tensors alive
        self._bufs = L.HHWindowMetricsBufs(
            T=T, N=N, n_agents=nA, reserved0=0, reward=collect["reward"].data_ptr(), vf=collect["vf"].data_ptr(),
            target=collect["target"].data_ptr(), done=collect["done"].data_ptr(), run_return=self.run_return.data_ptr(),
            run_len=self.run_len.data_ptr(), ep_return=self.ep_return.data_ptr(), ep_len=self.ep_len.data_ptr(),
            ep_arena=self.ep_arena.data_ptr(), ep_end=self.ep_end.data_ptr(), counts=self.counts.data_ptr(),
            summary=self._summary.data_ptr(), totals=self._totals.data_ptr(), scratch=self._scratch.data_ptr(), scratch_bytes=nbytes.value)
        self._outcomes = None                    # attach_outcomes puts an EpisodeOutcomes here
        self.reset()

    def attach_outcomes(self, outcome):
        """outcome i8 [T, N]: the rollout's tapped window (World.outcome_tap behind every tick).  From now on every call also fills
        `ep_outcome` and the outcomes' summary (see the class)."""
        self._outcomes = EpisodeOutcomes(self._collect["done"], outcome, self.n_episodes, self.ep_arena, self.ep_len, self.ep_return)
        self.ep_outcome = self._outcomes.ep_outcome
        self.TABLES = type(self).TABLES + ("ep_outcome",)
        self._host = None

    def reset(self):
        """no episode spans a reset: the carry and the running totals start again, and the summary is that of a window without a
        finished episode, with 0 rows, until the next collect"""
        self.run_return.zero_()
        self.run_len.zero_()
        self._totals.zero_()
        self.counts.zero_()
        self._summary.fill_(float("nan"))
        self._summary[:2] = 0.0
        if self._outcomes is not None:
            self._outcomes.reset()

    def enqueue(self, stream):
        """hh_window_metrics over the window as it stands, on `stream` (what the rollout's collect does right behind the GAE).  Every
        call advances the carry and the totals by one window.  With outcomes, hh_episode_outcomes follows it."""
        L.check(L.lib().hh_window_metrics(C.byref(self._bufs), stream))
        if self._outcomes is not None:
            self._outcomes.enqueue(stream)

    def metrics_device(self):
        """the device tensors of the last collect's metrics, without synchronising: `summary` (slots: _lib.EP_METRICS_SLOT), `totals`,
        the table `ep_return` / `ep_len` / `ep_arena` / `ep_end` (the first counts[0] entries are valid) and `counts`.  Overwritten by
        the next collect."""
        out = {"summary": self._summary, "totals": self._totals, "ep_return": self.ep_return, "ep_len": self.ep_len,
               "ep_arena": self.ep_arena, "ep_end": self.ep_end, "counts": self.counts}
        if self._outcomes is not None:   # ep_outcome [T N] like the table; outcome_summary: _lib.EO_SUMMARY's slots; outcome_flags i32 [2]
            out.update(ep_outcome=self.ep_outcome, **self._outcomes.whole())
        return out

    def metrics(self):
        """-> the last window's metrics under RLlib's result names, the keys and types of `EpisodeBatch.metrics()` (per-agent entries are
        dicts keyed by AGENT_KEYS); copies the summary and the totals to the host: one synchronisation of the current stream.  After
        reset() / start() and before the next collect: 0 episodes, 0 timesteps, nan, totals 0.  With outcomes: also outcome_metrics' keys
        (see the class); RuntimeError if the outcomes did not match the table or an entry carries none."""
        src = (self._summary, self._totals) + (() if self._outcomes is None else (self._outcomes.summary, self._outcomes.flags))
        if self._host is None:
            self._host = tuple(torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in src)
        for h, d in zip(self._host, src):
            h.copy_(d, non_blocking=True)
        torch.cuda.current_stream(self._device).synchronize()
        s, totals, *eo = (h.tolist() for h in self._host)
        out = metrics_dict(s, totals, self.AGENT_KEYS)
        if eo:
            if EpisodeOutcomes.failed(*eo):
                raise RuntimeError("WindowMetrics: the window's outcomes do not match its episode table (an entry of another arena, or a "
                                   "done row without an outcome): the outcome metrics since that collect are incomplete")
            out.update(outcome_metrics(eo[0]))
        return out

    def episodes(self):
        """synchronises; -> dict of views cut to the episodes that finished in the last window: ep_return, ep_len, ep_arena, ep_end
        (with outcomes: ep_outcome too)"""
        torch.cuda.synchronize(self._device)
        n = int(self.counts[0])
        return {k: getattr(self, k)[:n] for k in self.TABLES}

    # ---- checkpointing (hhmarl_2d_amd/checkpoint.py)
    def _options(self):
        return dict({"T": self.T, "N": self.N, "n_agents": self.n_agents}, **({} if self._outcomes is None else {"outcomes": True}))

    def _whole(self):
        return dict({"run_return": self.run_return, "run_len": self.run_len, "counts": self.counts, "summary": self._summary, "totals": self._totals},
                    **({} if self._outcomes is None else self._outcomes.whole()))

    def state_dict(self):
        """the carry, the counts, the summary and the totals whole, the table cut to the count.  Scratch is not saved.  Synchronises the
        device."""
        torch.cuda.synchronize(self._device)
        n = int(self.counts[0])
        return {"options": self._options(), "state": {k: ck.cpu(v) for k, v in self._whole().items()},
                "table": {k: ck.cpu(getattr(self, k)[:n]) for k in self.TABLES}}

    def _load_plan(self, sd):
        who = type(self).__name__
        ck.need_keys(who, sd, ("options", "state", "table"))
        ck.check_options(who, sd["options"], self._options())
        pairs = ck.plan_tensors(who, sd["state"], self._whole())
        n = int(sd["state"]["counts"][0])
        if not 0 <= n <= self.T * self.N:
            raise ValueError(f"{who}: `counts` names {n} episodes, a window of {self.T * self.N} rows ends at most that many")
        ck.need_keys(who + " table", sd["table"], self.TABLES)
        for k in self.TABLES:
            ck.check_tensor(who, "table." + k, sd["table"][k], getattr(self, k), lead=n)
            pairs.append((getattr(self, k)[:n], sd["table"][k]))
        return lambda: ck.copy_pairs(pairs)

    def load_state_dict(self, sd):
        """state_dict()'s dict back, in place; validated first (ValueError names the field, nothing changed)"""
        self._load_plan(sd)()


def check_window_metrics(window_metrics, batch_mode, semantics="rllib"):
    """window_metrics as both rollouts' constructors take it -> bool, or ValueError"""
    if not window_metrics:
        return False
    if batch_mode != "truncate_episodes":
        raise ValueError("window_metrics=True needs batch_mode='truncate_episodes': batch_mode='complete_episodes' already has metrics=True")
    if semantics != "rllib":
        raise ValueError("window_metrics=True is defined for RLlib's trajectory view only (semantics='rllib'): its targets are hh_gae_rllib's")
    return True


def window_metrics_keyword(agent_keys):
    """Decorator of both rollouts' `__init__`: adds the keyword-only `window_metrics=False` behind the positional parameters.  It is
    validated (check_window_metrics) before the constructor runs, so before the world is touched, and afterwards `self.window_metrics`
    is a WindowMetrics over the new rollout's window buffers, or None.  A wrapper instead of one more parameter in the `def`: the
    constructors' positional signature — what `inspect.signature` reports through `__wrapped__` — ends with `record_logits`, where its
    callers and the signature tests expect it, and stays as it was."""
    def wrap(init):
        sig = inspect.signature(init)

        @functools.wraps(init)
        def __init__(self, *args, window_metrics=False, **kw):
            a = sig.bind(self, *args, **kw)          # TypeError for arguments the constructor does not take, as from the constructor
            a.apply_defaults()
            on = check_window_metrics(window_metrics, a.arguments["batch_mode"], a.arguments.get("semantics", "rllib"))
            init(self, *args, **kw)
            self.window_metrics = WindowMetrics({k: getattr(self, k) for k in ("reward", "vf", "target", "done")}, agent_keys) if on else None
        return __init__
    return wrap


def check_outcomes(outcomes, batch_mode, metrics, window_metrics):
    """outcomes as both rollouts' constructors take it -> bool, or ValueError"""
    if not isinstance(outcomes, bool):
        raise ValueError(f"outcomes: False or True, got {outcomes!r}")
    if outcomes and not ((metrics and batch_mode == "complete_episodes") or window_metrics):
        raise ValueError("outcomes=True needs a consumer of the episode table: metrics=True with batch_mode='complete_episodes', or "
                         "window_metrics=True")
    return outcomes


def outcomes_keyword(init):
    """Decorator of both rollouts' `__init__`, around window_metrics_keyword's: adds the keyword-only `outcomes=False` the same way (the
    positional signature, and `inspect.signature` through `__wrapped__`, stay as they were; `window_metrics` is declared again and
    handed on, so that the outermost signature still shows it).  Validated (check_outcomes) before the
    constructor runs, so before the world is touched.  With True, `self.outcome` is the tapped window — i8 [T, N], row [t, n] the outcome
    of the episode whose done row it is (1 agents win, -1 opponents win, 0 draw) and 2 elsewhere, written by World.outcome_tap right
    behind every tick of `_run` — and the rollout's episode batch / WindowMetrics owns the table's outcomes (`attach_outcomes`).  With the
    default it is None: no allocation, no launch, the same graph."""
    sig = inspect.signature(init)                    # the constructor's own parameters (through __wrapped__)

    @functools.wraps(init)
    def __init__(self, *args, window_metrics=False, outcomes=False, **kw):   # window_metrics: handed on as it came
        a = sig.bind(self, *args, **kw)              # TypeError for arguments the constructor does not take, as from the constructor
        a.apply_defaults()
        on = check_outcomes(outcomes, a.arguments["batch_mode"], a.arguments["metrics"], window_metrics)
        init(self, *args, window_metrics=window_metrics, **kw)
        if on:
            self.outcome = torch.full(tuple(self.done.shape), L.OUTCOME_NONE, dtype=torch.int8, device=self.done.device)
            for consumer in (self.episodes, self.window_metrics):
                if consumer is not None:
                    consumer.attach_outcomes(self.outcome)
    return __init__


def rollout_outcome_names(ro):
    """what `outcomes=True` adds to a rollout's saved window buffers and options"""
    return (("outcome",), {"outcomes": True}) if ro.outcome is not None else ((), {})


def rollout_state_dict(ro, names, options):
    """what both rollouts save: their options, the [T(+1), N, ...] window buffers `names` as the last collect left them (the hand-over
    rows obs[T] / vf[T] among them; update_window directly after a load trains on them), `collects`, `_started` and their episode batch;
    with window_metrics=True one more entry, `window_metrics`"""
    torch.cuda.synchronize(ro.w.device)
    sd = {"options": options, "window": {k: ck.cpu(getattr(ro, k)) for k in names}, "collects": int(ro.collects), "started": bool(ro._started),
          "episodes": None if ro.episodes is None else ro.episodes.state_dict()}
    if ro.window_metrics is not None:
        sd["window_metrics"] = ro.window_metrics.state_dict()
    return sd


def rollout_load_plan(ro, sd, names, options):
    who = type(ro).__name__
    ck.need_keys(who, sd, ("options", "window", "collects", "started", "episodes") + (("window_metrics",) if ro.window_metrics is not None else ()))
    ck.check_options(who, sd["options"], options)
    wm = (lambda: None) if ro.window_metrics is None else ro.window_metrics._load_plan(sd["window_metrics"])
    pairs = ck.plan_tensors(who + " window", sd["window"], {k: getattr(ro, k) for k in names})
    if isinstance(sd["collects"], bool) or not isinstance(sd["collects"], int) or sd["collects"] < 0 or not isinstance(sd["started"], bool):
        raise ValueError(f"{who}: `collects` is a count and `started` a bool")
    if (sd["episodes"] is None) != (ro.episodes is None):
        raise ValueError(f"{who}: `episodes` was {'not ' if sd['episodes'] is None else ''}saved, the live rollout has {'none' if ro.episodes is None else 'one'}")
    sub = (lambda: None) if ro.episodes is None else ro.episodes._load_plan(sd["episodes"])

    def commit():
        ck.copy_pairs(pairs)
        sub()
        wm()
        ro.collects, ro._started = sd["collects"], sd["started"]
        if sd["started"] and getattr(ro, "_graph", None) is None:
            # a started rollout never calls start(), whose launches are the first of this library in a fresh process: give the next
            # collect's capture a process that has already launched from the library (a read-only kernel; nothing of the state changes)
            ro.w.arena_status()
    return commit


class PPORollout:
    """What RLlib's rollout workers produce for train_hetero.py's PPO (train_hetero.py:206-243), for every arena of a `World` at once and
    without leaving the device: per tick the two trainable policies are sampled by `hh_policy_sample` (actor forward, Categorical draw
    per action component from the keyed RNG, its log-probability, and the centralised value branch on central_critic_observer's row —
    the other agent's observation, action inputs zero while sampling) and the world takes one `hh_step`; after T ticks the rewards and
    value predictions become advantages and value targets (gamma 0.99, lambda 0.95: train_hetero.py:216).  The 2 T + 2 launches of a
    collect are one HIP graph (4 T + 2 at curriculum levels 4-5, where the frozen opponents' networks run between the two halves of
    every step).

    semantics = "rllib" (default) — the batch RLlib 2.4 hands the reference's learner (ray's sampler + compute_advantages as restated in
    oracle/gae_ref.py; include/hh_abi.h: hh_gae_rllib):
      * every agent's trajectory spans the whole episode: the rows of an agent that died earlier STAY IN with reward 0.0 (the reference
        returns an observation for every agent id, zeros for dead ones, and a reward only for ids alive at step start; RLlib fills
        `rewards.get(agent_id, 0.0)`) — nothing is masked, `valid` is only reported;
      * last_r = 0.0 at every episode end (terminateds["__all__"] also at the horizon, env_base.py:108): the recursion is cut there and
        no value is bootstrapped across it; float64 delta and discounted sum, float32 results;
      * train_hetero.py:212 batch_mode = "complete_episodes": RLlib trains on whole episodes only.  `complete` (bool [T, N]) marks the
        rows of episodes that END inside this collect; the trailing fragment of every arena (its episode is still running after
        tick T - 1) gets RLlib's truncated-trajectory bootstrap from one more value evaluation and is flagged complete = False
        (`segments` numbers the episodes per arena).  The head of an episode that began in an earlier collect is not in this window,
        so these rows are not RLlib's batch: batch_mode = "complete_episodes" (below) builds that one.
    semantics = "masked": the pre-round-5 convention (`hh_gae`): rows without a reward key have advantage = target = 0 and do not
    propagate, float32 throughout — for learners that cut dead agents' rows out.

    Buffers (device, overwritten by every `collect`):  obs f32 [T+1, N, 2, D] (row t = what the policy saw at tick t), actions i8
    [T, N, 2, 4], logp f32 [T, N, 2], vf f32 [T+1, N, 2], reward f32 [T, N, 2] (0.0 where valid = 0), valid u8 [T, N, 2], done u8
    [T, N], adv / target f32 [T, N, 2]; `complete` / `segments` are derived from `done` on demand.  `critic_rows(agent)` gives the
    flattened CUR_OBS rows the reference's critic is trained on (actions filled in the way on_postprocess_trajectory does).

    batch_mode = "truncate_episodes" (default): the buffers above are the result, and `PPOLearner.update_window(rollout, bank)` trains on
    them as they stand (semantics = "rllib").  batch_mode = "complete_episodes" (train_hetero.py:212;
    semantics = "rllib" only): every collect still fills the buffers above exactly the same way, and then also `episodes`, an
    `EpisodeBatch` of every episode that ended in it — whole, its earlier rows carried on the device from the collects before — with
    advantages / value targets over the whole episode (last_r = 0): the batch RLlib hands its learner.  Its 4 launches are part of the
    collect's graph.

    record_logits = True: every tick's sampler call also writes its logits — the rows its actions were drawn from and its logp was taken
    of, RLlib's ACTION_DIST_INPUTS — into `logits` f32 [T, N, 2, 32] (zero padded past the kind's 26 | 24), and with batch_mode =
    "complete_episodes" the column travels with the rows: `episodes.rows()["logits"]` f32 [R, 2, 32] holds, for every emitted row,
    the logits of the forward that sampled it, whatever weights the bank held then — also for the head of an episode that was running at
    a `publish`.  `PPOLearner.update` then takes its old logits from there instead of recomputing them.  The bootstrap evaluation and
    `start()` keep discarding theirs.  Opt-in because of its size: 256 B per row, next to 8 D + 47 — 256 T N bytes of collect buffer,
    and at N = 16384, H = 300, T = 64 about 1.25 GB more carry and 1.52 GB more batch.  With the default False nothing is allocated and
    the launches, the graph and the results are what they were.

    metrics = True (batch_mode = "complete_episodes" only): `episodes.metrics()` gives the collect's line of RLlib's training result
    (`episode_reward_mean` and the rest: train_hetero.py:285) from three more launches in the collect's graph; see EpisodeBatch.

    train_batch_size = B (batch_mode = "complete_episodes" only; train_hetero.py:216 `train_batch_size=args.batch_size`): `episodes`
    accumulates the collects on the device until it holds at least B rows — whole collects, nothing trimmed — instead of being
    overwritten by each; the launches of a collect and its graph stay the same.  `collect_batch()` collects until `episodes.ready()`;
    the collect after a complete batch starts the next one.  See EpisodeBatch for the capacities.

    window_metrics = True (keyword-only; batch_mode = "truncate_episodes" and semantics = "rllib" only): the same result line for a run
    that trains from the windows — `window_metrics`, a `WindowMetrics`, carries every arena's running return and length on the device
    across collects and reports the episodes that finish inside each window (`window_metrics.metrics()`: the keys of
    `episodes.metrics()`): five more launches in the collect's graph right behind the GAE.  With the default False it is None, nothing
    is allocated and the launches, the graph, the buffers and `state_dict()` are what they were.

    outcomes = True (keyword-only; needs metrics = True with batch_mode = "complete_episodes", or window_metrics = True): win, lose and
    draw of every training episode.  `outcome` i8 [T, N] is one more window buffer, overwritten by every collect: row [t, n] is the outcome
    of the episode whose done row it is — 1 agents win, -1 opponents win, 0 draw, `World.episode_stats()`' codes — and 2 elsewhere, tapped
    right behind every tick (`World.outcome_tap`: T more launches in the collect's graph).  `episodes` / `window_metrics` then own
    `ep_outcome`, one entry per episode of their table, and their `metrics()` gains agents_win / opps_win / draw, outcome_pct and the
    mean reward and length per outcome (two more launches; see EpisodeBatch).  `state_dict()` holds all of it.  With the default False
    `outcome` is None, nothing is allocated and the launches, the graph, `metrics()` and `state_dict()` are what they were."""

    @outcomes_keyword
    @window_metrics_keyword(EpisodeBatch.AGENT_KEYS)
    def __init__(self, world, bank, T, gamma=0.99, lam=0.95, use_graph=True, opponents=None, semantics="rllib", batch_mode="truncate_episodes",
                 metrics=False, train_batch_size=None, record_logits=False):
        """metrics / train_batch_size / record_logits: pass them by keyword (record_logits stays the last parameter, where its callers and
        its test expect it); window_metrics is keyword-only (window_metrics_keyword).
        opponents: levels 4-5 only (env_hetero.py:160-172: frozen-policy opponents observe and act between the agents' actions and the tick) —
        a `pilots.OpponentNets(world, skip_first=False)` (its bank bound, so that hh_step_begin lists the opponents' rows itself) or any
        callable(opp_obs f32 [N, 2, 30] on the device, None) -> int8 [N, 2, 4] that only enqueues work on the current stream"""
        if batch_mode not in ("truncate_episodes", "complete_episodes"):
            raise ValueError("batch_mode: 'truncate_episodes' (fixed [T, N] windows) or 'complete_episodes' (whole episodes: EpisodeBatch)")
        if batch_mode == "complete_episodes" and semantics == "masked":
            raise ValueError("batch_mode='complete_episodes' is defined for RLlib's trajectory view only (semantics='rllib')")
        if metrics and batch_mode != "complete_episodes":
            raise ValueError("metrics=True needs batch_mode='complete_episodes': the episode metrics are those of the whole-episode batch")
        if train_batch_size is not None and batch_mode != "complete_episodes":
            raise ValueError("train_batch_size needs batch_mode='complete_episodes': it is the whole-episode batch that accumulates")
        train_batch_size = EpisodeBatch.check_train_batch_size(train_batch_size)
        from . import pilots
        assert world.cfg.env_kind == L.ENV_LOWLEVEL and world.n_agents == 2 and world.cfg.auto_reset, "PPORollout drives an auto-resetting LowLevelEnv world"
        if semantics not in ("rllib", "masked"):
            raise ValueError("semantics: 'rllib' (RLlib 2.4's trajectory view, the reference's) or 'masked' (rows without a reward key cut out)")
        self.semantics = semantics
        self.split = bool(world.cfg.ext_opp_actions)
        if self.split and opponents is None:
            raise ValueError("levels 4-5 fly frozen opponent policies (envs/env_base.py:312-398): pass opponents = pilots.OpponentNets(world, skip_first=False)")
        if getattr(opponents, "_skip", 0):
            # OpponentNets(skip_first=True) serves a facade whose reset() already ran one step_begin: its one-shot path re-bins rows that
            # hh_step_begin listed, and captured into the collect's graph it would do so on every replay (every row evaluated twice).  The
            # object may be shared with such a facade, so it is refused rather than silently changed
            raise ValueError("PPORollout needs opponents = pilots.OpponentNets(world, skip_first=False): this one still holds the one-shot skip of a "
                             "facade-style binding (skip_first=True)")
        self.opponents = opponents
        self.w, self.bank, self.T, self.gamma, self.lam = world, bank, int(T), float(gamma), float(lam)
        N, D, dev = world.N, world.D, world.device
        esc = world.cfg.agent_mode == L.MODE_ESCAPE
        self.sel = torch.tensor([pilots.SEL_ESC1 if esc else pilots.SEL_FIGHT1, pilots.SEL_ESC2 if esc else pilots.SEL_FIGHT2],
                                dtype=torch.uint8, device=dev).repeat(N, 1).contiguous()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.obs = z((self.T + 1, N, 2, D), torch.float32)
        self.actions = z((self.T, N, 2, 4), torch.int8)
        self.logp = z((self.T, N, 2), torch.float32)
        self.vf = z((self.T + 1, N, 2), torch.float32)
        self.reward = z((self.T, N, 2), torch.float32)
        self.valid = z((self.T, N, 2), torch.uint8)
        self.done = z((self.T, N), torch.uint8)
        self.adv = z((self.T, N, 2), torch.float32)
        self.target = z((self.T, N, 2), torch.float32)
        self._tmp_act, self._tmp_logp = z((N, 2, 4), torch.int8), z((N, 2), torch.float32)
        self._opp_obs = z((N, world.A - 2, 30), torch.float32) if self.split else None
        # level 5 in fight mode: every arena observes in the mode of its own episode's draw (HH_OPP_MODE_EPISODE); otherwise fight mode
        self._opp_mode = L.OPP_MODE_EPISODE if (world.cfg.level == 5 and world.cfg.agent_mode == L.MODE_FIGHT) else 0
        self.batch_mode = batch_mode
        self.record_logits = bool(record_logits)
        if self.record_logits:
            self.logits = z((self.T, N, 2, L.POLICY_LOGITS), torch.float32)
        self.episodes = None
        if batch_mode == "complete_episodes":
            self.episodes = EpisodeBatch({k: getattr(self, k) for k in EpisodeBatch.ROW_INPUTS + ("done",)}, max(world.cfg.horizon - 1, 0),
                                         self.gamma, self.lam, aux=("logits", self.logits) if self.record_logits else None, metrics=bool(metrics),
                                         train_batch_size=train_batch_size)
        self.window_metrics = None          # window_metrics_keyword puts a WindowMetrics here
        self.outcome = None                 # outcomes_keyword puts the tapped window here
        self.use_graph = use_graph
        self._graph = None
        self._started = False
        self.collects = 0                   # collects so far: the window buffers hold a batch once it is non-zero

    def start(self):
        """reset every arena; the first observation becomes row 0 of the next collect.  Also builds the row lists of the fixed agent ->
        network mapping (a greedy evaluation whose results are discarded), so that every later call re-uses them (sel = NULL)."""
        self.w.reset(obs=self.obs[self.T])
        if self.episodes is not None:
            self.episodes.reset()
        if self.window_metrics is not None:
            self.window_metrics.reset()
        self.bank.sample(self.obs[self.T], self.sel, greedy=True, actions=self._tmp_act, logp=self._tmp_logp, vf=self.vf[self.T])
        self._started = True

    def _run(self):
        T = self.T
        self.obs[0].copy_(self.obs[T])      # where the previous collect (or start) left every arena
        for t in range(T):                  # every launch reads and writes its tick's rows of the [T, ...] buffers in place
            self.bank.sample(self.obs[t], None, world=self.w, actions=self.actions[t], logp=self.logp[t], vf=self.vf[t],
                             logits=self.logits[t] if self.record_logits else None)
            out = (self.obs[t + 1], self.reward[t], self.valid[t], self.done[t])
            if self.split:   # agents act -> the frozen opponents observe (the agents' same-tick weapon flags included) and act -> tick
                self.w.step_begin(self.actions[t], self._opp_mode, opp_obs=self._opp_obs)
                self.w.step_finish(self.opponents(self._opp_obs, None).contiguous(), out=out)
            else:
                self.w.step(self.actions[t], out=out)
            if self.outcome is not None:
                self.w.outcome_tap(self.done[t], self.outcome[t])
        # value of the observation after the last tick: the bootstrap of every arena's unfinished tail (an arena that just finished starts a
        # new episode there: both recursions cut at done and never read it)
        self.bank.sample(self.obs[T], None, greedy=True, actions=self._tmp_act, logp=self._tmp_logp, vf=self.vf[T])
        st = C.c_void_p(torch.cuda.current_stream(self.w.device).cuda_stream)
        if self.semantics == "rllib":
            # the world writes reward 0.0 wherever it reports valid = 0 (a dead agent's row): exactly RLlib's rewards.get(agent_id, 0.0)
            L.check(L.lib().hh_gae_rllib(T, self.w.N, 2, _p(self.reward), _p(self.vf), _p(self.done), self.gamma, self.lam,
                                         _p(self.adv), _p(self.target), st))
        else:
            L.check(L.lib().hh_gae(T, self.w.N, 2, _p(self.reward), _p(self.vf), _p(self.valid), _p(self.done), self.gamma, self.lam,
                                   _p(self.adv), _p(self.target), st))
        if self.window_metrics is not None:
            self.window_metrics.enqueue(st)
        if self.episodes is not None:
            self.episodes.emit(st)

    def collect(self):
        """T ticks of every arena -> self (the buffers above): 2 T + 2 launches, replayed from ONE HIP graph; no host synchronisation."""
        if not self._started:
            self.start()
        if not self.use_graph:
            self._run()
        else:
            if self._graph is None:
                torch.cuda.synchronize(self.w.device)
                self._graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph):
                    self._run()
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
        return (("obs", "actions", "logp", "vf", "reward", "valid", "done", "adv", "target") + (("logits",) if self.record_logits else ())
                + rollout_outcome_names(self)[0])

    def _options(self):
        return dict({"T": self.T, "N": self.w.N, "D": self.w.D, "gamma": self.gamma, "lam": self.lam, "semantics": self.semantics,
                     "batch_mode": self.batch_mode, "record_logits": self.record_logits, "split": self.split}, **rollout_outcome_names(self)[1])

    def state_dict(self):
        """the window buffers of the last collect (obs[T] / vf[T] are the hand-over rows of the next one), `collects`, `_started` and the
        EpisodeBatch; the world and the banks are saved by themselves.  The captured graph is not saved: a fresh rollout captures at its
        first collect as always, a rollout that has captured keeps replaying (the load writes in place).  Synchronises the device."""
        return rollout_state_dict(self, self._window_names(), self._options())

    def _load_plan(self, sd):
        return rollout_load_plan(self, sd, self._window_names(), self._options())

    def load_state_dict(self, sd):
        """state_dict()'s dict back in place; validated first (ValueError names the field, nothing changed)"""
        self._load_plan(sd)()

    @property
    def segments(self):
        """int64 [T, N]: index of the episode a row belongs to, counted per arena from the start of this collect (episode_segments)"""
        return episode_segments(self.done)[0]

    @property
    def complete(self):
        """bool [T, N]: the row's episode ends inside this collect — batch_mode = "complete_episodes" (train_hetero.py:212) trains on these"""
        return episode_segments(self.done)[1]

    def critic_rows(self, agent):
        """the CUR_OBS rows of `agent` (1 | 2) for the T collected ticks with both agents' actions filled in (central_critic_rows)"""
        return central_critic_rows(self.obs[: self.T], self.actions, agent)
