"""PPOLearner: the PPO update of train_hetero.py's two policies"""
import weakref

import numpy as np
import torch

from .. import _lib as L
from .. import pilots
from .. import policy_nets as PN
from ..rollout import central_critic_rows
from .batch import chunk_mask, cut_chunks, pad_chunks, standardize, window_cut, window_gather
from .loss import OLD_LD, _loss_kw, heads_loss, n_comp_of, ppo_loss, ppo_loss_torch
from .nets import TrainableNet, tie
from .ops import _trunk_mode
from .. import checkpoint as ck
from .shards import standardize_shards
from .step import _heads_keyword, _learner_options, _learner_saved_options, _module_plan, _PolicySGD, _shard_group

# ------------------------------------------------------------------------------------------------------------------ the learner
class PPOLearner:
    """One PPO update of train_hetero.py's two policies from the `EpisodeBatch` of a `PPORollout(batch_mode="complete_episodes")`:

        learner = PPOLearner.trainable_init(device, mode="fight", seed=0)     # the weights of PolicyBank.trainable_init(seed)
        stats = learner.update(ro.episodes, bank)
        learner.publish(bank)

    Defaults: train_hetero.py:216 (lr, clip_param, kl_target), config.py:36-37 (sgd_minibatch_size) and RLlib 2.4's PPO defaults for the
    rest.  Per policy (agent 1, then agent 2; each with its own Adam over its module's parameters, the tied shared layer in both):
      * rows: the agent's column of every emitted row — nothing is masked by `valid` (semantics = "rllib"); own observation cut to the
        kind's width, critic rows from central_critic_rows (actions filled in);
      * old_logits (RLlib's ACTION_DIST_INPUTS, which the KL term and so kl_coeff are computed from): `batch_old_logits`.  With
        PPORollout(record_logits=True) the batch carries a `logits` column — for every row the logits of the sampler call that drew its
        action and wrote its logp, whatever weights the bank held at that tick — and that column is used as it stands: no bank call,
        and rows sampled before the last publish (the head of an episode that was still running then) keep the logits of the weights
        that sampled them, so old_logp and old_logits of a row always come from one forward.
        Without the column they are recomputed once per update from `bank`, which still holds the pre-update weights, in
        ceil(R / N) greedy calls of the rollout's own shape ([N, 2] rows, the same selectors, so the row lists a captured collect
        re-uses stay what they were).  Only then does this approximation apply: rows carried over from before the last publish were
        sampled by older weights — their stored logp, and so the ratio, is exact, but their recomputed old_logits are the newer
        weights', so the KL term sees them as on-policy (`rollout.start()` after `publish` avoids it by throwing the running episodes
        away; record_logits = True makes that unnecessary);
      * advantages standardised over the policy's whole batch;
      * fight kinds: each episode cut into chunks of max_seq_len, zero-padded, mask = the unpadded rows;
      * num_sgd_iter passes; in each the chunks (escape: rows), in batch order, are split into consecutive minibatches of at least
        sgd_minibatch_size unpadded rows, visited in the order of minibatch_order(seed, update count, policy, pass).  RLlib's own
        order is drawn from an unseeded generator and shuffles the chunks themselves; this one is reproducible by construction, and
        shuffle_sequences=True shuffles the chunks themselves as well, per pass, from a seeded stream of its own (shuffled_schedule);
      * after the passes KLCoeffMixin.update_kl on the mean of the minibatches' mean_kl.
    fused = False computes the loss with torch ops (ppo_loss_torch) instead of hh_ppo_loss; nothing else differs.
    Inside a minibatch step nothing synchronises with the host (beyond what torch.optim.Adam does by itself); `update` itself synchronises
    when it reads the batch's row count, cuts the minibatches and reads the statistics.  (CommanderRollout's batches: CommanderLearner.)"""

    @_heads_keyword
    def __init__(self, kinds, state_dicts, device, lr=1e-4, clip_param=0.25, kl_target=0.025, kl_coeff=0.2, vf_clip_param=10.0,
                 vf_loss_coeff=1.0, entropy_coeff=0.0, num_sgd_iter=30, sgd_minibatch_size=256, max_seq_len=20, seed=0, fused=True, attention="torch", inputs="torch", trunk="torch",
                 optimizer="torch", step="eager", shuffle_sequences=False, grad_clip=None):
        """kinds: (kind of ac1_policy, kind of ac2_policy); state_dicts: per policy the actor and value-branch tensors in one dict (numpy or
        torch), keyed like the reference's state_dict().  The shared layer is tied to the first policy's.  attention: TrainableNet's
        argument, handed to both modules ("fused": the fight networks' chunk attention through hh_chunk_attn_* / hh_residual_normalize_*;
        "block": each whole attention block, projections included, through hh_attn_block_*).
        inputs: TrainableNet's argument as well ("fused": everything in front of shared_layer through hh_input_stage_*).
        trunk: TrainableNet's argument too ("fused": shared_layer, bias and tanh of both sides through hh_dense_tanh_*).
        optimizer: "torch" (the default) steps with torch.optim.Adam; "fused" keeps each policy's m, v and step count on the device
        (DeviceAdam: hh_adam_step) and gathers the steps' statistics in a device table (hh_train_commit).
        step: "eager" (the default) issues every minibatch step's launches from Python; "graph" (needs optimizer="fused") captures
        stage -> forward -> loss -> backward -> Adam -> commit once per policy as ONE HIP graph and replays it per step (graph_prepare).
        grad_clip: RLlib's grad_clip.  None (the default, and the reference's value): nothing is clipped and nothing changes.  A finite float
        > 0: in every minibatch step the gradients of ONE optimizer — one policy's parameter list, the tied shared layer in it, as RLlib's
        apply_grad_clipping takes one optimizer's param groups — are scaled so that their global L2 norm does not exceed it, and every dict
        of update() also has grad_gnorm, the mean over the update's steps of the norm BEFORE clipping (RLlib reports it under the same
        condition).  optimizer="torch" calls torch.nn.utils.clip_grad_norm_ (float32 norm, scales .grad in place); "fused" computes the
        norm in float64 on the device and scales inside the Adam step (DeviceAdam(max_norm=...): .grad keeps the unscaled gradient), and
        the graph's chain becomes stage -> forward -> loss -> backward -> norm -> clipped Adam -> commit.
        shuffle_sequences: RLlib's shuffle_sequences (its default is True; here False, and then nothing changes).  True: every pass draws
        its own order of the chunks (escape: rows), sequence_order(seed, update count, policy, pass), and cuts THAT order into consecutive
        minibatches of at least sgd_minibatch_size unpadded rows (shuffled_schedule), visited in position order: the minibatches hold
        different chunks in every pass, and a pass may take one step more or fewer than another.  The eager modes gather each minibatch with
        index_select; step="graph" stages through hh_minibatch_stage_gather from an order table uploaded once per update into a persistent
        device buffer of 4 * num_sgd_iter * S bytes for S chunks, grown to twice the need so that its address outlives batches of varying
        size (30 passes: about 6.6 MB for 1.09 M fight rows in chunks of 20, about 131 MB for the same rows as escape rows).  RLlib's own
        permutation is unseeded, so equality with it is not claimed; what shuffling does to learning curves has not been measured here.
        heads (keyword only, taken by _heads_keyword in front of this signature): "torch" (the default): nothing changes.  "fused" (needs fused=True and trunk="torch"): the modules are built
        with heads="fused", every minibatch step's forward stops at shared_layer's pre-activations (TrainableNet.pre_heads) and tanh, the
        two heads, the loss and their backward run as one hh_heads_loss (heads_loss, unscaled: the step calls total.backward()), in all
        three step modes, with grad_clip and shuffle_sequences as before.
        group (keyword only, taken like heads): None (the default: one process, nothing changes) or a learner/shards.py group, eager step modes only.  The update is then
        data-parallel over group.W shards and writes the bytes ONE process over the W shards writes (_PolicySGD.run_sharded): every shard
        cuts its own batch into minibatches of max(1, sgd_minibatch_size // W) rows, the shards' gradients are packed (hh_grad_pack),
        gathered and added in shard order (hh_grad_combine) before the unchanged clip, Adam step and commit, and the advantages are
        standardised over all shards' rows (standardize_shards).  ShardGroup(): this process is one of W torch.distributed ranks; `update`
        and `update_window` are collective and take what they take today.  LocalShards(K): the in-process twin; they take sequences of K
        batches or rollouts, and one bank or K.  The dicts gain rows_local; steps and rows count all shards.  What W ranks gain on real
        hardware is unmeasured."""
        self.optimizer = _learner_options(
            self, "PPOLearner", device, optimizer, step, grad_clip, shuffle_sequences, kl_coeff, fused,
            dict(clip_param=clip_param, kl_target=kl_target, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff, entropy_coeff=entropy_coeff),
            dict(num_sgd_iter=num_sgd_iter, sgd_minibatch_size=sgd_minibatch_size, max_seq_len=max_seq_len, seed=seed), self._heads_arg, trunk)
        self.group = _shard_group(self._group_arg, self.step)
        self.kinds = tuple(int(k) for k in kinds)
        assert len(self.kinds) == 2 and PN.HAS_ATT[self.kinds[0]] == PN.HAS_ATT[self.kinds[1]]
        self.attention, self.inputs, self.trunk = attention, inputs, _trunk_mode(trunk)
        # tied once, before the move: tie hands every module the first one's shared_layer MODULE, and nn.Module.to() moves a module's
        # tensors in place without ever replacing a submodule object, so the one layer stays the one layer on the device
        self.modules = tie([TrainableNet(k, attention=attention, inputs=inputs, trunk=trunk, heads=self.heads).load_numpy({k2: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k2, v in sd.items()})
                            for k, sd in zip(self.kinds, state_dicts)])
        for m in self.modules:
            m.to(self.device)
        self.recurrent = PN.HAS_ATT[self.kinds[0]]
        esc = not self.recurrent
        # per policy its own driver: the module's Adam, the step book, kl_coeff; one stage launch of every column
        # (heads="fused": the forward callable stops at the pre-activations and the loss callable is the fused tail)
        tail = self.heads == "fused"
        # the drivers and their callables reach the learner through a weak proxy: no reference cycle, so a dropped learner and its captured
        # graphs are freed at once by reference counting, never later by the cyclic collector in the middle of some other capture
        me = weakref.proxy(self)
        self._sgd = [_PolicySGD(me, m, lr, kl_coeff, self.optimizer == "fused",
                                forward=(lambda mb, m=m: m.pre_heads(mb["obs"], mb["critic"])) if tail else (lambda mb, m=m: m(mb["obs"], mb["critic"])),
                                loss=(lambda za, zc, mb, kl, a=a: me.heads_loss(a, za, zc, mb, kl)) if tail else (lambda logits, vf, mb, kl, a=a: me.loss(a, logits, vf, mb, kl)),
                                stage_groups=lambda names: [(names, 1 if esc else me.max_seq_len)], policy=a, noun="chunks")
                     for a, m in enumerate(self.modules)]
        self.optimizers = [d.optimizer for d in self._sgd]
        self._books = [d.book for d in self._sgd] if self.optimizer == "fused" else None
        self._sel = (pilots.SEL_ESC1 if esc else pilots.SEL_FIGHT1, pilots.SEL_ESC2 if esc else pilots.SEL_FIGHT2)
        self._tmp = None

    @property
    def kl_coeff(self):
        """per policy the current coefficient of the KL term (the drivers hold them; update_kl moves each after its policy's passes)"""
        return [d.kl_coeff for d in self._sgd]

    @kl_coeff.setter
    def kl_coeff(self, values):
        for d, v in zip(self._sgd, values):
            d.kl_coeff = float(v)

    @classmethod
    def trainable_init(cls, device, mode="fight", seed=0, **kw):
        """the learner whose weights equal PolicyBank.trainable_init(device, mode, seed)'s (tied shared layer)"""
        kinds = (PN.FIGHT1, PN.FIGHT2) if mode == "fight" else (PN.ESC1, PN.ESC2)
        sds = [dict(PN.random_weights(k, seed), **PN.random_critic_weights(k, seed)) for k in kinds]
        return cls(kinds, sds, device, seed=seed, **kw)

    # ---- the batch
    def old_logits(self, obs, bank, n_arenas):
        """the sampler's logits of every row of obs f32 [R, 2, D] from `bank` -> f32 [R, 2, 32]; calls of [n_arenas, 2] rows each"""
        R, _, D = obs.shape
        N = int(n_arenas)
        assert 2 * N <= bank.max_rows, "the bank serves the rollout's [N, 2] rows"
        n_calls = (R + N - 1) // N
        out = torch.zeros((max(n_calls, 1) * N, 2, OLD_LD), dtype=torch.float32, device=obs.device)
        if self._tmp is None or self._tmp[0].shape[0] != N or self._tmp[0].shape[2] != D:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=obs.device)
            self._tmp = (z((N, 2, D), torch.float32), z((N, 2, 4), torch.int8), z((N, 2), torch.float32),
                         torch.tensor(self._sel, dtype=torch.uint8, device=obs.device).repeat(N, 1).contiguous())
        stage, act, logp, sel = self._tmp
        for i in range(n_calls):
            src = obs[i * N:(i + 1) * N]
            if src.shape[0] < N:
                stage.zero_()
                stage[:src.shape[0]].copy_(src)
                src = stage
            bank.sample(src, sel, greedy=True, actions=act, logp=logp, logits=out[i * N:(i + 1) * N], want_vf=False)
        return out[:R]

    def batch_old_logits(self, rows, bank, n_arenas=None):
        """old_logits f32 [R, 2, 32] of an emitted batch (`rows`: EpisodeBatch.rows()): the batch's own `logits` column where the
        rollout recorded one (the very tensor, no bank call); otherwise recomputed from `bank` (old_logits; n_arenas: the rollout's N)"""
        if "logits" in rows:
            lg = rows["logits"]
            if lg.dtype != torch.float32 or tuple(lg.shape) != (rows["obs"].shape[0], 2, OLD_LD):
                raise ValueError(f"the batch's logits column must be f32 [R, 2, {OLD_LD}], got {lg.dtype} {tuple(lg.shape)}")
            return lg
        if bank is None or n_arenas is None:
            raise ValueError("the batch has no logits column (PPORollout(record_logits=True)): a bank and n_arenas are needed to recompute them")
        return self.old_logits(rows["obs"], bank, n_arenas)

    def policy_batch(self, rows, old_logits, agent, adv=None):
        """the training batch of policy `agent` (0 | 1) from the emitted rows: dict of [S, L, ...] chunks (fight) or [R, ...] rows (escape)
        and, for chunks, seq_len [S] and mask [S, L].  adv: the agent's advantages f32 [R] already standardised (over all shards of a
        group); default: standardised here over this batch"""
        kind = self.kinds[agent]
        b = {"obs": rows["obs"][:, agent, :PN.OBS_DIM[kind]].contiguous(),
             "critic": central_critic_rows(rows["obs"], rows["actions"], agent + 1),
             "actions": rows["actions"][:, agent].contiguous(), "old_logp": rows["logp"][:, agent].contiguous(),
             "adv": standardize(rows["adv"][:, agent]) if adv is None else adv, "target": rows["target"][:, agent].contiguous(),
             "old_logits": old_logits[:, agent].contiguous()}
        if not self.recurrent:
            return b
        seq_start, seq_len = cut_chunks(rows["ep_start"], rows["ep_len"], self.max_seq_len)
        b = {k: pad_chunks(v, seq_start, seq_len, self.max_seq_len) for k, v in b.items()}
        b["seq_len"] = seq_len
        b["mask"] = chunk_mask(seq_len, self.max_seq_len).to(torch.uint8)
        return b

    # ---- one minibatch step
    def loss(self, agent, logits, vf, mb, kl_coeff=None):
        """the policy's loss of one minibatch; kl_coeff: the KL term's coefficient, default the policy's current one"""
        return (ppo_loss if self.fused else ppo_loss_torch)(logits, vf, mb, n_comp=n_comp_of(self.kinds[agent]), **_loss_kw(self, self._sgd[agent], kl_coeff))

    def heads_loss(self, agent, za, zc, mb, kl_coeff=None):
        """heads="fused": the policy's loss of one minibatch from pre_heads' (za, zc), through heads_loss with the module's act_out and
        val_out; the gradients are handed to total.backward() unscaled"""
        m = self.modules[agent]
        return heads_loss(za, zc, m.act_out, m.val_out, mb, n_comp=n_comp_of(self.kinds[agent]), scale_grad=False, **_loss_kw(self, self._sgd[agent], kl_coeff))

    def _columns(self, b, staged=False):
        """policy_batch's dict as the driver takes it -> (columns [S, ...], host seq_len [S]: the chunks' lengths, ones for escape rows).
        staged: as the graph's stage reads them — contiguous, the mask uint8, and for the escape kinds a mask of ones, which the padding
        rows of the staging buffers need"""
        cols = {k: (v.contiguous() if staged else v) for k, v in b.items() if k != "seq_len"}
        S = cols["obs"].shape[0]
        seq_len = b["seq_len"].cpu().numpy() if self.recurrent else np.ones(S, dtype=np.int64)
        if staged:
            if not self.recurrent:
                cols["mask"] = torch.ones((S,), dtype=torch.uint8, device=self.device)
            cols["mask"] = cols["mask"].to(torch.uint8)
        return cols, seq_len

    # the steps themselves are the driver's (_PolicySGD): one per policy
    def minibatch_step(self, agent, mb):
        """forward, loss, backward, Adam step on one minibatch (a dict sliced from policy_batch's, with n_valid) -> stats f64 [6] (device)"""
        return self._sgd[agent].minibatch_step(mb)

    def graph_prepare(self, agent, b, cap=None):
        """Everything one policy's pass needs before its first replay (_PolicySGD.graph_prepare on policy_batch `b`): the schedule and the
        batch's columns uploaded, the cursor set to 0, and the graph of ONE minibatch step — stage, forward, loss, backward, Adam, commit —
        captured unless an earlier one still fits.  cap: the staging capacity in chunks (escape: rows).  -> (n_steps, rows)"""
        if self.step != "graph":
            raise ValueError('graph_prepare needs PPOLearner(step="graph")')
        return self._sgd[agent].graph_prepare(*self._columns(b, staged=True), cap)

    def graph_replay(self, agent, n=1):
        """n minibatch steps of policy `agent` from its captured graph, no host work between them"""
        self._sgd[agent].graph_replay(n)

    def graph_stats(self, agent, n):
        """the statistics rows f64 [n, 6] of the first n steps since graph_prepare (one device tensor; reading it synchronises)"""
        return self._sgd[agent].graph_stats(n)

    def grad_gnorm(self, agent, n):
        """grad_clip: the mean of the first n steps' norms before clipping since the update began (a float; reading it synchronises)"""
        return self._sgd[agent].grad_gnorm(n)

    # ---- one update
    def update(self, episodes, bank=None):
        """one PPO update of both policies from episodes (an EpisodeBatch after a collect) -> per policy a dict: total_loss, policy_loss,
        vf_loss, kl, entropy (means over the minibatch steps), kl_coeff (after the update), steps (minibatch steps taken), rows.
        `bank` is read only when the batch has no `logits` column (batch_old_logits).  With grad_clip also grad_gnorm.
        An EpisodeBatch built with train_batch_size hands over its accumulated batch (RLlib's train_batch_size: update once
        `episodes.ready()`, e.g. after `PPORollout.collect_batch()`); nothing else changes here."""
        if self.group is not None:
            return self._update_sharded(episodes, bank, window=False)
        rows = episodes.rows()
        if rows["obs"].shape[0] == 0:
            return [d.empty() for d in self._sgd]
        with torch.no_grad():
            old = self.batch_old_logits(rows, bank, episodes.N)
            batches = [self.policy_batch(rows, old, a) for a in range(2)]
        out = [d.run(*self._columns(b, staged=self.step == "graph")) for d, b in zip(self._sgd, batches)]
        self.updates += 1
        return out

    # ---- one update from a fixed window (batch_mode = "truncate_episodes")
    def _check_window(self, rollout):
        """the refusals of window_batch / update_window -> (T, N)"""
        if getattr(rollout, "semantics", "rllib") != "rllib":
            raise ValueError("PPOLearner trains RLlib's unmasked view: a PPORollout(semantics='masked') window has its dead agents' rows cut out of adv and target")
        for k in ("obs", "actions", "logp", "adv", "target", "done", "T", "w"):
            if not hasattr(rollout, k):
                raise ValueError(f"window_batch takes a PPORollout (its [T, N] buffers); this object has no `{k}`")
        esc = rollout.w.cfg.agent_mode == L.MODE_ESCAPE
        if rollout.obs.dim() != 4 or rollout.obs.shape[2] != 2 or esc == self.recurrent or rollout.obs.shape[3] < max(PN.OBS_DIM[k] for k in self.kinds):
            raise ValueError(f"the rollout's world flies {'escape' if esc else 'fight'} mode with observations {tuple(rollout.obs.shape[2:])}; "
                             f"this learner trains kinds {self.kinds} ({'fight' if self.recurrent else 'escape'})")
        if not getattr(rollout, "collects", 0):
            raise RuntimeError("the rollout has not collected yet: its window buffers hold nothing (rollout.collect() first)")
        return rollout.T, rollout.w.N

    def _window_shared(self, rollout, bank):
        """what both policies' window batches share: the cut, the sampler's logits [T, N, 2, 32] and the advantages in arena-major rows"""
        T, N = self._check_window(rollout)
        tables = window_cut(rollout.done, self.max_seq_len if self.recurrent else 1)
        if getattr(rollout, "record_logits", False):
            logits = rollout.logits
        else:
            if bank is None:
                raise ValueError("the rollout recorded no logits (PPORollout(record_logits=True)): a bank is needed to recompute them")
            logits = self.old_logits(rollout.obs[:T].reshape(T * N, 2, rollout.obs.shape[3]), bank, N).reshape(T, N, 2, OLD_LD)
        adv_rows = rollout.adv.transpose(0, 1).reshape(N * T, 2)      # [R, 2], r = n T + t: what the episode path's rows["adv"] would hold
        return T, N, tables, logits.contiguous(), adv_rows

    def window_batch(self, rollout, bank, agent, shared=None, adv=None):
        """the training batch of policy `agent` (0 | 1) from a PPORollout's [T, N] window, in policy_batch's format and — fed the same
        rows as episodes (the window's fragments, arena-major) — with policy_batch's values: fight kinds [S, L, ...] chunks with seq_len
        and mask (a chunk ends at a done row, at max_seq_len rows or at the window's end: window_cut), escape kinds [R, ...] with R = T N
        rows, arena-major (r = n T + t: the cut with max_seq_len = 1, the length-1 axis dropped).  One hh_window_gather launch of seven
        columns reads the rollout's buffers as they lie.  The trailing fragment of an arena carries RLlib's truncation bootstrap from
        vf[T] in adv and target (hh_gae_rllib).  `bank` is read only when the rollout recorded no logits.  The advantages are standardised
        over the agent's T N values (standardize).  shared: _window_shared's tuple (update_window builds it once for both policies).
        adv: the agent's advantages f32 [N T], arena-major, already standardised (over all shards of a group) in place of that."""
        T, N, tables, logits, adv_rows = self._window_shared(rollout, bank) if shared is None else shared
        kind = self.kinds[agent]
        Lm = self.max_seq_len if self.recurrent else 1
        D, Dk = rollout.obs.shape[3], PN.OBS_DIM[kind]
        critic = central_critic_rows(rollout.obs[:T], rollout.actions, agent + 1).contiguous()
        adv = (standardize(adv_rows[:, agent]) if adv is None else adv).reshape(N, T).t().contiguous()          # back to [T, N]: where the gather reads a row (t, n)
        names = ("obs", "critic", "actions", "old_logp", "adv", "target", "old_logits")
        got = window_gather([(rollout.obs, (Dk,), agent * D * 4, False), (critic, (critic.shape[2],), 0, False),
                             (rollout.actions, (4,), agent * 4, False), (rollout.logp, (), agent * 4, False), (adv, (), 0, False),
                             (rollout.target, (), agent * 4, False), (logits, (OLD_LD,), agent * OLD_LD * 4, False)], tables, Lm)
        if not self.recurrent:
            return {k: v[:, 0] for k, v in zip(names, got)}
        b = dict(zip(names, got))
        b["seq_len"] = tables[2].long()
        b["mask"] = chunk_mask(b["seq_len"], Lm).to(torch.uint8)
        return b

    def update_window(self, rollout, bank=None):
        """one PPO update of both policies from a PPORollout's [T, N] window as the last collect left it (batch_mode =
        "truncate_episodes", the rollouts' default; the buffers are the same in both modes) -> what `update` returns, with rows = T N.
        Every row of the window was sampled by the weights the sampler holds, so nothing is carried, nothing overflows and no start()
        is needed after publish:

            ro.collect();  stats = learner.update_window(ro, bank);  learner.publish(bank)

        The batches are window_batch's; from there on it is `update`: the same _columns and driver, so fused, attention, inputs, trunk,
        heads, optimizer, step="graph", grad_clip and shuffle_sequences act as they do there, and the row count T N is the same in every
        update.  The rollout's buffers are only read."""
        if self.group is not None:
            return self._update_sharded(rollout, bank, window=True)
        with torch.no_grad():
            shared = self._window_shared(rollout, bank)
            batches = [self.window_batch(rollout, bank, a, shared) for a in range(2)]
        out = [d.run(*self._columns(b, staged=self.step == "graph")) for d, b in zip(self._sgd, batches)]
        self.updates += 1
        return out

    # ---- one update over the shards of a group (learner/shards.py)
    def _per_shard(self, x, what):
        """what this process's shards train on, one entry per group.local: a ShardGroup rank holds one shard and takes `x` as it is; a
        LocalShards(K) learner takes a sequence of K"""
        K = len(self.group.local)
        if not getattr(self.group, "in_process", False):
            return [x]
        if not isinstance(x, (list, tuple)) or len(x) != K:
            raise ValueError(f"a LocalShards({K}) learner takes a sequence of {K} {what}, one per shard")
        return list(x)

    def _update_sharded(self, sources, bank, window):
        """`update` (window False: EpisodeBatches) or `update_window` (True: PPORollouts) with a group: the batches are today's, except
        that every policy's advantages are standardised over all shards' rows, then the drivers' run_sharded.  Collective.  A shard
        without rows takes part with empty steps; when no shard has a row the result is the empty update's and nothing is counted."""
        group = self.group
        srcs = self._per_shard(sources, "rollouts" if window else "EpisodeBatches")
        banks = list(bank) if isinstance(bank, (list, tuple)) else [bank] * len(srcs)
        if len(banks) != len(srcs):
            raise ValueError(f"one bank or one per shard ({len(srcs)}), got {len(banks)}")
        with torch.no_grad():
            pre, advs = [], []
            for src, bk in zip(srcs, banks):
                if window:
                    pre.append(self._window_shared(src, bk))
                    advs.append(pre[-1][4])
                else:
                    rows = src.rows()
                    pre.append((rows, self.batch_old_logits(rows, bk, src.N)) if rows["obs"].shape[0] else None)
                    advs.append(rows["adv"])
            batches = []
            for a in range(2):
                std, n_all = standardize_shards([x[:, a] for x in advs], group)
                if n_all == 0:
                    return [dict(d.empty(), rows_local=0) for d in self._sgd]
                batches.append([None if p is None else
                                (self.window_batch(src, bk, a, p, adv=x) if window else self.policy_batch(p[0], p[1], a, adv=x))
                                for src, bk, p, x in zip(srcs, banks, pre, std)])
        out = [d.run_sharded(group, [(None, []) if b is None else self._columns(b) for b in bs]) for d, bs in zip(self._sgd, batches)]
        self.updates += 1
        return out

    # ---- checkpointing (hhmarl_2d_amd/checkpoint.py)
    _SHARED = ("shared_layer._model.0.weight", "shared_layer._model.0.bias")

    def _options(self):
        sharded = {} if self.group is None else dict(shards=self.group.W)      # a learner without a group saves what it always saved
        return _learner_saved_options(self, self.optimizer, kinds=self.kinds, attention=self.attention, inputs=self.inputs, trunk=self.trunk, **sharded)

    def state_dict(self):
        """the two modules (the tied shared layer once, with the first), `updates` — it seeds minibatch_order and sequence_order —, per
        policy kl_coeff and the Adam state (DeviceAdam's m, v, t or torch.optim.Adam's own), and the constructor options that decide the
        arithmetic or the schedule.  Captured step graphs are not saved."""
        mods = [{k: ck.cpu(v) for k, v in m.state_dict().items() if not (a and k in self._SHARED)} for a, m in enumerate(self.modules)]
        return {"options": self._options(), "updates": int(self.updates), "modules": mods, "policies": [d.state_dict() for d in self._sgd]}

    def _load_plan(self, sd):
        ck.need_keys("PPOLearner", sd, ("options", "updates", "modules", "policies"))
        ck.check_options("PPOLearner", sd["options"], self._options())
        if isinstance(sd["updates"], bool) or not isinstance(sd["updates"], int) or sd["updates"] < 0:
            raise ValueError("PPOLearner: `updates` is a count")
        for k in ("modules", "policies"):
            if not isinstance(sd[k], (list, tuple)) or len(sd[k]) != 2:
                raise ValueError(f"PPOLearner: `{k}` holds one entry per policy (2)")
        pairs = []
        for a, m in enumerate(self.modules):
            pairs += _module_plan(f"PPOLearner modules[{a}]", m, sd["modules"][a], self._SHARED if a else ())
        drivers = [d._load_plan(p) for d, p in zip(self._sgd, sd["policies"])]

        def commit():
            ck.copy_pairs(pairs)
            for d in drivers:
                d()
            self.updates = sd["updates"]
        return commit

    def load_state_dict(self, sd):
        """state_dict()'s dict back in place (parameters, m, v, t by copy_: captured step graphs replay, the shared layer stays tied);
        everything is validated first — ValueError names the field and nothing was changed"""
        self._load_plan(sd)()

    def publish(self, bank):
        """the new weights into the sampler's bank on the current stream (PolicyBank.refresh_trainable): captured collects replay with them"""
        bank.refresh_trainable(self.modules)

    # ---- the curriculum's policy files (hhmarl_2d_amd/policy_files.py)
    def export_policies(self, policy_dir, level, agent_mode=None):
        """The two modules' current weights as `L{level}_AC1_{mode}.pt` and `L{level}_AC2_{mode}.pt` in policy_dir (created where it is
        missing), in policy_files' plain format: what train_hetero.py:101-105 writes through policy_export.py, and what the next
        levels, HighLevelEnv and the evaluators pick up by name (PolicyBank.from_reference_dir).  The reference exports from level 3 on;
        any level 1..5 is taken here.  agent_mode defaults to the mode of the learner's kinds; one that contradicts them is refused.
        Both files carry the one tied shared_layer.  Synchronises (the weights are read back to the host).  -> the two paths"""
        import os
        from .. import policy_files as PF
        mode = PF.mode_of_kinds(self.kinds)
        if agent_mode is not None and agent_mode != mode:
            raise ValueError(f"export_policies: this learner trains the {mode} policies (kinds {self.kinds}), not agent_mode={agent_mode!r}")
        names = [PF.policy_file_name(level, ac, mode) for ac in (1, 2)]
        os.makedirs(policy_dir, exist_ok=True)
        torch.cuda.synchronize(self.device)
        return [PF.save_policy(os.path.join(policy_dir, name), kind, m.state_dict(), level=level, agent_mode=mode)
                for name, kind, m in zip(names, self.kinds, self.modules)]

    @classmethod
    def from_policy_files(cls, device, policy_dir, level, agent_mode, **kw):
        """The learner whose modules hold the weights of `L{level}_AC{1,2}_{agent_mode}.pt` in policy_dir (files of policy_files' plain
        format: export_policies).  The weights only: Adam state, kl_coeff and the update count start fresh (a run is continued with all
        of them through checkpoint.load_subset).  The two files of one export hold the same shared_layer; files whose shared layers
        differ in any bit are refused with ValueError, not silently tied to the first.  kw: the constructor's options."""
        import os
        from .. import policy_files as PF
        PF.policy_file_name(level, 1, agent_mode)      # level and agent_mode refused here, before a file is looked for
        kinds = PF.MODE_KINDS[agent_mode]
        sds = []
        for ac, want in zip((1, 2), kinds):
            path = os.path.join(policy_dir, PF.policy_file_name(level, ac, agent_mode))
            kind, sd = PF.load_policy(path)
            if kind != want:
                raise ValueError(f"from_policy_files: {path} holds a {PN.KIND_NAMES[kind]} network, the {agent_mode} policy of aircraft type {ac} is {PN.KIND_NAMES[want]}")
            sds.append(sd)
        for k in cls._SHARED:
            if not torch.equal(sds[0][k].view(torch.int32), sds[1][k].view(torch.int32)):
                raise ValueError(f"from_policy_files: `{k}` differs between the two files of {policy_dir}: the two policies of a trainer "
                                 "hold ONE shared layer (files of two different exports?)")
        return cls(kinds, sds, device, **kw)
