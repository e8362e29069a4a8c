"""CommanderLearner: the PPO update of train_hier.py's commander_policy"""
import weakref

import torch
import torch.nn.functional as F

from .. import _lib as L
from ..rollout import central_critic_rows_hl
from .batch import chunk_mask, standardize_masked, window_cut, window_gather
from .loss import CMD_LD, _loss_kw, heads_loss, ppo_loss_categorical, ppo_loss_categorical_torch
from .nets import CommanderTrainable
from .ops import GRU_H, _trunk_mode
from .. import checkpoint as ck
from .step import _heads_keyword, _learner_options, _learner_saved_options, _module_plan, _PolicySGD

# what CommanderLearner(step="graph") stages per minibatch: eight columns [S, L, ...] per step, then two per sequence
COMMANDER_STAGE_COLS = ("obs", "critic", "actions", "old_logp", "adv", "target", "mask", "old_logits", "state_in", "seq_len")


# ------------------------------------------------------------------------------------------------------------------ the learner
class CommanderLearner:
    """One PPO update of train_hier.py's commander_policy from the `CommanderEpisodeBatch` of a
    `CommanderRollout(batch_mode="complete_episodes")` — for the commander what `PPOLearner` is for the 2-vs-2 policies:

        learner = CommanderLearner.trainable_init(device, seed=6)          # the weights of commander.random_weights(6)
        stats = learner.update(ro.episodes, net)
        learner.publish(net)                                               # CommanderNet.refresh_weights: captured collects replay with them

    Defaults: train_hier.py:186 (lr 1e-4, clip_param 0.25, kl_target 0.05, sgd_minibatch_size 256) and RLlib 2.4's PPO defaults for the
    rest (kl_coeff 0.2, vf_clip_param 10, num_sgd_iter 30, max_seq_len 20 — the rollout cuts the sequences, with the same max_seq_len:
    `update` refuses a batch cut to another length).
      * the three agents map to ONE policy: one module, one Adam.  The batch is the three agents' trajectories: 3 S sequences from
        `episodes.sequences()`'s S, AGENT-MAJOR — sequence a S + s is agent a's column of arena-row sequence s, with that agent's
        state_in[s, a], its own observation, and critic rows from central_critic_rows_hl (actions filled in, while the batch's `vf` and
        the stored rnn_val states were sampled with zero action inputs: RLlib has that difference, and so does this);
      * nothing is masked by `valid`; the mask is the unpadded steps.  Advantages are standardised over the whole batch (all three
        agents' unpadded rows);
      * old_logits (RLlib's ACTION_DIST_INPUTS): `batch_old_logits`.  With CommanderRollout(record_logits=True) the sequences carry a
        `logits` column — for every step the logits of the sampler's own forward (the split-fp16 MFMA kernel that drew the action
        and wrote logp), with the weights it held at that step — and it is used as it stands, agent-major like the other columns:
        old_logp and old_logits of a row come from one forward, also for rows sampled before the last publish.
        Without the column they are recomputed once per update, under no_grad, by the module's own float32 forward with the
        pre-update weights from the stored sequence-start states.  Only then does this approximation apply: that forward is not the
        sampler's, and rows carried over from before the last publish (the head of an episode that was still running) were sampled
        by older weights — their stored logp, and so the ratio, is exact, but their recomputed old_logits are the newer weights', so
        the KL term sees them as on-policy (`rollout.start()` after `publish` avoids that part by throwing the running episodes away);
      * num_sgd_iter passes; in each the sequences, in batch order, are split into consecutive minibatches of at least
        sgd_minibatch_size unpadded rows (minibatch_partition), visited in the order of minibatch_order(seed, update count, 0, pass);
      * after the passes KLCoeffMixin.update_kl (kl_coeff_update) on the mean of the minibatches' mean_kl.
    fused = False computes the loss with torch ops (ppo_loss_categorical_torch) and steps the GRU cell with torch ops
    (gru_sequence_torch) instead of hh_ppo_loss_categorical and hh_gru_seq_*; nothing else differs.
    optimizer="fused", step="graph" replays every minibatch step from one captured HIP graph, as PPOLearner's do (graph_prepare;
    DESIGN.md section 19): the same minibatches in the same order, no Python, autograd dispatch or torch.optim.Adam between launches."""

    @_heads_keyword
    def __init__(self, state_dict, device, lr=1e-4, clip_param=0.25, kl_target=0.05, kl_coeff=0.2, vf_clip_param=10.0, vf_loss_coeff=1.0,
                 entropy_coeff=0.0, num_sgd_iter=30, sgd_minibatch_size=256, max_seq_len=20, seed=0, fused=True, inputs="torch", trunk="torch",
                 optimizer="torch", step="eager", shuffle_sequences=False, grad_clip=None):
        """state_dict: CommanderGru's tensors (numpy or torch), keyed like commander.state_keys().  inputs: CommanderTrainable's argument
        ("fused": inp1..inp4 and v1..v4 through hh_input_stage_*); trunk: its argument too ("fused": shared_layer through hh_dense_tanh_*).
        optimizer, step: PPOLearner's arguments, with its values, defaults and validation.  optimizer="fused" makes `self.optimizer` a
        DeviceAdam (m, v and the step count on the device: hh_adam_step) and gathers the steps' statistics in a device table
        (hh_train_commit); step="graph" (needs optimizer="fused") captures stage -> stage -> forward -> loss -> backward -> Adam -> commit
        once as ONE HIP graph and replays it per minibatch step (graph_prepare).  The modes are kept in `optimizer_mode` and `step`.
        grad_clip: PPOLearner's argument (None: nothing changes; else the global L2 norm of the module's gradients is clipped to it in every
        step — norm -> clipped Adam in the fused modes and in the graph — and update() also returns grad_gnorm).
        shuffle_sequences: PPOLearner's argument (False, the default: nothing changes).  True: every pass draws its own order of the 3 S
        sequences, sequence_order(seed, update count, 0, pass), and cuts that order into minibatches (shuffled_schedule); state_in and
        seq_len travel with their sequences.  The eager modes gather with index_select; the graph's two stage launches become
        hh_minibatch_stage_gather through one order table of 4 * num_sgd_iter * 3 S bytes, uploaded once per update into a persistent
        buffer (grown to twice the need).  Slot 0 of a staged minibatch is a real sequence, so seq_len[0] >= 1 holds as before.  What
        shuffling does to learning curves has not been measured here.
        heads (keyword only, taken by _heads_keyword in front of this signature): PPOLearner's argument ("torch", the default: nothing changes; "fused", with fused=True and trunk="torch": the
        step's forward stops at CommanderTrainable.pre_heads and the tail is one hh_heads_loss with n_comp = 1).
        group (keyword only, taken like heads): PPOLearner's argument; only None is taken for now (the driver's sharded run is shared, the commander's batch code over
        shards is not written), anything else is a ValueError."""
        if self._group_arg is not None:
            raise ValueError("CommanderLearner takes group=None for now: sharded updates are PPOLearner's (learner/shards.py)")
        self.optimizer_mode = _learner_options(
            self, "CommanderLearner", device, optimizer, step, grad_clip, shuffle_sequences, kl_coeff, fused,
            dict(clip_param=clip_param, kl_target=kl_target, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff, entropy_coeff=entropy_coeff),
            dict(num_sgd_iter=num_sgd_iter, sgd_minibatch_size=sgd_minibatch_size, max_seq_len=max_seq_len, seed=seed), self._heads_arg, trunk)
        self.inputs, self.trunk = inputs, _trunk_mode(trunk)
        self.module = CommanderTrainable(inputs=inputs, trunk=trunk, heads=self.heads).load_numpy({k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
                                                       for k, v in state_dict.items()}).to(self.device)
        # the one policy's driver.  hh_minibatch_stage takes 8 columns: the per-step columns (chunks of max_seq_len rows) in one launch, the
        # per-sequence ones (state_in, seq_len: chunks of one row) in a second
        # (heads="fused": the forward callable stops at the pre-activations and the loss callable is the fused tail)
        args = lambda mb: (mb["obs"], mb["critic"], mb["state_in"], mb["seq_len"])
        tail = self.heads == "fused"
        # the driver and its callables reach the learner through a weak proxy (a bound method would hold it): no reference cycle, so a
        # dropped learner and its captured graph are freed at once by reference counting, never later by the cyclic collector in the
        # middle of some other capture
        me = weakref.proxy(self)
        self._sgd = _PolicySGD(me, self.module, lr, kl_coeff, self.optimizer_mode == "fused",
                               forward=(lambda mb: me.module.pre_heads(*args(mb), fused_gru=me.fused)) if tail else (lambda mb: me.module(*args(mb), fused_gru=me.fused)),
                               loss=(lambda za, zc, mb, kl: me.heads_loss(za, zc, mb, kl)) if tail else (lambda logits, vf, mb, kl: me.loss(logits, vf, mb, kl)),
                               stage_groups=lambda names: [(names[:L.STAGE_MAX_COLS], me.max_seq_len), (names[L.STAGE_MAX_COLS:], 1)],
                               policy=0, noun="sequences")
        self.optimizer, self._book = self._sgd.optimizer, self._sgd.book

    @property
    def kl_coeff(self):
        """the current coefficient of the KL term (the driver holds it; update_kl moves it after the passes)"""
        return self._sgd.kl_coeff

    @kl_coeff.setter
    def kl_coeff(self, value):
        self._sgd.kl_coeff = float(value)

    @classmethod
    def trainable_init(cls, device, seed=0, **kw):
        """the learner whose weights equal commander.random_weights(seed)'s (what CommanderNet.set_weights(random_weights(seed)) samples with)"""
        from ..commander import random_weights
        return cls(random_weights(seed), device, seed=seed, **kw)

    # ---- the batch
    @staticmethod
    def policy_batch(seqs, old_logits=None):
        """the training batch from CommanderEpisodeBatch.sequences()' dict (S arena-row sequences of L steps): dict of agent-major
        [3 S, L, ...] tensors — obs [.., 34], critic [.., 105], actions i8, old_logp, adv (standardised over all unpadded rows), target,
        mask u8, and per sequence state_in [3 S, 2, 200] and seq_len i32 [3 S]; old_logits f32 [3 S, L, 4] where given"""
        obs, actions, mask = seqs["obs"], seqs["actions"], seqs["mask"]
        agents = range(obs.shape[2])
        cat = lambda f: torch.cat([f(a) for a in agents], dim=0).contiguous()
        m3 = cat(lambda a: mask)
        b = {"obs": cat(lambda a: obs[:, :, a]),
             "critic": cat(lambda a: central_critic_rows_hl(obs, actions, a + 1)),
             "actions": cat(lambda a: actions[:, :, a]), "old_logp": cat(lambda a: seqs["logp"][:, :, a]),
             "adv": standardize_masked(cat(lambda a: seqs["adv"][:, :, a]), m3), "target": cat(lambda a: seqs["target"][:, :, a]),
             "mask": m3.to(torch.uint8), "state_in": cat(lambda a: seqs["state_in"][:, a]),
             "seq_len": cat(lambda a: seqs["seq_lens"]).to(torch.int32)}
        if old_logits is not None:
            b["old_logits"] = old_logits
        return b

    def old_logits(self, b, chunk=4096):
        """the module's logits of every row of policy_batch's dict with the weights as they stand, no autograd -> f32 [3 S, L, 4] (column 3 zero)"""
        out = []
        with torch.no_grad():
            for s0 in range(0, b["obs"].shape[0], chunk):
                sl = slice(s0, s0 + chunk)
                lg, _ = self.module(b["obs"][sl], b["critic"][sl], b["state_in"][sl], b["seq_len"][sl], fused_gru=self.fused)
                out.append(F.pad(lg, (0, 1)))
        return torch.cat(out, dim=0) if out else torch.zeros(tuple(b["obs"].shape[:2]) + (CMD_LD,), device=b["obs"].device)

    def batch_old_logits(self, seqs, b=None):
        """old_logits f32 [3 S, L, 4], agent-major, of CommanderEpisodeBatch.sequences()' dict: its own `logits` column [S, L, 3, 4] where
        the rollout recorded one (no forward); otherwise the module's (old_logits; b: policy_batch(seqs), built when not given)"""
        if "logits" in seqs:
            lg = seqs["logits"]
            if lg.dtype != torch.float32 or tuple(lg.shape) != tuple(seqs["obs"].shape[:3]) + (CMD_LD,):
                raise ValueError(f"the sequences' logits column must be f32 [S, L, 3, {CMD_LD}], got {lg.dtype} {tuple(lg.shape)}")
            return torch.cat([lg[:, :, a] for a in range(lg.shape[2])], dim=0).contiguous()
        return self.old_logits(self.policy_batch(seqs) if b is None else b)

    # ---- one minibatch step
    def loss(self, logits, vf, mb, kl_coeff=None):
        """the loss of one minibatch; kl_coeff: the KL term's coefficient, default the current one"""
        return (ppo_loss_categorical if self.fused else ppo_loss_categorical_torch)(logits, vf, mb, **_loss_kw(self, self._sgd, kl_coeff))

    def heads_loss(self, za, zc, mb, kl_coeff=None):
        """heads="fused": the loss of one minibatch from pre_heads' (za, zc), through heads_loss(n_comp=1) with the module's act_out and
        val_out; the gradients are handed to total.backward() unscaled"""
        m = self.module
        return heads_loss(za, zc, m.act_out, m.val_out, mb, n_comp=1, scale_grad=False, **_loss_kw(self, self._sgd, kl_coeff))

    def _columns(self, b, staged=False):
        """policy_batch's dict (with old_logits) as the driver takes it -> (columns [3 S, ...], host seq_len [3 S]).  staged: as the graph's
        two stages read them — the ten COMMANDER_STAGE_COLS in that order, eight per step and then state_in and seq_len per sequence,
        contiguous, mask uint8 and seq_len int32.  The sequences of the staging buffers beyond a minibatch's are zero in every column:
        sequences of length 0 (hh_gru_seq_*'s contract) whose rows the mask drops"""
        if not staged:
            return b, b["seq_len"].cpu().numpy()
        missing = [k for k in COMMANDER_STAGE_COLS if k not in b]
        if missing:
            raise ValueError(f"graph_prepare: the policy batch lacks {missing} (policy_batch, then old_logits from batch_old_logits)")
        cols = {k: b[k].contiguous() for k in COMMANDER_STAGE_COLS}
        cols["mask"], cols["seq_len"] = cols["mask"].to(torch.uint8), cols["seq_len"].to(torch.int32)
        return cols, cols["seq_len"].cpu().numpy()

    # the steps themselves are the driver's (_PolicySGD), as PPOLearner's are
    def minibatch_step(self, mb):
        """forward, loss, backward, Adam step on one minibatch (a dict sliced from policy_batch's, with old_logits and n_valid)
        -> stats f64 [6] (device)"""
        return self._sgd.minibatch_step(mb)

    def graph_prepare(self, b, cap=None):
        """Everything one update needs before its first replay (_PolicySGD.graph_prepare on policy_batch `b` with old_logits): the schedule
        and the batch's ten columns uploaded, the cursor set to 0, and the graph of ONE minibatch step — stage (per-step columns), stage
        (per-sequence columns), forward, loss, backward, Adam, commit — captured unless an earlier one still fits.  cap: the staging
        capacity in sequences.  -> (n_steps, rows)"""
        if self.step != "graph":
            raise ValueError('graph_prepare needs CommanderLearner(step="graph")')
        return self._sgd.graph_prepare(*self._columns(b, staged=True), cap)

    def graph_replay(self, n=1):
        """n minibatch steps from the captured graph, no host work between them"""
        self._sgd.graph_replay(n)

    def graph_stats(self, n):
        """the statistics rows f64 [n, 6] of the first n steps since graph_prepare (one device tensor; reading it synchronises)"""
        return self._sgd.graph_stats(n)

    def grad_gnorm(self, n):
        """grad_clip: the mean of the first n steps' norms before clipping since the update began (a float; reading it synchronises)"""
        return self._sgd.grad_gnorm(n)

    # ---- one update
    def update(self, episodes, net=None):
        """one PPO update of commander_policy from episodes (a CommanderEpisodeBatch after a collect) -> dict: total_loss, policy_loss,
        vf_loss, kl, entropy (means over the minibatch steps), kl_coeff (after the update), steps (minibatch steps taken), rows (unpadded,
        all three agents).  `net` (the sampler's CommanderNet) is not read: the old logits are the batch's own `logits` column or, without
        one, come from the module, which holds the weights the sampler was given at the last publish (batch_old_logits).  With grad_clip
        also grad_gnorm.  A CommanderEpisodeBatch built with train_batch_size hands over its accumulated batch (update once
        `episodes.ready()`, e.g. after `CommanderRollout.collect_batch()`); nothing else changes here."""
        seqs = episodes.sequences()
        if seqs["obs"].shape[1] != self.max_seq_len:
            raise ValueError(f"CommanderLearner(max_seq_len={self.max_seq_len}) was given sequences of {seqs['obs'].shape[1]} steps: the rollout "
                             "cuts them, so both take the same max_seq_len")
        if seqs["obs"].shape[0] == 0:
            return self._sgd.empty()
        with torch.no_grad():
            b = self.policy_batch(seqs)
            b["old_logits"] = self.batch_old_logits(seqs, b)
        out = self._sgd.run(*self._columns(b, staged=self.step == "graph"))
        self.updates += 1
        return out

    # ---- one update from a fixed window (batch_mode = "truncate_episodes")
    def window_sequences(self, rollout):
        """a CommanderRollout's [T, N] window in CommanderEpisodeBatch.sequences()' format: the window cut by THIS learner's max_seq_len
        (window_cut; the rollout's own max_seq_len is not read) and whole step-rows gathered by hh_window_gather — obs f32 [S, L, 3, 34],
        actions i8 / logp / vf / adv / target [S, L, 3] (zero past seq_len), seq_lens i32 [S], mask bool [S, L], state_in f32
        [S, 3, 2, 200] = rollout.state_in[seq_t0, seq_arena] (the state the sequence's first step used: zero at an episode start, the
        carried one where the window or a length cut opens mid-episode), and logits f32 [S, L, 3, 4] where the rollout recorded them.
        Sequences arena-major, then time."""
        for k in ("obs", "actions", "logp", "vf", "adv", "target", "done", "state_in", "T"):
            if not hasattr(rollout, k):
                raise ValueError(f"window_sequences takes a CommanderRollout (its [T, N] buffers and state_in); this object has no `{k}`")
        if rollout.obs.dim() != 4 or tuple(rollout.obs.shape[2:]) != (3, 34) or tuple(rollout.state_in.shape[2:]) != (3, 2, GRU_H):
            raise ValueError(f"the rollout's observations {tuple(rollout.obs.shape[2:])} / states {tuple(rollout.state_in.shape[2:])} are not the "
                             "3-agent commander's ((3, 34) / (3, 2, 200))")
        if not getattr(rollout, "collects", 0):
            raise RuntimeError("the rollout has not collected yet: its window buffers hold nothing (rollout.collect() first)")
        Lm = self.max_seq_len
        tables = window_cut(rollout.done, Lm)
        names = ["obs", "actions", "logp", "vf", "adv", "target"] + (["logits"] if getattr(rollout, "record_logits", False) else [])
        cols = [(getattr(rollout, k), tuple(getattr(rollout, k).shape[2:]), 0, k == "state_in") for k in names + ["state_in"]]   # eight at most: one launch
        out = dict(zip(names + ["state_in"], window_gather(cols, tables, Lm)))
        out["seq_lens"] = tables[2]
        out["mask"] = chunk_mask(tables[2].long(), Lm)
        return out

    def update_window(self, rollout):
        """one PPO update of commander_policy from a CommanderRollout's [T, N] window as the last collect left it (batch_mode =
        "truncate_episodes", the rollouts' default; the buffers are the same in both modes) -> what `update` returns, rows = 3 T N:

            ro.collect();  stats = learner.update_window(ro);  learner.publish(net)

        window_sequences, then `update`'s own policy_batch, batch_old_logits and driver.  The trailing fragment of an arena carries
        RLlib's truncation bootstrap from vf[T] in adv and target.  The rollout's buffers are only read."""
        with torch.no_grad():
            seqs = self.window_sequences(rollout)
            b = self.policy_batch(seqs)
            b["old_logits"] = self.batch_old_logits(seqs, b)
        out = self._sgd.run(*self._columns(b, staged=self.step == "graph"))
        self.updates += 1
        return out

    # ---- checkpointing (hhmarl_2d_amd/checkpoint.py)
    def _options(self):
        return _learner_saved_options(self, self.optimizer_mode, inputs=self.inputs, trunk=self.trunk)

    def state_dict(self):
        """the module (its one shared layer once), `updates` — it seeds minibatch_order and sequence_order —, kl_coeff and the Adam state
        (DeviceAdam's m, v, t or torch.optim.Adam's own), and the constructor options that decide the arithmetic or the schedule.  The
        captured step graph is not saved."""
        return {"options": self._options(), "updates": int(self.updates), "module": {k: ck.cpu(v) for k, v in self.module.state_dict().items()},
                "policy": self._sgd.state_dict()}

    def _load_plan(self, sd):
        ck.need_keys("CommanderLearner", sd, ("options", "updates", "module", "policy"))
        ck.check_options("CommanderLearner", sd["options"], self._options())
        if isinstance(sd["updates"], bool) or not isinstance(sd["updates"], int) or sd["updates"] < 0:
            raise ValueError("CommanderLearner: `updates` is a count")
        pairs = _module_plan("CommanderLearner module", self.module, sd["module"])
        driver = self._sgd._load_plan(sd["policy"])

        def commit():
            ck.copy_pairs(pairs)
            driver()
            self.updates = sd["updates"]
        return commit

    def load_state_dict(self, sd):
        """state_dict()'s dict back in place (parameters, m, v, t by copy_: a captured step graph replays); everything is validated first —
        ValueError names the field and nothing was changed"""
        self._load_plan(sd)()

    def publish(self, net):
        """the new weights into the sampler's CommanderNet on the current stream (refresh_weights): captured collects replay with them"""
        net.refresh_weights(self.module.state_dict())

    def export_commander(self, path):
        """the module's current weights under commander.state_keys() as one file of policy_files' plain format ("hhmarl_2d_amd.commander":
        float32 CPU tensors, read with torch.load(weights_only=True)) — what `evaluation.Evaluator(commander=path)` takes.  Written
        atomically; synchronises (the weights are read back to the host).  -> the path"""
        from ..policy_files import save_commander
        torch.cuda.synchronize(self.device)
        return save_commander(path, self.module.state_dict())
