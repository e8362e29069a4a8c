"""The learner half of train_hetero.py's and train_hier.py's PPO on the device (train_hetero.py:206-243 with RLlib 2.4's PPO): the fused loss kernel
`hh_ppo_loss` (include/hh_learner.h) behind a torch.autograd.Function, the four trainable networks as torch modules in TRAINING form, and
`PPOLearner`, which turns the `EpisodeBatch` of a `PPORollout(batch_mode="complete_episodes")` into one PPO update of ac1_policy and
ac2_policy and hands the new weights back to the sampler's `PolicyBank` — collect -> update -> publish -> collect on one GPU, the
batch never leaving it.  The network GEMMs stay in PyTorch / rocBLAS; the loss and its gradient are one HIP pass.  Opt-in
(`attention="fused"`): what the fight networks' two attention blocks do between and after their projections runs in HIP too
(`chunk_attention`: hh_chunk_attn_*, `residual_normalize`: hh_residual_normalize_*); the default path is nn.MultiheadAttention.
And (`attention="block"`): each whole block, both projections included, as ONE launch forward and two backward (`attention_block`:
hh_attn_block_*).
Opt-in as well (`inputs="fused"`, all five networks): the layers in front of shared_layer as one grouped launch per side
(`input_stage`: hh_input_stage_*); the default path slices, concatenates and runs them one by one.
And (`trunk="fused"`, all five networks): shared_layer with its bias and tanh over the actor's and the critic's rows as ONE call
on the matrix cores (`dense_tanh`: hh_dense_tanh_*, split-fp16 MFMA); the default path is two float32 GEMMs and two tanh.
And (`heads="fused"`, all five networks, not with trunk="fused"): what follows shared_layer's GEMM — tanh, act_out and val_out, the PPO
loss, and the backward of all of it down to shared_layer's pre-activations — as ONE row pass and a fixed-order final sum (`heads_loss`:
hh_heads_loss); the default path is tanh, two GEMMs, hh_ppo_loss and autograd's backward of each.
And (`PPOLearner(optimizer="fused", step="graph")`): Adam on the device (`adam_step`: hh_adam_step) and the whole minibatch step — the
minibatch staged by a device schedule (`minibatch_stage`: hh_minibatch_stage), forward, loss, backward, Adam and the step's bookkeeping
(`train_commit`: hh_train_commit) — replayed from ONE HIP graph per policy; the default is torch.optim.Adam and the eager step.
Both learners also train from the rollouts' default batch_mode="truncate_episodes" (`update_window`): the fixed [T, N] window is cut into
sequences (`window_cut`: hh_window_cut) and its columns gathered into the padded form (`window_gather`: hh_window_gather); from there on
it is `update`.
And (`PPOLearner(group=LocalShards(K) | ShardGroup())`, eager steps): the update data-parallel over W shards with the bytes of one
process over the W shards — the gradients packed (`grad_pack`: hh_grad_pack), all-gathered and added in shard order (`grad_combine`:
hh_grad_combine); `shards` holds the groups, the step alignment and the moments over all shards.

The reference's learner does not compute what its sampler computes, and this module keeps the difference:
  * Fight1 / Fight2 are RLlib `RecurrentNetwork`s with a dummy state.  The sampler sees sequences of length 1 (attention =
    out_proj(v_proj(x)), what hh_policy_sample folds).  The learner sees each agent trajectory cut into chunks of max_seq_len = 20 rows,
    the last one zero-padded (rnn_sequencing.pad_batch_to_sequences_of_same_size), and `add_time_dimension` makes att_act / att_val
    attend over the 20 steps of a chunk, padded rows included as keys (no key padding mask).  ModelV2.__call__ hands the dummy state_in
    back as the state, so PPOTorchPolicy.loss takes its RNN branch: the loss is averaged over the unpadded rows only.
    Esc1 / Esc2 are plain TorchModelV2s: no chunks, no mask.
  * The critic is trained on rows with the actions filled in (rollout.central_critic_rows), while the batch's `vf` was predicted with
    zero action inputs.
  * ac1_policy and ac2_policy hold the same 500 x 500 shared_layer tensor (models/ac_models_hetero.py:22) and each has its own optimizer.

The commander half (train_hier.py with models/ac_models_hier.py:CommanderGru): `gru_sequence`, both
200-wide GRUs over whole chunks of max_seq_len steps in one fused launch each way (hh_gru_seq_forward / hh_gru_seq_backward),
`ppo_loss_categorical` (hh_ppo_loss_categorical), `CommanderTrainable` and `CommanderLearner`, which does for
`commander.CommanderRollout(batch_mode="complete_episodes")` what `PPOLearner` does for `PPORollout`.

The pieces, in dependency order: `_ffi` (pointers, stream, refusals), `loss` (the three PPO losses), `ops` (the fused layer ops and the GRU
sequence op), `nets` (the five networks), `batch` (chunks, schedules, the window cut and gather), `step` (device Adam, stage, commit, the
step book and the minibatch driver), `ppo_learner`, `commander_learner`.  Importing the package touches neither the GPU nor the library."""

# every top-level name of the former single module, private ones included: the tests and tools read them as attributes of this package
from ._ffi import _fused_input, _need_gpu, _p, _stream
from .loss import (CMD_LD, HEADS_MODES, OLD_LD, _head_params, _heads_mode, _HeadsLoss, _PPOLoss, heads_loss, heads_loss_torch, n_comp_of, ppo_loss,
                   ppo_loss_categorical, ppo_loss_categorical_torch, ppo_loss_torch)
from .ops import (ATTENTION_MODES, COMMANDER_STAGE_LAYERS, GRU_H, INPUT_MODES, TRUNK_MODES, _check_gru, _ChunkAttn, _dense_args, _dense_rows,
                  _DenseTanh, _gru_io, _gru_scratch_bytes, _GruSeq, _InputStage, _ResidualNormalize, _stage_layout, _trunk_mode, _AttnBlock,
                  attention_block, attention_block_tile, attention_block_torch, chunk_attention,
                  chunk_attention_torch, commander_stage_tables, dense_tanh, dense_tanh_torch, gru_cell_torch, gru_seq_backward, gru_seq_forward,
                  gru_seq_tile, gru_sequence, gru_sequence_pair, gru_sequence_torch, input_stage, input_stage_torch, residual_normalize,
                  residual_normalize_torch, stage_groups, stage_layers, stage_tables, grad_combine, grad_combine_torch, grad_layout, grad_pack,
                  grad_pack_torch)
from .nets import _FC, CommanderTrainable, TrainableNet, _GRUWeights, tie
from .batch import (_cut_args, _gather_args, chunk_mask, cut_chunks, kl_coeff_update, minibatch_order, minibatch_partition, minibatch_schedule,
                    pad_chunks, sequence_order, sequence_schedule, shuffled_schedule, standardize, standardize_masked, update_schedule, window_cut,
                    window_cut_torch, window_gather, window_gather_torch)
from .step import (ADAM_BETAS, ADAM_EPS, OPTIMIZER_MODES, STEP_MODES, DeviceAdam, _adam_desc, _grad_clip, _heads_keyword, _is_clip, _learner_options,
                   _optimizer_mode, _PolicySGD, _shuffle_flag, _stage_desc, _step_mode, _StepBook, adam_step, adam_step_torch, grad_norm,
                   grad_norm_scratch, grad_norm_torch, minibatch_stage, minibatch_stage_gather, minibatch_stage_gather_torch, minibatch_stage_torch,
                   train_commit, _shard_group)
from .shards import LocalShards, ShardGroup, combine_stats, combined_mean, combined_std, ordered_sum, standardize_shards, step_weights
from .ppo_learner import PPOLearner
from .commander_learner import COMMANDER_STAGE_COLS, CommanderLearner
