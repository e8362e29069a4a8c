"""ctypes binding of libhh_world.so (include/hh_abi.h).  Fails loudly when the HIP library is
missing: there is NO CPU fallback in the product path."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HH_WORLD_LIB") or os.path.join(HERE, "lib", "libhh_world.so")  # override only for A/B experiments

ENV_LOWLEVEL, ENV_HIGHLEVEL = 0, 1
MODE_FIGHT, MODE_ESCAPE = 0, 1
OPP_MODE_EPISODE = -1  # hh_step_begin: every arena observes in the mode of its own level-5 draw
ACF_K, ACI_K, RKF_K, RKI_K, ARI_K, TGT_K = 6, 10, 4, 4, 6, 3
POLICY_LOGITS, CMD_LOGITS, EP_AUX_MAX_DIM = 32, 4, 32  # HH_POLICY_LOGITS (hh_policy.h), HH_CMD_LOGITS (hh_commander.h), HH_EP_AUX_MAX_DIM (hh_abi.h)


def hl_slots(n_agents, n_opps):
    """unit slots of a HighLevelEnv arena (include/hh_spec.h: HH_HL_SLOTS)"""
    return 10 if max(n_agents, n_opps) > 3 else 6


def tgt_k_of(n_agents, n_opps):
    """entries of a unit's stored target list in the state views (include/hh_spec.h: HH_TGT_K_OF)"""
    return 5 if max(n_agents, n_opps) > 3 else TGT_K
EVAL_KEYS = ("agents_win", "opps_win", "draw", "agent_fight", "agent_escape", "opp_fight", "opp_escape", "agent_steps", "opp_steps",
             "opp1", "opp2", "opp3")  # columns of hh_eval_info (env_base.py:104-106)


class HHConfig(C.Structure):
    """hh_config (include/hh_abi.h); field order is ABI."""
    _fields_ = [
        ("n_arenas", C.c_int32), ("env_kind", C.c_int32), ("n_agents", C.c_int32), ("n_opps", C.c_int32),
        ("level", C.c_int32), ("agent_mode", C.c_int32), ("horizon", C.c_int32), ("friendly_kill", C.c_int32),
        ("friendly_punish", C.c_int32), ("esc_dist_rew", C.c_int32), ("hier_action_assess", C.c_int32),
        ("hier_opp_fight_ratio", C.c_int32), ("auto_reset", C.c_int32), ("ext_opp_actions", C.c_int32),
        ("opp_side_selector", C.c_int32), ("reserved0", C.c_int32),
        ("map_size", C.c_double), ("glob_frac", C.c_double), ("rew_scale", C.c_double),
        ("seed", C.c_uint64), ("arena_offset", C.c_uint64),
    ]


class HHStateView(C.Structure):
    _fields_ = [
        ("ac_f", C.POINTER(C.c_double)), ("ac_i", C.POINTER(C.c_int32)), ("rk_f", C.POINTER(C.c_double)),
        ("rk_i", C.POINTER(C.c_int32)), ("ar_i", C.POINTER(C.c_int32)), ("tgt_id", C.POINTER(C.c_int32)),
        ("tgt_d", C.POINTER(C.c_double)),
    ]


class HHNetWeights(C.Structure):
    """hh_net_weights (include/hh_policy.h): pointers to one network's tensors, nn.Linear layout (host; device for hh_policy_refresh)"""
    _fields_ = [("kind", C.c_int32), ("inp_w", C.c_void_p * 3), ("inp_b", C.c_void_p * 3),
                ("att_in_proj_w", C.c_void_p), ("att_in_proj_b", C.c_void_p), ("att_out_w", C.c_void_p), ("att_out_b", C.c_void_p),
                ("shared_w", C.c_void_p), ("shared_b", C.c_void_p), ("out_w", C.c_void_p), ("out_b", C.c_void_p)]


class HHCriticWeights(C.Structure):
    """hh_critic_weights (include/hh_policy.h): pointers to one network's value branch, nn.Linear layout (host; device for hh_policy_refresh)"""
    _fields_ = [("kind", C.c_int32), ("v_w", C.c_void_p * 3), ("v_b", C.c_void_p * 3),
                ("att_in_proj_w", C.c_void_p), ("att_in_proj_b", C.c_void_p), ("att_out_w", C.c_void_p), ("att_out_b", C.c_void_p),
                ("shared_w", C.c_void_p), ("shared_b", C.c_void_p), ("val_w", C.c_void_p), ("val_b", C.c_void_p)]


class HHCommanderWeights(C.Structure):
    """hh_commander_weights (include/hh_commander.h): host pointers to CommanderGru's tensors, nn.Linear / nn.GRU layout; field order is ABI"""
    _fields_ = [("inp_w", C.c_void_p * 4), ("inp_b", C.c_void_p * 4),
                ("act_w_ih", C.c_void_p), ("act_w_hh", C.c_void_p), ("act_b_ih", C.c_void_p), ("act_b_hh", C.c_void_p),
                ("shared_w", C.c_void_p), ("shared_b", C.c_void_p), ("act_out_w", C.c_void_p), ("act_out_b", C.c_void_p),
                ("v_w", C.c_void_p * 4), ("v_b", C.c_void_p * 4),
                ("val_w_ih", C.c_void_p), ("val_w_hh", C.c_void_p), ("val_b_ih", C.c_void_p), ("val_b_hh", C.c_void_p),
                ("val_out_w", C.c_void_p), ("val_out_b", C.c_void_p)]


class HHEpisodeBufs(C.Structure):
    """hh_episode_bufs (include/hh_abi.h): sizes, then device pointers (collect, carry, batch); field order is ABI"""
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("n_agents", C.c_int32), ("obs_dim", C.c_int32), ("carry_cap", C.c_int32),
                ("reserved0", C.c_int32), ("row_cap", C.c_int64), ("ep_cap", C.c_int64), ("gamma", C.c_double), ("lam", C.c_double)] + [
        (name, C.c_void_p) for name in (
            "obs", "actions", "logp", "vf", "reward", "valid", "done",
            "c_obs", "c_actions", "c_logp", "c_vf", "c_reward", "c_valid", "carried", "episode", "scratch",
            "o_obs", "o_actions", "o_logp", "o_vf", "o_reward", "o_valid", "o_adv", "o_target", "o_done", "o_arena", "o_episode", "o_t",
            "ep_start", "ep_len", "ep_arena", "counts")]


class HHCommanderEpisodeBufs(C.Structure):
    """hh_commander_episode_bufs (include/hh_commander.h): sizes, then device pointers (collect, carry, batch); field order is ABI"""
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("max_seq_len", C.c_int32), ("carry_cap", C.c_int32), ("row_cap", C.c_int64),
                ("ep_cap", C.c_int64), ("seq_cap", C.c_int64), ("gamma", C.c_double), ("lam", C.c_double)] + [
        (name, C.c_void_p) for name in (
            "obs", "actions", "logp", "vf", "reward", "valid", "done", "state_in",
            "c_obs", "c_actions", "c_logp", "c_vf", "c_reward", "c_valid", "c_state", "carried", "episode", "scratch",
            "o_obs", "o_actions", "o_logp", "o_vf", "o_reward", "o_valid", "o_adv", "o_target", "o_done", "o_arena", "o_episode", "o_t",
            "ep_start", "ep_len", "ep_arena", "seq_start", "seq_len", "seq_ep", "o_state_in", "counts")]


class HHEpisodeAux(C.Structure):
    """hh_episode_aux (include/hh_abi.h): the optional per-agent float column of the _aux emitters; field order is ABI"""
    _fields_ = [("aux_dim", C.c_int32), ("reserved0", C.c_int32), ("aux", C.c_void_p), ("c_aux", C.c_void_p), ("o_aux", C.c_void_p)]


class HHEpisodeMetricsBufs(C.Structure):
    """hh_episode_metrics_bufs (include/hh_abi.h): sizes, then device pointers; field order is ABI"""
    _fields_ = [("n_agents", C.c_int32), ("reserved0", C.c_int32), ("row_cap", C.c_int64), ("ep_cap", C.c_int64)] + [
        (name, C.c_void_p) for name in ("reward", "vf", "target", "ep_start", "ep_len", "counts", "ep_return", "summary", "totals", "scratch")] + [
        ("scratch_bytes", C.c_int64)]


class HHWindowMetricsBufs(C.Structure):
    """hh_window_metrics_bufs (include/hh_abi.h): sizes, then device pointers; field order is ABI"""
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("n_agents", C.c_int32), ("reserved0", C.c_int32)] + [
        (name, C.c_void_p) for name in ("reward", "vf", "target", "done", "run_return", "run_len", "ep_return", "ep_len", "ep_arena", "ep_end",
                                        "counts", "summary", "totals", "scratch")] + [("scratch_bytes", C.c_int64)]


class HHEpisodeOutcomeBufs(C.Structure):
    """hh_episode_outcome_bufs (include/hh_abi.h): sizes, then device pointers; field order is ABI"""
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("n_agents", C.c_int32), ("reserved0", C.c_int32), ("ep_cap", C.c_int64)] + [
        (name, C.c_void_p) for name in ("done", "outcome", "n_episodes", "ep_arena", "ep_len", "ep_return", "ep_outcome", "summary", "flags",
                                        "scratch")] + [("scratch_bytes", C.c_int64)]


OUTCOME_WIN, OUTCOME_LOSE, OUTCOME_DRAW, OUTCOME_NONE = 1, -1, 0, 2  # HH_OUTCOME_*: hh_episode_stats' codes
# slot names of hh_episode_outcomes' summary f64 [HH_EO_SUMMARY], in slot order
EO_SUMMARY = ("episodes", "agents_win", "opps_win", "draw", "reward_mean_win", "reward_mean_lose", "reward_mean_draw",
              "len_mean_win", "len_mean_lose", "len_mean_draw", "other_codes", "reserved")
EP_METRICS_MAX_AGENTS = 5  # HH_EP_METRICS_MAX_AGENTS
# hh_episodes_emit_append's accumulator i32 [HH_EP_ACC], in slot order (slot 7 is reserved and stays 0)
EP_ACC = ("rows", "episodes", "overflow", "sequences", "complete", "collects", "batches", "reserved")
# slot names of hh_episodes_metrics's summary f64 [HH_EP_METRICS], in slot order (HH_EPM_*: the per-agent blocks hold 5 slots each)
EP_METRICS = ("episodes", "rows", "episode_reward_mean", "episode_reward_min", "episode_reward_max",
              "episode_len_mean", "episode_len_min", "episode_len_max") + tuple(
    f"{k}_{a}" for k in ("agent_return_mean", "agent_return_min", "agent_return_max", "vf_explained_var") for a in range(EP_METRICS_MAX_AGENTS))
EP_METRICS_SLOT = {name: i for i, name in enumerate(EP_METRICS)}


EXPORTS = ["hh_world_create", "hh_world_destroy", "hh_last_error", "hh_obs_dim", "hh_n_ctrl", "hh_reset", "hh_step",
           "hh_rollout", "hh_episode_stats", "hh_get_state", "hh_set_state", "hh_get_event_masks", "hh_observe",
           "hh_hl_begin", "hh_hl_agents_act", "hh_hl_tick", "hh_hl_end", "hh_step_begin", "hh_step_finish", "hh_gae", "hh_hl_commands",
           "hh_episode_stats_packed", "hh_hl_tick_count", "hh_rollout_kernel_name", "hh_opp_policy", "hh_eval_info", "hh_arena_status", "hh_hl_rollout", "hh_trace_enable", "hh_trace_read",
           "hh_policy_create", "hh_policy_destroy", "hh_policy_set_net", "hh_policy_set_lut", "hh_policy_set_tile_rows", "hh_policy_act",
           "hh_bind_policy", "hh_policy_act_binned", "hh_kernel_instance", "hh_gae_rllib", "hh_math_eval",
           "hh_policy_set_critic", "hh_policy_sample", "hh_policy_kernel_name", "hh_action_faults", "hh_action_tape_uniform",
           "hh_hl_begin_variants", "hh_hl_act_tick", "hh_policy_act_binned_live", "hh_episodes_emit", "hh_policy_refresh", "hh_policy_copy_packed", "hh_episodes_emit_aux",
           "hh_episodes_metrics_scratch_bytes", "hh_episodes_metrics", "hh_episodes_emit_append",
           "hh_window_metrics_scratch_bytes", "hh_window_metrics",
           "hh_outcome_tap", "hh_episode_outcomes_scratch_bytes", "hh_episode_outcomes",
           "hh_world_snapshot_bytes", "hh_world_snapshot", "hh_world_restore", "hh_policy_snapshot_bytes", "hh_policy_snapshot", "hh_policy_restore"]
COMMANDER_EXPORTS = ["hh_commander_create", "hh_commander_destroy", "hh_commander_set_weights", "hh_commander_sample",
                     "hh_commander_kernel_name", "hh_commander_episodes_emit", "hh_commander_refresh_weights",
                     "hh_commander_copy_packed", "hh_commander_act_chain", "hh_commander_chain_kernel_name", "hh_commander_episodes_emit_aux",
                     "hh_commander_episodes_emit_append", "hh_commander_snapshot_bytes", "hh_commander_snapshot",
                     "hh_commander_restore"]  # include/hh_commander.h

LEARNER_EXPORTS = ["hh_ppo_loss_scratch_bytes", "hh_ppo_loss", "hh_ppo_loss_categorical", "hh_gru_seq_scratch_bytes", "hh_gru_seq_forward",
                   "hh_gru_seq_backward", "hh_chunk_attn_forward", "hh_chunk_attn_backward", "hh_residual_normalize_forward",
                   "hh_residual_normalize_backward", "hh_input_stage_scratch_bytes", "hh_input_stage_forward",
                   "hh_input_stage_backward", "hh_dense_tanh_scratch_bytes", "hh_dense_tanh_forward", "hh_dense_tanh_backward",
                   "hh_adam_step", "hh_minibatch_stage", "hh_train_commit", "hh_gru_seq_tile",
                   "hh_grad_norm_scratch_bytes", "hh_grad_norm", "hh_adam_step_clipped", "hh_minibatch_stage_gather",
                   "hh_heads_loss_scratch_bytes", "hh_heads_loss_geometry", "hh_heads_loss", "hh_window_cut", "hh_window_gather",
                   "hh_grad_pack", "hh_grad_combine", "hh_attn_block_tile", "hh_attn_block_save_bytes", "hh_attn_block_scratch_bytes",
                   "hh_attn_block_forward", "hh_attn_block_backward"]  # include/hh_learner.h
GRU_TILES = (16, 8, 4)  # the compiled instances of hh_k_gru_seq_fwd / _bwd (HH_GRU_TILE forces one; hh_gru_seq_tile tells which a call uses)
ATTN_HEADS, ATTN_MAX_LEN, ATTN_WIDTHS = 2, 32, (100, 150)  # HH_ATTN_HEADS, HH_ATTN_MAX_LEN and the compiled widths of hh_chunk_attn_* / hh_residual_normalize_*
ATTN_BLOCK_ROWS, ATTN_BLOCK_MAX_WG = 32, 128  # HH_ATTN_BLOCK_ROWS, HH_ATTN_BLOCK_MAX_WG: rows of a tile and the backward's workgroup cap of hh_attn_block_*
PPO_STATS = ("total_loss", "mean_policy_loss", "mean_vf_loss", "mean_kl", "mean_entropy", "n_valid")  # hh_ppo_loss's stats f64 [HH_PPO_STATS]


class HHPpoLossParams(C.Structure):
    """hh_ppo_loss_params (include/hh_learner.h); field order is ABI"""
    _fields_ = [("n_comp", C.c_int32), ("reserved0", C.c_int32), ("clip_param", C.c_float), ("vf_clip_param", C.c_float),
                ("vf_loss_coeff", C.c_float), ("entropy_coeff", C.c_float), ("kl_coeff", C.c_float), ("reserved1", C.c_float)]


class HHGruSeqIO(C.Structure):
    """hh_gru_seq_io (include/hh_learner.h): one GRU's device pointers; field order is ABI"""
    _fields_ = [(name, C.c_void_p) for name in ("gi", "h0", "w_hh", "b_hh", "y", "dy", "d_gi", "d_gh", "d_h0")]


INSTAGE_MAX_GROUPS, INSTAGE_MAX_SEGS, INSTAGE_MAX_K, INSTAGE_MAX_OUT = 4, 6, 112, 500  # HH_INSTAGE_MAX_* (include/hh_learner.h)


class HHInputGroup(C.Structure):
    """hh_input_group (include/hh_learner.h): one layer of hh_input_stage_*, sizes and segments, then device pointers; field order is ABI"""
    _fields_ = [("n_out", C.c_int32), ("n_seg", C.c_int32), ("seg_col", C.c_int16 * INSTAGE_MAX_SEGS), ("seg_len", C.c_int16 * INSTAGE_MAX_SEGS),
                ("w", C.c_void_p), ("b", C.c_void_p), ("y", C.c_void_p), ("y_ld", C.c_int64), ("d_y", C.c_void_p), ("d_y_ld", C.c_int64),
                ("d_w", C.c_void_p), ("d_b", C.c_void_p)]


DENSE_MAX_SRC, DENSE_MAX_DIM, DENSE_ROW_TILE, DENSE_MAX_PARTS, DENSE_FWD_SCRATCH_BYTES = 2, 512, 64, 32, 2048  # HH_DENSE_* (include/hh_learner.h)


class HHDenseSrc(C.Structure):
    """hh_dense_src (include/hh_learner.h): one row block of hh_dense_tanh_*, its row count, then device pointers; field order is ABI"""
    _fields_ = [("n_rows", C.c_int64), ("x", C.c_void_p), ("ld", C.c_int64), ("y", C.c_void_p), ("d_y", C.c_void_p), ("d_x", C.c_void_p)]


HEADS_K, HEADS_N_OUT = 500, {4: 26, 3: 24, 1: 3}  # hh_heads_loss: shared_layer's width, the logits per n_comp (include/hh_learner.h)
ADAM_MAX_TENSORS, STAGE_MAX_COLS = 64, 8  # HH_ADAM_MAX_TENSORS, HH_STAGE_MAX_COLS (include/hh_learner.h)
CLIP_OUT = 2  # HH_CLIP_OUT: hh_grad_norm's clip f64 [2] = (the norm before clipping, the coefficient)


class HHAdamTensor(C.Structure):
    """hh_adam_tensor (include/hh_learner.h): one parameter tensor of hh_adam_step, device pointers, then the element count; field order is ABI"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64)]


class HHStageCol(C.Structure):
    """hh_stage_col (include/hh_learner.h): one column of hh_minibatch_stage; field order is ABI"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("chunk_bytes", C.c_int64)]


WINDOW_MAX_LEN = 32  # HH_WINDOW_MAX_LEN (include/hh_learner.h)


class HHWindowCol(C.Structure):
    """hh_window_col (include/hh_learner.h): one column of hh_window_gather; field order is ABI"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("step_bytes", C.c_int64), ("offset", C.c_int64), ("width", C.c_int64),
                ("per_seq", C.c_int32), ("reserved0", C.c_int32)]


GRAD_MAX_SHARDS = 64  # HH_GRAD_MAX_SHARDS (include/hh_learner.h)


class HHGradTensor(C.Structure):
    """hh_grad_tensor (include/hh_learner.h): one gradient of hh_grad_pack / hh_grad_combine and its place in the bucket; field order is ABI"""
    _fields_ = [("g", C.c_void_p), ("n", C.c_int64), ("off", C.c_int64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). The MI355X world has no CPU fallback.")
        import torch  # noqa: F401  — BEFORE the library: torch ships its own HIP runtime; a process that loads libhh_world.so (linked against the system's) first and
        #                  imports torch afterwards ends up with two, and hh_world_create then reports "no HIP device"
        L = C.CDLL(LIB_PATH)
        L.hh_last_error.restype = C.c_char_p
        vp = C.c_void_p
        L.hh_world_create.argtypes = [C.POINTER(HHConfig), C.c_int, C.POINTER(vp)]
        L.hh_world_destroy.argtypes = [vp]
        L.hh_obs_dim.argtypes = [vp]
        L.hh_n_ctrl.argtypes = [vp]
        L.hh_reset.argtypes = [vp, vp, vp, vp]
        L.hh_step.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.hh_rollout.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp]
        L.hh_episode_stats.argtypes = [vp, vp, vp, vp, vp]
        L.hh_get_state.argtypes = [vp, C.POINTER(HHStateView)]
        L.hh_set_state.argtypes = [vp, C.POINTER(HHStateView)]
        L.hh_get_event_masks.argtypes = [vp, vp, vp]
        L.hh_episode_stats_packed.argtypes = [vp, vp, vp]
        L.hh_hl_tick_count.argtypes = [vp, C.POINTER(C.c_uint64), vp]
        L.hh_rollout_kernel_name.argtypes = [vp, C.c_char_p, C.c_int32]
        L.hh_kernel_instance.argtypes = [vp, C.c_int32, C.c_char_p, C.c_int32]
        L.hh_observe.argtypes = [vp, vp, vp]
        L.hh_hl_begin.argtypes = [vp, vp, vp, vp, vp]
        L.hh_hl_agents_act.argtypes = [vp, vp, vp, vp, vp]
        L.hh_hl_tick.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int32), vp]
        L.hh_hl_end.argtypes = [vp, vp, vp, vp, vp, vp]
        L.hh_step_begin.argtypes = [vp, vp, C.c_int32, vp, vp]
        L.hh_step_finish.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.hh_hl_commands.argtypes = [vp, vp]
        L.hh_trace_enable.argtypes = [vp, C.c_int32, C.c_int32]
        L.hh_trace_read.argtypes = [vp, vp, vp]
        L.hh_hl_rollout.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
        L.hh_opp_policy.argtypes = [vp, vp, vp]
        L.hh_eval_info.argtypes = [vp, vp, vp, C.c_int32, vp]
        L.hh_arena_status.argtypes = [vp, vp, vp]
        L.hh_gae.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp]
        L.hh_gae_rllib.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp]
        L.hh_episodes_emit.argtypes = [C.POINTER(HHEpisodeBufs), vp]
        L.hh_episodes_emit_aux.argtypes = [C.POINTER(HHEpisodeBufs), C.POINTER(HHEpisodeAux), vp]
        L.hh_episodes_emit_append.argtypes = [C.POINTER(HHEpisodeBufs), C.POINTER(HHEpisodeAux), C.c_int64, vp, vp, vp]
        L.hh_episodes_metrics_scratch_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.hh_episodes_metrics.argtypes = [C.POINTER(HHEpisodeMetricsBufs), vp]
        L.hh_window_metrics_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.hh_window_metrics.argtypes = [C.POINTER(HHWindowMetricsBufs), vp]
        L.hh_outcome_tap.argtypes = [vp, vp, vp, vp]
        L.hh_episode_outcomes_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]
        L.hh_episode_outcomes.argtypes = [C.POINTER(HHEpisodeOutcomeBufs), vp]
        L.hh_math_eval.argtypes =[C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
        L.hh_policy_create.argtypes = [C.c_int, C.c_int32, C.POINTER(vp)]
        L.hh_policy_destroy.argtypes = [vp]
        L.hh_policy_set_net.argtypes = [vp, C.c_int32, C.POINTER(HHNetWeights)]
        L.hh_policy_set_lut.argtypes = [vp, vp]
        L.hh_policy_set_tile_rows.argtypes = [vp, C.c_int32]
        L.hh_policy_act.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.hh_bind_policy.argtypes = [vp, vp]
        L.hh_policy_act_binned.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
        L.hh_policy_act_binned_live.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp]
        L.hh_hl_begin_variants.argtypes = [vp, vp, vp, vp, vp]
        L.hh_hl_act_tick.argtypes = [vp, vp, vp, vp, vp, vp]
        L.hh_policy_set_critic.argtypes = [vp, C.c_int32, C.POINTER(HHCriticWeights)]
        L.hh_policy_sample.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
        L.hh_policy_kernel_name.argtypes = [vp, C.c_int32, C.c_int32, C.c_char_p, C.c_int32]
        L.hh_policy_refresh.argtypes = [vp, C.c_int32, C.POINTER(HHNetWeights), C.POINTER(HHCriticWeights), vp]
        L.hh_policy_copy_packed.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int64, C.POINTER(C.c_int64), vp]
        L.hh_action_faults.argtypes = [vp, vp, C.c_int32, vp]
        L.hh_action_tape_uniform.argtypes = [C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp]
        L.hh_commander_create.argtypes = [C.c_int, C.c_int32, C.POINTER(vp)]
        L.hh_commander_destroy.argtypes = [vp]
        L.hh_commander_set_weights.argtypes = [vp, C.POINTER(HHCommanderWeights)]
        L.hh_commander_sample.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
        L.hh_commander_kernel_name.argtypes = [vp, C.c_int32, C.c_char_p, C.c_int32]
        L.hh_commander_episodes_emit.argtypes = [C.POINTER(HHCommanderEpisodeBufs), vp]
        L.hh_commander_episodes_emit_aux.argtypes = [C.POINTER(HHCommanderEpisodeBufs), C.POINTER(HHEpisodeAux), vp]
        L.hh_commander_episodes_emit_append.argtypes = [C.POINTER(HHCommanderEpisodeBufs), C.POINTER(HHEpisodeAux), C.c_int64, vp, vp, vp]
        L.hh_commander_refresh_weights.argtypes = [vp, C.POINTER(HHCommanderWeights), vp]
        L.hh_commander_copy_packed.argtypes = [vp, C.c_int32, vp, C.c_int64, C.POINTER(C.c_int64), vp]
        L.hh_commander_act_chain.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.hh_commander_chain_kernel_name.argtypes = [vp, C.c_int32, C.c_int32, C.c_char_p, C.c_int32]
        L.hh_ppo_loss_scratch_bytes.argtypes = [C.c_int64, C.POINTER(C.c_int64)]
        L.hh_ppo_loss.argtypes = [C.c_int64, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(HHPpoLossParams), vp, vp, vp, vp, C.c_int64, vp]
        L.hh_ppo_loss_categorical.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(HHPpoLossParams), vp, vp, vp, vp, C.c_int64, vp]
        L.hh_gru_seq_scratch_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.hh_gru_seq_forward.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.POINTER(HHGruSeqIO), vp, vp, C.c_int64, vp]
        L.hh_gru_seq_backward.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.POINTER(HHGruSeqIO), vp, vp, C.c_int64, vp]
        L.hh_gru_seq_tile.argtypes = [C.c_int64]
        L.hh_chunk_attn_forward.argtypes = [C.c_int64, C.c_int32, C.c_int32, vp, vp, vp]
        L.hh_chunk_attn_backward.argtypes = [C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.hh_residual_normalize_forward.argtypes = [C.c_int64, C.c_int32, vp, vp, vp, vp, vp]
        L.hh_residual_normalize_backward.argtypes = [C.c_int64, C.c_int32, vp, vp, vp, vp, vp]
        L.hh_attn_block_tile.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.hh_attn_block_save_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.hh_attn_block_scratch_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.hh_attn_block_forward.argtypes = [C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp]
        L.hh_attn_block_backward.argtypes = [C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp]
        L.hh_input_stage_scratch_bytes.argtypes = [C.c_int32, C.POINTER(HHInputGroup), C.c_int64, C.POINTER(C.c_int64)]
        L.hh_input_stage_forward.argtypes = [C.c_int64, vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(HHInputGroup), vp]
        L.hh_input_stage_backward.argtypes = [C.c_int64, vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(HHInputGroup), vp, C.c_int64, vp]
        L.hh_dense_tanh_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(HHDenseSrc), C.POINTER(C.c_int64)]
        L.hh_dense_tanh_forward.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(HHDenseSrc), vp, vp, vp, C.c_int64, vp]
        L.hh_dense_tanh_backward.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(HHDenseSrc), vp, vp, vp, vp, C.c_int64, vp]
        L.hh_adam_step.argtypes = [C.c_int32, C.POINTER(HHAdamTensor), vp, C.c_double, C.c_double, C.c_double, C.c_double, vp]
        L.hh_minibatch_stage.argtypes = [C.c_int32, C.POINTER(HHStageCol), C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, vp, vp, vp]
        L.hh_minibatch_stage_gather.argtypes = [C.c_int32, C.POINTER(HHStageCol), C.c_int32, C.c_int32, C.c_int64, vp, C.c_int64, vp, C.c_int32, vp, vp, vp]
        L.hh_train_commit.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
        L.hh_grad_norm_scratch_bytes.argtypes = [C.c_int32, C.POINTER(HHAdamTensor), C.POINTER(C.c_int64)]
        L.hh_grad_norm.argtypes = [C.c_int32, C.POINTER(HHAdamTensor), C.c_double, vp, vp, vp, C.c_int32, vp, C.c_int64, vp]
        L.hh_adam_step_clipped.argtypes = [C.c_int32, C.POINTER(HHAdamTensor), vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp]
        L.hh_heads_loss_scratch_bytes.argtypes = [C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.hh_heads_loss_geometry.argtypes = [C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.hh_heads_loss.argtypes = [C.c_int64] + [vp] * 13 + [C.POINTER(HHPpoLossParams)] + [vp] * 10 + [C.c_int64, vp]
        L.hh_window_cut.argtypes = [C.c_int32, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
        L.hh_window_gather.argtypes = [C.c_int32, C.POINTER(HHWindowCol), C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.hh_grad_pack.argtypes = [C.c_int32, C.POINTER(HHGradTensor), vp, C.c_int64, vp]
        L.hh_grad_combine.argtypes = [C.c_int32, C.POINTER(HHGradTensor), vp, C.c_int64, C.c_int32, C.POINTER(C.c_double), vp]
        for obj in ("world", "policy", "commander"):   # the snapshot triplets (hh_abi.h, hh_policy.h, hh_commander.h): handle, [host] buffer, bytes, stream
            getattr(L, f"hh_{obj}_snapshot_bytes").argtypes = [vp, C.POINTER(C.c_int64)]
            getattr(L, f"hh_{obj}_snapshot").argtypes = [vp, vp, C.c_int64, vp]
            getattr(L, f"hh_{obj}_restore").argtypes = [vp, vp, C.c_int64, vp]
        _lib = L
    return _lib


SNAPSHOT_MAGIC = {"world": b"HHSW", "policy": b"HHSP", "commander": b"HHSC"}   # HH_SNAP_MAGIC_* (csrc/hh_snapshot.h)


def snapshot(obj, handle, stream):
    """hh_<obj>_snapshot of `handle` (obj: "world" | "policy" | "commander") -> the blob, a uint8 CPU tensor; synchronises `stream`"""
    import torch
    n = C.c_int64(0)
    check(getattr(lib(), f"hh_{obj}_snapshot_bytes")(handle, C.byref(n)))
    blob = torch.empty((n.value,), dtype=torch.uint8)
    check(getattr(lib(), f"hh_{obj}_snapshot")(handle, C.c_void_p(blob.data_ptr()), n.value, stream))
    return blob


def snapshot_bytes(obj, handle):
    n = C.c_int64(0)
    check(getattr(lib(), f"hh_{obj}_snapshot_bytes")(handle, C.byref(n)))
    return n.value


def restore(obj, handle, blob, stream):
    """hh_<obj>_restore of a blob (uint8 CPU tensor, contiguous) into `handle`; a refusal (HH_E_ARG: the object is untouched) raises
    ValueError with the library's message, any other failure RuntimeError"""
    rc = getattr(lib(), f"hh_{obj}_restore")(handle, C.c_void_p(blob.data_ptr()), blob.numel(), stream)
    if rc == -1:
        raise ValueError(f"blob: {lib().hh_last_error().decode()}")
    check(rc)


def check(rc):
    if rc != 0:
        raise RuntimeError(f"libhh_world error {rc}: {lib().hh_last_error().decode()}")
