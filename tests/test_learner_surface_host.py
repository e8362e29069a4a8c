"""The attribute surface of the hhmarl_2d_amd.learner package without a GPU or the library: every top-level name of the single module it
was split from (its defs, classes and assignment targets, private ones included, read with ast from that file; the four helpers the
one loss front end replaced are left out), the pinned signatures as that file had them, and the package's own imports."""
import inspect
import sys

from hhmarl_2d_amd import learner as LR

NAMES = (
    "OLD_LD", "n_comp_of", "_p", "_PPOLoss", "ppo_loss", "ppo_loss_torch", "ATTENTION_MODES", "_need_gpu", "_stream", "_ChunkAttn",
    "_ResidualNormalize", "_fused_input", "chunk_attention", "residual_normalize", "chunk_attention_torch", "residual_normalize_torch",
    "INPUT_MODES", "_stage_layout", "_InputStage", "input_stage", "input_stage_torch", "stage_layers", "COMMANDER_STAGE_LAYERS", "stage_tables",
    "commander_stage_tables", "stage_groups", "TRUNK_MODES", "_dense_rows", "_DenseTanh", "_dense_args", "dense_tanh", "dense_tanh_torch",
    "_trunk_mode", "HEADS_MODES", "_heads_mode", "_heads_keyword", "_HeadsLoss", "_head_params", "heads_loss", "heads_loss_torch", "_FC",
    "TrainableNet", "tie", "cut_chunks", "pad_chunks", "chunk_mask", "minibatch_partition", "minibatch_order", "sequence_order",
    "shuffled_schedule", "update_schedule", "_shuffle_flag", "kl_coeff_update", "standardize", "OPTIMIZER_MODES", "STEP_MODES", "ADAM_BETAS",
    "ADAM_EPS", "_optimizer_mode", "_step_mode", "_grad_clip", "_adam_desc", "_is_clip", "grad_norm_scratch", "grad_norm", "grad_norm_torch",
    "adam_step", "adam_step_torch", "minibatch_schedule", "sequence_schedule", "minibatch_stage", "_stage_desc", "minibatch_stage_gather",
    "minibatch_stage_gather_torch", "minibatch_stage_torch", "train_commit", "_cut_args", "window_cut", "window_cut_torch", "_gather_args",
    "window_gather", "window_gather_torch", "DeviceAdam", "_StepBook", "_PolicySGD", "_learner_options", "PPOLearner", "CMD_LD", "GRU_H",
    "COMMANDER_STAGE_COLS", "_gru_io", "_gru_scratch_bytes", "gru_seq_tile", "gru_seq_forward", "gru_seq_backward", "_GruSeq", "_check_gru",
    "gru_sequence", "gru_sequence_pair", "gru_cell_torch", "gru_sequence_torch", "ppo_loss_categorical", "ppo_loss_categorical_torch",
    "_GRUWeights", "CommanderTrainable", "standardize_masked", "CommanderLearner")

SIGNATURES = {       # str(inspect.signature(...)) as recorded from the single module
    "PPOLearner.__init__":
        "(self, kinds, state_dicts, device, lr=0.0001, clip_param=0.25, kl_target=0.025, kl_coeff=0.2, vf_clip_param=10.0, vf_loss_coeff=1.0, "
        "entropy_coeff=0.0, num_sgd_iter=30, sgd_minibatch_size=256, max_seq_len=20, seed=0, fused=True, attention='torch', inputs='torch', "
        "trunk='torch', optimizer='torch', step='eager', shuffle_sequences=False, grad_clip=None)",
    "CommanderLearner.__init__":
        "(self, state_dict, device, lr=0.0001, clip_param=0.25, kl_target=0.05, kl_coeff=0.2, vf_clip_param=10.0, vf_loss_coeff=1.0, "
        "entropy_coeff=0.0, num_sgd_iter=30, sgd_minibatch_size=256, max_seq_len=20, seed=0, fused=True, inputs='torch', trunk='torch', "
        "optimizer='torch', step='eager', shuffle_sequences=False, grad_clip=None)",
    "ppo_loss": "(logits, vf, batch, *, n_comp, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2)",
    "ppo_loss_categorical": "(logits, vf, batch, *, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2)",
    "heads_loss": "(za, zc, act_out, val_out, batch, *, n_comp, clip_param=0.25, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, "
                  "kl_coeff=0.2, scale_grad=True)",
}


def test_every_name_of_the_single_module_is_an_attribute_of_the_package():
    assert len(NAMES) == len(set(NAMES)) == 107
    missing = [n for n in NAMES if not hasattr(LR, n)]
    assert not missing, missing


def test_pinned_signatures_are_the_single_modules():
    for path, want in SIGNATURES.items():
        obj = LR
        for part in path.split("."):
            obj = getattr(obj, part)
        assert str(inspect.signature(obj)) == want, path


def test_the_package_imports_no_commander_but_the_parent_packages():
    assert "hhmarl_2d_amd.learner.commander_learner" in sys.modules
    assert [m for m in sys.modules if m.endswith(".commander") and m != "hhmarl_2d_amd.commander"] == []
