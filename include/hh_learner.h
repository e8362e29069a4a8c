/*
 * hh_learner.h — C ABI of the learner side of train_hetero.py's and train_hier.py's PPO (part of libhh_world.so): the fused PPO loss,
 * forward and backward, for the TorchMultiCategorical action distribution of the 2-vs-2 policies and for the commander's Categorical,
 * the commander's GRUs over whole sequences, forward and backward (hh_gru_seq_*), and the fight networks' chunk attention without its
 * GEMMs (hh_chunk_attn_*, hh_residual_normalize_*) and as one whole block with its projections (hh_attn_block_*), the networks' input
 * layers as one grouped stage (hh_input_stage_*), and the layer they share on the matrix cores (hh_dense_tanh_*).
 *
 * What RLlib 2.4's PPOTorchPolicy.loss (ray/rllib/algorithms/ppo/ppo_torch_policy.py) computes from the learner's logits and value
 * predictions, per row that the mask keeps (n = number of such rows):
 *     logp      = sum_c log_softmax(logits_c)[a_c]                          TorchMultiCategorical.logp
 *     ratio     = exp(logp - old_logp)                                      logp_ratio
 *     surrogate = min(adv * ratio, adv * clamp(ratio, 1 - clip, 1 + clip))  surrogate_loss
 *     kl        = sum_c KL(old_c || new_c)                                  prev_action_dist.kl(curr_action_dist)
 *     entropy   = sum_c H(new_c)                                            curr_action_dist.entropy()
 *     vf_loss   = clamp((vf - target)^2, 0, vf_clip_param)                  vf_loss_clipped
 *     total     = sum(-surrogate + vf_loss_coeff * vf_loss - entropy_coeff * entropy) / n  [+ kl_coeff * sum(kl) / n  when kl_coeff > 0]
 * with c over the components of MultiDiscrete([13, 9, 2, 2]) (n_comp = 4, 26 logits) or ([13, 9, 2]) (n_comp = 3, 24 logits).  With
 * kl_coeff <= 0 the KL term is left out and mean_kl is reported as 0.0, as ray does.
 *
 * Conventions as in hh_abi.h: 0 on success or a negative HH_E_* code, never throws; [dev] = caller-owned device memory; `stream` is a
 * hipStream_t passed as void*.
 */
#ifndef HH_LEARNER_H
#define HH_LEARNER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HH_PPO_STATS 6 /* stats f64: total_loss, mean_policy_loss, mean_vf_loss, mean_kl, mean_entropy, n_valid */

typedef struct hh_ppo_loss_params {
    int32_t n_comp; /* 4: splits [13, 9, 2, 2], 26 logits; 3: splits [13, 9, 2], 24 logits */
    int32_t reserved0; /* must be 0 */
    float clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff;
    float reserved1; /* must be 0 */
} hh_ppo_loss_params;

/* bytes of `scratch` a call of n_rows rows needs (the per-workgroup float64 partial sums) */
int hh_ppo_loss_scratch_bytes(int64_t n_rows, int64_t *bytes);

/* Loss and gradients in one pass over the rows (two launches: the row pass, which also writes every gradient, and the final sum of the
 * per-workgroup partials), ordered on `stream`; no host synchronisation, no allocation, HIP-graph capturable.
 *   logits      [dev] f32 [n_rows, ld]   the learner's logits, ld >= 26 | 24 (the columns from there on are ignored)
 *   old_logits  [dev] f32 [n_rows, 32]   the sampler's logits (HH_POLICY_LOGITS rows: hh_policy_act / hh_policy_sample)
 *   actions     [dev] i8  [n_rows, 4]    the sampled action (components outside their range are clamped into it)
 *   old_logp, adv, vf, target [dev] f32 [n_rows]    ACTION_LOGP, standardised advantages, the learner's value predictions, VALUE_TARGETS
 *   mask        [dev] u8  [n_rows]       rows with mask != 0 count (the unpadded rows of RLlib's sequence chunks); NULL = all rows.  A row
 *                                        with mask == 0 may hold anything in every other input, NaN included: nothing of it reaches an output
 *   n_valid     [dev] i32 [1]            the number of rows with mask != 0 (n_rows with mask == NULL): the divisor, known before the pass, which
 *                                        is what makes every row's gradient local.  It is taken as given (stats[5] reports it).  With
 *                                        n_valid = 0 (every row masked) the gradients are all 0.0f, stats[5] is 0 and the means are 0 / 0:
 *                                        total_loss, mean_policy_loss, mean_vf_loss and mean_entropy are NaN, mean_kl is NaN with
 *                                        kl_coeff > 0 and 0.0 otherwise
 *   stats       [dev] f64 [HH_PPO_STATS]
 *   d_logits    [dev] f32 [n_rows, ld]   d total / d logits; exactly 0.0f in masked rows and in the columns beyond the policy's logits
 *   d_vf        [dev] f32 [n_rows]       d total / d vf; exactly 0.0f in masked rows
 *   scratch     [dev] scratch_bytes >= hh_ppo_loss_scratch_bytes(n_rows)
 * logits, old_logits, d_logits and actions must be 16-byte / 4-byte aligned at row 0 (whole tensors are).  Per-row arithmetic is float32;
 * the five sums are float64 in a fixed order (no floating-point atomics): the same inputs give the same bytes on every run.
 * The gradient of min / clamp at their kinks follows PyTorch's autograd (clamp passes the gradient on its closed interval; where
 * the two arguments of min are equal their gradients add up). */
int hh_ppo_loss(int64_t n_rows, int32_t ld, const float *logits, const float *old_logits, const int8_t *actions, const float *old_logp,
                const float *adv, const float *vf, const float *target, const uint8_t *mask, const int32_t *n_valid,
                const hh_ppo_loss_params *prm, double *stats, float *d_logits, float *d_vf, void *scratch, int64_t scratch_bytes, void *stream);

/* The same loss, statistics, determinism and kink conventions for ONE Categorical over HH_CMD_ACTIONS = 3 logits (the commander of
 * train_hier.py: TorchCategorical), another instance of the same row kernel.  The differences from hh_ppo_loss:
 *   logits, old_logits, d_logits  f32 [n_rows, HH_CMD_LOGITS = 4] (hh_commander_sample's logits rows); column 3 is ignored and its
 *                                 gradient is exactly 0.0f
 *   actions                       i8  [n_rows] (values outside 0..2 are clamped into it), no alignment requirement
 *   prm->n_comp                   must be 1 (one component)
 * scratch as for hh_ppo_loss (hh_ppo_loss_scratch_bytes). */
int hh_ppo_loss_categorical(int64_t n_rows, const float *logits, const float *old_logits, const int8_t *actions, const float *old_logp,
                            const float *adv, const float *vf, const float *target, const uint8_t *mask, const int32_t *n_valid,
                            const hh_ppo_loss_params *prm, double *stats, float *d_logits, float *d_vf, void *scratch, int64_t scratch_bytes,
                            void *stream);

/* ---- the learner's GRU over whole sequences (CommanderGru's rnn_act and rnn_val under RLlib's max_seq_len chunks) ----
 *
 * n_gru = 1 | 2 GRUs of width HH_GRU_HIDDEN = 200 (two: the actor's and the critic's in one launch, over the same sequences), n_seq
 * sequences of max_len <= HH_GRU_MAX_LEN steps, sequence s holding seq_len[s] steps followed by padding: 0 <= seq_len[s] <= max_len, and
 * seq_len[0] >= 1 (row 0 of every tensor is what a sequence that has ended loads and drops).  A sequence of length 0 — a padding slot of a
 * staged minibatch — gives exact zeros in all of y, d_gi, d_gh and d_h0, its gi, h0 and dy are not read, and it changes no other
 * sequence's bytes.  Per step,
 * torch.nn.GRU's cell with the input projection taken out (it is time-parallel: one GEMM in front):
 *     gh = W_hh h + b_hh;  r = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z);  n = tanh(gi_n + r gh_n);  h' = (1 - z) n + z h
 * Everything is float32 and ordered on `stream`; no allocation, no host synchronisation, no floating-point atomics, HIP-graph capturable;
 * the same inputs give the same bytes on every run.  All pointers are [dev], 16-byte aligned (seq_len: 4-byte); an output may not overlap
 * any other tensor of the call.  The fields a call does not use are ignored. */
#define HH_GRU_HIDDEN 200
#define HH_GRU_MAX_LEN 32

typedef struct hh_gru_seq_io {
    const float *gi;   /* [n_seq, max_len, 600]  x W_ih^T + b_ih, gate columns r | z | n                      forward */
    const float *h0;   /* [n_seq, 200]           the state each sequence starts from                          forward, backward */
    const float *w_hh; /* [600, 200]             gate rows r | z | n, as nn.GRU holds weight_hh_l0            forward, backward */
    const float *b_hh; /* [600]                                                                               forward */
    float *y;          /* [n_seq, max_len, 200]  h after every step; exactly 0.0f at steps t >= seq_len       forward out, backward in */
    const float *dy;   /* [n_seq, max_len, 200]  d loss / d y; steps t >= seq_len are not read                backward */
    float *d_gi;       /* [n_seq, max_len, 600]  d loss / d gi                                                backward out */
    float *d_gh;       /* [n_seq, max_len, 600]  d loss / d gh: d_gi's r and z columns, its n columns times r backward out */
    float *d_h0;       /* [n_seq, 200]                                                                        backward out */
} hh_gru_seq_io;

/* bytes of `scratch`: the k-major copy of every W_hh that the forward makes, then r, z, n and gh_n of every (GRU, sequence, step, unit) */
int hh_gru_seq_scratch_bytes(int32_t n_gru, int64_t n_seq, int32_t max_len, int64_t *bytes);

/* io[n_gru] (host array of device pointers), seq_len [dev] i32 [n_seq].  Writes y and `scratch`.  Steps t >= seq_len[s] compute nothing
 * that a valid step depends on (padding is at the tail) and leave their part of `scratch` unwritten. */
int hh_gru_seq_forward(int32_t n_gru, int64_t n_seq, int32_t max_len, const hh_gru_seq_io *io, const int32_t *seq_len, void *scratch,
                       int64_t scratch_bytes, void *stream);

/* From the forward's `scratch`, y, h0 and w_hh: d_gi, d_gh and d_h0, the recursion dh <- dh z + d_gh W_hh running inside the kernel.
 * Exactly 0.0f at steps t >= seq_len[s].  d_gi and d_gh are separate tensors (they differ in the n columns only; sharing the other two
 * thirds would save 1600 B per step of the 4800 B written).  What is left to the caller: dW_hh = sum over steps of d_gh^T h_prev (one
 * GEMM), db_hh = the column sums of d_gh, and everything upstream of gi. */
int hh_gru_seq_backward(int32_t n_gru, int64_t n_seq, int32_t max_len, const hh_gru_seq_io *io, const int32_t *seq_len, const void *scratch,
                        int64_t scratch_bytes, void *stream);

/* The sequences per workgroup (16, 8 or 4: the compiled instances) that hh_gru_seq_forward / _backward use for n_seq sequences; every
 * instance writes the same bytes, and `scratch` does not depend on it.  The environment variable HH_GRU_TILE, read at every call, forces
 * an instance (for A/B runs); any other value of it is HH_E_ARG, here and in the two entry points, with nothing enqueued.  Without it the
 * tile follows from n_seq alone, so the forward and the backward of one pair always agree.  Host only. */
int hh_gru_seq_tile(int64_t n_seq);

/* ---- the fight networks' self-attention over RLlib's max_seq_len chunks, without its GEMMs (Fight1 / Fight2: att_act of width 100 and
 * att_val of width 150, models/ac_models_hetero.py) ----
 *
 * What nn.MultiheadAttention(embed, 2, batch_first=True)(x, x, x) and F.normalize(x + att) compute between and after the in- and the
 * out-projection, which stay GEMMs with the caller.  Everything is float32 and ordered on `stream`; no allocation, no host
 * synchronisation, no floating-point atomics, HIP-graph capturable; the same inputs give the same bytes on every run.  All pointers are
 * [dev], whole contiguous tensors (4-byte aligned for the core, 8-byte for normalize; norm 4-byte); an output may not overlap any other
 * tensor of the call.  embed and width are 100 or 150 (compile-time instances), 1 <= len <= HH_ATTN_MAX_LEN, n_seq <= 2^24,
 * n_rows <= 2^32; anything else is HH_E_ARG and launches nothing.  n_seq == 0 or n_rows == 0 succeeds without a launch.
 * The exponentials are expf's, the softmax subtracts the row maximum, every sum runs in index order. */
#define HH_ATTN_HEADS 2
#define HH_ATTN_MAX_LEN 32
/* qkv [n_seq, len, 3*embed] = x W_in^T + b_in, columns q | k | v, each split into HH_ATTN_HEADS contiguous head slices of d = embed/2;
 * ctx [n_seq, len, embed]: per sequence and head softmax(Q K^T / sqrt(d)) V, heads concatenated (what nn.MultiheadAttention hands its
 * out_proj).  No mask: all `len` rows of a sequence are keys, zero-padded rows included (the reference passes no key_padding_mask).
 * With len == 1 ctx equals the v columns bit for bit. */
int hh_chunk_attn_forward (int64_t n_seq, int32_t len, int32_t embed, const float *qkv, float *ctx, void *stream);
/* P recomputed from qkv (nothing saved by the forward):  dV = P^T dO;  dP = dO V^T;  dS = P o (dP - rowsum(P o dP));
 * dQ = dS K / sqrt(d);  dK = dS^T Q / sqrt(d);  d_qkv in qkv's layout, so the in-projection's backward stays ONE GEMM */
int hh_chunk_attn_backward(int64_t n_seq, int32_t len, int32_t embed, const float *qkv, const float *d_ctx, float *d_qkv, void *stream);
/* y = s / max(|s|_2, 1e-12), s = x + a, per row (F.normalize(x + att), p = 2, eps = 1e-12); norm [n_rows] = |s|_2 saved for the backward */
int hh_residual_normalize_forward (int64_t n_rows, int32_t width, const float *x, const float *a, float *y, float *norm, void *stream);
/* d_s (= d_x = d_a) = (d_y - y (y . d_y)) / norm where norm >= 1e-12, d_y / 1e-12 elsewhere (autograd of clamp_min and of norm at 0) */
int hh_residual_normalize_backward(int64_t n_rows, int32_t width, const float *y, const float *norm, const float *d_y, float *d_s, void *stream);

/* ---- one whole attention block of a fight network as one launch forward and two backward (learner.attention_block) ----
 *
 *     qkv = x W_in^T + b_in                      [n_seq, len, 3 embed]
 *     ctx = per sequence and head softmax(Q K^T / sqrt(d)) V, heads concatenated      (d = embed / 2, HH_ATTN_HEADS heads, no mask)
 *     a   = ctx W_out^T + b_out
 *     s   = x + a;   y = s / max(|s|_2, 1e-12)   per row
 * what the in-projection GEMM, hh_chunk_attn_forward, the out-projection GEMM and hh_residual_normalize_forward compute one after the
 * other, with their conventions: zero-padded rows are keys like any other, expf with the row maximum subtracted, and backward autograd's
 * clamp branch d_s = d_y / 1e-12 where the norm is below 1e-12.  With len == 1 (the networks' 2-D form) ctx is the v columns bit for bit.
 *   x, y, d_y, d_x  f32 [n_seq, len, embed];  w_in [3 embed, embed], b_in [3 embed] (nn.MultiheadAttention's in_proj_weight / _bias:
 *                   rows q | k | v);  w_out [embed, embed], b_out [embed] (out_proj);  d_w_in .. d_b_out in their shapes
 * embed is 100 or 150 (compile-time instances), 1 <= len <= HH_ATTN_MAX_LEN, 0 <= n_seq <= 2^24; anything else, a null or not 16-byte
 * aligned pointer, an output that overlaps another tensor of the call, or a save / scratch smaller than the queries below say is
 * HH_E_ARG and launches nothing.  n_seq == 0 succeeds without a launch and writes nothing.  Everything is float32 (the five
 * products on the float32-input MFMA, the rest fmaf chains; every sum in an order that the shapes alone decide) and ordered on `stream`; no allocation, no host synchronisation, no atomics, HIP-graph capturable; the same inputs
 * give the same bytes on every run, and a row's y and d_x do not depend on which other sequences the call holds.
 * Tiles: a workgroup owns HH_ATTN_BLOCK_ROWS / len whole sequences (at most HH_ATTN_BLOCK_ROWS rows).  The forward is one launch of one
 * workgroup per tile.  It keeps in `save`, per row, qkv, ctx and |s|_2: (4 embed + 1) * 4 = 1604 | 2404 bytes, each of the three parts
 * rounded up to 16 bytes over the whole call (hh_attn_block_save_bytes); the probabilities are recomputed.  The backward is two launches.
 * The first walks the tiles grid-stride with min(tiles, HH_ATTN_BLOCK_MAX_WG) workgroups (tile t goes to workgroup t mod that number);
 * each writes its tiles' rows of d_x — the complete input gradient: d_s + d_qkv W_in — and keeps its partial d_w_in | d_b_in | d_w_out |
 * d_b_out, (4 embed^2 + 4 embed) floats, in `scratch`, summed over its tiles in tile order (within a tile in row order).  The second adds
 * every element's partials in workgroup order in float64 and rounds once.  Every output is overwritten.  `scratch` stops growing at
 * HH_ATTN_BLOCK_MAX_WG tiles: at most 20.7 | 46.4 MB. */
#define HH_ATTN_BLOCK_ROWS   32    /* rows of a workgroup's tile */
#define HH_ATTN_BLOCK_MAX_WG 128   /* the cap on the backward's workgroups, and so on the partial sums per weight element */
/* the sequences per tile and the workgroups of the backward's first launch for such a call (either pointer may be NULL).  Host only. */
int hh_attn_block_tile(int64_t n_seq, int32_t len, int32_t embed, int32_t *seq_per_tile, int32_t *n_workgroups);
int hh_attn_block_save_bytes(int64_t n_seq, int32_t len, int32_t embed, int64_t *bytes);
int hh_attn_block_scratch_bytes(int64_t n_seq, int32_t len, int32_t embed, int64_t *bytes);
int hh_attn_block_forward(int64_t n_seq, int32_t len, int32_t embed, const float *x, const float *w_in, const float *b_in,
                          const float *w_out, const float *b_out, float *y, void *save, int64_t save_bytes, void *stream);
/* x, w_in, w_out, y and save as the forward took and left them (the biases are not needed) */
int hh_attn_block_backward(int64_t n_seq, int32_t len, int32_t embed, const float *x, const float *w_in, const float *w_out,
                           const float *y, const void *save, int64_t save_bytes, const float *d_y, float *d_x, float *d_w_in,
                           float *d_b_in, float *d_w_out, float *d_b_out, void *scratch, int64_t scratch_bytes, void *stream);

/* ---- the input stage: what every trainable network does in front of shared_layer (inp1..inp4, v1..v4, inp1_val) ----
 *
 * n_groups <= HH_INSTAGE_MAX_GROUPS layers  y_g = tanh(W_g gather_g(src) + b_g)  from ONE source matrix src [n_rows, src_width] (row
 * stride src_ld floats), each layer's input the concatenation of up to HH_INSTAGE_MAX_SEGS column runs of a source row, each output written
 * to its own place: g->y is the first element of the group's columns in a wider (concatenated) tensor of row stride y_ld.
 * Backward, from the saved y (no pre-activation is kept):
 *     d_pre = d_y (1 - y^2);   d_b[n] = sum_r d_pre[r, n];   d_w[n, k] = sum_r d_pre[r, n] src[r, col_k]
 * There is no gradient for src: observations and critic rows are data.
 * All tensors are float32 and everything is ordered on `stream`; no allocation, no host synchronisation, HIP-graph capturable.  The
 * forward is one launch, the backward two: per-workgroup partial sums over the rows into `scratch` (float32 products and sums for d_w;
 * d_b's sum of d_pre runs in float64 and is stored as float32), then the partial sums of every element added in slot order in float64
 * and rounded to float32 once — no floating-point atomics, the same inputs give the same bytes on every run.  The workgroups of the first backward launch walk the row tiles (32 rows)
 * grid-stride, HH_INSTAGE_MAX_PARTS of them at most per column block, so hh_input_stage_scratch_bytes stops growing at
 * HH_INSTAGE_MAX_PARTS * 32 = 2048 rows (it is then HH_INSTAGE_MAX_PARTS * sum_g n_out (K + 1) * 4 bytes).
 * All pointers are [dev] and need 4-byte alignment only; an output may not overlap any other tensor of the call.  HH_E_ARG, with nothing
 * launched: n_groups outside 1..HH_INSTAGE_MAX_GROUPS, n_seg outside 1..HH_INSTAGE_MAX_SEGS, K outside 1..HH_INSTAGE_MAX_K, n_out < 1,
 * sum n_out > HH_INSTAGE_MAX_OUT, an empty segment or one that reaches outside [0, src_width), src_ld < src_width, y_ld < n_out (backward:
 * d_y_ld < n_out too), n_rows < 0, a null pointer among those the call uses, a scratch that is too small.  n_rows == 0 succeeds without a
 * launch.  The fields a call does not use are ignored. */
#define HH_INSTAGE_MAX_GROUPS 4
#define HH_INSTAGE_MAX_SEGS   6     /* commander v4: [o1|a1|o2|a2|o3|a3] */
#define HH_INSTAGE_MAX_K      112   /* widest input: 105 */
#define HH_INSTAGE_MAX_OUT    500   /* sum of n_out over the groups of one call */
#define HH_INSTAGE_MAX_PARTS  64    /* the cap on the backward's partial sums per output element */

typedef struct hh_input_group {     /* field order is ABI; host struct of device pointers, like hh_gru_seq_io */
    int32_t n_out, n_seg;
    int16_t seg_col[HH_INSTAGE_MAX_SEGS], seg_len[HH_INSTAGE_MAX_SEGS]; /* the layer's input = these column runs of a src row, in order; K = sum seg_len */
    const float *w, *b;             /* [n_out, K] (nn.Linear layout), [n_out]                                   forward */
    float *y;  int64_t y_ld;        /* forward out / backward in: first element of this group's columns, row stride in floats */
    const float *d_y; int64_t d_y_ld; /* backward in: d loss / d y, placed like y */
    float *d_w, *d_b;               /* backward out: [n_out, K], [n_out] */
} hh_input_group;

/* bytes of `scratch` that hh_input_stage_backward needs for these groups (n_out, n_seg and the segments are read) and n_rows rows */
int hh_input_stage_scratch_bytes(int32_t n_groups, const hh_input_group *g, int64_t n_rows, int64_t *bytes);
int hh_input_stage_forward (int64_t n_rows, const float *src, int64_t src_ld, int32_t src_width, int32_t n_groups, const hh_input_group *g, void *stream);
int hh_input_stage_backward(int64_t n_rows, const float *src, int64_t src_ld, int32_t src_width, int32_t n_groups, const hh_input_group *g,
                            void *scratch, int64_t scratch_bytes, void *stream);

/* ---- the shared layer: y = tanh(x W^T + b) on the matrix cores, for up to two row blocks that go through the same weights ----
 *
 * n_src <= HH_DENSE_MAX_SRC row blocks x_i [n_rows_i, K] (row stride ld_i >= K floats; the columns from K on are never read), ONE
 * w [N, K] (nn.Linear's layout) and b [N]; y_i [n_rows_i, N] contiguous.  1 <= K, N <= HH_DENSE_MAX_DIM, any value in that range (the
 * networks use 500 / 500); n_rows_i >= 0.  Backward, from the saved y_i (no pre-activation is kept):
 *     d_pre_i = d_y_i (1 - y_i^2);  d_x_i = d_pre_i W  [n_rows_i, K] contiguous;  d_w = sum_i d_pre_i^T x_i;  d_b = sum_i column sums of d_pre_i
 * Arithmetic: every product except d_b's sum is v_mfma_f32_16x16x32_f16 on an fp16 (hi, lo) split of both operands (hi hi + lo hi + hi lo,
 * float32 accumulators).  Every operand is scaled by powers of two before the split (forward: x per row, w per row n; d_x: d_pre per
 * row, w per column k; d_w: d_pre and x per row tile and column) and the scale is undone on the float32 result (both exact: a power-of-two
 * change of a row or column that has a scale of its own moves the matching outputs by that power of two, bit for bit), so d_y of order 1e-12 keeps
 * its 22 bits as well as weights of order 0.03.  Against float64, with n the length of the sum, where the elements that share a scale lie within 2^17 of each other, componentwise:
 *     |C - C64| <= (4 * 2^-22 + (n + 2) * 2^-24) (|A| |B|)      (tests/dense_tanh_ref.py)
 * and otherwise with 2^-38 (amax_i sum_k |b_kj| + bmax_j sum_k |a_ik|) on top: a scale follows the largest element, amax, of its row
 * (tile column for d_w), an element below 2^-17 amax is staged to 2^-39 amax, not to 2^-22 of itself (derivation: tests/dense_tanh_ref.py,
 * "The extended bound").  A row or tile column with a maximum below 2^-111 keeps fewer bits; a row of x or of d_pre (for d_w: a tile column of d_pre) with one above
 * about 2^100 gives inf (the epilogues undo that scale first, on a sum of up to 2^30 n), even where the product with a tiny other operand is representable.
 * Everything is ordered on `stream`; no allocation, no host synchronisation, HIP-graph capturable.  The forward is two launches (the row scales of w into
 * `scratch`; the layer), the backward four: the column scales of w; d_x; per-workgroup partial sums of d_w and d_b over the row tiles (HH_DENSE_ROW_TILE rows; the tiles of block 0, then
 * those of block 1, walked grid-stride by min(HH_DENSE_MAX_PARTS, tiles) workgroups per 128 x 128 block of d_w) into `scratch`; the slots
 * of every element added in slot order in float64 and rounded once (d_b: float64 sums inside a workgroup as well).  No floating-point
 * atomics: the same inputs give the same bytes on every run.  hh_dense_tanh_scratch_bytes (what the backward needs) is HH_DENSE_FWD_SCRATCH_BYTES
 * + min(HH_DENSE_MAX_PARTS, tiles) (N K + N) * 4 (w's scales, then the slots; the forward needs the first HH_DENSE_FWD_SCRATCH_BYTES only, and
 * the two calls need not share a buffer) and stops growing at HH_DENSE_MAX_PARTS * HH_DENSE_ROW_TILE rows; no split copy of w is kept (every workgroup splits the chunks it reads).
 * All pointers are [dev] and need 4-byte alignment only; an output may not overlap any other tensor of the call.  HH_E_ARG, with nothing
 * launched: K or N outside 1..HH_DENSE_MAX_DIM, n_src outside 1..HH_DENSE_MAX_SRC, n_rows < 0, ld < K (forward, backward), a null pointer
 * among those the call uses (the pointers of a block of 0 rows are not used), a scratch that is too small.  With every block at 0 rows the
 * call succeeds without a launch.  The fields a call does not use are ignored. */
#define HH_DENSE_MAX_SRC   2
#define HH_DENSE_MAX_DIM   512
#define HH_DENSE_ROW_TILE  64    /* rows per tile of the backward's partial sums (the forward and d_x take two such tiles per workgroup) */
#define HH_DENSE_MAX_PARTS 32    /* the cap on the backward's partial sums per element of d_w and d_b */
#define HH_DENSE_FWD_SCRATCH_BYTES 2048   /* the forward's `scratch`: HH_DENSE_MAX_DIM exponents */

typedef struct hh_dense_src {     /* field order is ABI; host struct of device pointers, like hh_input_group */
    int64_t n_rows;
    const float *x; int64_t ld;   /* [n_rows, K], row stride in floats                      forward, backward */
    float *y;                     /* [n_rows, N]                                            forward out, backward in */
    const float *d_y;             /* [n_rows, N]  d loss / d y                              backward */
    float *d_x;                   /* [n_rows, K]  d loss / d x                              backward out */
} hh_dense_src;

/* bytes of `scratch` that hh_dense_tanh_backward needs (n_rows of every block is read) */
int hh_dense_tanh_scratch_bytes(int32_t K, int32_t N, int32_t n_src, const hh_dense_src *src, int64_t *bytes);
int hh_dense_tanh_forward (int32_t K, int32_t N, int32_t n_src, const hh_dense_src *src, const float *w, const float *b,
                           void *scratch, int64_t scratch_bytes, void *stream);
int hh_dense_tanh_backward(int32_t K, int32_t N, int32_t n_src, const hh_dense_src *src, const float *w, float *d_w, float *d_b,
                           void *scratch, int64_t scratch_bytes, void *stream);

/* ---- the minibatch step as a fixed chain of launches: staging by a device schedule, Adam on the device, the step's bookkeeping ----
 *
 * What lets PPOLearner(step="graph") replay  stage -> forward -> loss -> backward -> adam -> commit  from ONE HIP graph with no host work
 * between the steps.  Two device counters steer a step: `cursor` (which row of the schedule the stage reads and which row of the
 * statistics table the commit fills) and `step` (Adam's t: the number of steps taken).  No launch reads a counter that a thread of the
 * same launch writes: hh_minibatch_stage and hh_adam_step only READ them, hh_train_commit — one launch of one thread, ordered by the
 * stream after the Adam launch — is the only writer.  All three are ordered on `stream`: no atomics, no allocation, no host
 * synchronisation, HIP-graph capturable; the same inputs give the same bytes on every run.  HH_E_ARG, with nothing enqueued: a null
 * pointer, a negative count, cap < 1, chunk_len < 1.  An empty tensor / column list succeeds without a launch. */
#define HH_ADAM_MAX_TENSORS 64   /* descriptors per launch: 64 x 48 bytes by value, inside the 4 KiB of kernel arguments; longer lists take more launches */
#define HH_STAGE_MAX_COLS   8    /* columns of one hh_minibatch_stage call */

typedef struct hh_adam_tensor {  /* field order is ABI; host struct of device pointers */
    float *p; const float *g; float *m; float *v;   /* parameter, gradient, first and second moment: f32 [n], 4-byte aligned */
    int64_t n;
} hh_adam_tensor;

/* One step of torch.optim.Adam (amsgrad = False, weight_decay = 0, maximize = False) on every tensor of t[n_tensors] (host array), float32:
 *     m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2;   p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * with t = step[0] + 1 read from the device ([dev] i32 [1]: the steps taken so far; hh_train_commit advances it).  The bias corrections
 * are computed once per workgroup in float64.  Every element is stepped in float64 from its float32 inputs and each stored value is rounded
 * to float32 once: m and v are the correctly rounded updates of the stored state, p moves by the float64 step from the stored m and v
 * (the kernel moves 28 bytes per element and stays memory-bound).  A gradient of 0 on fresh state leaves p bit for bit.  A tensor
 * whose four pointers are 16-byte aligned is stepped in float4s with a scalar tail of n % 4 elements; any other tensor element by element
 * (the same arithmetic).  ceil(n_tensors / HH_ADAM_MAX_TENSORS) launches, the descriptors by value.  Tensors may not overlap. */
int hh_adam_step(int32_t n_tensors, const hh_adam_tensor *t, const int32_t *step, double lr, double beta1, double beta2, double eps, void *stream);

/* Gradient clipping by global norm (RLlib's grad_clip, torch.nn.utils.clip_grad_norm_ with norm_type 2) as two more links of the chain:
 * stage -> forward -> loss -> backward -> norm -> clipped Adam -> commit.
 *
 * The norm, over EVERY element of EVERY tensor of t[n_tensors] (only g and n are read; p, m, v may be NULL), in float64:
 *     norm = sqrt(sum (double)g * (double)g);   coef = min(1.0, max_norm / (norm + 1e-6))
 *     clip[0] = norm;  clip[1] = coef;  and, where cursor and table are given, table[cursor[0]] = norm
 * ([dev] clip f64 [HH_CLIP_OUT], cursor i32 [1], table f64 [table_rows]; the row is skipped when cursor[0] is outside [0, table_rows); the
 * cursor is only read).  No atomics and a fixed order of additions: one float64 partial per tensor and HTS_ADAM_TILE (4096) elements, in list
 * order, goes into scratch ([dev], 8-byte aligned, at least the bytes the _scratch_bytes query returns = 8 x tiles) — per workgroup thread
 * k sums elements 4k .. 4k+3 of each 1024-element row of its tile in ascending order, a 64-lane shuffle tree folds each wave, the waves are
 * added in order through LDS — and ONE final launch of one workgroup adds the slots the same way (thread k: slots k, k + 256, ..).  The
 * same inputs give the same bytes on every run, whatever g's alignment (float4 loads where g is 16-byte aligned, four float loads
 * otherwise: the same elements in the same order).  The squares are exact in float64, so the norm is within n x 2^-53 (relative) of the
 * exact one for n elements, for gradients whose float32 squares would overflow or vanish as well.  Launches: one per HH_ADAM_MAX_TENSORS
 * non-empty tensors, then the final one — which is also enqueued for an empty list or all n == 0: clip = (0.0, 1.0) for max_norm >= 1e-6.
 * Non-finite gradients give what IEEE arithmetic gives (a NaN norm gives a NaN coefficient), as clip_grad_norm_(error_if_nonfinite=False).
 * HH_E_ARG, with nothing enqueued: a null clip, a negative count, max_norm not finite or not > 0, exactly one of cursor / table,
 * table_rows < 0, a scratch that is too small, a tensor that hh_adam_step would refuse for its g or n. */
#define HH_CLIP_OUT 2   /* clip f64 [2]: the norm before clipping, the coefficient */
int hh_grad_norm_scratch_bytes(int32_t n_tensors, const hh_adam_tensor *t, int64_t *bytes);
int hh_grad_norm(int32_t n_tensors, const hh_adam_tensor *t, double max_norm, double *clip, const int32_t *cursor,
                 double *table, int32_t table_rows, void *scratch, int64_t scratch_bytes, void *stream);

/* hh_adam_step with every gradient read as g' = (float)((double)g * clip[1]) ([dev] clip f64 [HH_CLIP_OUT], hh_grad_norm's): the product is
 * rounded to float32 once, then the step is hh_adam_step's, so clip[1] == 1.0 writes exactly its bytes.  The gradients are not written
 * back (g keeps the unscaled values); the same 28 bytes per element move.  Arguments, launches and refusals as hh_adam_step, and a null clip. */
int hh_adam_step_clipped(int32_t n_tensors, const hh_adam_tensor *t, const int32_t *step, const double *clip,
                         double lr, double beta1, double beta2, double eps, void *stream);

typedef struct hh_stage_col {    /* field order is ABI; host struct of device pointers */
    const void *src;             /* the policy batch's column: [src_chunks] chunks of chunk_bytes bytes */
    void *dst;                   /* its staging buffer: [cap] chunks */
    int64_t chunk_bytes;         /* bytes of one chunk (chunk_len rows): a positive multiple of chunk_len */
} hh_stage_col;

/* ONE launch: with (s0, s1, nv, 0) = schedule[cursor[0]] ([dev] i32 [sched_rows, 4]: first chunk, last chunk + 1, unpadded rows) every column's
 * chunks s0 .. s1-1 go byte for byte to the front of its staging buffer, chunks s1-s0 .. cap-1 of every staging buffer become zero (on
 * every call: a previous, larger minibatch leaves nothing behind), and n_valid[0] = nv.  The copy unit of a column is the widest of 16, 8,
 * 4, 2, 1 bytes that src, dst and chunk_bytes are all multiples of.  chunk_len is the rows per chunk (20 for the fight networks, 1 for rows).
 * The kernel clamps what it reads from the table to 0 <= s0 <= s1 <= src_chunks and s1 - s0 <= cap, and a cursor outside
 * [0, sched_rows) stages an empty minibatch, so no table content makes it touch memory outside the columns.  cursor is not written. */
int hh_minibatch_stage(int32_t n_cols, const hh_stage_col *cols, int32_t chunk_len, int32_t cap, int64_t src_chunks, const int32_t *schedule,
                       int32_t sched_rows, const int32_t *cursor, int32_t *n_valid, void *stream);

/* hh_minibatch_stage with the chunks named by an ORDER TABLE, so that a minibatch may hold any chunks of the batch in any order (the
 * learners' shuffle_sequences).  ONE launch: with (o0, o1, nv, 0) = schedule[cursor[0]] — o0, o1 positions in order ([dev] i32 [order_len]) —
 * clamped to 0 <= o0 <= o1 <= order_len and o1 - o0 <= cap, staged chunk i < o1 - o0 of every column is its source chunk c = order[o0 + i],
 * byte for byte, where 0 <= c < src_chunks, and zero for any other c; chunks o1-o0 .. cap-1 of every staging buffer become zero (on every
 * call), and n_valid[0] = nv.  A cursor outside [0, sched_rows) stages an empty minibatch.  cursor, order and schedule are only read, and no
 * content of either table makes the kernel touch memory outside the tables, the columns and the staging buffers.  Arguments, refusals, copy
 * units and the column limit are hh_minibatch_stage's, and HH_E_ARG also for a null order or order_len < 0.  A group of 1 .. 64 lanes
 * copies one staged chunk (about four copy units per lane) and reads its order entry once.  The same inputs give the same bytes. */
int hh_minibatch_stage_gather(int32_t n_cols, const hh_stage_col *cols, int32_t chunk_len, int32_t cap, int64_t src_chunks,
                              const int32_t *order, int64_t order_len, const int32_t *schedule, int32_t sched_rows,
                              const int32_t *cursor, int32_t *n_valid, void *stream);

/* The step's bookkeeping, one thread: table[cursor[0]] = stats (f64 [HH_PPO_STATS], hh_ppo_loss's; skipped when cursor[0] is outside
 * [0, table_rows)), cursor[0] += 1, step[0] += 1.  All pointers [dev]. */
int hh_train_commit(const double *stats, double *table, int32_t table_rows, int32_t *cursor, int32_t *step, void *stream);

/* ---- the tail of the minibatch step as ONE row pass: tanh, both output heads, the PPO loss, and the backward of all three ----
 *
 * What lies between shared_layer's GEMM and the gradient that flows back into it (learner.heads_loss), for n_rows rows:
 *     h = tanh(za);  y = tanh(zc);  logits = h w_act^T + b_act;  vf = y . w_val + b_val
 *     stats, d_logits, d_vf: hh_ppo_loss's (prm->n_comp = 4 | 3) or hh_ppo_loss_categorical's (prm->n_comp = 1), by the same device code
 *     d_za = (d_logits w_act) (1 - h^2);  d_zc = d_vf w_val (1 - y^2)
 *     d_w_act = d_logits^T h;  d_b_act = column sums of d_logits;  d_w_val = d_vf^T y;  d_b_val = sum of d_vf
 * with n_out = 26 | 24 | 3 logits for n_comp = 4 | 3 | 1.  All [dev], float32 unless said:
 *   za, zc          [n_rows, 500]   shared_layer's output for the actor's and the critic's rows, bias added, BEFORE tanh
 *   w_act, b_act    [n_out, 500], [n_out]   act_out;    w_val, b_val  [500], [1]   val_out
 *   old_logits      [n_rows, 32] (n_comp 4 | 3) or [n_rows, 4] (n_comp 1);  actions i8 [n_rows, 4] or i8 [n_rows]
 *   old_logp, adv, target [n_rows];  mask u8 [n_rows] or NULL;  n_valid i32 [1]: as hh_ppo_loss / hh_ppo_loss_categorical take them
 *   stats           f64 [HH_PPO_STATS]: the same six slots (hh_train_commit takes it as it stands)
 *   d_za, d_zc      [n_rows, 500]   d total / d pre-activation;  d_w_act [n_out, 500], d_b_act [n_out], d_w_val [500], d_b_val [1]
 *   logits, vf      [n_rows, n_out], [n_rows]: optional (NULL = not written); 0.0f in masked rows
 *   scratch         scratch_bytes >= hh_heads_loss_scratch_bytes(n_rows, n_comp): per workgroup 4 + n_out + 1 float64 sums and
 *                   (n_out + 1) * 500 float32 partial sums; at most 256 workgroups (13.9 MB at n_out = 26)
 * Two launches, ordered on `stream`; no host synchronisation, no allocation, no atomics, HIP-graph capturable.  The same inputs give the
 * same bytes on every run: the mapping of the 16-row tiles to workgroups and the order of every addition depend on n_rows and n_comp
 * only (hh_heads_loss_geometry reports both numbers).  Per-row arithmetic is float32 fmaf, accumulated in float32; d_w's partial sums are
 * float32 inside a workgroup and added across workgroups in float64, rounded once; d_b and the five loss sums are float64 throughout.
 * A row with mask == 0 may hold anything, NaN included, in every input, za and zc among them: nothing of it reaches an output, its d_za
 * and d_zc rows are exactly 0.0f, and the weight sums step over it (selection, not a multiplication by 0).  With n_valid <= 0 every row
 * counts as masked: every gradient is exactly 0.0f and stats is what hh_ppo_loss documents for n_valid = 0.
 * HH_E_ARG, with nothing written: a NULL pointer other than mask, logits, vf; za, zc, d_za or d_zc not 16-byte aligned (scratch, stats:
 * 8-byte; actions of n_comp 4 | 3: 4-byte); n_comp outside {1, 3, 4}; a non-zero reserved field; n_rows < 1 (or > 2^30); a scratch
 * smaller than hh_heads_loss_scratch_bytes says.  An output may not overlap any other tensor of the call. */
int hh_heads_loss_scratch_bytes(int64_t n_rows, int32_t n_comp, int64_t *bytes);
/* the geometry a call of n_rows rows uses: rows per tile, and the workgroups that walk the tiles grid-stride (tile t goes to workgroup
 * t mod n_workgroups).  Host only. */
int hh_heads_loss_geometry(int64_t n_rows, int32_t n_comp, int32_t *tile_rows, int32_t *n_workgroups);
int hh_heads_loss(int64_t n_rows, const float *za, const float *zc, const float *w_act, const float *b_act, const float *w_val,
                  const float *b_val, const float *old_logits, const int8_t *actions, const float *old_logp, const float *adv,
                  const float *target, const uint8_t *mask, const int32_t *n_valid, const hh_ppo_loss_params *prm, double *stats,
                  float *d_za, float *d_zc, float *d_w_act, float *d_b_act, float *d_w_val, float *d_b_val, float *logits, float *vf,
                  void *scratch, int64_t scratch_bytes, void *stream);

/* ---- the window batch: a rollout's fixed [T, N] window (batch_mode = "truncate_episodes") as the learners' padded sequences ----
 *
 * The rollouts' collect buffers are step-rows [T, N, ...]: row (t, n) of a column starts (t N + n) * step_bytes bytes into it, so the rows
 * of one arena lie N step-rows apart.  hh_window_cut names the sequences of the window, hh_window_gather copies any columns of it into
 * the [S, L, ...] form that the learners' drivers take.  Both are ordered on `stream`: no atomics, no allocation, no host
 * synchronisation, HIP-graph capturable; the same inputs give the same bytes on every run.  All pointers are [dev]. */
#define HH_WINDOW_MAX_LEN 32   /* the longest sequence (max_seq_len) */

/* The cut, per arena n, walking t = 0 .. T-1: a sequence ends at row t when done[t, n] != 0 (done u8 [T, N]: any non-zero byte), or it
 * holds max_seq_len rows, or t == T-1; the next one starts at t + 1.  Every row belongs to exactly one sequence, no sequence holds a done
 * row except as its last, and a sequence never leaves its arena — RLlib's chop_into_sequences on the window's fragments (an arena's rows
 * up to and including each done row, the last fragment ending at T-1).
 *   seq_t0, seq_arena, seq_len  i32, capacity T N each: sequence s is rows seq_t0[s] .. seq_t0[s] + seq_len[s] - 1 of arena seq_arena[s],
 *                               1 <= seq_len[s] <= max_seq_len; ARENA-MAJOR, then time.  Entries at and beyond n_seq are not written
 *   n_seq                       i32 [1]: S <= T N, so there is no overflow case
 *   scratch                     i32 [N]
 * Three launches: one lane per arena counts its sequences (the lanes of a wave read neighbouring bytes of done at every t), one
 * workgroup turns the counts into exclusive offsets and writes n_seq, the walk again writes every arena's entries from its offset.
 * HH_E_ARG, with nothing enqueued: a null pointer, T < 1, N < 1, T N >= 2^31, max_seq_len outside 1 .. HH_WINDOW_MAX_LEN. */
int hh_window_cut(int32_t T, int32_t N, const uint8_t *done, int32_t max_seq_len, int32_t *seq_t0, int32_t *seq_arena, int32_t *seq_len,
                  int32_t *n_seq, int32_t *scratch, void *stream);

typedef struct hh_window_col {   /* field order is ABI; host struct of device pointers, passed by value like hh_stage_col */
    const void *src;             /* the window's column: [T_src, N] step-rows */
    void *dst;                   /* [S, max_seq_len, width] bytes, or [S, width] with per_seq */
    int64_t step_bytes;          /* bytes from step-row (t, n) to (t, n + 1) */
    int64_t offset;              /* bytes from the step-row's start to the slice wanted (one agent's part); offset + width <= step_bytes */
    int64_t width;               /* bytes copied per row, 1 .. 2^20 */
    int32_t per_seq;             /* 0: every row of the sequence; 1: its first row only (the state a sequence starts from) */
    int32_t reserved0;           /* must be 0 */
} hh_window_col;

/* ONE launch for n_cols <= HH_STAGE_MAX_COLS columns and S sequences (a host argument: hh_window_cut's n_seq, read back once).  With
 * (t0, n, len) = (seq_t0[s], seq_arena[s], seq_len[s]):
 *   per_seq = 0:  dst[s, j] = the `width` bytes at src + ((t0 + j) N + n) * step_bytes + offset  for j < len, and zero for len <= j < max_seq_len,
 *                 written on every call (a destination need not be cleared)
 *   per_seq = 1:  dst[s] = those bytes of row j = 0 (zero where len == 0)
 * T_src is the step-rows per arena that every column of the call holds (the window's T, or T + 1 where all of them carry the row after
 * the window) and N the arenas.  The kernel clamps what it reads from the tables: an entry with t0 < 0, len < 0, len > max_seq_len,
 * t0 + len > T_src or an arena outside [0, N) stages zeros, so no table content makes it touch memory outside the columns and the
 * destinations (hh_minibatch_stage's contract).  The copy unit of a column is the widest of 16, 8, 4, 2, 1 bytes that src, dst, step_bytes,
 * offset and width are all multiples of.  A group of 1 .. 64 lanes copies one sequence of one column (about four copy units per lane) and
 * reads its table entry once.  S == 0 succeeds without a launch.  HH_E_ARG, with nothing enqueued: a null pointer, n_cols outside
 * 1 .. HH_STAGE_MAX_COLS, max_seq_len outside 1 .. HH_WINDOW_MAX_LEN, S < 0 (or >= 2^31), T_src < 1, N < 1, a width outside 1 .. 2^20, a negative
 * offset, offset + width > step_bytes, per_seq other than 0 | 1, a non-zero reserved field. */
int hh_window_gather(int32_t n_cols, const hh_window_col *cols, int64_t S, int32_t max_seq_len, int32_t T_src, int32_t N,
                     const int32_t *seq_t0, const int32_t *seq_arena, const int32_t *seq_len, void *stream);

/* ---- a data-parallel minibatch step whose bytes do not depend on the number of ranks: pack, (all-gather), combine ----
 *
 * W shards each run forward, loss and backward on their own minibatch; the step's gradient is the weighted sum of the shards' gradients
 * (weight_r = the shard's unpadded rows / the step's rows over all shards).  A ring or tree all-reduce adds in an order that depends on W
 * and on the rank; here every rank receives all W gradients (one all-gather of a flat bucket) and adds them itself in SHARD ORDER, so a
 * W-rank step writes the bytes that one process holding the W shards writes.  Both launches are ordered on `stream`: no atomics, no
 * scratch, no allocation, no host synchronisation, HIP-graph capturable; descriptors by value, HH_ADAM_MAX_TENSORS per launch. */
#define HH_GRAD_MAX_SHARDS 64    /* the weights travel by value: 64 x 8 bytes beside the descriptors */

typedef struct hh_grad_tensor {  /* field order is ABI; host struct of a device pointer */
    float *g;                    /* the gradient: f32 [n], 4-byte aligned (float4 accesses where it is 16-byte aligned).  NULL: a parameter without one */
    int64_t n;
    int64_t off;                 /* its first element in the bucket: a multiple of 4 */
} hh_grad_tensor;

/* bucket[t[i].off .. + t[i].n) = t[i].g, byte for byte, for every tensor of t[n_tensors] (host array, off ascending from t[0].off = 0, the
 * ranges disjoint); every other element of bucket[0 .. bucket_elems) — the padding behind a tensor up to the next one's off, behind the
 * last one up to bucket_elems, and the whole range of a tensor with g == NULL — is written as +0.0f, on every call.  [dev] bucket f32
 * [bucket_elems], 16-byte aligned, bucket_elems a multiple of 4.  HH_E_ARG, with nothing enqueued: n_tensors < 1, a null t or bucket, a
 * bucket that is not 16-byte aligned, bucket_elems negative or no multiple of 4, t[0].off != 0, an off that is no multiple of 4 or not
 * ascending, a range that leaves the bucket or reaches into the next tensor's, n < 0, a gradient that is not 4-byte aligned. */
int hh_grad_pack(int32_t n_tensors, const hh_grad_tensor *t, float *bucket, int64_t bucket_elems, void *stream);

/* For every tensor with g != NULL and every element i < n, from [dev] buckets f32 [n_shards, bucket_elems] (16-byte aligned) and the HOST
 * array weight f64 [n_shards] (copied into the launch; 1 <= n_shards <= HH_GRAD_MAX_SHARDS), with b[r] = buckets[r, off + i]:
 *     acc = (double)b[0] * weight[0];   for r = 1 .. n_shards-1:  acc = acc + (double)b[r] * weight[r];   g[i] = (float)acc
 * every product and every sum rounded on its own (never fused), the additions in shard order, one rounding to float32 at the end.
 * Starting from shard 0's product, not from 0.0, makes n_shards = 1 with weight 1.0 the exact identity (-0.0 and denormals included).
 * Non-finite inputs give what IEEE arithmetic gives (inf x 0.0 is NaN).  A tensor with g == NULL or n == 0 is skipped; an empty list
 * succeeds without a launch.  g may not overlap the buckets.  HH_E_ARG, with nothing enqueued: a negative count, a null t, buckets or
 * weight, n_shards outside 1 .. HH_GRAD_MAX_SHARDS, the bucket refusals of hh_grad_pack, an off that is negative or no multiple of 4, a
 * range that leaves the bucket, n < 0, a gradient that is not 4-byte aligned. */
int hh_grad_combine(int32_t n_tensors, const hh_grad_tensor *t, const float *buckets, int64_t bucket_elems, int32_t n_shards,
                    const double *weight, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HH_LEARNER_H */
