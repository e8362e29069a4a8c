/*
 * hh_ppo_loss.h — the fused PPO loss of train_hetero.py's learner, forward and backward in one pass (C ABI and the formulas:
 * include/hh_learner.h; RLlib 2.4 PPOTorchPolicy.loss over a TorchMultiCategorical).
 *
 * HBM-streaming: per row ld + 32 floats of logits in, ld floats of gradient out, 25 B of scalars in, 4 B out (361 B at ld = 26), against
 * 2 exp per logit and 2 log per action component.
 *
 * Access pattern — rows staged through LDS.  A row is 24, 26 or 32 floats, so one lane per row reading global memory would touch
 * 64 different 128-byte lines per load instruction.  Instead a workgroup of 256 lanes owns a tile of 256 consecutive rows, which is one
 * CONTIGUOUS span of memory in every one of the three row-major arrays: the tile is copied with 16-byte-per-lane loads in flat element
 * order (fully coalesced, 1 KiB per wave instruction) into LDS rows of ODD stride (ld | 1 for the learner's logits, 27 for the n_out <= 26
 * columns of the sampler's 32-wide rows), then lane r works on row r — consecutive lanes sit an odd number of banks apart, so the
 * per-lane row reads and writes are conflict-free — writes its row's gradient over its logits, and the tile goes back to global
 * memory in flat order again.  The alternative, a group of 32 lanes per row with shuffles for the per-component soft-max, keeps the loads
 * coalesced too but spends 5 shuffle steps per reduction for components of 13, 9, 2 and 2 elements and leaves 6 to 8 of 32 lanes idle;
 * with a lane per row each component's logits live in registers (fully unrolled, width known at compile time) and need no cross-lane
 * traffic at all.  LDS: 256 x 33 x 4 + 256 x 27 x 4 = 61440 B per workgroup (two workgroups per CU).
 *
 * One pass: the divisor n_valid is an input, so every row's gradient is complete when the row has been read once —
 *     d total / d logit_j = -(wr / n) (onehot_j - p_j) + (entropy_coeff / n) p_j (log p_j + H_c) + (kl_coeff / n) (p_j - q_j)
 *     wr = adv * ratio where the surrogate's min picks the unclipped term or the ratio is inside the clip range, else 0
 *     d total / d vf = (vf_loss_coeff / n) 2 (vf - target) where (vf - target)^2 <= vf_clip_param, else 0
 * — the part that needs the row's ratio (all components' logp) is applied in a second sweep over the lane's own LDS row, no exp in it.
 * Reductions: each lane's four row terms (-surrogate, vf_loss, kl, entropy) go to float64, a fixed shuffle tree per wave, the four
 * waves in index order, one partial per workgroup into `scratch`; hh_k_ppo_loss_final adds the partials in a fixed order.  No atomics.
 *
 * The commander's Categorical (hh_ppo_loss_categorical) is the instance NCOMP = 1 of the same kernel: one component of 3 logits, the
 * sampler's rows 4 floats wide instead of 32, one action byte per row instead of a word of four.
 */
#ifndef HH_PPO_LOSS_H
#define HH_PPO_LOSS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hh_commander.h"
#include "hh_learner.h"

#define HHL_ROWS 256       /* rows per workgroup tile = lanes per workgroup */
#define HHL_OLD_LD 32      /* HH_POLICY_LOGITS */
#define HHL_OLD_STRIDE 27  /* LDS row stride of the sampler's logits: the 26 columns that carry logits, padded to an odd stride */
#define HHL_NEW_STRIDE_MAX 33

/* one action component of width W at columns [LO, LO + W) of the lane's LDS rows: accumulates logp / entropy / kl, leaves
 * g0_j = cE p_j (log p_j + H) + cK (p_j - q_j) in the learner's row and t_j = onehot_j - p_j in the sampler's row */
template <int W, int LO>
__device__ __forceinline__ void hhl_component(float *__restrict__ rn, float *__restrict__ ro, int a, float cE, float cK, bool want_kl,
                                              float &logp, float &ent, float &kl) {
    float x[W], y[W];
    float m = rn[LO], mo = ro[LO];
#pragma unroll
    for (int i = 0; i < W; i++) {
        x[i] = rn[LO + i];
        y[i] = ro[LO + i];
        m = fmaxf(m, x[i]);
        mo = fmaxf(mo, y[i]);
    }
    float S = 0.0f, So = 0.0f;
    float e[W], eo[W];
#pragma unroll
    for (int i = 0; i < W; i++) {
        x[i] -= m;
        y[i] -= mo;
        e[i] = expf(x[i]);
        eo[i] = expf(y[i]);
        S += e[i];
        So += eo[i];
    }
    const float lS = logf(S), lSo = logf(So);
    const float rS = 1.0f / S, rSo = 1.0f / So;
    float H = 0.0f, K = 0.0f;
#pragma unroll
    for (int i = 0; i < W; i++) {
        x[i] -= lS;           /* log p_i */
        y[i] -= lSo;          /* log q_i */
        e[i] *= rS;           /* p_i */
        eo[i] *= rSo;         /* q_i */
        H -= e[i] * x[i];
        K += eo[i] * (y[i] - x[i]);
    }
    a = a < 0 ? 0 : (a > W - 1 ? W - 1 : a);
#pragma unroll
    for (int i = 0; i < W; i++) {
        if (i == a) logp += x[i];
        rn[LO + i] = cE * (e[i] * (x[i] + H)) + (want_kl ? cK * (e[i] - eo[i]) : 0.0f);
        ro[LO + i] = (i == a ? 1.0f : 0.0f) - e[i];
    }
    ent += H;
    if (want_kl) kl += K;
}

/* one row that the mask keeps, on the lane's LDS rows rn (the learner's logits, NOUT of them; the columns up to ld are zeroed) and ro (the
 * sampler's): rn becomes d total / d logits, the four row terms come back as float64, -> d total / d vf.  Shared by hh_k_ppo_loss and
 * hh_k_heads_loss (hh_heads_loss.h), so the formulas and the kink conventions exist once. */
template <int NCOMP>
__device__ __forceinline__ float hhl_row(float *__restrict__ rn, float *__restrict__ ro, int ld, int64_t row, const int32_t *__restrict__ actions,
                                         float old_logp, float A, float vf, float target, float inv_n, float clip, float vf_clip, float vf_coeff,
                                         float ent_coeff, float kl_coeff, double &t_pol, double &t_vf, double &t_kl, double &t_ent) {
    constexpr int NOUT = NCOMP == 4 ? 26 : (NCOMP == 3 ? 24 : HH_CMD_ACTIONS);
    const bool want_kl = kl_coeff > 0.0f;
    const float cE = ent_coeff * inv_n, cK = kl_coeff * inv_n;
    float logp = 0.0f, ent = 0.0f, kl = 0.0f;
    if constexpr (NCOMP == 1) {
        hhl_component<HH_CMD_ACTIONS, 0>(rn, ro, (int)reinterpret_cast<const int8_t *>(actions)[row], cE, cK, want_kl, logp, ent, kl);
    } else {
        const int32_t aw = actions[row];
        hhl_component<13, 0>(rn, ro, (int)(int8_t)(aw & 0xff), cE, cK, want_kl, logp, ent, kl);
        hhl_component<9, 13>(rn, ro, (int)(int8_t)((aw >> 8) & 0xff), cE, cK, want_kl, logp, ent, kl);
        hhl_component<2, 22>(rn, ro, (int)(int8_t)((aw >> 16) & 0xff), cE, cK, want_kl, logp, ent, kl);
        if (NCOMP == 4) hhl_component<2, 24>(rn, ro, (int)(int8_t)((aw >> 24) & 0xff), cE, cK, want_kl, logp, ent, kl);
    }
    const float ratio = expf(logp - old_logp);
    const float lo = 1.0f - clip, hi = 1.0f + clip;
    const float s1 = A * ratio, s2 = A * fminf(fmaxf(ratio, lo), hi);
    const float surr = fminf(s1, s2);
    const bool inside = ratio >= lo && ratio <= hi;
    const float wr = (inside || s1 < s2) ? s1 * inv_n : 0.0f;   /* d surrogate / d logp = adv * ratio where the gradient passes */
    const float dv = vf - target;
    const float sq = dv * dv;
    const float vl = fminf(fmaxf(sq, 0.0f), vf_clip);
    float gv = 0.0f;
    if (sq <= vf_clip) gv = vf_coeff * inv_n * (2.0f * dv);
#pragma unroll
    for (int j = 0; j < NOUT; j++) rn[j] = rn[j] - wr * ro[j];
    for (int j = NOUT; j < ld; j++) rn[j] = 0.0f;
    t_pol = (double)(-surr);
    t_vf = (double)vl;
    t_kl = (double)kl;
    t_ent = (double)ent;
    return gv;
}

template <int NCOMP>
__global__ __launch_bounds__(HHL_ROWS) void hh_k_ppo_loss(int64_t R, int ld, const float *__restrict__ logits, const float *__restrict__ old_logits,
                                                          const int32_t *__restrict__ actions /* i8 [R, 4] as one word per row; NCOMP = 1: i8 [R] */,
                                                          const float *__restrict__ old_logp, const float *__restrict__ adv,
                                                          const float *__restrict__ vf, const float *__restrict__ target,
                                                          const uint8_t *__restrict__ mask, const int32_t *__restrict__ n_valid, float clip,
                                                          float vf_clip, float vf_coeff, float ent_coeff, float kl_coeff,
                                                          double *__restrict__ partial, float *__restrict__ d_logits, float *__restrict__ d_vf) {
    constexpr int NOUT = NCOMP == 4 ? 26 : (NCOMP == 3 ? 24 : HH_CMD_ACTIONS);
    constexpr int OLD_LD = NCOMP == 1 ? HH_CMD_LOGITS : HHL_OLD_LD;   /* row width of the sampler's logits */
    __shared__ float s_new[HHL_ROWS * HHL_NEW_STRIDE_MAX];
    __shared__ float s_old[HHL_ROWS * HHL_OLD_STRIDE];
    __shared__ double s_red[4][4];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * HHL_ROWS;
    const int rows = (int)((R - row0) < HHL_ROWS ? (R - row0) : HHL_ROWS);   /* >= 1: the grid is ceil(R / 256) */
    const int sn = ld | 1;
    const int nf = rows * ld, nfo = rows * OLD_LD;

    /* ---- the tile in: flat element order, 16 B per lane; the last elements of a partial tile one by one */
    {
        const float *__restrict__ g = logits + row0 * ld;
        for (int e0 = tid * 4; e0 < nf; e0 += HHL_ROWS * 4) {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const int cnt = nf - e0 < 4 ? nf - e0 : 4;
            if (cnt == 4) {
                const float4 q = *reinterpret_cast<const float4 *>(g + e0);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                for (int k = 0; k < cnt; k++) v[k] = g[e0 + k];
            }
            int r = e0 / ld, c = e0 - r * ld;
            for (int k = 0; k < cnt; k++) {
                s_new[r * sn + c] = v[k];
                if (++c == ld) { c = 0; r++; }
            }
        }
        const float *__restrict__ go = old_logits + row0 * OLD_LD;
        for (int e0 = tid * 4; e0 < nfo; e0 += HHL_ROWS * 4) {   /* nfo is a multiple of 4 */
            const float4 q = *reinterpret_cast<const float4 *>(go + e0);
            const int r = e0 / OLD_LD, c = e0 % OLD_LD;
            float *d = s_old + r * HHL_OLD_STRIDE + c;
            if (c + 0 < NOUT) d[0] = q.x;
            if (c + 1 < NOUT) d[1] = q.y;
            if (c + 2 < NOUT) d[2] = q.z;
            if (c + 3 < NOUT) d[3] = q.w;
        }
    }
    __syncthreads();

    /* ---- lane r, row r */
    double t_pol = 0.0, t_vf = 0.0, t_kl = 0.0, t_ent = 0.0;
    if (tid < rows) {
        const int64_t row = row0 + tid;
        float *rn = s_new + tid * sn;
        float *ro = s_old + tid * HHL_OLD_STRIDE;
        const bool on = mask == nullptr || mask[row] != 0;
        float gv = 0.0f;
        if (on) {
            gv = hhl_row<NCOMP>(rn, ro, ld, row, actions, old_logp[row], adv[row], vf[row], target[row], 1.0f / (float)n_valid[0], clip, vf_clip,
                                vf_coeff, ent_coeff, kl_coeff, t_pol, t_vf, t_kl, t_ent);
        } else {
            for (int j = 0; j < ld; j++) rn[j] = 0.0f;
        }
        d_vf[row] = gv;
    }

    /* ---- the workgroup's partial sums: shuffle tree per wave, waves in index order */
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        t_pol += __shfl_down(t_pol, off, 64);
        t_vf += __shfl_down(t_vf, off, 64);
        t_kl += __shfl_down(t_kl, off, 64);
        t_ent += __shfl_down(t_ent, off, 64);
    }
    if ((tid & 63) == 0) {
        s_red[tid >> 6][0] = t_pol; s_red[tid >> 6][1] = t_vf; s_red[tid >> 6][2] = t_kl; s_red[tid >> 6][3] = t_ent;
    }
    __syncthreads();   /* also: every lane's gradient row is in s_new */
    if (tid < 4) partial[(int64_t)blockIdx.x * 4 + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];

    /* ---- the gradient tile out, flat order again */
    float *__restrict__ gd = d_logits + row0 * ld;
    for (int e0 = tid * 4; e0 < nf; e0 += HHL_ROWS * 4) {
        float v[4];
        const int cnt = nf - e0 < 4 ? nf - e0 : 4;
        int r = e0 / ld, c = e0 - r * ld;
        for (int k = 0; k < cnt; k++) {
            v[k] = s_new[r * sn + c];
            if (++c == ld) { c = 0; r++; }
        }
        if (cnt == 4) {
            *reinterpret_cast<float4 *>(gd + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int k = 0; k < cnt; k++) gd[e0 + k] = v[k];
        }
    }
}

/* the partials of all workgroups in a fixed order: lane t adds workgroups t, t + 256, ...; then a fixed tree over the 256 lanes.  One
 * workgroup of 256 lanes, all of them in the call (hh_k_ppo_loss_final, and the last workgroup of hh_k_heads_final) */
__device__ __forceinline__ void hhl_final_stats(int n_blocks, const double *__restrict__ partial, const int32_t *__restrict__ n_valid, float vf_coeff,
                                                float ent_coeff, float kl_coeff, double *__restrict__ stats) {
    __shared__ double s[4][256];
    const int tid = threadIdx.x;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < n_blocks; b += 256)
        for (int k = 0; k < 4; k++) a[k] += partial[(int64_t)b * 4 + k];
    for (int k = 0; k < 4; k++) s[k][tid] = a[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
            for (int k = 0; k < 4; k++) s[k][tid] += s[k][tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const double n = (double)n_valid[0];
        const double pol = s[0][0] / n, vfl = s[1][0] / n, kl = s[2][0] / n, ent = s[3][0] / n;
        double total = (s[0][0] + (double)vf_coeff * s[1][0] - (double)ent_coeff * s[3][0]) / n;
        if (kl_coeff > 0.0f) total += (double)kl_coeff * kl;
        stats[0] = total;
        stats[1] = pol;
        stats[2] = vfl;
        stats[3] = kl_coeff > 0.0f ? kl : 0.0;
        stats[4] = ent;
        stats[5] = n;
    }
}

__global__ __launch_bounds__(256) void hh_k_ppo_loss_final(int n_blocks, const double *__restrict__ partial, const int32_t *__restrict__ n_valid,
                                                           float vf_coeff, float ent_coeff, float kl_coeff, double *__restrict__ stats) {
    hhl_final_stats(n_blocks, partial, n_valid, vf_coeff, ent_coeff, kl_coeff, stats);
}

static inline int64_t hhl_blocks(int64_t n_rows) { return (n_rows + HHL_ROWS - 1) / HHL_ROWS; }

extern "C" int hh_ppo_loss_scratch_bytes(int64_t n_rows, int64_t *bytes) {
    if (n_rows <= 0 || n_rows > ((int64_t)1 << 30) || !bytes) { g_err = "hh_ppo_loss_scratch_bytes: bad argument"; return HH_E_ARG; }
    *bytes = hhl_blocks(n_rows) * 4 * (int64_t)sizeof(double);
    return HH_OK;
}

extern "C" int hh_ppo_loss(int64_t n_rows, int32_t ld, const float *logits, const float *old_logits, const int8_t *actions, const float *old_logp,
                           const float *adv, const float *vf, const float *target, const uint8_t *mask, const int32_t *n_valid,
                           const hh_ppo_loss_params *prm, double *stats, float *d_logits, float *d_vf, void *scratch, int64_t scratch_bytes,
                           void *stream) {
    if (n_rows <= 0 || n_rows > ((int64_t)1 << 30) || !logits || !old_logits || !actions || !old_logp || !adv || !vf || !target || !n_valid || !prm ||
        !stats || !d_logits || !d_vf || !scratch) { g_err = "hh_ppo_loss: null or out-of-range argument"; return HH_E_ARG; }
    if ((prm->n_comp != 3 && prm->n_comp != 4) || prm->reserved0 != 0 || prm->reserved1 != 0.0f) {
        g_err = "hh_ppo_loss: n_comp must be 4 ([13, 9, 2, 2]) or 3 ([13, 9, 2]) and the reserved fields 0"; return HH_E_ARG;
    }
    const int n_out = prm->n_comp == 4 ? 26 : 24;
    if (ld < n_out || ld > 32) { g_err = "hh_ppo_loss: ld must be between the policy's logits (26 | 24) and 32"; return HH_E_ARG; }
    if ((reinterpret_cast<uintptr_t>(logits) & 15) || (reinterpret_cast<uintptr_t>(old_logits) & 15) || (reinterpret_cast<uintptr_t>(d_logits) & 15) ||
        (reinterpret_cast<uintptr_t>(actions) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(stats) & 7)) {
        g_err = "hh_ppo_loss: logits / old_logits / d_logits must be 16-byte aligned, actions 4-byte, scratch / stats 8-byte"; return HH_E_ARG;
    }
    const int64_t nb = hhl_blocks(n_rows);
    if (scratch_bytes < nb * 4 * (int64_t)sizeof(double)) { g_err = "hh_ppo_loss: scratch is smaller than hh_ppo_loss_scratch_bytes(n_rows)"; return HH_E_ARG; }
    hipStream_t st = (hipStream_t)stream;
    double *partial = static_cast<double *>(scratch);
    const int32_t *aw = reinterpret_cast<const int32_t *>(actions);
    if (prm->n_comp == 4)
        hipLaunchKernelGGL(hh_k_ppo_loss<4>, dim3((unsigned)nb), dim3(HHL_ROWS), 0, st, n_rows, ld, logits, old_logits, aw, old_logp, adv, vf, target, mask,
                           n_valid, prm->clip_param, prm->vf_clip_param, prm->vf_loss_coeff, prm->entropy_coeff, prm->kl_coeff, partial, d_logits, d_vf);
    else
        hipLaunchKernelGGL(hh_k_ppo_loss<3>, dim3((unsigned)nb), dim3(HHL_ROWS), 0, st, n_rows, ld, logits, old_logits, aw, old_logp, adv, vf, target, mask,
                           n_valid, prm->clip_param, prm->vf_clip_param, prm->vf_loss_coeff, prm->entropy_coeff, prm->kl_coeff, partial, d_logits, d_vf);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_ppo_loss_final, dim3(1), dim3(256), 0, st, (int)nb, partial, n_valid, prm->vf_loss_coeff, prm->entropy_coeff, prm->kl_coeff, stats);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_ppo_loss_categorical(int64_t n_rows, const float *logits, const float *old_logits, const int8_t *actions, const float *old_logp,
                                       const float *adv, const float *vf, const float *target, const uint8_t *mask, const int32_t *n_valid,
                                       const hh_ppo_loss_params *prm, double *stats, float *d_logits, float *d_vf, void *scratch,
                                       int64_t scratch_bytes, void *stream) {
    if (n_rows <= 0 || n_rows > ((int64_t)1 << 30) || !logits || !old_logits || !actions || !old_logp || !adv || !vf || !target || !n_valid || !prm ||
        !stats || !d_logits || !d_vf || !scratch) { g_err = "hh_ppo_loss_categorical: null or out-of-range argument"; return HH_E_ARG; }
    if (prm->n_comp != 1 || prm->reserved0 != 0 || prm->reserved1 != 0.0f) {
        g_err = "hh_ppo_loss_categorical: n_comp must be 1 (one Categorical over 3 logits) and the reserved fields 0"; return HH_E_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(logits) & 15) || (reinterpret_cast<uintptr_t>(old_logits) & 15) || (reinterpret_cast<uintptr_t>(d_logits) & 15) ||
        (reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(stats) & 7)) {
        g_err = "hh_ppo_loss_categorical: logits / old_logits / d_logits must be 16-byte aligned, scratch / stats 8-byte"; return HH_E_ARG;
    }
    const int64_t nb = hhl_blocks(n_rows);
    if (scratch_bytes < nb * 4 * (int64_t)sizeof(double)) { g_err = "hh_ppo_loss_categorical: scratch is smaller than hh_ppo_loss_scratch_bytes(n_rows)"; return HH_E_ARG; }
    hipStream_t st = (hipStream_t)stream;
    double *partial = static_cast<double *>(scratch);
    hipLaunchKernelGGL(hh_k_ppo_loss<1>, dim3((unsigned)nb), dim3(HHL_ROWS), 0, st, n_rows, (int)HH_CMD_LOGITS, logits, old_logits,
                       reinterpret_cast<const int32_t *>(actions), old_logp, adv, vf, target, mask, n_valid, prm->clip_param, prm->vf_clip_param,
                       prm->vf_loss_coeff, prm->entropy_coeff, prm->kl_coeff, partial, d_logits, d_vf);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_ppo_loss_final, dim3(1), dim3(256), 0, st, (int)nb, partial, n_valid, prm->vf_loss_coeff, prm->entropy_coeff, prm->kl_coeff, stats);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

#endif /* HH_PPO_LOSS_H */
