/*
 * hh_heads_loss.h — everything between shared_layer's GEMM and the gradient that flows back into it, for the learners
 * (learner.heads_loss; C ABI: include/hh_learner.h): tanh, the two output heads (act_out: 500 -> 26 | 24 | 3, val_out: 500 -> 1), the PPO
 * loss of hh_ppo_loss.h, the heads' backward and tanh's backward in ONE row pass, and the head weights' gradients from per-workgroup
 * partial sums that a second launch adds in a fixed order.  The loss formulas and kink conventions are hh_ppo_loss.h's own device
 * functions (hhl_component, hhl_row, hhl_final_stats), not a copy.
 *
 * Layout.  A workgroup of 256 lanes keeps W = [w_act ; w_val] (NH = n_out + 1 rows of 500 floats, 54 KB at n_out = 26) in LDS for its whole
 * life and walks the row tiles (HHH_TILE = 16 rows) grid-stride, min(tiles, HHH_MAX_WG) workgroups.  Per tile:
 *   in        za, zc rows -> h = tanhf(za), y = tanhf(zc) into LDS (float4 loads in flat order; 2 x 32 KB), the sampler's logits beside them
 *   forward   lane (row r = t & 15, k slice q = t >> 4) takes the float4 groups g = q, q + 16, ... of k: one h / y read and NH weight
 *             reads (the 16 lanes of a slice read the same weights: LDS broadcast) per 4 NH fmaf; the 16 slices' partial dot products go
 *             through LDS and are added in slice order, then the bias
 *   loss      lane r < 16 runs hhl_row on its LDS row, as hh_k_ppo_loss does: d_logits replaces the logits in LDS, d_vf beside it
 *   backward  item (r, g): d_za = (sum_j d_logits[r][j] W[j][k]) (1 - h^2), d_zc = d_vf[r] w_val[k] (1 - y^2), float4 stores in flat order
 *   weights   item (j, g), 14 per lane at n_out = 26, held in registers over ALL the workgroup's tiles: += d[r][j] h[r][k] (j < n_out) or
 *             d_vf[r] y[r][k], rows in order; the NH bias sums in float64, one lane each
 * h and y never leave the chip; a row costs its 8 KB (za, zc in, d_za, d_zc out) and 110 B of batch columns.  LDS: 149.4 KB at n_out = 26
 * (one workgroup per CU), 141.2 KB at 24, 73.0 KB at 3.
 *
 * Masked rows (mask == 0, rows past the end of the last tile, and every row when n_valid <= 0) are skipped by branches on a flag in LDS:
 * their loss terms are not computed, their d_za / d_zc are stored as 0.0f, and the weight sums step over them, so a NaN in such a row
 * reaches nothing.
 *
 * Reduction order (it depends on n_rows and n_comp only): a workgroup adds its tiles in walk order and the rows of a tile in row
 * order, float32 fmaf for d_w, float64 for d_b and for the four loss sums (lane r's rows over the tiles, then a shuffle tree over wave
 * 0); hh_k_heads_final adds the workgroups' slots of every element in slot order in float64 and rounds once, and its last workgroup
 * is hhl_final_stats over the loss partials.  No atomics.
 *
 * Code object (tools/kernel_meta.sh, gfx950): hh_k_heads_loss<4> 225 VGPR, <3> 222, <1> 167 (the 56 weight-gradient accumulators and the
 * forward's 27 live across the tile loop; with 149 KB of LDS a CU holds one workgroup, one wave per SIMD, so the count costs no
 * occupancy), 30 / 26 / 0 SGPRs spilled to VGPR lanes; hh_k_heads_final<4 | 3 | 1> 24 VGPR.  No scratch memory in any of them.
 */
#ifndef HH_HEADS_LOSS_H
#define HH_HEADS_LOSS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hh_learner.h"
#include "hh_ppo_loss.h"

#define HHH_THREADS 256
#define HHH_TILE 16                          /* rows per tile */
#define HHH_K 500                            /* shared_layer's width */
#define HHH_K4 (HHH_K / 4)
#define HHH_SLICES (HHH_THREADS / HHH_TILE)  /* k slices of the forward */
#define HHH_MAX_WG 256                       /* workgroups: beyond this many tiles they walk grid-stride */

static_assert(HHH_K % 4 == 0 && HHH_SLICES * HHH_TILE == HHH_THREADS, "float4 groups of k; one forward lane per (row, slice)");

template <int NCOMP>
struct hhh_dims {
    static constexpr int NOUT = NCOMP == 4 ? 26 : (NCOMP == 3 ? 24 : HH_CMD_ACTIONS);
    static constexpr int NH = NOUT + 1;                        /* heads: the logits, then the value */
    static constexpr int SN = NOUT | 1;                        /* LDS row stride of the logits: odd, as in hh_k_ppo_loss */
    static constexpr int PS = NH | 1;                          /* LDS row stride of a (slice, row)'s partial dot products */
    static constexpr int OLD_LD = NCOMP == 1 ? HH_CMD_LOGITS : HHL_OLD_LD;
    static constexpr int NW = NH * HHH_K;                      /* elements of [d_w_act ; d_w_val] */
    static constexpr int NACC = (NH * HHH_K4 + HHH_THREADS - 1) / HHH_THREADS;   /* float4 weight-gradient items per lane */
    /* floats of LDS: W, h, y (float4-aligned), partials, logits, old logits, vf | d_vf | flags, bias */
    static constexpr int LDS_FLOATS = NW + 2 * HHH_TILE * HHH_K + HHH_THREADS * PS + HHH_TILE * SN + HHH_TILE * HHL_OLD_STRIDE + 3 * HHH_TILE + NH;
    static constexpr int LDS_BYTES = (LDS_FLOATS * 4 + 15) & ~15;
};

struct hhh_args {
    int64_t R;
    int32_t n_tiles;
    const float *za, *zc, *w_act, *b_act, *w_val, *b_val, *old_logits;
    const int32_t *actions;
    const float *old_logp, *adv, *target;
    const uint8_t *mask;
    const int32_t *n_valid;
    float clip, vf_clip, vf_coeff, ent_coeff, kl_coeff;
    float *d_za, *d_zc, *logits, *vf;
    double *part_s, *part_b;   /* [n_wg][4] loss sums, [n_wg][NH] bias sums */
    float *part_w;             /* [n_wg][NH * 500] */
};

__device__ __forceinline__ float4 hhh_fma4(float d, float4 x, float4 a) {
    return make_float4(fmaf(d, x.x, a.x), fmaf(d, x.y, a.y), fmaf(d, x.z, a.z), fmaf(d, x.w, a.w));
}

template <int NCOMP>
__global__ __launch_bounds__(HHH_THREADS) void hh_k_heads_loss(hhh_args a) {
    using D = hhh_dims<NCOMP>;
    constexpr int NOUT = D::NOUT, NH = D::NH, SN = D::SN, PS = D::PS, OLD_LD = D::OLD_LD, NACC = D::NACC;
    extern __shared__ float4 hhh_lds[];
    float *s_w = reinterpret_cast<float *>(hhh_lds);        /* [NH][500] */
    float *s_h = s_w + D::NW;                               /* [16][500] */
    float *s_y = s_h + HHH_TILE * HHH_K;                    /* [16][500] */
    float *s_part = s_y + HHH_TILE * HHH_K;                 /* [16 slices][16 rows][PS] */
    float *s_new = s_part + HHH_THREADS * PS;               /* [16][SN]: logits, then d_logits */
    float *s_old = s_new + HHH_TILE * SN;                   /* [16][27] */
    float *s_vf = s_old + HHH_TILE * HHL_OLD_STRIDE;        /* [16] */
    float *s_dvf = s_vf + HHH_TILE;                         /* [16] */
    int *s_on = reinterpret_cast<int *>(s_dvf + HHH_TILE);  /* [16] */
    float *s_bias = s_dvf + 2 * HHH_TILE;                   /* [NH] */
    const float4 *s_w4 = reinterpret_cast<const float4 *>(s_w);
    float4 *s_h4 = reinterpret_cast<float4 *>(s_h), *s_y4 = reinterpret_cast<float4 *>(s_y);
    const int tid = threadIdx.x;

    /* ---- the heads' weights, once per workgroup (4-byte loads: the ABI asks no alignment of them) */
    for (int e = tid; e < NOUT * HHH_K; e += HHH_THREADS) s_w[e] = a.w_act[e];
    for (int e = tid; e < HHH_K; e += HHH_THREADS) s_w[NOUT * HHH_K + e] = a.w_val[e];
    if (tid < NOUT) s_bias[tid] = a.b_act[tid];
    if (tid == NOUT) s_bias[NOUT] = a.b_val[0];
    const bool any = a.n_valid[0] > 0;
    const float inv_n = 1.0f / (float)a.n_valid[0];

    float4 accw[NACC];
#pragma unroll
    for (int ii = 0; ii < NACC; ii++) accw[ii] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    double accb = 0.0;
    double t_pol = 0.0, t_vf = 0.0, t_kl = 0.0, t_ent = 0.0;

    for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const int64_t row0 = (int64_t)t * HHH_TILE;
        const int rows = (int)((a.R - row0) < HHH_TILE ? (a.R - row0) : HHH_TILE);   /* >= 1 */
        /* ---- the tile in: h and y, rows past the end as zeros */
        {
            const float4 *__restrict__ ga = reinterpret_cast<const float4 *>(a.za) + row0 * HHH_K4;
            const float4 *__restrict__ gc = reinterpret_cast<const float4 *>(a.zc) + row0 * HHH_K4;
            const int nf4 = rows * HHH_K4;
            for (int e = tid; e < HHH_TILE * HHH_K4; e += HHH_THREADS) {
                float4 u = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = u;
                if (e < nf4) {
                    u = ga[e];
                    v = gc[e];
                    u = make_float4(tanhf(u.x), tanhf(u.y), tanhf(u.z), tanhf(u.w));
                    v = make_float4(tanhf(v.x), tanhf(v.y), tanhf(v.z), tanhf(v.w));
                }
                s_h4[e] = u;
                s_y4[e] = v;
            }
            const float *__restrict__ go = a.old_logits + row0 * OLD_LD;
            for (int e = tid; e < rows * OLD_LD; e += HHH_THREADS) {
                const int r = e / OLD_LD, c = e % OLD_LD;
                if (c < NOUT) s_old[r * HHL_OLD_STRIDE + c] = go[e];
            }
            if (tid < HHH_TILE) s_on[tid] = (any && tid < rows && (a.mask == nullptr || a.mask[row0 + tid] != 0)) ? 1 : 0;
        }
        __syncthreads();

        /* ---- forward: lane (row, slice), the slice's share of every head's dot product */
        {
            const int r = tid & (HHH_TILE - 1), q = tid / HHH_TILE;
            float acc[NH];
#pragma unroll
            for (int j = 0; j < NH; j++) acc[j] = 0.0f;
            for (int g = q; g < HHH_K4; g += HHH_SLICES) {
                const float4 h = s_h4[r * HHH_K4 + g], y = s_y4[r * HHH_K4 + g];
#pragma unroll
                for (int j = 0; j < NH; j++) {
                    const float4 w = s_w4[j * HHH_K4 + g];
                    const float4 x = j < NOUT ? h : y;
                    acc[j] = fmaf(x.w, w.w, fmaf(x.z, w.z, fmaf(x.y, w.y, fmaf(x.x, w.x, acc[j]))));
                }
            }
#pragma unroll
            for (int j = 0; j < NH; j++) s_part[(q * HHH_TILE + r) * PS + j] = acc[j];
        }
        __syncthreads();
        /* the slices in order, then the bias; masked rows are written as 0.0f to the optional outputs */
        for (int p = tid; p < HHH_TILE * NH; p += HHH_THREADS) {
            const int r = p / NH, j = p - r * NH;
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < HHH_SLICES; q++) s += s_part[(q * HHH_TILE + r) * PS + j];
            s += s_bias[j];
            const bool on = s_on[r] != 0;
            if (j < NOUT) {
                s_new[r * SN + j] = s;
                if (a.logits && r < rows) a.logits[(row0 + r) * NOUT + j] = on ? s : 0.0f;
            } else {
                s_vf[r] = s;
                if (a.vf && r < rows) a.vf[row0 + r] = on ? s : 0.0f;
            }
        }
        __syncthreads();

        /* ---- the loss: lane r, row r (hh_ppo_loss.h's row code) */
        if (tid < HHH_TILE) {
            float *rn = s_new + tid * SN;
            float gv = 0.0f;
            if (s_on[tid]) {
                const int64_t row = row0 + tid;
                double r_pol, r_vf, r_kl, r_ent;
                gv = hhl_row<NCOMP>(rn, s_old + tid * HHL_OLD_STRIDE, NOUT, row, a.actions, a.old_logp[row], a.adv[row], s_vf[tid], a.target[row], inv_n,
                                    a.clip, a.vf_clip, a.vf_coeff, a.ent_coeff, a.kl_coeff, r_pol, r_vf, r_kl, r_ent);
                t_pol += r_pol; t_vf += r_vf; t_kl += r_kl; t_ent += r_ent;
            } else {
#pragma unroll
                for (int j = 0; j < NOUT; j++) rn[j] = 0.0f;
            }
            s_dvf[tid] = gv;
        }
        __syncthreads();

        /* ---- backward through the heads and tanh: item (row, float4 group of k), flat order out */
        {
            float4 *__restrict__ da = reinterpret_cast<float4 *>(a.d_za) + row0 * HHH_K4;
            float4 *__restrict__ dc = reinterpret_cast<float4 *>(a.d_zc) + row0 * HHH_K4;
            for (int e = tid; e < rows * HHH_K4; e += HHH_THREADS) {
                const int r = e / HHH_K4, g = e - r * HHH_K4;
                float4 u = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = u;
                if (s_on[r]) {
#pragma unroll
                    for (int j = 0; j < NOUT; j++) u = hhh_fma4(s_new[r * SN + j], s_w4[j * HHH_K4 + g], u);
                    const float4 h = s_h4[e], y = s_y4[e], wv = s_w4[NOUT * HHH_K4 + g];
                    const float dv = s_dvf[r];
                    u = make_float4(u.x * (1.0f - h.x * h.x), u.y * (1.0f - h.y * h.y), u.z * (1.0f - h.z * h.z), u.w * (1.0f - h.w * h.w));
                    v = make_float4((dv * wv.x) * (1.0f - y.x * y.x), (dv * wv.y) * (1.0f - y.y * y.y), (dv * wv.z) * (1.0f - y.z * y.z),
                                    (dv * wv.w) * (1.0f - y.w * y.w));
                }
                da[e] = u;
                dc[e] = v;
            }
        }
        /* ---- the head weights' gradients: this tile's rows onto the lane's items, rows in order and by selection */
        for (int r = 0; r < HHH_TILE; r++) {
            if (!s_on[r]) continue;
#pragma unroll
            for (int ii = 0; ii < NACC; ii++) {
                const int i = tid + ii * HHH_THREADS;
                if (i < NH * HHH_K4) {
                    const int j = i / HHH_K4, g = i - j * HHH_K4;
                    const float d = j < NOUT ? s_new[r * SN + j] : s_dvf[r];
                    const float4 x = j < NOUT ? s_h4[r * HHH_K4 + g] : s_y4[r * HHH_K4 + g];
                    accw[ii] = hhh_fma4(d, x, accw[ii]);
                }
            }
            if (tid < NH) accb += (double)(tid < NOUT ? s_new[r * SN + tid] : s_dvf[r]);
        }
        __syncthreads();   /* the next tile overwrites h, y and the rows */
    }

    /* ---- the workgroup's slots */
    float *__restrict__ pw = a.part_w + (int64_t)blockIdx.x * D::NW;
#pragma unroll
    for (int ii = 0; ii < NACC; ii++) {
        const int i = tid + ii * HHH_THREADS;
        if (i < NH * HHH_K4) {
            pw[i * 4 + 0] = accw[ii].x; pw[i * 4 + 1] = accw[ii].y; pw[i * 4 + 2] = accw[ii].z; pw[i * 4 + 3] = accw[ii].w;
        }
    }
    if (tid < NH) a.part_b[(int64_t)blockIdx.x * NH + tid] = accb;
    if (tid < 64) {   /* lanes 16 .. 63 of wave 0 hold zeros */
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            t_pol += __shfl_down(t_pol, off, 64);
            t_vf += __shfl_down(t_vf, off, 64);
            t_kl += __shfl_down(t_kl, off, 64);
            t_ent += __shfl_down(t_ent, off, 64);
        }
        if (tid == 0) {
            double *ps = a.part_s + (int64_t)blockIdx.x * 4;
            ps[0] = t_pol; ps[1] = t_vf; ps[2] = t_kl; ps[3] = t_ent;
        }
    }
}

/* every element of d_w_act | d_w_val | d_b_act | d_b_val: the workgroups' slots in slot order, float64, rounded once; the last workgroup
 * adds the loss partials (hhl_final_stats) */
template <int NCOMP>
__global__ __launch_bounds__(256) void hh_k_heads_final(int n_wg, const double *__restrict__ part_s, const double *__restrict__ part_b,
                                                        const float *__restrict__ part_w, const int32_t *__restrict__ n_valid, float vf_coeff,
                                                        float ent_coeff, float kl_coeff, double *__restrict__ stats, float *__restrict__ d_w_act,
                                                        float *__restrict__ d_b_act, float *__restrict__ d_w_val, float *__restrict__ d_b_val) {
    using D = hhh_dims<NCOMP>;
    if (blockIdx.x == gridDim.x - 1) {
        hhl_final_stats(n_wg, part_s, n_valid, vf_coeff, ent_coeff, kl_coeff, stats);
        return;
    }
    const int e = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (e < D::NW) {
        for (int p = 0; p < n_wg; p++) s += (double)part_w[(int64_t)p * D::NW + e];
        if (e < D::NOUT * HHH_K) d_w_act[e] = (float)s;
        else d_w_val[e - D::NOUT * HHH_K] = (float)s;
    } else if (e < D::NW + D::NH) {
        const int j = e - D::NW;
        for (int p = 0; p < n_wg; p++) s += part_b[(int64_t)p * D::NH + j];
        if (j < D::NOUT) d_b_act[j] = (float)s;
        else d_b_val[0] = (float)s;
    }
}

static inline int hhh_n_out(int n_comp) { return n_comp == 4 ? 26 : (n_comp == 3 ? 24 : (n_comp == 1 ? HH_CMD_ACTIONS : 0)); }
static inline int64_t hhh_tiles(int64_t n_rows) { return (n_rows + HHH_TILE - 1) / HHH_TILE; }
static inline int64_t hhh_wgs(int64_t n_rows) { const int64_t t = hhh_tiles(n_rows); return t < HHH_MAX_WG ? t : HHH_MAX_WG; }
/* the doubles (loss sums, then bias sums) lie in front of the float slots */
static inline int64_t hhh_scratch_doubles(int64_t n_wg, int nh) { return n_wg * (4 + nh); }

extern "C" int hh_heads_loss_geometry(int64_t n_rows, int32_t n_comp, int32_t *tile_rows, int32_t *n_workgroups) {
    if (n_rows < 1 || n_rows > ((int64_t)1 << 30) || !hhh_n_out(n_comp) || !tile_rows || !n_workgroups) {
        g_err = "hh_heads_loss_geometry: bad argument"; return HH_E_ARG;
    }
    *tile_rows = HHH_TILE;
    *n_workgroups = (int32_t)hhh_wgs(n_rows);
    return HH_OK;
}

extern "C" int hh_heads_loss_scratch_bytes(int64_t n_rows, int32_t n_comp, int64_t *bytes) {
    if (n_rows < 1 || n_rows > ((int64_t)1 << 30) || !hhh_n_out(n_comp) || !bytes) { g_err = "hh_heads_loss_scratch_bytes: bad argument"; return HH_E_ARG; }
    const int nh = hhh_n_out(n_comp) + 1;
    const int64_t n_wg = hhh_wgs(n_rows);
    *bytes = hhh_scratch_doubles(n_wg, nh) * 8 + n_wg * nh * HHH_K * 4;
    return HH_OK;
}

template <int NCOMP>
static int hhh_launch(const hhh_args &a, int n_wg, const hh_ppo_loss_params *prm, double *stats, float *d_w_act, float *d_b_act, float *d_w_val,
                      float *d_b_val, hipStream_t st) {
    using D = hhh_dims<NCOMP>;
    static_assert(D::LDS_BYTES <= 160 * 1024, "one workgroup's LDS");
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(hh_k_heads_loss<NCOMP>), hipFuncAttributeMaxDynamicSharedMemorySize, D::LDS_BYTES));
    hipLaunchKernelGGL(hh_k_heads_loss<NCOMP>, dim3((unsigned)n_wg), dim3(HHH_THREADS), D::LDS_BYTES, st, a);
    HIPCHK(hipGetLastError());
    const int blocks = (D::NW + D::NH + 255) / 256 + 1;
    hipLaunchKernelGGL(hh_k_heads_final<NCOMP>, dim3((unsigned)blocks), dim3(256), 0, st, n_wg, a.part_s, a.part_b, a.part_w, a.n_valid, prm->vf_loss_coeff,
                       prm->entropy_coeff, prm->kl_coeff, stats, d_w_act, d_b_act, d_w_val, d_b_val);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_heads_loss(int64_t n_rows, const float *za, const float *zc, const float *w_act, const float *b_act, const float *w_val,
                             const float *b_val, const float *old_logits, const int8_t *actions, const float *old_logp, const float *adv,
                             const float *target, const uint8_t *mask, const int32_t *n_valid, const hh_ppo_loss_params *prm, double *stats,
                             float *d_za, float *d_zc, float *d_w_act, float *d_b_act, float *d_w_val, float *d_b_val, float *logits, float *vf,
                             void *scratch, int64_t scratch_bytes, void *stream) {
    if (n_rows < 1 || n_rows > ((int64_t)1 << 30) || !za || !zc || !w_act || !b_act || !w_val || !b_val || !old_logits || !actions || !old_logp || !adv ||
        !target || !n_valid || !prm || !stats || !d_za || !d_zc || !d_w_act || !d_b_act || !d_w_val || !d_b_val || !scratch) {
        g_err = "hh_heads_loss: null or out-of-range argument"; return HH_E_ARG;
    }
    const int n_out = hhh_n_out(prm->n_comp);
    if (!n_out || prm->reserved0 != 0 || prm->reserved1 != 0.0f) {
        g_err = "hh_heads_loss: n_comp must be 4 ([13, 9, 2, 2]), 3 ([13, 9, 2]) or 1 (the commander's Categorical) and the reserved fields 0"; return HH_E_ARG;
    }
    auto off = [](const void *p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    if (off(za, 15) || off(zc, 15) || off(d_za, 15) || off(d_zc, 15) || off(scratch, 7) || off(stats, 7) || off(old_logits, 3) ||
        (prm->n_comp != 1 && off(actions, 3))) {
        g_err = "hh_heads_loss: za / zc / d_za / d_zc must be 16-byte aligned, scratch / stats 8-byte, actions (n_comp 4 | 3) 4-byte"; return HH_E_ARG;
    }
    const int64_t n_wg = hhh_wgs(n_rows);
    const int nh = n_out + 1;
    if (scratch_bytes < hhh_scratch_doubles(n_wg, nh) * 8 + n_wg * nh * HHH_K * 4) {
        g_err = "hh_heads_loss: scratch is smaller than hh_heads_loss_scratch_bytes(n_rows, n_comp)"; return HH_E_ARG;
    }
    hhh_args a;
    a.R = n_rows; a.n_tiles = (int32_t)hhh_tiles(n_rows);
    a.za = za; a.zc = zc; a.w_act = w_act; a.b_act = b_act; a.w_val = w_val; a.b_val = b_val; a.old_logits = old_logits;
    a.actions = reinterpret_cast<const int32_t *>(actions);
    a.old_logp = old_logp; a.adv = adv; a.target = target; a.mask = mask; a.n_valid = n_valid;
    a.clip = prm->clip_param; a.vf_clip = prm->vf_clip_param; a.vf_coeff = prm->vf_loss_coeff; a.ent_coeff = prm->entropy_coeff; a.kl_coeff = prm->kl_coeff;
    a.d_za = d_za; a.d_zc = d_zc; a.logits = logits; a.vf = vf;
    a.part_s = static_cast<double *>(scratch);
    a.part_b = a.part_s + n_wg * 4;
    a.part_w = reinterpret_cast<float *>(a.part_s + hhh_scratch_doubles(n_wg, nh));
    hipStream_t st = (hipStream_t)stream;
    if (prm->n_comp == 4) return hhh_launch<4>(a, (int)n_wg, prm, stats, d_w_act, d_b_act, d_w_val, d_b_val, st);
    if (prm->n_comp == 3) return hhh_launch<3>(a, (int)n_wg, prm, stats, d_w_act, d_b_act, d_w_val, d_b_val, st);
    return hhh_launch<1>(a, (int)n_wg, prm, stats, d_w_act, d_b_act, d_w_val, d_b_val, st);
}

#endif /* HH_HEADS_LOSS_H */
