/*
 * hh_gru_seq.h — the learner's GRU over whole sequences, forward and backward, one launch each for up to two GRUs (rnn_act and rnn_val
 * of CommanderGru) over all L <= 32 steps (C ABI and the arithmetic: include/hh_learner.h).
 *
 * Shape.  A workgroup of 256 lanes owns a tile of TILE sequences of one GRU for all steps (blockIdx.x = tile, blockIdx.y = GRU); TILE is
 * a template parameter, instantiated at 16, 8 and 4 (hhg_pick_tile chooses).  Lane j < 200 owns hidden unit j of
 * all TILE sequences: its h (forward) or its dh carry (backward) lives in registers for the whole launch, and the three gates of a unit
 * meet in one lane, so the gate arithmetic needs no exchange.  The h tile (forward) or the d_gh tile (backward) is kept in LDS unit-major
 * ([unit][TILE]), so the contraction reads it as TILE / 4 16-byte broadcasts per k.  A sequence's arithmetic is its own fmaf chain in k
 * order whatever the tile, and the save buffer is indexed by sequence, so every instance writes the same bytes.
 *
 * Arithmetic: plain float32 fmaf chains in k order, one per output (no split-fp16 MFMA: see DESIGN.md — the result is what a float32
 * GEMM gives, and the test's bound, 4 x the error of the float32 torch-op cell, is met with room instead of depending on a dropped
 * lo x lo term).  exp / tanh are the device library's.
 *
 * Weights.  The forward contraction gh[s, c] = sum_k h[s, k] W_hh[c, k] wants W_hh k-major so that the 200 lanes of a k read consecutive
 * floats: hh_k_gru_pack transposes W_hh [600, 200] into the head of the scratch buffer ([200, 600] per GRU) — the weights change with every
 * minibatch step, so this runs in front of every forward (480 KB per GRU, L2 resident afterwards).  The backward contraction
 * dh[s, k] = sum_c d_gh[s, c] W_hh[c, k] reads W_hh as nn.GRU holds it.  Either way a lane streams its weights from L2 eight k (or c)
 * ahead of the fmaf chain that uses them; a tile of 16 instead of the sampler's 32 halves the accumulators (48 per lane) so that two
 * workgroups fit a CU and twice as many CUs are busy at the learner's sizes (13 sequences at 256 rows, ~820 at 16384).  The narrow
 * instances (8, 4) shorten the per-k chain further (24, 12 accumulators forward) and hand a small minibatch to more workgroups.
 *
 * Tail padding: a tile runs to the longest of its sequences; steps t >= seq_len[s] write exact zeros and leave the sequence's state alone
 * (backward: such a step loads row 0 of dy, of the save buffer and of h0 in place of its own and drops what it loaded, so nothing past
 * seq_len reaches a result).  A sequence of length 0 is all tail: exact zeros in y, d_gi, d_gh and d_h0, its h0 never read, and a tile
 * made of such sequences only runs no step at all.  Row 0 is what ended sequences read, so sequence 0 has at least one step (the contract
 * in hh_learner.h).  Fixed summation order, no atomics: the same bytes on every run.
 */
#ifndef HH_GRU_SEQ_H
#define HH_GRU_SEQ_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hh_learner.h"

#define HHG_H HH_GRU_HIDDEN      /* 200 */
#define HHG_G3 (3 * HH_GRU_HIDDEN) /* 600 gate rows r | z | n */
#define HHG_TILE_WIDE 16         /* sequences per workgroup: the widest instance (8 and 4 are the narrow ones) */
#define HHG_THREADS 256
#define HHG_KB 8                 /* weights in flight per lane and gate */
#define HHG_SAVE 4               /* floats kept per (sequence, step, unit): r, z, n, W_hn h + b_hn */

struct hhg_dev_io {
    const float *gi[2], *h0[2], *w[2], *b_hh[2], *dy[2];
    float *y[2], *d_gi[2], *d_gh[2], *d_h0[2];
};

static inline int64_t hhg_pack_floats(int G) { return (int64_t)G * HHG_G3 * HHG_H; }

/* W_hh [600, 200] -> [200, 600], per GRU (blockIdx.z) */
__global__ __launch_bounds__(256) void hh_k_gru_pack(hhg_dev_io io, float *__restrict__ wt) {
    __shared__ float tile[32][33];
    const int g = blockIdx.z;
    const float *__restrict__ w = io.w[g];
    float *__restrict__ o = wt + (int64_t)g * HHG_G3 * HHG_H;
    const int k0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, k = k0 + tx;
        tile[i][tx] = (c < HHG_G3 && k < HHG_H) ? w[c * HHG_H + k] : 0.0f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int k = k0 + i, c = c0 + tx;
        if (k < HHG_H && c < HHG_G3) o[k * HHG_G3 + c] = tile[tx][i];
    }
}

__device__ __forceinline__ float hhg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int TILE>
__global__ __launch_bounds__(HHG_THREADS) void hh_k_gru_seq_fwd(hhg_dev_io io, int64_t S, int L, const int32_t *__restrict__ seq_len,
                                                                const float *__restrict__ wt_all, float *__restrict__ save_all) {
    static_assert(TILE == 4 || TILE == 8 || TILE == 16, "a tile is whole float4s of sequences");
    __shared__ float4 s_h[HHG_H][TILE / 4];
    __shared__ int s_len[TILE];
    const int g = blockIdx.y, j = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * TILE;
    const float *__restrict__ gi = io.gi[g];
    const float *__restrict__ wt = wt_all + (int64_t)g * HHG_G3 * HHG_H;
    float *__restrict__ y = io.y[g];
    float *__restrict__ save = save_all + (int64_t)g * S * L * (HHG_SAVE * HHG_H);
    if (j < TILE) {
        int n = s0 + j < S ? seq_len[s0 + j] : 0;
        s_len[j] = n < 0 ? 0 : (n > L ? L : n);     /* the entry point documents 0..L; a stray value cannot take a lane out of bounds */
    }
    __syncthreads();
    int len[TILE], t_max = 0;
#pragma unroll
    for (int s = 0; s < TILE; s++) {
        len[s] = s_len[s];
        t_max = len[s] > t_max ? len[s] : t_max;
    }
    const bool unit = j < HHG_H;
    float h[TILE];
    float br = 0.0f, bz = 0.0f, bn = 0.0f;
    if (unit) {
        br = io.b_hh[g][j]; bz = io.b_hh[g][HHG_H + j]; bn = io.b_hh[g][2 * HHG_H + j];
#pragma unroll
        for (int s = 0; s < TILE; s++) h[s] = len[s] > 0 ? io.h0[g][(s0 + s) * HHG_H + j] : 0.0f;
#pragma unroll
        for (int q = 0; q < TILE / 4; q++) s_h[j][q] = make_float4(h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]);
    }
    __syncthreads();

    for (int t = 0; t < t_max; t++) {
        if (unit) {
            /* this step's gi, in flight under the contraction (a sequence that has ended reads row 0 of the tensor and drops it) */
            float xr[TILE], xz[TILE], xn[TILE];
#pragma unroll
            for (int s = 0; s < TILE; s++) {
                const int64_t row = t < len[s] ? (s0 + s) * L + t : 0;
                const float *gp = gi + row * HHG_G3 + j;
                xr[s] = gp[0]; xz[s] = gp[HHG_H]; xn[s] = gp[2 * HHG_H];
            }
            float ar[TILE], az[TILE], an[TILE];
#pragma unroll
            for (int s = 0; s < TILE; s++) { ar[s] = br; az[s] = bz; an[s] = bn; }
            float wr[HHG_KB], wz[HHG_KB], wn[HHG_KB];
#pragma unroll
            for (int u = 0; u < HHG_KB; u++) {
                wr[u] = wt[u * HHG_G3 + j]; wz[u] = wt[u * HHG_G3 + HHG_H + j]; wn[u] = wt[u * HHG_G3 + 2 * HHG_H + j];
            }
            for (int k0 = 0; k0 < HHG_H; k0 += HHG_KB) {       /* 200 = 25 x 8 */
                float cr[HHG_KB], cz[HHG_KB], cn[HHG_KB];
#pragma unroll
                for (int u = 0; u < HHG_KB; u++) { cr[u] = wr[u]; cz[u] = wz[u]; cn[u] = wn[u]; }
                if (k0 + HHG_KB < HHG_H) {
#pragma unroll
                    for (int u = 0; u < HHG_KB; u++) {
                        const float *p = wt + (k0 + HHG_KB + u) * HHG_G3 + j;
                        wr[u] = p[0]; wz[u] = p[HHG_H]; wn[u] = p[2 * HHG_H];
                    }
                }
#pragma unroll
                for (int u = 0; u < HHG_KB; u++) {
#pragma unroll
                    for (int q = 0; q < TILE / 4; q++) {
                        const float4 hv = s_h[k0 + u][q];
                        const float hk[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            ar[4 * q + i] = fmaf(cr[u], hk[i], ar[4 * q + i]);
                            az[4 * q + i] = fmaf(cz[u], hk[i], az[4 * q + i]);
                            an[4 * q + i] = fmaf(cn[u], hk[i], an[4 * q + i]);
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < TILE; s++) {
                if (t < len[s]) {
                    const int64_t row = (s0 + s) * L + t;
                    const float r = hhg_sigmoid(xr[s] + ar[s]);
                    const float z = hhg_sigmoid(xz[s] + az[s]);
                    const float n = tanhf(xn[s] + r * an[s]);
                    h[s] = (1.0f - z) * n + z * h[s];
                    y[row * HHG_H + j] = h[s];
                    float *sp = save + row * (HHG_SAVE * HHG_H) + j;
                    sp[0] = r; sp[HHG_H] = z; sp[2 * HHG_H] = n; sp[3 * HHG_H] = an[s];
                }
            }
        }
        __syncthreads();   /* every lane has read this step's h tile */
        if (unit) {
#pragma unroll
            for (int q = 0; q < TILE / 4; q++) s_h[j][q] = make_float4(h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]);
        }
        __syncthreads();
    }
    /* the padded tail: exact zeros */
    if (unit) {
#pragma unroll
        for (int s = 0; s < TILE; s++)
            if (s0 + s < S)
                for (int t = len[s]; t < L; t++) y[((s0 + s) * L + t) * HHG_H + j] = 0.0f;
    }
}

template <int TILE>
__global__ __launch_bounds__(HHG_THREADS) void hh_k_gru_seq_bwd(hhg_dev_io io, int64_t S, int L, const int32_t *__restrict__ seq_len,
                                                                const float *__restrict__ save_all) {
    static_assert(TILE == 4 || TILE == 8 || TILE == 16, "a tile is whole float4s of sequences");
    __shared__ float4 s_d[HHG_G3][TILE / 4];
    __shared__ int s_len[TILE];
    const int g = blockIdx.y, j = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * TILE;
    const float *__restrict__ w = io.w[g];
    const float *__restrict__ dy = io.dy[g];
    const float *__restrict__ y = io.y[g];
    const float *__restrict__ save = save_all + (int64_t)g * S * L * (HHG_SAVE * HHG_H);
    float *__restrict__ d_gi = io.d_gi[g];
    float *__restrict__ d_gh = io.d_gh[g];
    if (j < TILE) {
        int n = s0 + j < S ? seq_len[s0 + j] : 0;
        s_len[j] = n < 0 ? 0 : (n > L ? L : n);
    }
    __syncthreads();
    int len[TILE], t_max = 0;
#pragma unroll
    for (int s = 0; s < TILE; s++) {
        len[s] = s_len[s];
        t_max = len[s] > t_max ? len[s] : t_max;
    }
    const bool unit = j < HHG_H;
    float dh[TILE];
#pragma unroll
    for (int s = 0; s < TILE; s++) dh[s] = 0.0f;

    for (int t = t_max - 1; t >= 0; t--) {
        float keep[TILE];    /* dh_total z: the part of the carry that does not go through the gates */
        if (unit) {
            float gr[TILE], gz[TILE], gn[TILE];
#pragma unroll
            for (int s = 0; s < TILE; s++) {
                /* unconditional loads, so that all the tile's sequences' are in flight together; a sequence that has ended reads row 0 of dy, of the
                 * save buffer and of h0 and drops it.  Row 0 is in bounds and, with seq_len[0] >= 1 as the contract asks, written by the
                 * forward; were a stray seq_len[0] clamped to 0, the save row would be read unwritten and still dropped */
                const bool on = t < len[s];
                const int64_t row = on ? (s0 + s) * L + t : 0;
                const float *sp = save + row * (HHG_SAVE * HHG_H) + j;
                const float r = sp[0], z = sp[HHG_H], n = sp[2 * HHG_H], hn = sp[3 * HHG_H];
                const float hp = (on && t > 0) ? y[(row - 1) * HHG_H + j] : io.h0[g][(on ? s0 + s : 0) * HHG_H + j];
                const float d = dy[row * HHG_H + j] + dh[s];
                const float dn = d * (1.0f - z);
                const float dz = d * (hp - n);
                const float pn = dn * (1.0f - n * n);
                const float pr = (pn * hn) * (r * (1.0f - r));
                const float pz = dz * (z * (1.0f - z));
                gr[s] = on ? pr : 0.0f; gz[s] = on ? pz : 0.0f; gn[s] = on ? pn * r : 0.0f;
                keep[s] = on ? d * z : 0.0f;
                if (on) {
                    float *o = d_gi + row * HHG_G3 + j;
                    o[0] = pr; o[HHG_H] = pz; o[2 * HHG_H] = pn;
                    o = d_gh + row * HHG_G3 + j;
                    o[0] = pr; o[HHG_H] = pz; o[2 * HHG_H] = gn[s];
                }
            }
#pragma unroll
            for (int q = 0; q < TILE / 4; q++) {
                s_d[j][q] = make_float4(gr[4 * q], gr[4 * q + 1], gr[4 * q + 2], gr[4 * q + 3]);
                s_d[HHG_H + j][q] = make_float4(gz[4 * q], gz[4 * q + 1], gz[4 * q + 2], gz[4 * q + 3]);
                s_d[2 * HHG_H + j][q] = make_float4(gn[4 * q], gn[4 * q + 1], gn[4 * q + 2], gn[4 * q + 3]);
            }
        }
        __syncthreads();
        if (unit) {
            float acc[TILE];
#pragma unroll
            for (int s = 0; s < TILE; s++) acc[s] = 0.0f;
            float wv[HHG_KB];
#pragma unroll
            for (int u = 0; u < HHG_KB; u++) wv[u] = w[u * HHG_H + j];
            for (int c0 = 0; c0 < HHG_G3; c0 += HHG_KB) {      /* 600 = 75 x 8 */
                float cv[HHG_KB];
#pragma unroll
                for (int u = 0; u < HHG_KB; u++) cv[u] = wv[u];
                if (c0 + HHG_KB < HHG_G3) {
#pragma unroll
                    for (int u = 0; u < HHG_KB; u++) wv[u] = w[(c0 + HHG_KB + u) * HHG_H + j];
                }
#pragma unroll
                for (int u = 0; u < HHG_KB; u++) {
#pragma unroll
                    for (int q = 0; q < TILE / 4; q++) {
                        const float4 dv = s_d[c0 + u][q];
                        acc[4 * q] = fmaf(cv[u], dv.x, acc[4 * q]);
                        acc[4 * q + 1] = fmaf(cv[u], dv.y, acc[4 * q + 1]);
                        acc[4 * q + 2] = fmaf(cv[u], dv.z, acc[4 * q + 2]);
                        acc[4 * q + 3] = fmaf(cv[u], dv.w, acc[4 * q + 3]);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < TILE; s++) dh[s] = t < len[s] ? keep[s] + acc[s] : 0.0f;
        }
        __syncthreads();   /* every lane has read this step's d_gh tile */
    }
    if (unit) {
#pragma unroll
        for (int s = 0; s < TILE; s++) {
            if (s0 + s < S) {
                io.d_h0[g][(s0 + s) * HHG_H + j] = dh[s];
                for (int t = len[s]; t < L; t++) {
                    const int64_t row = (s0 + s) * L + t;
                    float *o = d_gi + row * HHG_G3 + j;
                    o[0] = 0.0f; o[HHG_H] = 0.0f; o[2 * HHG_H] = 0.0f;
                    o = d_gh + row * HHG_G3 + j;
                    o[0] = 0.0f; o[HHG_H] = 0.0f; o[2 * HHG_H] = 0.0f;
                }
            }
        }
    }
}

/* ---- the C ABI ---- */
static bool hhg_range(const void *p, int64_t bytes, const void *q, int64_t qbytes) {   /* do [p, p + bytes) and [q, q + qbytes) overlap */
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)qbytes && b < a + (uintptr_t)bytes;
}

static int hhg_check_shape(const char *who, int32_t G, int64_t S, int32_t L) {
    if (G < 1 || G > 2 || S < 1 || S > ((int64_t)1 << 24) || L < 1 || L > HH_GRU_MAX_LEN) {
        g_err = std::string(who) + ": need 1 <= n_gru <= 2, 1 <= n_seq <= 2^24, 1 <= max_len <= 32";
        return HH_E_ARG;
    }
    return HH_OK;
}

/* The tile of a call over n_seq sequences: HH_GRU_TILE (read at every call; 16 | 8 | 4, for A/B runs) or, without it, the rule measured
 * in DESIGN.md section 19: each narrow tile up to the largest measured n_seq at which it still beat tile 16 by more than both runs' spread.
 * While the workgroups fit the device side by side the launch lasts as long as one workgroup's dependent chain, which the narrow tile
 * shortens (3.0 x at 13 sequences, 1.6 x at 1708); once they queue, the narrow tiles' extra passes over W_hh cost more than they save
 * (tile 4 loses from 6832 sequences on).  Forward and backward of a pair see the same n_seq and so the same tile. */
#define HHG_TILE4_MAX_SEQ 1708
#define HHG_TILE8_MAX_SEQ 3416

static int hhg_pick_tile(const char *who, int64_t n_seq, int *tile) {
    const char *e = getenv("HH_GRU_TILE");
    if (e && *e) {
        const int v = atoi(e);
        if (v != 16 && v != 8 && v != 4) {
            g_err = std::string(who) + ": HH_GRU_TILE is one of the instantiated tiles 16, 8, 4, got \"" + e + "\"";
            return HH_E_ARG;
        }
        *tile = v;
        return HH_OK;
    }
    *tile = n_seq <= HHG_TILE4_MAX_SEQ ? 4 : (n_seq <= HHG_TILE8_MAX_SEQ ? 8 : HHG_TILE_WIDE);
    return HH_OK;
}

extern "C" int hh_gru_seq_tile(int64_t n_seq) {
    int tile = 0;
    if (int rc = hhg_pick_tile("hh_gru_seq_tile", n_seq, &tile)) return rc;
    return tile;
}

template <int TILE>
static void hhg_launch_fwd(const hhg_dev_io &d, int64_t n_seq, int n_gru, int max_len, const int32_t *seq_len, const float *wt, float *save,
                           hipStream_t st) {
    const unsigned tiles = (unsigned)((n_seq + TILE - 1) / TILE);
    hipLaunchKernelGGL(hh_k_gru_seq_fwd<TILE>, dim3(tiles, n_gru), dim3(HHG_THREADS), 0, st, d, n_seq, max_len, seq_len, wt, save);
}

template <int TILE>
static void hhg_launch_bwd(const hhg_dev_io &d, int64_t n_seq, int n_gru, int max_len, const int32_t *seq_len, const float *save, hipStream_t st) {
    const unsigned tiles = (unsigned)((n_seq + TILE - 1) / TILE);
    hipLaunchKernelGGL(hh_k_gru_seq_bwd<TILE>, dim3(tiles, n_gru), dim3(HHG_THREADS), 0, st, d, n_seq, max_len, seq_len, save);
}

extern "C" int hh_gru_seq_scratch_bytes(int32_t n_gru, int64_t n_seq, int32_t max_len, int64_t *bytes) {
    if (!bytes) { g_err = "hh_gru_seq_scratch_bytes: null argument"; return HH_E_ARG; }
    if (int rc = hhg_check_shape("hh_gru_seq_scratch_bytes", n_gru, n_seq, max_len)) return rc;
    *bytes = (hhg_pack_floats(n_gru) + (int64_t)n_gru * n_seq * max_len * HHG_SAVE * HHG_H) * (int64_t)sizeof(float);
    return HH_OK;
}

/* every pointer non-null and 16-byte aligned (span 0, seq_len: 4-byte); no output range meets an input or another output */
struct hhg_span { const void *p; int64_t bytes; bool out; };

static int hhg_check_spans(const char *who, const hhg_span *sp, int n) {
    for (int i = 0; i < n; i++) {
        if (!sp[i].p) { g_err = std::string(who) + ": null argument"; return HH_E_ARG; }
        if (reinterpret_cast<uintptr_t>(sp[i].p) & (i == 0 ? 3 : 15)) {
            g_err = std::string(who) + ": every float tensor must be 16-byte aligned, seq_len 4-byte";
            return HH_E_ARG;
        }
    }
    for (int i = 0; i < n; i++)
        for (int k = i + 1; k < n; k++)
            if ((sp[i].out || sp[k].out) && hhg_range(sp[i].p, sp[i].bytes, sp[k].p, sp[k].bytes)) {
                g_err = std::string(who) + ": an output overlaps another tensor of the call";
                return HH_E_ARG;
            }
    return HH_OK;
}

extern "C" int hh_gru_seq_forward(int32_t n_gru, int64_t n_seq, int32_t max_len, const hh_gru_seq_io *io, const int32_t *seq_len, void *scratch,
                                  int64_t scratch_bytes, void *stream) {
    if (int rc = hhg_check_shape("hh_gru_seq_forward", n_gru, n_seq, max_len)) return rc;
    if (!io || !seq_len || !scratch) { g_err = "hh_gru_seq_forward: null argument"; return HH_E_ARG; }
    int64_t need = 0;
    hh_gru_seq_scratch_bytes(n_gru, n_seq, max_len, &need);
    if (scratch_bytes < need) { g_err = "hh_gru_seq_forward: scratch is smaller than hh_gru_seq_scratch_bytes"; return HH_E_ARG; }
    const int64_t rows = n_seq * max_len;
    hhg_span sp[2 + 2 * 5];
    int n = 0;
    sp[n++] = {seq_len, n_seq * 4, false};
    sp[n++] = {scratch, need, true};
    hhg_dev_io d = {};
    for (int g = 0; g < n_gru; g++) {
        sp[n++] = {io[g].gi, rows * HHG_G3 * 4, false};
        sp[n++] = {io[g].h0, n_seq * HHG_H * 4, false};
        sp[n++] = {io[g].w_hh, (int64_t)HHG_G3 * HHG_H * 4, false};
        sp[n++] = {io[g].b_hh, (int64_t)HHG_G3 * 4, false};
        sp[n++] = {io[g].y, rows * HHG_H * 4, true};
        d.gi[g] = io[g].gi; d.h0[g] = io[g].h0; d.w[g] = io[g].w_hh; d.b_hh[g] = io[g].b_hh; d.y[g] = io[g].y;
    }
    if (int rc = hhg_check_spans("hh_gru_seq_forward", sp, n)) return rc;
    int tile = 0;
    if (int rc = hhg_pick_tile("hh_gru_seq_forward", n_seq, &tile)) return rc;
    hipStream_t st = (hipStream_t)stream;
    float *wt = static_cast<float *>(scratch);
    float *save = wt + hhg_pack_floats(n_gru);
    hipLaunchKernelGGL(hh_k_gru_pack, dim3((HHG_H + 31) / 32, (HHG_G3 + 31) / 32, n_gru), dim3(256), 0, st, d, wt);
    HIPCHK(hipGetLastError());
    if (tile == 4) hhg_launch_fwd<4>(d, n_seq, n_gru, max_len, seq_len, wt, save, st);
    else if (tile == 8) hhg_launch_fwd<8>(d, n_seq, n_gru, max_len, seq_len, wt, save, st);
    else hhg_launch_fwd<16>(d, n_seq, n_gru, max_len, seq_len, wt, save, st);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_gru_seq_backward(int32_t n_gru, int64_t n_seq, int32_t max_len, const hh_gru_seq_io *io, const int32_t *seq_len,
                                   const void *scratch, int64_t scratch_bytes, void *stream) {
    if (int rc = hhg_check_shape("hh_gru_seq_backward", n_gru, n_seq, max_len)) return rc;
    if (!io || !seq_len || !scratch) { g_err = "hh_gru_seq_backward: null argument"; return HH_E_ARG; }
    int64_t need = 0;
    hh_gru_seq_scratch_bytes(n_gru, n_seq, max_len, &need);
    if (scratch_bytes < need) { g_err = "hh_gru_seq_backward: scratch is smaller than hh_gru_seq_scratch_bytes"; return HH_E_ARG; }
    const int64_t rows = n_seq * max_len;
    hhg_span sp[2 + 2 * 8];
    int n = 0;
    sp[n++] = {seq_len, n_seq * 4, false};
    sp[n++] = {scratch, need, false};
    hhg_dev_io d = {};
    for (int g = 0; g < n_gru; g++) {
        sp[n++] = {io[g].dy, rows * HHG_H * 4, false};
        sp[n++] = {io[g].h0, n_seq * HHG_H * 4, false};
        sp[n++] = {io[g].y, rows * HHG_H * 4, false};
        sp[n++] = {io[g].w_hh, (int64_t)HHG_G3 * HHG_H * 4, false};
        sp[n++] = {io[g].d_gi, rows * HHG_G3 * 4, true};
        sp[n++] = {io[g].d_gh, rows * HHG_G3 * 4, true};
        sp[n++] = {io[g].d_h0, n_seq * HHG_H * 4, true};
        d.dy[g] = io[g].dy; d.h0[g] = io[g].h0; d.y[g] = io[g].y; d.w[g] = io[g].w_hh;
        d.d_gi[g] = io[g].d_gi; d.d_gh[g] = io[g].d_gh; d.d_h0[g] = io[g].d_h0;
    }
    if (int rc = hhg_check_spans("hh_gru_seq_backward", sp, n)) return rc;
    int tile = 0;
    if (int rc = hhg_pick_tile("hh_gru_seq_backward", n_seq, &tile)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const float *save = static_cast<const float *>(scratch) + hhg_pack_floats(n_gru);
    if (tile == 4) hhg_launch_bwd<4>(d, n_seq, n_gru, max_len, seq_len, save, st);
    else if (tile == 8) hhg_launch_bwd<8>(d, n_seq, n_gru, max_len, seq_len, save, st);
    else hhg_launch_bwd<16>(d, n_seq, n_gru, max_len, seq_len, save, st);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

#endif /* HH_GRU_SEQ_H */
