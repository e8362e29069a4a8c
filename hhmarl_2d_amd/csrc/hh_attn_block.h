/*
 * hh_attn_block.h — one whole attention block of a fight network, normalize(x + out_proj(attention(in_proj(x)))), as ONE launch forward
 * and TWO backward (learner.TrainableNet(attention="block"); C ABI and the formulas: include/hh_learner.h).  Everything float32.
 *
 * Tile.  A workgroup of 512 lanes (8 waves) owns a tile of HH_ATTN_BLOCK_ROWS / len whole sequences, at most HH_ATTN_BLOCK_ROWS = 32
 * rows: the largest operand of any product, a tile's [32, 3E] qkv or d_qkv, then fits LDS (57.9 KB at E = 150) beside the [32, E] tiles,
 * and a chunk of 20 rows is a tile of its own, so the 14 chunks of a default minibatch spread over 14 CUs.  The weights are read from L2
 * once per tile.  Row strides in LDS: 300 | 452 words for the 3E-wide tile and 100 | 156 for the E-wide ones — multiples of 4 (16-byte
 * rows for the broadcast reads) and odd multiples of 4 modulo 32 (the 8 rows that the lanes of a score row group read fall on 8 banks).
 *
 * Products.  All five are v_mfma_f32_32x32x2_f32 (float32 in, float32 fused multiply-adds: on gfx950 the vector rate, but one issue slot
 * per 2048 of them, and no broadcast reads).  hab_gemm: a wave owns blocks of 32 output columns over the tile's 32 rows; per step a lane
 * reads 4 | 2 floats of its A row from LDS (one 16- | 8-byte read) and 4 | 2 floats of the weights from global memory — along k from the
 * lane's own weight row for x W^T (W_in rows are 400 | 600 B: 16- | 8-byte aligned), across the lanes for d W — and issues 4 | 2 MFMAs.
 * Rows of the tile beyond the call's are garbage in, garbage out, and dropped: a result row depends on its own A row only.  hab_gemm_tn
 * sums over the rows of the tile for the weight gradients, a wave per 32 x 32 block of d_W, two rows per MFMA.  Every sum runs in a
 * fixed order that depends on the shapes alone.
 *
 * Core.  hh_chunk_attn.h's lane maps on 256 lanes per (sequence, head) unit, both heads of a sequence at a time, reading q, k, v where
 * the in-projection left them in LDS.  The backward writes d_qkv over qkv in place: d_v at once, d_q held in registers (8 | 12 per lane)
 * until the unit's k has been read, then d_k over k and d_q over q, a barrier between each.  len == 1 needs no core: ctx is the v columns, d_v = d_ctx and d_q = d_k = 0.
 *
 * Backward.  Launch one walks the tiles grid-stride with min(tiles, HH_ATTN_BLOCK_MAX_WG) workgroups; each writes its tiles' d_x rows and
 * keeps its own partial d_W_in | d_b_in | d_W_out | d_b_out (4 E^2 + 4 E floats) in `scratch`, overwritten by its first tile and added
 * to by the later ones in tile order, element (n, c) always by the same lane.  Launch two adds the workgroups' partials of every element
 * in workgroup order in float64 and rounds once.  No atomics.
 */
#ifndef HH_ATTN_BLOCK_H
#define HH_ATTN_BLOCK_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hh_chunk_attn.h"
#include "hh_learner.h"

#define HAB_THREADS 512
#define HAB_WAVES 8
#define HAB_ST 4         /* hab_gemm: steps of 2 KV columns of k whose loads are in flight together */
#define HAB_PS 36        /* row stride of the probability tiles, as HCA_PS */
#define HAB_PT (HH_ATTN_MAX_LEN * HAB_PS)

static_assert(HH_ATTN_BLOCK_ROWS == HH_ATTN_MAX_LEN, "a tile holds at least one sequence of the longest length");

template <int E>
struct hab_dims {
    static_assert(E == 100 || E == 150, "compiled widths");
    static constexpr int D = E / 2, E3 = 3 * E;
    static constexpr int EP = E == 100 ? 100 : 156;     /* LDS row stride of the E-wide tiles */
    static constexpr int LQ = E == 100 ? 300 : 452;     /* LDS row stride of the 3E-wide tile */
    static constexpr int KV = E % 4 == 0 ? 4 : 2;       /* floats per load along k: the weight rows are 16- | 8-byte aligned */
    static constexpr int PART = 4 * E * E + 4 * E;      /* floats of one workgroup's partial sums */
    static constexpr int LDS_FWD = (HH_ATTN_BLOCK_ROWS * (2 * EP + LQ) + 2 * HAB_PT) * 4;
    static constexpr int LDS_BWD = (HH_ATTN_BLOCK_ROWS * (2 * EP + LQ) + 6 * HAB_PT) * 4;
    static_assert(EP % 4 == 0 && LQ % 4 == 0 && (EP / 4) % 2 == 1 && (LQ / 4) % 2 == 1 && EP >= E && LQ >= E3, "row strides");
    static_assert(E3 <= HAB_THREADS && E % KV == 0, "the bias sums take one lane per column");
};

template <int KV>
__device__ __forceinline__ void hab_load(float (&o)[KV], const float *p) {
    if constexpr (KV == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        o[0] = t.x; o[1] = t.y;
    }
}

typedef float hab_v16 __attribute__((ext_vector_type(16)));

/* v_mfma_f32_32x32x2_f32: lane l supplies A[l % 32][l / 32] and B[l / 32][l % 32]; element i of its 16 results is
 * C[8 (i / 4) + 4 (l / 32) + i % 4][l % 32].  Float32 inputs, float32 fused multiply-adds. */
__device__ __forceinline__ int hab_c_row(int i, int kh) { return 8 * (i >> 2) + 4 * kh + (i & 3); }

/* out[r][c] = sum_k A[r][k] B(c, k) for r < rows, c < N.  A: LDS, the tile's 32 rows, row stride lda; the rows from `rows` on are read
 * (they lie inside the tile) and their results dropped: a row of the product depends on its own row of A only.  NT: B(c, k) = b[c ldb + k]
 * (a weight's rows, KV floats per load); else B(c, k) = b[k ldb + c] (across the lanes).  A wave owns blocks of 32 columns; per step a
 * lane loads KV floats of A and of B at k0 + KV (lane / 32) and issues KV MFMAs (HAB_ST steps' loads first, then their MFMAs; beyond K
 * zeros go in), so the sum over k runs in a fixed order that depends on K and KV only.  store(r, c, sum) is called once per element. */
template <int N, int K, int KV, bool NT, class Store>
__device__ __forceinline__ void hab_gemm(const float *as, int lda, const float *__restrict__ b, int ldb, int rows, int wave, int lane, Store store) {
    constexpr int NB = (N + 31) / 32;
    const int l32 = lane & 31, kh = lane >> 5;
    for (int nb = wave; nb < NB; nb += HAB_WAVES) {
        const int c = nb * 32 + l32, cc = c < N ? c : N - 1;
        const float *ap = as + l32 * lda + KV * kh;
        hab_v16 acc;
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = 0.0f;
#pragma unroll 1
        for (int k0 = 0; k0 < K; k0 += 2 * KV * HAB_ST) {      /* HAB_ST steps' loads are issued before their MFMAs: the loop is bound by load latency */
            float a[HAB_ST][KV], w[HAB_ST][KV];
#pragma unroll
            for (int s = 0; s < HAB_ST; s++) {
                const int kk = k0 + 2 * KV * s + KV * kh;
#pragma unroll
                for (int u = 0; u < KV; u++) a[s][u] = w[s][u] = 0.0f;
                if (kk < K) {
                    hab_load<KV>(a[s], ap + k0 + 2 * KV * s);
                    if constexpr (NT) {
                        hab_load<KV>(w[s], b + (int64_t)cc * ldb + kk);
                    } else {
#pragma unroll
                        for (int u = 0; u < KV; u++) w[s][u] = b[(int64_t)(kk + u) * ldb + cc];
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < HAB_ST; s++) {
#pragma unroll
                for (int u = 0; u < KV; u++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][u], w[s][u], acc, 0, 0, 0);
            }
        }
        if (c < N) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int r = hab_c_row(i, kh);
                if (r < rows) store(r, c, acc[i]);
            }
        }
    }
}

/* part[n][c] = (first ? 0 : part[n][c]) + sum_{r < rows} A[r][n] b[r ldb + c] for n < NO, c < NC; A: LDS, row stride lda.  A wave owns
 * 32 x 32 blocks of the result, two rows of the tile per MFMA, in row order.  Element (n, c) belongs to the same lane in every call. */
template <int NO, int NC>
__device__ __forceinline__ void hab_gemm_tn(const float *as, int lda, const float *__restrict__ b, int ldb, int rows, int wave, int lane,
                                            float *__restrict__ part, bool first) {
    constexpr int NBC = (NC + 31) / 32, NBO = (NO + 31) / 32;
    const int l32 = lane & 31, kh = lane >> 5;
    for (int it = wave; it < NBC * NBO; it += HAB_WAVES) {
        const int cb = it % NBC, n0 = (it / NBC) * 32;
        const int c = cb * 32 + l32, cc = c < NC ? c : NC - 1;
        const int nn = n0 + l32 < NO ? n0 + l32 : NO - 1;
        hab_v16 acc;
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = 0.0f;
        for (int r0 = 0; r0 < rows; r0 += 2) {
            const int r = r0 + kh;
            const bool on = r < rows;
            const float av = on ? as[r * lda + nn] : 0.0f;
            const float bv = on ? b[(int64_t)r * ldb + cc] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        if (c < NC) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int n = n0 + hab_c_row(i, kh);
                if (n < NO) {
                    float *p = part + n * NC + c;
                    *p = first ? acc[i] : *p + acc[i];
                }
            }
        }
    }
}

/* part[n] = (first ? 0 : part[n]) + sum_{r < rows} A[r][n], r ascending, one lane per column */
template <int NO>
__device__ __forceinline__ void hab_colsum(const float *as, int lda, int rows, int t, float *__restrict__ part, bool first) {
    if (t < NO) {
        float acc = 0.0f;
        for (int r = 0; r < rows; r++) acc += as[r * lda + t];
        part[t] = first ? acc : part[t] + acc;
    }
}

/* hca_scores on tiles with row strides LQ (q, k, v) and LO (dO): softmax(Q K^T / sqrt(D)) of row ic for the lane's keys part + 8 jj */
template <int D, int LQ, int LO, bool BWD>
__device__ __forceinline__ void hab_scores(const float *q, const float *k, const float *v, const float *dO, int len, int ic, int part,
                                           float p[HCA_JJ], float dp[HCA_JJ]) {
    const float scale = (float)(1.0 / sqrt((double)D));
    int jo[HCA_JJ];
    float acc[HCA_JJ];
#pragma unroll
    for (int jj = 0; jj < HCA_JJ; jj++) {
        const int j = part + 8 * jj;
        jo[jj] = j < len ? j : 0;
        acc[jj] = 0.0f;
        dp[jj] = 0.0f;
    }
    const float *qi = q + ic * LQ, *di = dO + ic * LO;
#pragma unroll 5
    for (int c = 0; c < D; c++) {
        const float qv = qi[c];
        const float dv = BWD ? di[c] : 0.0f;
#pragma unroll
        for (int jj = 0; jj < HCA_JJ; jj++) {
            if (8 * jj < len) {
                acc[jj] = fmaf(qv, k[jo[jj] * LQ + c], acc[jj]);
                if (BWD) dp[jj] = fmaf(dv, v[jo[jj] * LQ + c], dp[jj]);
            }
        }
    }
    float m = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < HCA_JJ; jj++) {
        acc[jj] = part + 8 * jj < len ? acc[jj] * scale : -INFINITY;
        m = fmaxf(m, acc[jj]);
    }
    m = fmaxf(m, __shfl_xor(m, 1));
    m = fmaxf(m, __shfl_xor(m, 2));
    m = fmaxf(m, __shfl_xor(m, 4));
    float sum = 0.0f;
#pragma unroll
    for (int jj = 0; jj < HCA_JJ; jj++) {
        p[jj] = expf(acc[jj] - m);
        sum += p[jj];
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 4);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int jj = 0; jj < HCA_JJ; jj++) p[jj] *= inv;
}

__device__ __forceinline__ float hab_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

/* ---- forward: one tile per workgroup ---- */
template <int E>
__global__ __launch_bounds__(HAB_THREADS) void hh_k_attn_block_fwd(int64_t n_seq, int len, int spt, const float *__restrict__ x,
                                                                   const float *__restrict__ w_in, const float *__restrict__ b_in,
                                                                   const float *__restrict__ w_out, const float *__restrict__ b_out,
                                                                   float *__restrict__ y, float *__restrict__ s_qkv, float *__restrict__ s_ctx,
                                                                   float *__restrict__ s_norm) {
    using DM = hab_dims<E>;
    constexpr int D = DM::D, E3 = DM::E3, EP = DM::EP, LQ = DM::LQ, KV = DM::KV;
    extern __shared__ float4 hab_lds_fwd[];
    float *xs = reinterpret_cast<float *>(hab_lds_fwd);                 /* x, then s = x + a */
    float *qs = xs + HH_ATTN_BLOCK_ROWS * EP;                           /* qkv */
    float *cs = qs + HH_ATTN_BLOCK_ROWS * LQ;                           /* ctx */
    float *pts = cs + HH_ATTN_BLOCK_ROWS * EP;                          /* P^T[j][i] per half */
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t seq0 = (int64_t)blockIdx.x * spt;
    const int ns = (int)(n_seq - seq0 < spt ? n_seq - seq0 : spt), rows = ns * len;
    const int64_t row0 = seq0 * len;

    for (int e = t; e < rows * (E / 2); e += HAB_THREADS) {
        const int r = e / (E / 2), c = 2 * (e - r * (E / 2));
        *reinterpret_cast<float2 *>(xs + r * EP + c) = *reinterpret_cast<const float2 *>(x + (row0 + r) * E + c);
    }
    __syncthreads();
    hab_gemm<E3, E, KV, true>(xs, EP, w_in, E, rows, wave, lane, [&](int r, int c, float acc) {
        const float val = acc + b_in[c];
        qs[r * LQ + c] = val;
        s_qkv[(row0 + r) * E3 + c] = val;
    });
    __syncthreads();
    if (len == 1) {
        for (int e = t; e < rows * E; e += HAB_THREADS) {
            const int r = e / E, c = e - r * E;
            const float val = qs[r * LQ + 2 * E + c];
            cs[r * EP + c] = val;
            s_ctx[(row0 + r) * E + c] = val;
        }
    } else {
        const int half = t >> 8, tt = t & 255, i = tt >> 3, part = tt & 7;
        float *pt = pts + half * HAB_PT;
        for (int u = half; u < 2 * ns; u += 2) {            /* unit u: sequence u / 2 of the tile, head u % 2; 2 ns is even: one trip count for all */
            const int r0 = (u >> 1) * len, h = u & 1;
            const float *q = qs + r0 * LQ + h * D, *k = q + E, *v = q + 2 * E;
            float p[HCA_JJ], unused[HCA_JJ];
            hab_scores<D, LQ, LQ, false>(q, k, v, q, len, i < len ? i : 0, part, p, unused);
            if (i < len) {
#pragma unroll
                for (int jj = 0; jj < HCA_JJ; jj++) {
                    const int j = part + 8 * jj;
                    if (j < len) pt[j * HAB_PS + i] = p[jj];
                }
            }
            __syncthreads();
            const int n = ((len + 3) >> 2) * D;
            for (int e = tt; e < n; e += 256) {
                const int b = e / D, c = e - b * D, i0 = 4 * b;
                float4 pr = *reinterpret_cast<const float4 *>(pt + i0);
                float vv = v[c];
                float a0 = pr.x * vv, a1 = pr.y * vv, a2 = pr.z * vv, a3 = pr.w * vv;
                for (int j = 1; j < len; j++) {
                    pr = *reinterpret_cast<const float4 *>(pt + j * HAB_PS + i0);
                    vv = v[j * LQ + c];
                    a0 = fmaf(pr.x, vv, a0); a1 = fmaf(pr.y, vv, a1); a2 = fmaf(pr.z, vv, a2); a3 = fmaf(pr.w, vv, a3);
                }
                float *ol = cs + (r0 + i0) * EP + h * D + c;
                float *og = s_ctx + (row0 + r0 + i0) * E + h * D + c;
                ol[0] = a0; og[0] = a0;
                if (i0 + 1 < len) { ol[EP] = a1; og[E] = a1; }
                if (i0 + 2 < len) { ol[2 * EP] = a2; og[2 * E] = a2; }
                if (i0 + 3 < len) { ol[3 * EP] = a3; og[3 * E] = a3; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    hab_gemm<E, E, KV, true>(cs, EP, w_out, E, rows, wave, lane, [&](int r, int c, float acc) {
        xs[r * EP + c] = xs[r * EP + c] + (acc + b_out[c]);
    });
    __syncthreads();
    for (int r = wave; r < rows; r += HAB_WAVES) {
        float sv[3];
        float ss = 0.0f;
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const int c = lane + 64 * u;
            sv[u] = c < E ? xs[r * EP + c] : 0.0f;
            ss = fmaf(sv[u], sv[u], ss);
        }
        ss = hab_wave_sum(ss);
        const float nrm = sqrtf(ss);
        const float den = fmaxf(nrm, HCA_EPS);
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const int c = lane + 64 * u;
            if (c < E) y[(row0 + r) * E + c] = sv[u] / den;
        }
        if (lane == 0) s_norm[row0 + r] = nrm;
    }
}

/* ---- backward, launch one: the tiles grid-stride; d_x and the workgroup's partial weight gradients ---- */
template <int E>
__global__ __launch_bounds__(HAB_THREADS) void hh_k_attn_block_bwd(int64_t n_seq, int len, int spt, int64_t n_tiles, const float *__restrict__ x,
                                                                   const float *__restrict__ w_in, const float *__restrict__ w_out,
                                                                   const float *__restrict__ y, const float *__restrict__ s_qkv,
                                                                   const float *__restrict__ s_ctx, const float *__restrict__ s_norm,
                                                                   const float *__restrict__ d_y, float *__restrict__ d_x, float *__restrict__ scratch) {
    using DM = hab_dims<E>;
    constexpr int D = DM::D, E3 = DM::E3, EP = DM::EP, LQ = DM::LQ, KV = DM::KV;
    constexpr int NIT = (8 * D + 255) / 256;        /* outputs of a unit: ceil(len / 4) D <= 8 D lanes' worth */
    extern __shared__ float4 hab_lds_bwd[];
    float *qs = reinterpret_cast<float *>(hab_lds_bwd);                 /* qkv, then d_qkv in place */
    float *ds = qs + HH_ATTN_BLOCK_ROWS * LQ;                           /* d_s = d_a */
    float *dc = ds + HH_ATTN_BLOCK_ROWS * EP;                           /* d_ctx */
    float *pts = dc + HH_ATTN_BLOCK_ROWS * EP;                          /* P, dS, dS^T per half */
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float *p_w_in = scratch + (int64_t)blockIdx.x * DM::PART, *p_b_in = p_w_in + E3 * E, *p_w_out = p_b_in + E3, *p_b_out = p_w_out + E * E;

    for (int tile = blockIdx.x; tile < (int)n_tiles; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int seq0 = tile * spt;
        const int ns = ((int)n_seq - seq0 < spt ? (int)n_seq - seq0 : spt), rows = ns * len;
        const int row0 = seq0 * len;

        /* normalize backward -> ds; qkv -> qs */
        for (int r = wave; r < rows; r += HAB_WAVES) {
            float yv[3], gv[3];
            float dot = 0.0f;
#pragma unroll
            for (int u = 0; u < 3; u++) {
                const int c = lane + 64 * u;
                yv[u] = c < E ? y[(int64_t)(row0 + r) * E + c] : 0.0f;
                gv[u] = c < E ? d_y[(int64_t)(row0 + r) * E + c] : 0.0f;
                dot = fmaf(yv[u], gv[u], dot);
            }
            dot = hab_wave_sum(dot);
            const float nrm = s_norm[row0 + r];
#pragma unroll
            for (int u = 0; u < 3; u++) {
                const int c = lane + 64 * u;
                if (c < E) ds[r * EP + c] = nrm >= HCA_EPS ? (gv[u] - yv[u] * dot) / nrm : gv[u] / HCA_EPS;
            }
        }
        if (len > 1) {
            for (int e = t; e < rows * (E3 / 2); e += HAB_THREADS) {
                const int r = e / (E3 / 2), c = 2 * (e - r * (E3 / 2));
                *reinterpret_cast<float2 *>(qs + r * LQ + c) = *reinterpret_cast<const float2 *>(s_qkv + (int64_t)(row0 + r) * E3 + c);
            }
        }
        __syncthreads();

        /* out-projection backward: d_ctx = d_a W_out; d_W_out += d_a^T ctx; d_b_out += column sums of d_a */
        hab_gemm<E, E, KV, false>(ds, EP, w_out, E, rows, wave, lane, [&](int r, int c, float acc) { dc[r * EP + c] = acc; });
        hab_gemm_tn<E, E>(ds, EP, s_ctx + (int64_t)row0 * E, E, rows, wave, lane, p_w_out, first);
        hab_colsum<E>(ds, EP, rows, t, p_b_out, first);
        __syncthreads();

        /* the core's backward, d_qkv over qkv */
        if (len == 1) {
            for (int e = t; e < rows * E; e += HAB_THREADS) {
                const int r = e / E, c = e - r * E;
                qs[r * LQ + c] = 0.0f;
                qs[r * LQ + E + c] = 0.0f;
                qs[r * LQ + 2 * E + c] = dc[r * EP + c];
            }
        } else {
            const int half = t >> 8;
            float *pn = pts + half * 3 * HAB_PT, *sn = pn + HAB_PT, *st = sn + HAB_PT;
            const float scale = (float)(1.0 / sqrt((double)D));
            for (int u = half; u < 2 * ns; u += 2) {
                int tt = t & 255;
                asm volatile("" : "+v"(tt));        /* the unit's lane predicates (j < len, i0 + w < len, ..) are made here, per unit: hoisted in front of
                                                       the tile loop they occupy some 40 scalar registers for the whole kernel, more than there are */
                const int i = tt >> 3, part = tt & 7;
                const int r0 = (u >> 1) * len, h = u & 1;
                float *q = qs + r0 * LQ + h * D, *k = q + E, *v = q + 2 * E;
                const float *dO = dc + r0 * EP + h * D;
                float p[HCA_JJ], dp[HCA_JJ];
                hab_scores<D, LQ, EP, true>(q, k, v, dO, len, i < len ? i : 0, part, p, dp);
                float rs = 0.0f;
#pragma unroll
                for (int jj = 0; jj < HCA_JJ; jj++) rs = fmaf(p[jj], dp[jj], rs);
                rs += __shfl_xor(rs, 1);
                rs += __shfl_xor(rs, 2);
                rs += __shfl_xor(rs, 4);
                if (i < len) {
#pragma unroll
                    for (int jj = 0; jj < HCA_JJ; jj++) {
                        const int j = part + 8 * jj;
                        if (j < len) {
                            const float dsv = p[jj] * (dp[jj] - rs) * scale;
                            pn[i * HAB_PS + j] = p[jj];
                            sn[i * HAB_PS + j] = dsv;
                            st[j * HAB_PS + i] = dsv;
                        }
                    }
                }
                __syncthreads();
                /* in place: d_v goes straight over v (read by the scores only); d_q waits in registers until every lane has read k for it,
                 * then d_k, which reads q, goes over k, and d_q over q last */
                const int n = ((len + 3) >> 2) * D;
                float oq[NIT][4];
#pragma unroll
                for (int it = 0; it < NIT; it++) {
                    const int e = tt + 256 * it;
#pragma unroll
                    for (int w = 0; w < 4; w++) oq[it][w] = 0.0f;
                    if (e < n) {
                        const int b = e / D, c = e - b * D, i0 = 4 * b;
                        float4 ps = *reinterpret_cast<const float4 *>(pn + i0), ts = *reinterpret_cast<const float4 *>(st + i0);
                        float og = dO[c], kv = k[c];
                        float v0 = ps.x * og, v1 = ps.y * og, v2 = ps.z * og, v3 = ps.w * og;
                        float q0 = ts.x * kv, q1 = ts.y * kv, q2 = ts.z * kv, q3 = ts.w * kv;
                        for (int r = 1; r < len; r++) {         /* dV = P^T dO over the queries, dQ = dS K over the keys, in order */
                            ps = *reinterpret_cast<const float4 *>(pn + r * HAB_PS + i0);
                            ts = *reinterpret_cast<const float4 *>(st + r * HAB_PS + i0);
                            og = dO[r * EP + c];
                            kv = k[r * LQ + c];
                            v0 = fmaf(ps.x, og, v0); v1 = fmaf(ps.y, og, v1); v2 = fmaf(ps.z, og, v2); v3 = fmaf(ps.w, og, v3);
                            q0 = fmaf(ts.x, kv, q0); q1 = fmaf(ts.y, kv, q1); q2 = fmaf(ts.z, kv, q2); q3 = fmaf(ts.w, kv, q3);
                        }
                        float *o = v + i0 * LQ + c;
                        o[0] = v0;
                        if (i0 + 1 < len) o[LQ] = v1;
                        if (i0 + 2 < len) o[2 * LQ] = v2;
                        if (i0 + 3 < len) o[3 * LQ] = v3;
                        oq[it][0] = q0; oq[it][1] = q1; oq[it][2] = q2; oq[it][3] = q3;
                    }
                }
                __syncthreads();
#pragma unroll 1
                for (int e = tt; e < n; e += 256) {
                    const int b = e / D, c = e - b * D, i0 = 4 * b;
                    float4 ss = *reinterpret_cast<const float4 *>(sn + i0);
                    float qv = q[c];
                    float k0 = ss.x * qv, k1 = ss.y * qv, k2 = ss.z * qv, k3 = ss.w * qv;
                    for (int r = 1; r < len; r++) {             /* dK = dS^T Q over the queries, in order */
                        ss = *reinterpret_cast<const float4 *>(sn + r * HAB_PS + i0);
                        qv = q[r * LQ + c];
                        k0 = fmaf(ss.x, qv, k0); k1 = fmaf(ss.y, qv, k1); k2 = fmaf(ss.z, qv, k2); k3 = fmaf(ss.w, qv, k3);
                    }
                    float *o = k + i0 * LQ + c;
                    o[0] = k0;
                    if (i0 + 1 < len) o[LQ] = k1;
                    if (i0 + 2 < len) o[2 * LQ] = k2;
                    if (i0 + 3 < len) o[3 * LQ] = k3;
                }
                __syncthreads();
#pragma unroll
                for (int it = 0; it < NIT; it++) {
                    const int e = tt + 256 * it;
                    if (e < n) {
                        const int b = e / D, c = e - b * D, i0 = 4 * b;
                        float *o = q + i0 * LQ + c;
                        o[0] = oq[it][0];
                        if (i0 + 1 < len) o[LQ] = oq[it][1];
                        if (i0 + 2 < len) o[2 * LQ] = oq[it][2];
                        if (i0 + 3 < len) o[3 * LQ] = oq[it][3];
                    }
                }
            }
        }
        __syncthreads();

        /* in-projection backward: d_x = d_s + d_qkv W_in; d_W_in += d_qkv^T x; d_b_in += column sums of d_qkv */
        hab_gemm<E, E3, KV, false>(qs, LQ, w_in, E, rows, wave, lane, [&](int r, int c, float acc) {
            d_x[(int64_t)(row0 + r) * E + c] = ds[r * EP + c] + acc;
        });
        hab_gemm_tn<E3, E>(qs, LQ, x + (int64_t)row0 * E, E, rows, wave, lane, p_w_in, first);
        hab_colsum<E3>(qs, LQ, rows, t, p_b_in, first);
        __syncthreads();        /* the next tile writes ds and qs */
    }
}

/* ---- backward, launch two: every element's partials added in workgroup order, float64, rounded once ---- */
template <int E>
__global__ __launch_bounds__(256) void hh_k_attn_block_sum(int n_wg, const float *__restrict__ scratch, float *__restrict__ d_w_in,
                                                           float *__restrict__ d_b_in, float *__restrict__ d_w_out, float *__restrict__ d_b_out) {
    using DM = hab_dims<E>;
    constexpr int E3 = DM::E3;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= DM::PART) return;
    double acc = (double)scratch[i];
    for (int w = 1; w < n_wg; w++) acc += (double)scratch[(int64_t)w * DM::PART + i];
    const float val = (float)acc;
    if (i < E3 * E) d_w_in[i] = val;
    else if (i < E3 * E + E3) d_b_in[i - E3 * E] = val;
    else if (i < E3 * E + E3 + E * E) d_w_out[i - E3 * E - E3] = val;
    else d_b_out[i - E3 * E - E3 - E * E] = val;
}

/* ---- the C ABI ---- */
struct hab_geom { int spt; int64_t n_tiles; int n_wg; int64_t rows, off_ctx, off_norm, save_floats; };

static int hab_geometry(const char *who, int64_t n_seq, int32_t len, int32_t embed, hab_geom *g) {
    if (int rc = hca_check_core(who, n_seq, len, embed)) return rc;
    g->spt = HH_ATTN_BLOCK_ROWS / len;
    g->n_tiles = (n_seq + g->spt - 1) / g->spt;
    g->n_wg = (int)(g->n_tiles < HH_ATTN_BLOCK_MAX_WG ? g->n_tiles : HH_ATTN_BLOCK_MAX_WG);
    g->rows = n_seq * len;
    g->off_ctx = (g->rows * 3 * embed + 3) / 4 * 4;                 /* every part starts 16-byte aligned */
    g->off_norm = g->off_ctx + (g->rows * embed + 3) / 4 * 4;
    g->save_floats = g->off_norm + (g->rows + 3) / 4 * 4;
    return HH_OK;
}

extern "C" int hh_attn_block_tile(int64_t n_seq, int32_t len, int32_t embed, int32_t *seq_per_tile, int32_t *n_workgroups) {
    hab_geom g;
    if (int rc = hab_geometry("hh_attn_block_tile", n_seq, len, embed, &g)) return rc;
    if (seq_per_tile) *seq_per_tile = g.spt;
    if (n_workgroups) *n_workgroups = g.n_wg;
    return HH_OK;
}

extern "C" int hh_attn_block_save_bytes(int64_t n_seq, int32_t len, int32_t embed, int64_t *bytes) {
    hab_geom g;
    if (int rc = hab_geometry("hh_attn_block_save_bytes", n_seq, len, embed, &g)) return rc;
    if (!bytes) { g_err = "hh_attn_block_save_bytes: null argument"; return HH_E_ARG; }
    *bytes = g.save_floats * 4;
    return HH_OK;
}

extern "C" int hh_attn_block_scratch_bytes(int64_t n_seq, int32_t len, int32_t embed, int64_t *bytes) {
    hab_geom g;
    if (int rc = hab_geometry("hh_attn_block_scratch_bytes", n_seq, len, embed, &g)) return rc;
    if (!bytes) { g_err = "hh_attn_block_scratch_bytes: null argument"; return HH_E_ARG; }
    *bytes = (int64_t)g.n_wg * (4 * embed * embed + 4 * embed) * 4;
    return HH_OK;
}

template <int E>
static int hab_launch_fwd(const hab_geom &g, int64_t n_seq, int len, const float *x, const float *w_in, const float *b_in, const float *w_out,
                          const float *b_out, float *y, float *save, hipStream_t st) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(hh_k_attn_block_fwd<E>), hipFuncAttributeMaxDynamicSharedMemorySize, hab_dims<E>::LDS_FWD));
    hipLaunchKernelGGL(hh_k_attn_block_fwd<E>, dim3((unsigned)g.n_tiles), dim3(HAB_THREADS), hab_dims<E>::LDS_FWD, st, n_seq, len, g.spt, x, w_in, b_in,
                       w_out, b_out, y, save, save + g.off_ctx, save + g.off_norm);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

template <int E>
static int hab_launch_bwd(const hab_geom &g, int64_t n_seq, int len, const float *x, const float *w_in, const float *w_out, const float *y,
                          const float *save, const float *d_y, float *d_x, float *d_w_in, float *d_b_in, float *d_w_out, float *d_b_out,
                          float *scratch, hipStream_t st) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(hh_k_attn_block_bwd<E>), hipFuncAttributeMaxDynamicSharedMemorySize, hab_dims<E>::LDS_BWD));
    hipLaunchKernelGGL(hh_k_attn_block_bwd<E>, dim3((unsigned)g.n_wg), dim3(HAB_THREADS), hab_dims<E>::LDS_BWD, st, n_seq, len, g.spt, g.n_tiles, x, w_in,
                       w_out, y, save, save + g.off_ctx, save + g.off_norm, d_y, d_x, scratch);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_attn_block_sum<E>, dim3((unsigned)((hab_dims<E>::PART + 255) / 256)), dim3(256), 0, st, g.n_wg, scratch, d_w_in, d_b_in,
                       d_w_out, d_b_out);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_attn_block_forward(int64_t n_seq, int32_t len, int32_t embed, const float *x, const float *w_in, const float *b_in,
                                     const float *w_out, const float *b_out, float *y, void *save, int64_t save_bytes, void *stream) {
    const char *who = "hh_attn_block_forward";
    hab_geom g;
    if (int rc = hab_geometry(who, n_seq, len, embed, &g)) return rc;
    if (n_seq == 0) return HH_OK;
    if (save_bytes < g.save_floats * 4) { g_err = std::string(who) + ": save is smaller than hh_attn_block_save_bytes says"; return HH_E_ARG; }
    const int64_t E = embed, xb = g.rows * E * 4;
    const hca_span sp[7] = {{x, xb, false}, {w_in, 3 * E * E * 4, false}, {b_in, 3 * E * 4, false}, {w_out, E * E * 4, false}, {b_out, E * 4, false},
                            {y, xb, true}, {save, g.save_floats * 4, true}};
    if (int rc = hca_check_spans(who, sp, 7, 16)) return rc;
    hipStream_t st = (hipStream_t)stream;
    float *sv = static_cast<float *>(save);
    return embed == 100 ? hab_launch_fwd<100>(g, n_seq, len, x, w_in, b_in, w_out, b_out, y, sv, st)
                        : hab_launch_fwd<150>(g, n_seq, len, x, w_in, b_in, w_out, b_out, y, sv, st);
}

extern "C" int hh_attn_block_backward(int64_t n_seq, int32_t len, int32_t embed, const float *x, const float *w_in, const float *w_out,
                                      const float *y, const void *save, int64_t save_bytes, const float *d_y, float *d_x, float *d_w_in,
                                      float *d_b_in, float *d_w_out, float *d_b_out, void *scratch, int64_t scratch_bytes, void *stream) {
    const char *who = "hh_attn_block_backward";
    hab_geom g;
    if (int rc = hab_geometry(who, n_seq, len, embed, &g)) return rc;
    if (n_seq == 0) return HH_OK;
    const int64_t E = embed, xb = g.rows * E * 4, need = (int64_t)g.n_wg * (4 * E * E + 4 * E) * 4;
    if (save_bytes < g.save_floats * 4 || scratch_bytes < need) {
        g_err = std::string(who) + ": save or scratch is smaller than hh_attn_block_save_bytes / hh_attn_block_scratch_bytes say";
        return HH_E_ARG;
    }
    const hca_span sp[12] = {{x, xb, false}, {w_in, 3 * E * E * 4, false}, {w_out, E * E * 4, false}, {y, xb, false}, {save, g.save_floats * 4, false},
                             {d_y, xb, false}, {d_x, xb, true}, {d_w_in, 3 * E * E * 4, true}, {d_b_in, 3 * E * 4, true}, {d_w_out, E * E * 4, true},
                             {d_b_out, E * 4, true}, {scratch, need, true}};
    if (int rc = hca_check_spans(who, sp, 12, 16)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const float *sv = static_cast<const float *>(save);
    float *sc = static_cast<float *>(scratch);
    return embed == 100 ? hab_launch_bwd<100>(g, n_seq, len, x, w_in, w_out, y, sv, d_y, d_x, d_w_in, d_b_in, d_w_out, d_b_out, sc, st)
                        : hab_launch_bwd<150>(g, n_seq, len, x, w_in, w_out, y, sv, d_y, d_x, d_w_in, d_b_in, d_w_out, d_b_out, sc, st);
}

#endif /* HH_ATTN_BLOCK_H */
