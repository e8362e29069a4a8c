/*
 * hh_dense_tanh.h — the layer all five trainable networks share, y = tanh(x W^T + b) over the actor's and the critic's rows, and its
 * backward, for the learners (learner.dense_tanh; C ABI and the formulas: include/hh_learner.h).  Float32 in and out; the three products
 *     y   [R, N] = x [R, K] W^T          (sum over k)
 *     d_x [R, K] = d_pre [R, N] W        (sum over n)
 *     d_W [N, K] = d_pre^T x             (sum over the rows of every block)
 * run on the matrix cores as v_mfma_f32_16x16x32_f16 on an fp16 (hi, lo) split of BOTH operands: hi hi + lo hi + hi lo into float32
 * accumulators, the lo lo term (2^-22 of the product) dropped — the form of the samplers' shared layer (hh_policy_kernel_w16.h), whose
 * split (hhx_split2) and fragment order this file uses.
 *
 * One tile scheme serves all three.  A workgroup of four waves computes a P x Q block of the result, P = 128 indices on the MFMA's A side
 * (they end up in the accumulator's registers: lane (q = l & 15, g = l >> 4) holds P indices 4 g .. 4 g + 3 of a 16 x 16 tile), Q = 128
 * on its B side; wave w owns P indices 32 w .. 32 w + 31 against all of Q (64 accumulator registers).  The sum runs in chunks of 32: both operands of a chunk
 * are read from global memory as float32, scaled, split in pairs (hhx_split2), and written to LDS as [index][32 halves of the sum] (row
 * stride 40 halves: 16-byte fragment reads), hi and lo apart; what lies beyond a matrix edge is staged as 0, so any 1 <= K, N <= 512 and
 * any row count work.  An operand whose memory runs along the sum (x and W forward, d_pre for d_x) is read by 16 lanes per row; one
 * that runs across it (W for d_x, d_pre and x for d_W) by lanes along the index, and lands transposed.  No LDS-DMA (hhw_glds): it
 * copies bytes, and every operand here has to be scaled and split on its way.
 *     forward   P = output column n, Q = 128 rows;   grid (row tiles, column blocks);  epilogue unscale, bias, tanhf, store
 *     d_x       P = input column k,  Q = 128 rows;   grid (row tiles, column blocks);  d_pre = d_y (1 - y^2) formed while staging
 *     d_W       P = n, Q = 128 columns k; grid (parts, n blocks, k blocks): a workgroup walks the row tiles (64 rows) grid-stride, its
 *               sums live in registers over the walk, and go to its slot of `scratch`; a second launch adds the slots of every
 *               element in slot order in float64.  parts = min(HH_DENSE_MAX_PARTS, row tiles): no atomics, the same bytes every run.
 *               d_b: the thread that stages column n sums its d_pre in float64 on the way (k block 0 only).
 *
 * Range.  d_pre is of order advantage / n_valid, far below fp16's normal range, so it is scaled by a power of two before the
 * split and the scale is undone on the float32 result (both exact):
 *     d_x  d_pre: one scale per ROW (it factors out of the sum over n), the row's largest |d_pre| goes to [2^14, 2^15);
 *          W: one scale per COLUMN k, from a small launch of its own in front (hh_k_dense_tanh_wscale: 512 exponents in `scratch`)
 *     d_W  d_pre: one scale per row tile and column n; x: one per row tile and column k (both factor out of the sum over the tile's
 *          rows).  A tile's sums are accumulated from zero, unscaled, and added to the walk's sums in float32.
 * The second operand is scaled as well because fp16's range is short at the lower end too: the lo half of a value below 2^-3 is a
 * subnormal fp16, and an element's relative error grows as it shrinks.  Inside a long sum that is covered by the larger elements; the
 * products of a single row (d_W of one row) have nothing to hide behind.
 * The forward scales for the same reason (x per row, W per row n from a small launch in front, hh_k_dense_tanh_wscale_rows): split as
 * they are, the network's weights (|W| ~ 0.03) keep 19 bits, and the learners' gradients then miss the project's 4 x float32 rule
 * (measured: 5.2 x on Fight2).
 * What that guarantees (derivation: tests/dense_tanh_ref.py, "The extended bound").  A scale follows the LARGEST of the elements that
 * share it (a row for the forward and d_x, a column of a 64-row tile for d_W), so a staged element a is off by at most
 * max(2^-22 |a|, 2^-39 amax).  Where the elements that share a scale lie within 2^17 of each other the error bound of a product is the
 * componentwise one, (4 * 2^-22 + (n + 2) * 2^-24) |A| |B|; otherwise 2^-38 (amax_i sum_k |b_kj| + bmax_j sum_k |a_ik|) comes on top
 * of it: relative to the row's or tile column's maximum, not to the element.  A dense sum hides that term behind its larger elements;
 * a W that picks the one small column of x does not.
 * Limits.  A maximum below 2^-111 meets the clamp of hdt_sf and keeps fewer bits.  The epilogues multiply acc * un before the other
 * operand's inverse scale, and acc is up to 2^30 n, so a row of x (forward) or of d_pre (d_x), or a tile column of d_pre (d_W), with
 * a maximum above about 2^100 gives inf even where the product with a tiny W or x is representable.  No input of the learners comes
 * near either.
 */
#ifndef HH_DENSE_TANH_H
#define HH_DENSE_TANH_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hh_learner.h"

#define HDT_THREADS 256
#define HDT_P 128                   /* A-side indices per workgroup */
#define HDT_Q 128                   /* B-side indices per workgroup: rows of a forward / d_x tile, columns k of a d_W block */
#define HDT_KC 32                   /* the sum's chunk: one MFMA */
#define HDT_LD 40                   /* halves per staged row: 80 bytes, 16-byte aligned fragments */

static_assert(HH_DENSE_ROW_TILE == 2 * HDT_KC, "d_W sums a row tile in two chunks");
static_assert(HH_DENSE_FWD_SCRATCH_BYTES == HH_DENSE_MAX_DIM * 4, "one exponent per row or column of W");

struct hdt_args {
    int32_t K, N;
    int64_t rows0, rows1, tiles0, tiles;    /* rows of the two blocks; d_W's row tiles (HH_DENSE_ROW_TILE rows) of block 0 and of both */
    int64_t wtiles0, wtiles;                /* the forward's and d_x's row tiles (HDT_Q rows) of block 0 and of both */
    const float *x0, *x1;
    int64_t ld0, ld1;
    float *y0, *y1;
    const float *dy0, *dy1;
    float *dx0, *dx1;
    const float *w, *b;
};

/* the row tile `tile` of the call (tiles of tile_rows rows, tiles0 of them in block 0): which block, its first row and how many of its rows exist */
struct hdt_tile {
    bool s1;
    int64_t row0;
    int rows;
};
__device__ __forceinline__ hdt_tile hdt_pick(const hdt_args &a, int64_t tile, int tile_rows, int64_t tiles0) {
    hdt_tile t;
    t.s1 = tile >= tiles0;
    t.row0 = (t.s1 ? tile - tiles0 : tile) * tile_rows;
    const int64_t left = (t.s1 ? a.rows1 : a.rows0) - t.row0;
    t.rows = (int)(left < tile_rows ? left : tile_rows);
    return t;
}

/* power-of-two scales from a maximum's exponent field: 2^(sf - 127) takes a value of exponent field ex to [2^14, 2^15); clamped to normal numbers */
__device__ __forceinline__ int hdt_ex(float m) { return (int)((__float_as_uint(m) >> 23) & 0xffu); }
__device__ __forceinline__ int hdt_sf(int ex) {
    const int s = 268 - ex;
    return s > 253 ? 253 : s;
}
__device__ __forceinline__ float hdt_pow2(int field) { return __uint_as_float((unsigned)field << 23); }

/* one chunk of MFMAs: this wave's 32 P indices against QT tiles of 16 Q indices; acc[i][j][e] = (P 32 wave + 16 i + 4 g + e, Q 16 j + (lane & 15)) */
template <int QT>
__device__ __forceinline__ void hdt_mma(const _Float16 *Ph, const _Float16 *Pl, const _Float16 *Qh, const _Float16 *Ql, int wave, int lane,
                                        hh_f32x4 (&acc)[2][QT]) {
    const int off = (lane & 15) * HDT_LD + 8 * (lane >> 4);
    hh_h8 ah[2], al[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        ah[i] = *reinterpret_cast<const hh_h8 *>(Ph + (32 * wave + 16 * i) * HDT_LD + off);
        al[i] = *reinterpret_cast<const hh_h8 *>(Pl + (32 * wave + 16 * i) * HDT_LD + off);
    }
#pragma unroll
    for (int j = 0; j < QT; j++) {
        const hh_h8 bh = *reinterpret_cast<const hh_h8 *>(Qh + 16 * j * HDT_LD + off);
        const hh_h8 bl = *reinterpret_cast<const hh_h8 *>(Ql + 16 * j * HDT_LD + off);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            HHX_MFMA(al[i], bh, acc[i][j]);
            HHX_MFMA(ah[i], bl, acc[i][j]);
            HHX_MFMA(ah[i], bh, acc[i][j]);
        }
    }
}

/* the largest magnitude of f(0 .. n - 1) over a wave's lanes, in every lane */
template <typename F>
__device__ __forceinline__ float hdt_wave_max(int n, int lane, F f) {
    float m = 0.0f;
    for (int i = lane; i < n; i += 64) m = fmaxf(m, fabsf(f(i)));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    return m;
}

/* ---- forward: the row scales of W.  sfn[n] = the exponent field of the power of two that takes max_k |W[n, k]| to [2^14, 2^15); a wave per row ---- */
__global__ __launch_bounds__(HDT_THREADS) void hh_k_dense_tanh_wscale_rows(int K, int N, const float *__restrict__ w, int32_t *__restrict__ sfn) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * (HDT_THREADS / 64) + (threadIdx.x >> 6);
    if (n >= N) return;
    const float m = hdt_wave_max(K, lane, [&](int k) { return w[(int64_t)n * K + k]; });
    if (lane == 0) sfn[n] = hdt_sf(hdt_ex(m));
}

/* a pair of one staged row: p[0], p[1], zero from column `left` on (left >= 2: both exist); vec2: p is 8-byte aligned */
__device__ __forceinline__ hh_f2 hdt_pair(const float *__restrict__ p, int left, bool vec2) {
    if (left >= 2) {
        if (vec2) return *reinterpret_cast<const hh_f2 *>(p);
        return hh_f2{p[0], p[1]};
    }
    return hh_f2{left >= 1 ? p[0] : 0.0f, 0.0f};
}
__device__ __forceinline__ void hdt_put(_Float16 *H, _Float16 *Lo, int at, hh_f2 v) {
    unsigned hi, lo;
    hhx_split2(v, hi, lo);
    *reinterpret_cast<unsigned *>(H + at) = hi;
    *reinterpret_cast<unsigned *>(Lo + at) = lo;
}

/* ---- forward ----
 * Staging without per-element edge tests: a row beyond the matrix reads the last real row with scale 0 (its products land in accumulators nobody stores),
 * and only the last chunk of the sum tests its columns. */
__global__ __launch_bounds__(HDT_THREADS) void hh_k_dense_tanh_fwd(hdt_args a, const int32_t *__restrict__ sfn) {
    __shared__ __attribute__((aligned(16))) _Float16 Ph[HDT_P * HDT_LD], Pl[HDT_P * HDT_LD], Qh[HDT_Q * HDT_LD], Ql[HDT_Q * HDT_LD];
    __shared__ __attribute__((aligned(16))) float scl[HDT_Q], inv[HDT_Q], sclw[HDT_P], invw[HDT_P];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const hdt_tile tl = hdt_pick(a, blockIdx.x, HDT_Q, a.wtiles0);
    const float *__restrict__ x = tl.s1 ? a.x1 : a.x0;
    const int64_t ld = tl.s1 ? a.ld1 : a.ld0;
    float *__restrict__ y = tl.s1 ? a.y1 : a.y0;
    const float *__restrict__ w = a.w;
    const int K = a.K, N = a.N, n0 = blockIdx.y * HDT_P, rows = tl.rows;
    const int64_t row0 = tl.row0;
    if (t < HDT_P) {
        const bool on = n0 + t < N;
        const int sf = on ? sfn[n0 + t] : 127;
        sclw[t] = on ? hdt_pow2(sf) : 0.0f;
        invw[t] = hdt_pow2(254 - sf);
    }
    /* the row scales of x: wave w takes rows 32 w .. 32 w + 31, its lanes along k */
    for (int u = 0; u < HDT_Q / 4; u++) {
        const int q = (HDT_Q / 4) * wave + u;
        const float m = q < rows ? hdt_wave_max(K, lane, [&](int k) { return x[(row0 + q) * ld + k]; }) : 0.0f;
        if (lane == 0) {
            const int sf = hdt_sf(hdt_ex(m));
            scl[q] = q < rows ? hdt_pow2(sf) : 0.0f;
            inv[q] = hdt_pow2(254 - sf);
        }
    }
    __syncthreads();
    const int sp2 = 2 * (t & 15), r0 = t >> 4;
    const float *wp[8], *xp[8];
    float ws[8], xs[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int p = r0 + 16 * j, n = n0 + p < N ? n0 + p : N - 1, r = p < rows ? p : rows - 1;
        wp[j] = w + (int64_t)n * K + sp2;
        xp[j] = x + (row0 + r) * ld + sp2;
        ws[j] = sclw[p];
        xs[j] = scl[p];
    }
    const bool wv2 = ((uintptr_t)w & 7) == 0 && (K & 1) == 0, xv2 = ((uintptr_t)x & 7) == 0 && (ld & 1) == 0;
    hh_f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) acc[i][j] = hh_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < K; k0 += HDT_KC) {
        const int left = k0 + HDT_KC <= K ? 2 : K - k0 - sp2;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int at = (r0 + 16 * j) * HDT_LD + sp2;
            hdt_put(Ph, Pl, at, hdt_pair(wp[j] + k0, left, wv2) * ws[j]);
            hdt_put(Qh, Ql, at, hdt_pair(xp[j] + k0, left, xv2) * xs[j]);
        }
        __syncthreads();
        hdt_mma<8>(Ph, Pl, Qh, Ql, wave, lane, acc);
        __syncthreads();
    }
    const int g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int pl = 32 * wave + 16 * i + 4 * g, n = n0 + pl;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int q = 16 * j + (lane & 15);
            if (q < rows) {
                const float un = inv[q];
                float *yo = y + (row0 + q) * N + n;
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (n + e < N) yo[e] = tanhf(acc[i][j][e] * un * invw[pl + e] + a.b[n + e]);
            }
        }
    }
}

/* ---- backward: the column scales of W for d_x.  sfk[k] = the exponent field of the power of two that takes max_n |W[n, k]| to [2^14, 2^15) ---- */
__global__ __launch_bounds__(HDT_THREADS) void hh_k_dense_tanh_wscale_cols(int K, int N, const float *__restrict__ w, int32_t *__restrict__ sfk) {
    __shared__ float cm[HDT_THREADS];
    const int t = threadIdx.x, k = blockIdx.x * 64 + (t & 63);
    float m = 0.0f;
    if (k < K)
        for (int n = t >> 6; n < N; n += HDT_THREADS / 64) m = fmaxf(m, fabsf(w[(int64_t)n * K + k]));
    cm[t] = m;
    __syncthreads();
    if (t < 64 && k < K) sfk[k] = hdt_sf(hdt_ex(fmaxf(fmaxf(cm[t], cm[t + 64]), fmaxf(cm[t + 128], cm[t + 192]))));
}

/* ---- backward: d_x (staged like the forward: rows beyond an edge read a real row with scale 0) ---- */
__global__ __launch_bounds__(HDT_THREADS) void hh_k_dense_tanh_dx(hdt_args a, const int32_t *__restrict__ sfk) {
    __shared__ __attribute__((aligned(16))) _Float16 Ph[HDT_P * HDT_LD], Pl[HDT_P * HDT_LD], Qh[HDT_Q * HDT_LD], Ql[HDT_Q * HDT_LD];
    __shared__ __attribute__((aligned(16))) float scl[HDT_Q], inv[HDT_Q], sclk[HDT_P], invk[HDT_P];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const hdt_tile tl = hdt_pick(a, blockIdx.x, HDT_Q, a.wtiles0);
    const float *__restrict__ yv = tl.s1 ? a.y1 : a.y0;
    const float *__restrict__ dy = tl.s1 ? a.dy1 : a.dy0;
    float *__restrict__ dx = tl.s1 ? a.dx1 : a.dx0;
    const float *__restrict__ w = a.w;
    const int K = a.K, N = a.N, kb = blockIdx.y * HDT_P, rows = tl.rows;
    const int64_t row0 = tl.row0;
    if (t < HDT_P) {
        const bool on = kb + t < K;
        const int sf = on ? sfk[kb + t] : 127;
        sclk[t] = on ? hdt_pow2(sf) : 0.0f;
        invk[t] = hdt_pow2(254 - sf);
    }
    /* the row scales: wave w takes rows 32 w .. 32 w + 31, its lanes along n */
    for (int u = 0; u < HDT_Q / 4; u++) {
        const int q = (HDT_Q / 4) * wave + u;
        const float m = q < rows ? hdt_wave_max(N, lane, [&](int n) {
            const float yy = yv[(row0 + q) * N + n];
            return dy[(row0 + q) * N + n] * (1.0f - yy * yy);
        }) : 0.0f;
        if (lane == 0) {
            const int sf = hdt_sf(hdt_ex(m));
            scl[q] = q < rows ? hdt_pow2(sf) : 0.0f;
            inv[q] = hdt_pow2(254 - sf);
        }
    }
    __syncthreads();
    /* W lands transposed: this thread's column k of W, rows n0 + 2 (sh + 2 j), + 1 */
    const int pc = t & (HDT_P - 1), sh = t >> 7;
    const float *wc = w + (kb + pc < K ? kb + pc : K - 1) + (int64_t)(2 * sh) * K;
    const float wsc = sclk[pc];
    /* d_pre: rows r0 + 16 j, columns n0 + sp2, + 1 */
    const int sp2 = 2 * (t & 15), r0 = t >> 4;
    int64_t qo[8];
    float qs[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int q = r0 + 16 * j;
        qo[j] = (row0 + (q < rows ? q : rows - 1)) * N + sp2;
        qs[j] = scl[q];
    }
    const bool v2 = ((uintptr_t)yv & 7) == 0 && ((uintptr_t)dy & 7) == 0 && (N & 1) == 0;
    hh_f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) acc[i][j] = hh_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int n0 = 0; n0 < N; n0 += HDT_KC) {
        const bool full = n0 + HDT_KC <= N;
        const int left = full ? 2 : N - n0 - sp2;
        const float *wn = wc + (int64_t)n0 * K;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int s = 2 * (sh + 2 * j);
            const float *p = wn + (int64_t)(4 * j) * K;
            hh_f2 wv;
            if (full) wv = hh_f2{p[0], p[K]};
            else wv = hh_f2{n0 + s < N ? p[0] : 0.0f, n0 + s + 1 < N ? p[K] : 0.0f};
            hdt_put(Ph, Pl, pc * HDT_LD + s, wv * wsc);
            const hh_f2 yy = hdt_pair(yv + qo[j] + n0, left, v2), gg = hdt_pair(dy + qo[j] + n0, left, v2);
            hdt_put(Qh, Ql, (r0 + 16 * j) * HDT_LD + sp2, gg * (1.0f - yy * yy) * qs[j]);
        }
        __syncthreads();
        hdt_mma<8>(Ph, Pl, Qh, Ql, wave, lane, acc);
        __syncthreads();
    }
    const int g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int pl = 32 * wave + 16 * i + 4 * g, k = kb + pl;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int q = 16 * j + (lane & 15);
            if (q < rows) {
                const float un = inv[q];
                float *o = dx + (row0 + q) * K + k;
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (k + e < K) o[e] = acc[i][j][e] * un * invk[pl + e];
            }
        }
    }
}

/* ---- backward: d_W and d_b, pass 1.  Slot blockIdx.x of part ([parts][N K + N]) = this workgroup's sums over its row tiles ---- */
/* this thread's 32 elements of a [64 rows][128 columns] tile of an operand of d_W: column pc, rows 32 c + 2 (sp0 + 2 j) + e -> their largest magnitude */
template <typename F>
__device__ __forceinline__ float hdt_tile_column(float (&v)[2][8][2], int sp0, F f) {
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                v[c][j][e] = f(32 * c + 2 * (sp0 + 2 * j) + e);
                m = fmaxf(m, fabsf(v[c][j][e]));
            }
    return m;
}
/* chunk c of those elements, scaled, into row pc of an LDS operand */
__device__ __forceinline__ void hdt_stage_column(_Float16 *H, _Float16 *Lo, const float (&v)[8][2], float scale, int pc, int sp0) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int sp = sp0 + 2 * j;
        const hh_f2 pv = {v[j][0] * scale, v[j][1] * scale};
        unsigned hi, lo;
        hhx_split2(pv, hi, lo);
        *reinterpret_cast<unsigned *>(H + pc * HDT_LD + 2 * sp) = hi;
        *reinterpret_cast<unsigned *>(Lo + pc * HDT_LD + 2 * sp) = lo;
    }
}

__global__ __launch_bounds__(HDT_THREADS) void hh_k_dense_tanh_dw(hdt_args a, float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) _Float16 Ph[HDT_P * HDT_LD], Pl[HDT_P * HDT_LD], Qh[HDT_P * HDT_LD], Ql[HDT_P * HDT_LD];
    __shared__ __attribute__((aligned(16))) float cm[HDT_THREADS], cx[HDT_THREADS], invn[HDT_P], invk[HDT_P];
    __shared__ double cs[HDT_THREADS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4;
    const int K = a.K, N = a.N, n0 = blockIdx.y * HDT_P, kb = blockIdx.z * HDT_P;
    const int pc = t & (HDT_P - 1), sp0 = t >> 7;      /* the column of d_pre and of x this thread stages, with thread t ^ 128 */
    const int n = n0 + pc, k = kb + pc;
    double bsum = 0.0;
    hh_f32x4 tot[2][8];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) tot[i][j] = hh_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const hdt_tile tl = hdt_pick(a, tile, HH_DENSE_ROW_TILE, a.tiles0);
        const float *__restrict__ x = tl.s1 ? a.x1 : a.x0;
        const int64_t ld = tl.s1 ? a.ld1 : a.ld0;
        const float *__restrict__ yv = tl.s1 ? a.y1 : a.y0;
        const float *__restrict__ dy = tl.s1 ? a.dy1 : a.dy0;
        const int rows = tl.rows;
        const int64_t row0 = tl.row0;
        float v[2][8][2], xv[2][8][2];
        const float mv = hdt_tile_column(v, sp0, [&](int r) {
            if (!(r < rows && n < N)) return 0.0f;
            const int64_t at = (row0 + r) * N + n;
            const float yy = yv[at];
            return dy[at] * (1.0f - yy * yy);
        });
        const float mx = hdt_tile_column(xv, sp0, [&](int r) { return r < rows && k < K ? x[(row0 + r) * ld + k] : 0.0f; });
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int j = 0; j < 8; j++) s += (double)v[c][j][0] + (double)v[c][j][1];
        bsum += s;
        cm[t] = mv;
        cx[t] = mx;
        __syncthreads();
        /* one scale per column of the tile, for either operand: it factors out of the sum over the tile's rows */
        const int sfn = hdt_sf(hdt_ex(fmaxf(mv, cm[t ^ HDT_P]))), sfx = hdt_sf(hdt_ex(fmaxf(mx, cx[t ^ HDT_P])));
        if (t < HDT_P) {
            invn[t] = hdt_pow2(254 - sfn);
            invk[t] = hdt_pow2(254 - sfx);
        }
        hh_f32x4 acc[2][8];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 8; j++) acc[i][j] = hh_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 2; c++) {
            hdt_stage_column(Ph, Pl, v[c], hdt_pow2(sfn), pc, sp0);
            hdt_stage_column(Qh, Ql, xv[c], hdt_pow2(sfx), pc, sp0);
            __syncthreads();
            hdt_mma<8>(Ph, Pl, Qh, Ql, wave, lane, acc);
            __syncthreads();
        }
        /* the tile's sums, unscaled (exact), onto the walk's */
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float4 un = *reinterpret_cast<const float4 *>(invn + 32 * wave + 16 * i + 4 * g);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float uk = invk[16 * j + (lane & 15)];
                tot[i][j][0] = fmaf(acc[i][j][0] * un.x, uk, tot[i][j][0]);
                tot[i][j][1] = fmaf(acc[i][j][1] * un.y, uk, tot[i][j][1]);
                tot[i][j][2] = fmaf(acc[i][j][2] * un.z, uk, tot[i][j][2]);
                tot[i][j][3] = fmaf(acc[i][j][3] * un.w, uk, tot[i][j][3]);
            }
        }
    }
    cs[t] = bsum;
    __syncthreads();
    const int64_t entries = (int64_t)N * K + N;
    float *slot = part + (int64_t)blockIdx.x * entries;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int pl = n0 + 32 * wave + 16 * i + 4 * g;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int kk = kb + 16 * j + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (pl + e < N && kk < K) slot[(int64_t)(pl + e) * K + kk] = tot[i][j][e];
        }
    }
    if (blockIdx.z == 0 && t < HDT_P && n < N) slot[(int64_t)N * K + n] = (float)(cs[t] + cs[t + HDT_P]);
}

/* pass 2: element e of [d_W | d_b] = the sum of the slots in slot order */
__global__ __launch_bounds__(HDT_THREADS) void hh_k_dense_tanh_reduce(int64_t nk, int64_t entries, int parts, const float *__restrict__ part,
                                                                      float *__restrict__ d_w, float *__restrict__ d_b) {
    const int64_t e = (int64_t)blockIdx.x * HDT_THREADS + threadIdx.x;
    if (e >= entries) return;
    double sum = part[e];
    for (int p = 1; p < parts; p++) sum += (double)part[(int64_t)p * entries + e];
    if (e < nk) d_w[e] = (float)sum;
    else d_b[e - nk] = (float)sum;
}

/* ---- the C ABI ---- */
static int64_t hdt_tiles(int64_t n_rows) { return (n_rows + HH_DENSE_ROW_TILE - 1) / HH_DENSE_ROW_TILE; }

/* the checks every call shares; fills the sizes of `a` */
static int hdt_check(const char *who, int32_t K, int32_t N, int32_t n_src, const hh_dense_src *src, bool need_ld, hdt_args *a) {
    const std::string w(who);
    if (K < 1 || K > HH_DENSE_MAX_DIM || N < 1 || N > HH_DENSE_MAX_DIM) { g_err = w + ": 1 <= K, N <= HH_DENSE_MAX_DIM"; return HH_E_ARG; }
    if (n_src < 1 || n_src > HH_DENSE_MAX_SRC || !src) { g_err = w + ": 1 .. HH_DENSE_MAX_SRC row blocks"; return HH_E_ARG; }
    memset(a, 0, sizeof(*a));
    a->K = K;
    a->N = N;
    for (int i = 0; i < n_src; i++) {
        if (src[i].n_rows < 0 || src[i].n_rows > ((int64_t)1 << 36)) { g_err = w + ": 0 <= n_rows <= 2^36"; return HH_E_ARG; }
        if (need_ld && (src[i].ld < K || src[i].ld > ((int64_t)1 << 40))) { g_err = w + ": ld < K"; return HH_E_ARG; }
    }
    a->rows0 = src[0].n_rows;
    a->rows1 = n_src > 1 ? src[1].n_rows : 0;
    a->tiles0 = hdt_tiles(a->rows0);
    a->tiles = a->tiles0 + hdt_tiles(a->rows1);
    a->wtiles0 = (a->rows0 + HDT_Q - 1) / HDT_Q;
    a->wtiles = a->wtiles0 + (a->rows1 + HDT_Q - 1) / HDT_Q;
    if (a->tiles > 0x7fffffff) { g_err = w + ": too many rows"; return HH_E_ARG; }
    a->x0 = src[0].x; a->ld0 = src[0].ld; a->y0 = src[0].y; a->dy0 = src[0].d_y; a->dx0 = src[0].d_x;
    if (n_src > 1) { a->x1 = src[1].x; a->ld1 = src[1].ld; a->y1 = src[1].y; a->dy1 = src[1].d_y; a->dx1 = src[1].d_x; }
    return HH_OK;
}

static int64_t hdt_parts(int64_t tiles) { return tiles < HH_DENSE_MAX_PARTS ? tiles : HH_DENSE_MAX_PARTS; }

extern "C" int hh_dense_tanh_scratch_bytes(int32_t K, int32_t N, int32_t n_src, const hh_dense_src *src, int64_t *bytes) {
    hdt_args a;
    if (!bytes) { g_err = "hh_dense_tanh_scratch_bytes: null argument"; return HH_E_ARG; }
    if (int rc = hdt_check("hh_dense_tanh_scratch_bytes", K, N, n_src, src, false, &a)) return rc;
    const int64_t parts = hdt_parts(a.tiles);
    *bytes = HH_DENSE_FWD_SCRATCH_BYTES + (parts < 1 ? 1 : parts) * ((int64_t)N * K + N) * 4;
    return HH_OK;
}

extern "C" int hh_dense_tanh_forward(int32_t K, int32_t N, int32_t n_src, const hh_dense_src *src, const float *w, const float *b, void *scratch,
                                     int64_t scratch_bytes, void *stream) {
    hdt_args a;
    if (int rc = hdt_check("hh_dense_tanh_forward", K, N, n_src, src, true, &a)) return rc;
    if (a.tiles == 0) return HH_OK;
    bool null = !w || !b || !scratch;
    for (int i = 0; i < n_src; i++) null = null || (src[i].n_rows > 0 && (!src[i].x || !src[i].y));
    if (null) { g_err = "hh_dense_tanh_forward: null argument"; return HH_E_ARG; }
    if (scratch_bytes < HH_DENSE_FWD_SCRATCH_BYTES) { g_err = "hh_dense_tanh_forward: scratch smaller than HH_DENSE_FWD_SCRATCH_BYTES"; return HH_E_ARG; }
    a.w = w;
    a.b = b;
    int32_t *sfn = static_cast<int32_t *>(scratch);                            /* W's row scales */
    hipLaunchKernelGGL(hh_k_dense_tanh_wscale_rows, dim3((unsigned)((N + 3) / 4)), dim3(HDT_THREADS), 0, (hipStream_t)stream, K, N, w, sfn);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_dense_tanh_fwd, dim3((unsigned)a.wtiles, (unsigned)((N + HDT_P - 1) / HDT_P)), dim3(HDT_THREADS), 0, (hipStream_t)stream, a, sfn);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_dense_tanh_backward(int32_t K, int32_t N, int32_t n_src, const hh_dense_src *src, const float *w, float *d_w, float *d_b,
                                      void *scratch, int64_t scratch_bytes, void *stream) {
    hdt_args a;
    if (int rc = hdt_check("hh_dense_tanh_backward", K, N, n_src, src, true, &a)) return rc;
    if (a.tiles == 0) return HH_OK;
    bool null = !w || !d_w || !d_b || !scratch;
    for (int i = 0; i < n_src; i++) null = null || (src[i].n_rows > 0 && (!src[i].x || !src[i].y || !src[i].d_y || !src[i].d_x));
    if (null) { g_err = "hh_dense_tanh_backward: null argument"; return HH_E_ARG; }
    const int64_t parts = hdt_parts(a.tiles), nk = (int64_t)N * K, entries = nk + N;
    if (scratch_bytes < HH_DENSE_FWD_SCRATCH_BYTES + parts * entries * 4) { g_err = "hh_dense_tanh_backward: scratch too small (hh_dense_tanh_scratch_bytes)"; return HH_E_ARG; }
    a.w = w;
    hipStream_t st = (hipStream_t)stream;
    float *part = reinterpret_cast<float *>(static_cast<char *>(scratch) + HH_DENSE_FWD_SCRATCH_BYTES);  /* behind the scales: the slots */
    int32_t *sfk = static_cast<int32_t *>(scratch);                            /* W's column scales */
    hipLaunchKernelGGL(hh_k_dense_tanh_wscale_cols, dim3((unsigned)((K + 63) / 64)), dim3(HDT_THREADS), 0, st, K, N, w, sfk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_dense_tanh_dx, dim3((unsigned)a.wtiles, (unsigned)((K + HDT_P - 1) / HDT_P)), dim3(HDT_THREADS), 0, st, a, sfk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_dense_tanh_dw, dim3((unsigned)parts, (unsigned)((N + HDT_P - 1) / HDT_P), (unsigned)((K + HDT_P - 1) / HDT_P)), dim3(HDT_THREADS), 0,
                       st, a, part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_dense_tanh_reduce, dim3((unsigned)((entries + HDT_THREADS - 1) / HDT_THREADS)), dim3(HDT_THREADS), 0, st, nk, entries, (int)parts,
                       part, d_w, d_b);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

#endif /* HH_DENSE_TANH_H */
