/*
 * hh_window_batch.h — the learners' batch geometry for batch_mode = "truncate_episodes" (C ABI: the window section of include/hh_learner.h):
 * a rollout's fixed [T, N] window cut into the sequences the learners train on (hh_window_cut) and its columns gathered into the padded
 * [S, L, ...] form (hh_window_gather).  Included from hh_world.hip (g_err, HIPCHK).
 *
 * The cut.  Arena n's rows t = 0 .. T-1 lie N step-rows apart, so ONE LANE walks one arena: at every t the 64 lanes of a wave read 64
 * neighbouring done bytes, one 64-byte line.  A sequence ends at a done row, at its L-th row, or at t = T-1.  Three launches, no atomics:
 * the walk counts every arena's sequences into scratch[n]; one workgroup turns the counts into exclusive offsets in place (tiles of 1024
 * arenas: a shuffle scan per wave, the wave sums through LDS, a running carry) and writes n_seq; the same walk again writes each arena's
 * entries from its offset.  Arena-major, then time: the order does not depend on how the workgroups are scheduled.
 *
 * The gather.  The unit of work is a SEQUENCE of one column, and a group of G = 2^g neighbouring lanes (1 .. 64, so a group never leaves
 * its wave) copies it, as hh_minibatch_stage_gather's groups copy a chunk: the destination of a sequence is one contiguous run of
 * rows x (width / unit) copy units, lane l of the group writes units l, l + G, .. of it, and unit q comes from row q / units_per_row of the
 * sequence, so the lanes of a group read consecutive units of a source row and write consecutive units.  Every lane of a group loads the
 * sequence's table entry itself — one address per group, once per sequence.  Up to four loads are in flight per lane.  The host picks G
 * per column so that a lane moves about four units.  Memory-bound, every byte once; no LDS, no atomics.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hh_learner.h"

#define HWB_THREADS 256
#define HWB_SCAN_THREADS 1024
#define HWB_MAX_BLOCKS 2048               /* workgroups per column of the gather (grid-stride beyond) */
#define HWB_MAX_WIDTH ((int64_t)1 << 20)  /* bytes of one row of a column */

/* ------------------------------------------------------------------------------------------------------------------ the cut */
template <bool WRITE>
__global__ __launch_bounds__(HWB_THREADS) void hh_k_window_walk(const uint8_t *__restrict__ done, int32_t T, int32_t N, int32_t L,
                                                                int32_t *__restrict__ scratch, int32_t *__restrict__ seq_t0,
                                                                int32_t *__restrict__ seq_arena, int32_t *__restrict__ seq_len) {
    const int32_t n = (int32_t)(blockIdx.x * HWB_THREADS + threadIdx.x);
    if (n >= N) return;
    int32_t at = WRITE ? scratch[n] : 0, len = 0;      /* WRITE: the arena's first entry (< T N: the entries of all arenas are T N at most) */
    const uint8_t *d = done + n;
#pragma unroll 4
    for (int32_t t = 0; t < T; t++) {
        const uint8_t flag = d[(int64_t)t * N];
        len++;
        if (flag != 0 || len == L || t == T - 1) {
            if (WRITE) { seq_t0[at] = t - len + 1; seq_arena[at] = n; seq_len[at] = len; }
            at++;
            len = 0;
        }
    }
    if (!WRITE) scratch[n] = at;
}

__global__ __launch_bounds__(HWB_SCAN_THREADS) void hh_k_window_scan(int32_t *__restrict__ scratch, int32_t N, int32_t *__restrict__ n_seq) {
    __shared__ int32_t wsum[HWB_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int32_t carry = 0;
    for (int32_t base = 0; base < N; base += HWB_SCAN_THREADS) {       /* uniform trip count: every thread reaches both barriers */
        const int32_t i = base + (int32_t)threadIdx.x;
        const int32_t v = i < N ? scratch[i] : 0;
        int32_t x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        int32_t pre = 0, tot = 0;
        for (int k = 0; k < HWB_SCAN_THREADS / 64; k++) {
            const int32_t s = wsum[k];
            if (k < w) pre += s;
            tot += s;
        }
        if (i < N) scratch[i] = carry + pre + x - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) n_seq[0] = carry;
}

extern "C" int hh_window_cut(int32_t T, int32_t N, const uint8_t *done, int32_t max_seq_len, int32_t *seq_t0, int32_t *seq_arena,
                             int32_t *seq_len, int32_t *n_seq, int32_t *scratch, void *stream) {
    if (T < 1 || N < 1 || (int64_t)T * N > INT32_MAX || max_seq_len < 1 || max_seq_len > HH_WINDOW_MAX_LEN || !done || !seq_t0 || !seq_arena ||
        !seq_len || !n_seq || !scratch) {
        g_err = "hh_window_cut: need T >= 1, N >= 1, T N < 2^31, 1 <= max_seq_len <= 32 and no null pointer"; return HH_E_ARG;
    }
    const unsigned blocks = (unsigned)((N + HWB_THREADS - 1) / HWB_THREADS);
    hipLaunchKernelGGL(hh_k_window_walk<false>, dim3(blocks), dim3(HWB_THREADS), 0, (hipStream_t)stream, done, T, N, max_seq_len, scratch, seq_t0,
                       seq_arena, seq_len);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_window_scan, dim3(1), dim3(HWB_SCAN_THREADS), 0, (hipStream_t)stream, scratch, N, n_seq);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_window_walk<true>, dim3(blocks), dim3(HWB_THREADS), 0, (hipStream_t)stream, done, T, N, max_seq_len, scratch, seq_t0,
                       seq_arena, seq_len);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ the gather */
struct hwb_col {
    const unsigned char *src; unsigned char *dst;
    int64_t step_bytes, offset;
    int32_t upr, rows, unit_log2, grp_log2;     /* copy units per row; rows per sequence (L, or 1 with per_seq) */
};
struct hwb_args {
    hwb_col c[HH_STAGE_MAX_COLS];
    int64_t S;
    int32_t L, T_src, N, pad;
};

template <typename U>
__device__ __forceinline__ void hwb_gather(const hwb_col &c, const hwb_args &a, const int32_t *__restrict__ seq_t0,
                                           const int32_t *__restrict__ seq_arena, const int32_t *__restrict__ seq_len) {
    const int g = c.grp_log2;
    const uint32_t G = 1u << g, lane = threadIdx.x & (G - 1);
    const uint32_t upr = (uint32_t)c.upr, ups = upr * (uint32_t)c.rows;              /* units per sequence: width <= 2^20, rows <= 32 */
    const int64_t groups = ((int64_t)gridDim.x * HWB_THREADS) >> g;
    const int64_t row_bytes = (int64_t)a.N * c.step_bytes;                          /* from step-row (t, n) to (t + 1, n) */
    const U zero{};
    for (int64_t s = ((int64_t)blockIdx.x * HWB_THREADS + threadIdx.x) >> g; s < a.S; s += groups) {
        int32_t t0 = seq_t0[s], n = seq_arena[s], len = seq_len[s];
        /* whatever the tables hold, nothing outside the column is read: such an entry stages zeros */
        if (t0 < 0 || len < 0 || len > a.L || n < 0 || n >= a.N || (int64_t)t0 + len > a.T_src) { t0 = 0; n = 0; len = 0; }
        const uint32_t n_copy = (uint32_t)(len < c.rows ? len : c.rows) * upr;
        const unsigned char *sp = c.src + ((int64_t)t0 * a.N + n) * c.step_bytes + c.offset;
        U *d = reinterpret_cast<U *>(c.dst) + s * ups;
        for (uint32_t q = lane; q < ups; q += 4 * G) {
            U v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {                                           /* the loads first: four in flight per lane */
                const uint32_t qi = q + (uint32_t)i * G;
                v[i] = zero;
                if (qi < n_copy) {
                    const uint32_t j = qi / upr, k = qi - j * upr;
                    v[i] = *reinterpret_cast<const U *>(sp + j * row_bytes + (int64_t)k * (int64_t)sizeof(U));
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t qi = q + (uint32_t)i * G;
                if (qi < ups) d[qi] = v[i];
            }
        }
    }
}

__global__ __launch_bounds__(HWB_THREADS) void hh_k_window_gather(const hwb_args a, const int32_t *__restrict__ seq_t0,
                                                                  const int32_t *__restrict__ seq_arena, const int32_t *__restrict__ seq_len) {
    const hwb_col c = a.c[blockIdx.y];
    switch (c.unit_log2) {
        case 4: hwb_gather<uint4>(c, a, seq_t0, seq_arena, seq_len); break;
        case 3: hwb_gather<uint2>(c, a, seq_t0, seq_arena, seq_len); break;
        case 2: hwb_gather<uint32_t>(c, a, seq_t0, seq_arena, seq_len); break;
        case 1: hwb_gather<uint16_t>(c, a, seq_t0, seq_arena, seq_len); break;
        default: hwb_gather<unsigned char>(c, a, seq_t0, seq_arena, seq_len); break;
    }
}

extern "C" int hh_window_gather(int32_t n_cols, const hh_window_col *cols, int64_t S, int32_t max_seq_len, int32_t T_src, int32_t N,
                                const int32_t *seq_t0, const int32_t *seq_arena, const int32_t *seq_len, void *stream) {
    if (n_cols < 1 || n_cols > HH_STAGE_MAX_COLS || !cols || S < 0 || S > INT32_MAX || max_seq_len < 1 || max_seq_len > HH_WINDOW_MAX_LEN || T_src < 1 ||
        N < 1 || !seq_t0 || !seq_arena || !seq_len) {
        g_err = "hh_window_gather: need 1 <= n_cols <= 8, 0 <= S < 2^31, 1 <= max_seq_len <= 32, T_src >= 1, N >= 1 and no null pointer"; return HH_E_ARG;
    }
    hwb_args a;
    memset(&a, 0, sizeof(a));
    a.S = S; a.L = max_seq_len; a.T_src = T_src; a.N = N;
    int64_t most = 0;
    for (int32_t i = 0; i < n_cols; i++) {
        const hh_window_col &c = cols[i];
        if (!c.src || !c.dst || c.width < 1 || c.width > HWB_MAX_WIDTH || c.offset < 0 || c.step_bytes < 1 || c.offset + c.width > c.step_bytes ||
            (c.per_seq != 0 && c.per_seq != 1) || c.reserved0 != 0) {
            g_err = "hh_window_gather: a column with a null pointer, a width outside 1 .. 2^20, a negative offset, a slice that leaves its step-row "
                    "(offset + width > step_bytes), per_seq other than 0 | 1 or a non-zero reserved field";
            return HH_E_ARG;
        }
        const uintptr_t bits = reinterpret_cast<uintptr_t>(c.src) | reinterpret_cast<uintptr_t>(c.dst) | (uintptr_t)c.step_bytes | (uintptr_t)c.offset |
                               (uintptr_t)c.width;
        int lg = 4;
        while (lg > 0 && (bits & (((uintptr_t)1 << lg) - 1))) lg--;
        const int32_t rows = c.per_seq ? 1 : max_seq_len;
        const int64_t ups = (c.width >> lg) * rows;
        int g = 0;
        while (g < 6 && ((int64_t)4 << g) < ups) g++;          /* the smallest group, up to a wave, whose lanes move at most four units each */
        a.c[i].src = (const unsigned char *)c.src; a.c[i].dst = (unsigned char *)c.dst; a.c[i].step_bytes = c.step_bytes; a.c[i].offset = c.offset;
        a.c[i].upr = (int32_t)(c.width >> lg); a.c[i].rows = rows; a.c[i].unit_log2 = lg; a.c[i].grp_log2 = g;
        const int64_t threads = S << g;
        if (threads > most) most = threads;
    }
    if (S == 0) return HH_OK;
    int64_t bx = (most + HWB_THREADS - 1) / HWB_THREADS;        /* a group per sequence of the widest column, grid-stride beyond the cap */
    if (bx > HWB_MAX_BLOCKS) bx = HWB_MAX_BLOCKS;
    hipLaunchKernelGGL(hh_k_window_gather, dim3((unsigned)bx, (unsigned)n_cols), dim3(HWB_THREADS), 0, (hipStream_t)stream, a, seq_t0, seq_arena, seq_len);
    HIPCHK(hipGetLastError());
    return HH_OK;
}
