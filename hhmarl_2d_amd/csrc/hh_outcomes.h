/*
 * hh_outcomes.h — win / lose / draw of every training episode, on the device (C ABI and the semantics: include/hh_abi.h, hh_outcome_tap
 * and hh_episode_outcomes).
 *
 * The tap.  Every step kernel writes last_outcome[n] when arena n finishes an episode (hh_episode_stats), and under auto-reset the next
 * finished episode overwrites it.  hh_k_outcome_tap copies it out right behind a tick, one lane per arena:
 * out_row[n] = done_row[n] ? last_outcome[n] : 2.  It only reads the world.
 *
 * The table.  The emitter's and hh_window_metrics' episode tables list the episodes that ended in a window arena-major, then in time: the
 * j-th done row of arena n is entry e0 + offset(n) + j, offset = the exclusive scan of the arenas' done counts, m their sum, e0 = e1 - m
 * (the window's segment is the table's last one).  One call = two launches on one stream, no host synchronisation, no allocation, no
 * atomics:
 *   1. hh_k_eo_count   ONE LANE per arena walks its T done bytes (arena n's rows lie N step-rows apart: at every t the 64 lanes of a wave
 *                      read 64 neighbouring bytes), counts its done rows and packs their outcome bytes, in time order, into
 *                      packed[j, n] (j-major: neighbouring lanes write neighbouring bytes).
 *   2. hh_k_eo_fill    one workgroup of 1024: the counts become exclusive offsets (tiles of 1024 arenas: a shuffle scan per wave, the wave
 *                      sums through LDS, a running carry — hh_k_window_scan's scheme); every lane checks ep_arena of its arenas' entries;
 *                      if all agree, the packed bytes go to ep_outcome[e0 + offset(n) + j]; then the summary over [0, e1): tiles of
 *                      HH_EO_TILE entries, one per lane, a butterfly per wave and the 16 waves in index order (hh_epm_block's order;
 *                      ten sums per tile behind two barriers), the tiles added in index order.  The work is N + m + e1 items on one compute unit: a window ends N T / (mean episode length)
 *                      episodes, a few thousand; the capacity N T is reached only if every episode had one row.
 * The order of every sum is fixed by indices alone: the same inputs give the same bytes on every run.
 * scratch: i32 [N] counts, i32 [N] offsets, i8 [T, N] packed.
 *
 * Included from hh_world.hip behind hh_episode_metrics.h (hh_epm_wave, hh_epm_fail, g_err, HIPCHK, hh_world).
 */
#ifndef HH_OUTCOMES_H
#define HH_OUTCOMES_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hh_abi.h"
#include "hh_episode_metrics.h"

#define HH_EO_THREADS 256
#define HH_EO_FILL 1024        /* lanes of the one workgroup of the second launch */
#define HH_EO_TILE HH_EO_FILL  /* table entries per tile of the summary: one per lane */
#define HH_EO_SUMS 10          /* sums of the summary: count, reward and length per class, and the entries of another code */

/* ------------------------------------------------------------------------------------------------------------------ the tap */
__global__ __launch_bounds__(256) void hh_k_outcome_tap(int N, const int8_t *__restrict__ last_outcome, const uint8_t *__restrict__ done_row,
                                                        int8_t *__restrict__ out_row) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    out_row[n] = done_row[n] != 0 ? last_outcome[n] : (int8_t)HH_OUTCOME_NONE;
}

extern "C" int hh_outcome_tap(hh_world *w, const uint8_t *done_row, int8_t *out_row, void *stream) {
    const char *fn = "hh_outcome_tap";
    if (!w || !done_row || !out_row) return hh_epm_fail(fn, "null argument");
    HH_GUARD(w);
    const int N = w->dc.N;
    hipLaunchKernelGGL(hh_k_outcome_tap, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, w->P.last_outcome, done_row, out_row);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ the table */
struct hh_eo_scratch {
    int32_t *cnt, *off;
    int8_t *packed;
};

__host__ __device__ __forceinline__ hh_eo_scratch hh_eo_split(void *scratch, int32_t N) {
    hh_eo_scratch s;
    s.cnt = static_cast<int32_t *>(scratch);
    s.off = s.cnt + N;
    s.packed = reinterpret_cast<int8_t *>(s.off + N);
    return s;
}

__global__ __launch_bounds__(HH_EO_THREADS) void hh_k_eo_count(hh_episode_outcome_bufs b) {
    const int32_t n = (int32_t)(blockIdx.x * HH_EO_THREADS + threadIdx.x);
    const int32_t T = b.T, N = b.N;
    if (n >= N) return;
    const hh_eo_scratch s = hh_eo_split(b.scratch, N);
    const uint8_t *__restrict__ d = b.done + n;
    const int8_t *__restrict__ o = b.outcome + n;
    int32_t c = 0;
#pragma unroll 4
    for (int32_t t = 0; t < T; t++) {
        if (d[(int64_t)t * N] != 0) {
            s.packed[(int64_t)c * N + n] = o[(int64_t)t * N];   /* c < T: inside [T, N] */
            c++;
        }
    }
    s.cnt[n] = c;
}

/* four arenas of one lane, FILL apart, with their counts and first entries: the loads of the four are in flight together (a lane alone would
   walk its N / 1024 arenas one dependent load after the other) */
struct hh_eo_four {
    int32_t n[4], at[4], c[4];
};

__device__ __forceinline__ hh_eo_four hh_eo_load4(const hh_eo_scratch &s, int32_t N, int32_t e0, int64_t first) {
    hh_eo_four f;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int64_t i = first + (int64_t)u * HH_EO_FILL;
        const bool in = i < N;
        f.n[u] = in ? (int32_t)i : 0;
        f.c[u] = in ? s.cnt[i] : 0;
        f.at[u] = in ? e0 + s.off[i] : 0;   /* at + c <= e0 + m = e1 <= ep_cap */
    }
    return f;
}

template <int NA>
__device__ __forceinline__ void hh_eo_entry(const hh_episode_outcome_bufs &b, int64_t e, int32_t e1, int &cls, double &rew, double &len) {
    cls = -1;   /* 0 win, 1 lose, 2 draw, 3 another code; -1: past the table */
    rew = 0.0;
    len = 0.0;
    if (e < e1) {
        const int8_t code = b.ep_outcome[e];
        cls = code == 1 ? 0 : (code == -1 ? 1 : (code == 0 ? 2 : 3));
#pragma unroll
        for (int a = 0; a < NA; a++) rew += b.ep_return[(size_t)e * NA + a];
        len = (double)b.ep_len[e];
    }
}

template <int NA>
__global__ __launch_bounds__(HH_EO_FILL) void hh_k_eo_fill(hh_episode_outcome_bufs b) {
    __shared__ int32_t wsum[HH_EO_FILL / 64];
    __shared__ double s_part[HH_EO_SUMS][HH_EO_FILL / 64];   /* the waves' sums of one tile, per slot */
    __shared__ double s_total[HH_EO_SUMS];
    __shared__ int32_t s_bad;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int32_t N = b.N;
    const hh_eo_scratch s = hh_eo_split(b.scratch, N);
    if (tid == 0) s_bad = 0;
    /* ---- the exclusive scan of the arenas' done counts; every lane ends with the total in `carry` */
    int32_t carry = 0;
    int32_t v_next = tid < N ? s.cnt[tid] : 0;
    for (int32_t base = 0; base < N; base += HH_EO_FILL) {   /* uniform trip count: every thread reaches both barriers */
        const int32_t i = base + tid;
        const int32_t v = v_next;
        const int64_t i_next = (int64_t)i + HH_EO_FILL;       /* the next tile's count is on its way while this one is scanned */
        v_next = i_next < N ? s.cnt[i_next] : 0;
        int32_t x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        int32_t pre = 0, tot = 0;
        for (int k = 0; k < HH_EO_FILL / 64; k++) {
            const int32_t sk = wsum[k];
            if (k < w) pre += sk;
            tot += sk;
        }
        if (i < N) s.off[i] = carry + pre + x - v;   /* read back below by this same lane */
        carry += tot;
        __syncthreads();
    }
    const int32_t m = carry;
    const int32_t c1 = b.n_episodes[0];
    const int32_t e1 = c1 < 0 ? 0 : ((int64_t)c1 > b.ep_cap ? (int32_t)b.ep_cap : c1);
    const int32_t e0 = e1 - m;
    /* ---- does the table's last segment hold this window's episodes?  (e0 < 0: no entry is looked at) */
    if (e0 >= 0) {
        bool bad = false;
        for (int64_t first = tid; first < N; first += 4 * HH_EO_FILL) {
            const hh_eo_four f = hh_eo_load4(s, N, e0, first);
            int32_t head[4];
#pragma unroll
            for (int u = 0; u < 4; u++) head[u] = f.c[u] > 0 ? b.ep_arena[f.at[u]] : f.n[u];   /* most arenas end 0 or 1 episodes */
#pragma unroll
            for (int u = 0; u < 4; u++) {
                bad |= head[u] != f.n[u];
                for (int32_t j = 1; j < f.c[u]; j++) bad |= b.ep_arena[f.at[u] + j] != f.n[u];
            }
        }
        if (bad) s_bad = 1;   /* every writer stores the same value */
    } else if (tid == 0) {
        s_bad = 1;
    }
    __syncthreads();
    const bool ok = s_bad == 0;
    if (tid == 0) { b.flags[0] = ok ? 0 : 1; b.flags[1] = m; }
    if (ok) {
        for (int64_t first = tid; first < N; first += 4 * HH_EO_FILL) {
            const hh_eo_four f = hh_eo_load4(s, N, e0, first);
            int8_t head[4];
#pragma unroll
            for (int u = 0; u < 4; u++) head[u] = f.c[u] > 0 ? s.packed[f.n[u]] : (int8_t)0;   /* packed[0, n] */
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (f.c[u] > 0) b.ep_outcome[f.at[u]] = head[u];
                for (int32_t j = 1; j < f.c[u]; j++) b.ep_outcome[f.at[u] + j] = s.packed[(int64_t)j * N + f.n[u]];
            }
        }
    }
    __syncthreads();   /* the entries written above are read by other lanes below */
    /* ---- the summary over [0, e1): slot q = 3 k + class for k = count, reward, length; slot 9 = codes outside -1 / 0 / 1.
       Per tile: a butterfly per wave and slot, the waves' sums through LDS, then lane q < HH_EO_SUMS adds slot q's 16 wave sums in index
       order (hh_epm_block's order) and the tile's sum to its running total: two barriers per tile, and only those lanes hold a total */
    double total = 0.0;
    int cls_next;
    double rew_next, len_next;
    hh_eo_entry<NA>(b, tid, e1, cls_next, rew_next, len_next);
    for (int32_t t0 = 0; t0 < e1; t0 += HH_EO_TILE) {   /* workgroup-uniform */
        const int cls = cls_next;
        const double rew = rew_next, len = len_next;
        hh_eo_entry<NA>(b, (int64_t)t0 + HH_EO_TILE + tid, e1, cls_next, rew_next, len_next);   /* the next tile's entry, ahead of the barriers */
#pragma unroll
        for (int q = 0; q < HH_EO_SUMS; q++) {
            const int k = q % 3;
            const double x = q == 9 ? (cls == 3 ? 1.0 : 0.0) : (cls != k ? 0.0 : (q < 3 ? 1.0 : (q < 6 ? rew : len)));
            const double r = hh_epm_wave<hh_epm_sum>(x);
            if (lane == 0) s_part[q][w] = r;
        }
        __syncthreads();
        if (tid < HH_EO_SUMS) {
            double r = s_part[tid][0];
            for (int k = 1; k < HH_EO_FILL / 64; k++) r += s_part[tid][k];
            total += r;
        }
        __syncthreads();   /* s_part is free again */
    }
    if (tid < HH_EO_SUMS) s_total[tid] = total;
    __syncthreads();
    if (tid == 0) {
        b.summary[0] = (double)e1;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double n = s_total[k];
            b.summary[1 + k] = n;
            b.summary[4 + k] = n > 0.0 ? s_total[3 + k] / n : (double)NAN;
            b.summary[7 + k] = n > 0.0 ? s_total[6 + k] / n : (double)NAN;
        }
        b.summary[10] = s_total[9];
        b.summary[11] = 0.0;
    }
}

/* ---- host side ---- */

static int hh_eo_check_sizes(const char *fn, int32_t T, int32_t N, int64_t ep_cap) {
    if (T < 1 || N < 1 || (int64_t)T * N > (int64_t)INT32_MAX - HH_EO_TILE + 1) return hh_epm_fail(fn, "need T >= 1, N >= 1 and T N <= 2^31 - 1024");
    if (ep_cap < 1 || ep_cap > (int64_t)INT32_MAX - HH_EO_TILE + 1) return hh_epm_fail(fn, "ep_cap must be 1 .. 2^31 - 1024");
    return HH_OK;
}

static inline int64_t hh_eo_scratch_size(int32_t T, int32_t N) {
    const int64_t bytes = 2 * (int64_t)N * (int64_t)sizeof(int32_t) + (int64_t)T * N;
    return (bytes + 7) & ~(int64_t)7;
}

extern "C" int hh_episode_outcomes_scratch_bytes(int32_t T, int32_t N, int64_t ep_cap, int64_t *bytes) {
    const char *fn = "hh_episode_outcomes_scratch_bytes";
    if (!bytes) return hh_epm_fail(fn, "null argument");
    const int rc = hh_eo_check_sizes(fn, T, N, ep_cap);
    if (rc != HH_OK) return rc;
    *bytes = hh_eo_scratch_size(T, N);
    return HH_OK;
}

template <int NA>
static int hh_eo_launch(const hh_episode_outcome_bufs &b, hipStream_t st) {
    hipLaunchKernelGGL(hh_k_eo_count, dim3((unsigned)((b.N + HH_EO_THREADS - 1) / HH_EO_THREADS)), dim3(HH_EO_THREADS), 0, st, b);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_eo_fill<NA>, dim3(1), dim3(HH_EO_FILL), 0, st, b);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_episode_outcomes(const hh_episode_outcome_bufs *b, void *stream) {
    const char *fn = "hh_episode_outcomes";
    if (!b) return hh_epm_fail(fn, "null argument");
    if (b->reserved0 != 0) return hh_epm_fail(fn, "reserved0 must be 0");
    if (b->n_agents < 1 || b->n_agents > HH_EP_METRICS_MAX_AGENTS) return hh_epm_fail(fn, "n_agents must be 1 .. 5");
    const int rc = hh_eo_check_sizes(fn, b->T, b->N, b->ep_cap);
    if (rc != HH_OK) return rc;
    const void *ptrs[] = {b->done, b->outcome, b->n_episodes, b->ep_arena, b->ep_len, b->ep_return, b->ep_outcome, b->summary, b->flags, b->scratch};
    for (const void *p : ptrs)
        if (!p) return hh_epm_fail(fn, "null buffer");
    if (((uintptr_t)b->n_episodes | (uintptr_t)b->ep_arena | (uintptr_t)b->ep_len | (uintptr_t)b->flags) & 3)
        return hh_epm_fail(fn, "n_episodes / ep_arena / ep_len / flags must be 4-byte aligned");
    if (((uintptr_t)b->ep_return | (uintptr_t)b->summary | (uintptr_t)b->scratch) & 7)
        return hh_epm_fail(fn, "ep_return / summary / scratch must be 8-byte aligned");
    if (b->scratch_bytes < hh_eo_scratch_size(b->T, b->N))
        return hh_epm_fail(fn, "scratch is smaller than hh_episode_outcomes_scratch_bytes(T, N, ep_cap)");
    hipStream_t st = (hipStream_t)stream;
    switch (b->n_agents) {
    case 1: return hh_eo_launch<1>(*b, st);
    case 2: return hh_eo_launch<2>(*b, st);
    case 3: return hh_eo_launch<3>(*b, st);
    case 4: return hh_eo_launch<4>(*b, st);
    default: return hh_eo_launch<5>(*b, st);
    }
}

#endif /* HH_OUTCOMES_H */
