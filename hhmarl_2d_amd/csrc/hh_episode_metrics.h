/*
 * hh_episode_metrics.h — RLlib's per-iteration episode metrics of one whole-episode batch, on the device right behind the emitter
 * (C ABI, the summary's slots and the conventions: include/hh_abi.h, hh_episodes_metrics).
 *
 * One call = three launches on one stream, no host synchronisation, no allocation; the numbers of rows and episodes come from the
 * emitter's counts on the device.  Everything is float64 with a fixed summation order, no atomics:
 *   1. hh_k_epm_episodes  one wave per episode (four per workgroup, grid-stride over the table): the episode's rows are contiguous in the
 *                         batch, lane l adds rows l, l + 64, ... of every agent in order (a wave instruction reads 64 consecutive
 *                         [n_agents] rows: every byte of the lines it touches is used), then a butterfly over the 64 lanes, whose
 *                         result does not depend on the lane that reads it; lane a writes ep_return[e, a].  One lane per agent, as
 *                         hh_k_ep_gae walks its sequential chain, would add a 300-row episode on two lanes.
 *   2. hh_k_epm_rows      one workgroup per tile of HH_EPM_TILE rows (grid-stride over the tiles; the partial's place is the tile's
 *                         index, so the grid size does not matter): every lane keeps its four rows' target and target - vf in
 *                         registers, the tile's sums give the tile's means, a second sweep over the registers the squared deviations
 *                         from them; 4 n_agents doubles per tile into `scratch` (sum and M2 of target, then of target - vf).
 *   3. hh_k_epm_final     one workgroup of 256: lane t folds episodes t, t + 256, ... and tiles t, t + 256, ..., then a butterfly per wave
 *                         and the 4 waves in index order (1024 lanes spill: 128 registers each).  The tiles' M2 are combined around the global mean
 *                         (sum M2_i + n_i (mean_i - mean)^2): two passes everywhere, never E[x^2] - E[x]^2.  Writes the summary and
 *                         accumulates the totals.  It reads 8 n_agents + 4 bytes per episode on one compute unit: a batch has a few
 *                         thousand episodes (N T / mean length), the table's capacity N T is reached only if every episode had one row.
 * The bodies of 2. and 3. are the device functions hh_epm_rows_pass / hh_epm_final_fold: hh_window_metrics.h runs the same code over a
 * rollout window's T N step-rows (its own kernels hh_k_wm_rows / hh_k_wm_final), with its own rule for a call without an episode.
 * Table entries that do not lie inside the emitted rows (possible only after an emitter overflow, which the sticky flag reports) are
 * not followed: their ep_return is NaN.
 *
 * Host part: needs g_err / HIPCHK of the including translation unit (hh_world.hip).
 */
#ifndef HH_EPISODE_METRICS_H
#define HH_EPISODE_METRICS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hh_abi.h"

#define HH_EPM_TILE 1024       /* rows per partial of the row pass: 4 per lane of a 256-lane workgroup */
#define HH_EPM_MAX_GRID 2048
#define HH_EPM_FINAL 256       /* lanes of the one workgroup of the last launch */

struct hh_epm_sum { static __device__ __forceinline__ double op(double a, double b) { return a + b; } };
struct hh_epm_min { static __device__ __forceinline__ double op(double a, double b) { return fmin(a, b); } };
struct hh_epm_max { static __device__ __forceinline__ double op(double a, double b) { return fmax(a, b); } };

/* every lane of the wave gets the same bits: at each step both partners compute op(x, y) of the same unordered pair */
template <typename OP>
__device__ __forceinline__ double hh_epm_wave(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = OP::op(x, __shfl_xor(x, off, 64));
    return x;
}

/* the whole workgroup (W waves, all lanes take part): butterfly per wave, then the waves in index order; s_w: W doubles of LDS */
template <typename OP, int W>
__device__ __forceinline__ double hh_epm_block(double x, double *s_w) {
    x = hh_epm_wave<OP>(x);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    double r = s_w[0];
#pragma unroll
    for (int w = 1; w < W; w++) r = OP::op(r, s_w[w]);
    __syncthreads();   // s_w is free again
    return r;
}

__device__ __forceinline__ int hh_epm_count(const int32_t *counts, int i, int64_t cap) {
    const int c = counts[i];
    return c < 0 ? 0 : ((int64_t)c > cap ? (int)cap : c);
}

template <int NA>
__global__ __launch_bounds__(256) void hh_k_epm_episodes(hh_episode_metrics_bufs m) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_rows = hh_epm_count(m.counts, 0, m.row_cap), n_eps = hh_epm_count(m.counts, 1, m.ep_cap);
    for (int64_t e = (int64_t)blockIdx.x * 4 + wave; e < n_eps; e += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int start = m.ep_start[e], len = m.ep_len[e];
        const bool ok = start >= 0 && len > 0 && (int64_t)start + len <= n_rows;
        double acc[NA];
#pragma unroll
        for (int a = 0; a < NA; a++) acc[a] = 0.0;
        if (ok) {
            const float *__restrict__ r = m.reward + (size_t)start * NA;
            for (int i = lane; i < len; i += 64) {
#pragma unroll
                for (int a = 0; a < NA; a++) acc[a] += (double)r[(size_t)i * NA + a];
            }
        }
        double mine = 0.0;
#pragma unroll
        for (int a = 0; a < NA; a++) {
            const double s = hh_epm_wave<hh_epm_sum>(acc[a]);
            if (lane == a) mine = s;
        }
        if (lane < NA) m.ep_return[e * NA + lane] = ok ? mine : (double)NAN;
    }
}

/* the row pass over n_rows rows of target / vf [n_rows, NA] -> partial [tiles, 4 NA]; shared by hh_k_epm_rows and the window metrics'
   hh_k_wm_rows (hh_window_metrics.h), whose rows are a rollout window's T N step-rows */
template <int NA>
__device__ __forceinline__ void hh_epm_rows_pass(const int n_rows, const float *__restrict__ target, const float *__restrict__ vf,
                                                 double *__restrict__ partial) {
    __shared__ double s_w[4];
    const int tid = threadIdx.x;
    const int tiles = (n_rows + HH_EPM_TILE - 1) / HH_EPM_TILE;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // workgroup-uniform
        const int r0 = tile * HH_EPM_TILE, n = n_rows - r0 < HH_EPM_TILE ? n_rows - r0 : HH_EPM_TILE;
        double x[4][2 * NA];   // per row of this lane: target [NA], target - vf [NA]
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = tid + j * 256;
#pragma unroll
            for (int a = 0; a < NA; a++) {
                double t = 0.0, v = 0.0;
                if (i < n) {
                    t = (double)target[(size_t)(r0 + i) * NA + a];
                    v = (double)vf[(size_t)(r0 + i) * NA + a];
                }
                x[j][a] = t;
                x[j][NA + a] = t - v;
            }
        }
        double out_s = 0.0, out_q = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * NA; k++) {
            const double s = hh_epm_block<hh_epm_sum, 4>(((x[0][k] + x[1][k]) + x[2][k]) + x[3][k], s_w);   // absent rows hold 0
            const double mean = s / (double)n;
            double q = 0.0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const double d = x[j][k] - mean;
                if (tid + j * 256 < n) q += d * d;
            }
            q = hh_epm_block<hh_epm_sum, 4>(q, s_w);
            if (tid == k) { out_s = s; out_q = q; }
        }
        if (tid < 2 * NA) {
            partial[(size_t)tile * 4 * NA + (tid < NA ? tid : 2 * NA + tid - NA)] = out_s;            // [sum t | M2 t | sum d | M2 d]
            partial[(size_t)tile * 4 * NA + (tid < NA ? NA + tid : 3 * NA + tid - NA)] = out_q;
        }
    }
}

template <int NA>
__global__ __launch_bounds__(256) void hh_k_epm_rows(hh_episode_metrics_bufs m) {
    hh_epm_rows_pass<NA>(hh_epm_count(m.counts, 0, m.row_cap), m.target, m.vf, static_cast<double *>(m.scratch));
}

/* the last launch's fold of n_eps table entries and the row pass's partials of n_rows rows into the summary and the totals; shared by
   hh_k_epm_final and the window metrics' hh_k_wm_final.  WINDOW: a call without an episode still has its rows — episodes = 0, rows and
   the explained variances as always, only the episode slots NaN, totals[1] += n_rows (hh_window_metrics in include/hh_abi.h) */
template <int NA, bool WINDOW>
__device__ __forceinline__ void hh_epm_final_fold(const int n_rows, const int n_eps, const double *__restrict__ ep_return,
                                                  const int32_t *__restrict__ ep_len, const double *__restrict__ partial,
                                                  double *__restrict__ out, int64_t *__restrict__ totals) {
    __shared__ double s_w[HH_EPM_FINAL / 64];
    const int tid = threadIdx.x;
    if (!WINDOW && n_eps == 0) {
        if (tid < HH_EP_METRICS) out[tid] = tid == HH_EPM_EPISODES || tid == HH_EPM_ROWS ? 0.0 : (double)NAN;
        return;
    }
    // ---- episodes: slot 0 .. NA - 1 the agents' returns, NA their sum (the episode's reward), NA + 1 the length
    constexpr int Q = NA + 2;
    double sum[Q], lo[Q], hi[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) { sum[q] = 0.0; lo[q] = (double)INFINITY; hi[q] = -(double)INFINITY; }
    for (int e = tid; e < n_eps; e += HH_EPM_FINAL) {
        double v[Q];
        double tot = 0.0;
#pragma unroll
        for (int a = 0; a < NA; a++) {
            v[a] = ep_return[(size_t)e * NA + a];
            tot += v[a];
        }
        v[NA] = tot;
        v[NA + 1] = (double)ep_len[e];
#pragma unroll
        for (int q = 0; q < Q; q++) { sum[q] += v[q]; lo[q] = fmin(lo[q], v[q]); hi[q] = fmax(hi[q], v[q]); }
    }
#pragma unroll
    for (int q = 0; q < Q; q++) {
        sum[q] = hh_epm_block<hh_epm_sum, HH_EPM_FINAL / 64>(sum[q], s_w);
        lo[q] = hh_epm_block<hh_epm_min, HH_EPM_FINAL / 64>(lo[q], s_w);
        hi[q] = hh_epm_block<hh_epm_max, HH_EPM_FINAL / 64>(hi[q], s_w);
    }
    // ---- rows: the tiles' partials [sum t | M2 t | sum d | M2 d] (NA each) -> global means, then M2 around them
    const int tiles = (n_rows + HH_EPM_TILE - 1) / HH_EPM_TILE;
    double ev[NA];
#pragma unroll
    for (int a = 0; a < NA; a++) {
        double m2[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {   // 0: target, 1: target - vf
            double s = 0.0;
            for (int t = tid; t < tiles; t += HH_EPM_FINAL) s += partial[(size_t)t * 4 * NA + c * 2 * NA + a];
            const double mean = hh_epm_block<hh_epm_sum, HH_EPM_FINAL / 64>(s, s_w) / (double)n_rows;
            double q = 0.0;
            for (int t = tid; t < tiles; t += HH_EPM_FINAL) {
                const int n = n_rows - t * HH_EPM_TILE < HH_EPM_TILE ? n_rows - t * HH_EPM_TILE : HH_EPM_TILE;
                const double d = partial[(size_t)t * 4 * NA + c * 2 * NA + a] / (double)n - mean;
                q += partial[(size_t)t * 4 * NA + c * 2 * NA + NA + a] + (double)n * (d * d);
            }
            m2[c] = hh_epm_block<hh_epm_sum, HH_EPM_FINAL / 64>(q, s_w);
        }
        const double e = 1.0 - m2[1] / m2[0];
        ev[a] = e < -1.0 ? -1.0 : e;   // NaN (no variance in either) stays NaN
    }
    if (tid == 0) {
        const bool none = WINDOW && n_eps == 0;   // the episode slots of a window without a finished episode: NaN (0 / 0, +-inf otherwise)
        const double ne = (double)n_eps, nan = (double)NAN;
        out[HH_EPM_EPISODES] = ne;
        out[HH_EPM_ROWS] = (double)n_rows;
        out[HH_EPM_REWARD_MEAN] = none ? nan : sum[NA] / ne; out[HH_EPM_REWARD_MIN] = none ? nan : lo[NA]; out[HH_EPM_REWARD_MAX] = none ? nan : hi[NA];
        out[HH_EPM_LEN_MEAN] = none ? nan : sum[NA + 1] / ne; out[HH_EPM_LEN_MIN] = none ? nan : lo[NA + 1]; out[HH_EPM_LEN_MAX] = none ? nan : hi[NA + 1];
#pragma unroll
        for (int a = 0; a < HH_EP_METRICS_MAX_AGENTS; a++) {
            const bool on = a < NA, ep = on && !none;
            out[HH_EPM_AGENT_MEAN + a] = ep ? sum[a < NA ? a : 0] / ne : nan;
            out[HH_EPM_AGENT_MIN + a] = ep ? lo[a < NA ? a : 0] : nan;
            out[HH_EPM_AGENT_MAX + a] = ep ? hi[a < NA ? a : 0] : nan;
            out[HH_EPM_AGENT_EXPLAINED_VAR + a] = on ? ev[a < NA ? a : 0] : nan;
        }
        totals[0] += (int64_t)n_eps;
        totals[1] += (int64_t)n_rows;
    }
}

template <int NA>
__global__ __launch_bounds__(HH_EPM_FINAL) void hh_k_epm_final(hh_episode_metrics_bufs m) {
    hh_epm_final_fold<NA, false>(hh_epm_count(m.counts, 0, m.row_cap), hh_epm_count(m.counts, 1, m.ep_cap), m.ep_return, m.ep_len,
                                 static_cast<const double *>(m.scratch), m.summary, m.totals);
}

/* ---- host side ---- */

static inline int64_t hh_epm_tiles(int64_t row_cap) { return (row_cap + HH_EPM_TILE - 1) / HH_EPM_TILE; }

static int hh_epm_fail(const char *fn, const char *what) {
    g_err = std::string(fn) + ": " + what;
    return HH_E_ARG;
}

static int hh_epm_check_sizes(const char *fn, int64_t ep_cap, int64_t row_cap, int32_t n_agents) {
    if (n_agents < 1 || n_agents > HH_EP_METRICS_MAX_AGENTS) return hh_epm_fail(fn, "n_agents must be 1 .. 5");
    // row_cap + HH_EPM_TILE - 1 must fit in int: the kernels count tiles in 32-bit arithmetic
    if (row_cap < 1 || row_cap > (int64_t)INT32_MAX - HH_EPM_TILE + 1 || ep_cap < 1 || ep_cap > INT32_MAX)
        return hh_epm_fail(fn, "row_cap must be 1 .. 2^31 - 1024 and ep_cap 1 .. 2^31 - 1");
    return HH_OK;
}

extern "C" int hh_episodes_metrics_scratch_bytes(int64_t ep_cap, int64_t row_cap, int32_t n_agents, int64_t *bytes) {
    const char *fn = "hh_episodes_metrics_scratch_bytes";
    if (!bytes) return hh_epm_fail(fn, "null argument");
    const int rc = hh_epm_check_sizes(fn, ep_cap, row_cap, n_agents);
    if (rc != HH_OK) return rc;
    *bytes = hh_epm_tiles(row_cap) * 4 * n_agents * (int64_t)sizeof(double);
    return HH_OK;
}

template <int NA>
static int hh_epm_launch(const hh_episode_metrics_bufs &m, hipStream_t st) {
    const int64_t waves = (m.ep_cap + 3) / 4, tiles = hh_epm_tiles(m.row_cap);
    hipLaunchKernelGGL(hh_k_epm_episodes<NA>, dim3((unsigned)(waves < HH_EPM_MAX_GRID ? waves : HH_EPM_MAX_GRID)), dim3(256), 0, st, m);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_epm_rows<NA>, dim3((unsigned)(tiles < HH_EPM_MAX_GRID ? tiles : HH_EPM_MAX_GRID)), dim3(256), 0, st, m);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_epm_final<NA>, dim3(1), dim3(HH_EPM_FINAL), 0, st, m);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_episodes_metrics(const hh_episode_metrics_bufs *m, void *stream) {
    const char *fn = "hh_episodes_metrics";
    if (!m) return hh_epm_fail(fn, "null argument");
    if (m->reserved0 != 0) return hh_epm_fail(fn, "reserved0 must be 0");
    int rc = hh_epm_check_sizes(fn, m->ep_cap, m->row_cap, m->n_agents);
    if (rc != HH_OK) return rc;
    const void *ptrs[] = {m->reward, m->vf, m->target, m->ep_start, m->ep_len, m->counts, m->ep_return, m->summary, m->totals, m->scratch};
    for (const void *p : ptrs)
        if (!p) return hh_epm_fail(fn, "null buffer");
    if (((uintptr_t)m->reward | (uintptr_t)m->vf | (uintptr_t)m->target | (uintptr_t)m->ep_start | (uintptr_t)m->ep_len | (uintptr_t)m->counts) & 3)
        return hh_epm_fail(fn, "reward / vf / target / ep_start / ep_len / counts must be 4-byte aligned");
    if (((uintptr_t)m->ep_return | (uintptr_t)m->summary | (uintptr_t)m->totals | (uintptr_t)m->scratch) & 7)
        return hh_epm_fail(fn, "ep_return / summary / totals / scratch must be 8-byte aligned");
    if (m->scratch_bytes < hh_epm_tiles(m->row_cap) * 4 * m->n_agents * (int64_t)sizeof(double))
        return hh_epm_fail(fn, "scratch is smaller than hh_episodes_metrics_scratch_bytes(ep_cap, row_cap, n_agents)");
    hipStream_t st = (hipStream_t)stream;
    switch (m->n_agents) {
    case 1: return hh_epm_launch<1>(*m, st);
    case 2: return hh_epm_launch<2>(*m, st);
    case 3: return hh_epm_launch<3>(*m, st);
    case 4: return hh_epm_launch<4>(*m, st);
    default: return hh_epm_launch<5>(*m, st);
    }
}

#endif /* HH_EPISODE_METRICS_H */
