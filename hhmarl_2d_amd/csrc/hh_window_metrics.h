/*
 * hh_window_metrics.h — RLlib's per-iteration episode metrics for fixed-window rollouts (batch_mode = "truncate_episodes"), on the device
 * right behind the window's GAE (C ABI and the semantics: include/hh_abi.h, hh_window_metrics; the summary's slots are
 * hh_episodes_metrics').
 *
 * A window cuts episodes, so every arena carries the return and the length of its running episode across calls (run_return f64 [N,
 * n_agents], run_len i32 [N]); the episodes that finish inside a window are tabulated, arena-major then t, and summarised.  One call =
 * five launches on one stream, no host synchronisation, no allocation, no atomics:
 *   1. hh_k_wm_walk<NA, false>  ONE LANE per arena walks its T done bytes (arena n's rows lie N step-rows apart: at every t the 64 lanes
 *                               of a wave read 64 neighbouring bytes) and counts its done rows into scratch.
 *   2. hh_k_window_scan         hh_window_cut's one workgroup (hh_window_batch.h): the N counts become exclusive offsets in place, their
 *                               sum goes to counts[0].
 *   3. hh_k_wm_walk<NA, true>   the same walk with the carry in registers: run_return[a] += (double)reward[t, n, a], ONE float64 addition
 *                               per row in time order (a host restatement that adds the same way gives the same bits, whatever the window
 *                               length: the sum of an episode does not depend on where the windows cut it), run_len += 1; at a done row
 *                               the arena's next table entry is written from its offset and both go back to 0.  Adjacent lanes read
 *                               adjacent [n_agents] rows of reward.  Writes the carry back and counts[1] = T N.
 *   4. hh_k_wm_rows             hh_episode_metrics.h's row pass (hh_epm_rows_pass) over the window's T N step-rows: target and vf[:T]
 *                               are already flat [T N, n_agents] columns.
 *   5. hh_k_wm_final            hh_episode_metrics.h's fold (hh_epm_final_fold<NA, true>) of the table and the tile partials.
 * The order of every sum is fixed by indices alone (arena, t, tile, lane), never by how the workgroups are scheduled: the same inputs
 * give the same bytes on every run and for every grid size.
 * scratch: [tiles, 4 n_agents] f64 partials of the row pass, then i32 [N] counts / offsets.
 *
 * Included from hh_world.hip behind hh_episode_metrics.h and hh_window_batch.h (g_err, HIPCHK).
 */
#ifndef HH_WINDOW_METRICS_H
#define HH_WINDOW_METRICS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hh_abi.h"
#include "hh_episode_metrics.h"
#include "hh_window_batch.h"

#define HH_WM_THREADS 256

__device__ __forceinline__ int32_t *hh_wm_offsets(const hh_window_metrics_bufs &m) {
    const int64_t tiles = ((int64_t)m.T * m.N + HH_EPM_TILE - 1) / HH_EPM_TILE;
    return reinterpret_cast<int32_t *>(static_cast<double *>(m.scratch) + tiles * 4 * m.n_agents);
}

template <int NA, bool WRITE>
__global__ __launch_bounds__(HH_WM_THREADS) void hh_k_wm_walk(hh_window_metrics_bufs m) {
    const int32_t n = (int32_t)(blockIdx.x * HH_WM_THREADS + threadIdx.x);
    const int32_t T = m.T, N = m.N;
    if (n >= N) return;
    int32_t *__restrict__ offsets = hh_wm_offsets(m);
    const uint8_t *__restrict__ d = m.done + n;
    if (!WRITE) {
        int32_t c = 0;
#pragma unroll 4
        for (int32_t t = 0; t < T; t++) c += d[(int64_t)t * N] != 0;
        offsets[n] = c;
        return;
    }
    int32_t at = offsets[n], len = m.run_len[n];   /* at + this arena's done rows <= counts[0] <= T N: the table cannot overflow */
    double ret[NA];
#pragma unroll
    for (int a = 0; a < NA; a++) ret[a] = m.run_return[(size_t)n * NA + a];
    const float *__restrict__ r = m.reward + (size_t)n * NA;
#pragma unroll 4
    for (int32_t t = 0; t < T; t++) {
        const uint8_t flag = d[(int64_t)t * N];
#pragma unroll
        for (int a = 0; a < NA; a++) ret[a] += (double)r[(size_t)t * N * NA + a];
        len++;
        if (flag != 0) {
#pragma unroll
            for (int a = 0; a < NA; a++) { m.ep_return[(size_t)at * NA + a] = ret[a]; ret[a] = 0.0; }
            m.ep_len[at] = len; m.ep_arena[at] = n; m.ep_end[at] = t;
            at++;
            len = 0;
        }
    }
#pragma unroll
    for (int a = 0; a < NA; a++) m.run_return[(size_t)n * NA + a] = ret[a];
    m.run_len[n] = len;
    if (n == 0) m.counts[1] = T * N;
}

template <int NA>
__global__ __launch_bounds__(256) void hh_k_wm_rows(hh_window_metrics_bufs m) {
    hh_epm_rows_pass<NA>(m.T * m.N, m.target, m.vf, static_cast<double *>(m.scratch));
}

template <int NA>
__global__ __launch_bounds__(HH_EPM_FINAL) void hh_k_wm_final(hh_window_metrics_bufs m) {
    hh_epm_final_fold<NA, true>(m.T * m.N, hh_epm_count(m.counts, 0, (int64_t)m.T * m.N), m.ep_return, m.ep_len,
                                static_cast<const double *>(m.scratch), m.summary, m.totals);
}

/* ---- host side ---- */

static int hh_wm_check_sizes(const char *fn, int32_t T, int32_t N, int32_t n_agents) {
    if (n_agents < 1 || n_agents > HH_EP_METRICS_MAX_AGENTS) return hh_epm_fail(fn, "n_agents must be 1 .. 5");
    // T N + HH_EPM_TILE - 1 must fit in int: the kernels count rows and tiles in 32-bit arithmetic
    if (T < 1 || N < 1 || (int64_t)T * N > (int64_t)INT32_MAX - HH_EPM_TILE + 1) return hh_epm_fail(fn, "need T >= 1, N >= 1 and T N <= 2^31 - 1024");
    return HH_OK;
}

static inline int64_t hh_wm_scratch(int32_t T, int32_t N, int32_t n_agents) {
    const int64_t bytes = hh_epm_tiles((int64_t)T * N) * 4 * n_agents * (int64_t)sizeof(double) + (int64_t)N * (int64_t)sizeof(int32_t);
    return (bytes + 7) & ~(int64_t)7;
}

extern "C" int hh_window_metrics_scratch_bytes(int32_t T, int32_t N, int32_t n_agents, int64_t *bytes) {
    const char *fn = "hh_window_metrics_scratch_bytes";
    if (!bytes) return hh_epm_fail(fn, "null argument");
    const int rc = hh_wm_check_sizes(fn, T, N, n_agents);
    if (rc != HH_OK) return rc;
    *bytes = hh_wm_scratch(T, N, n_agents);
    return HH_OK;
}

template <int NA>
static int hh_wm_launch(const hh_window_metrics_bufs &m, hipStream_t st) {
    const unsigned arenas = (unsigned)((m.N + HH_WM_THREADS - 1) / HH_WM_THREADS);
    const int64_t tiles = hh_epm_tiles((int64_t)m.T * m.N);
    int32_t *offsets = reinterpret_cast<int32_t *>(static_cast<double *>(m.scratch) + tiles * 4 * NA);
    hipLaunchKernelGGL((hh_k_wm_walk<NA, false>), dim3(arenas), dim3(HH_WM_THREADS), 0, st, m);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_window_scan, dim3(1), dim3(HWB_SCAN_THREADS), 0, st, offsets, m.N, m.counts);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((hh_k_wm_walk<NA, true>), dim3(arenas), dim3(HH_WM_THREADS), 0, st, m);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_wm_rows<NA>, dim3((unsigned)(tiles < HH_EPM_MAX_GRID ? tiles : HH_EPM_MAX_GRID)), dim3(256), 0, st, m);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_wm_final<NA>, dim3(1), dim3(HH_EPM_FINAL), 0, st, m);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_window_metrics(const hh_window_metrics_bufs *m, void *stream) {
    const char *fn = "hh_window_metrics";
    if (!m) return hh_epm_fail(fn, "null argument");
    if (m->reserved0 != 0) return hh_epm_fail(fn, "reserved0 must be 0");
    const int rc = hh_wm_check_sizes(fn, m->T, m->N, m->n_agents);
    if (rc != HH_OK) return rc;
    const void *ptrs[] = {m->reward, m->vf, m->target, m->done, m->run_return, m->run_len, m->ep_return, m->ep_len, m->ep_arena, m->ep_end,
                          m->counts, m->summary, m->totals, m->scratch};
    for (const void *p : ptrs)
        if (!p) return hh_epm_fail(fn, "null buffer");
    if (((uintptr_t)m->reward | (uintptr_t)m->vf | (uintptr_t)m->target | (uintptr_t)m->run_len | (uintptr_t)m->ep_len | (uintptr_t)m->ep_arena |
         (uintptr_t)m->ep_end | (uintptr_t)m->counts) & 3)
        return hh_epm_fail(fn, "reward / vf / target / run_len / ep_len / ep_arena / ep_end / counts must be 4-byte aligned");
    if (((uintptr_t)m->run_return | (uintptr_t)m->ep_return | (uintptr_t)m->summary | (uintptr_t)m->totals | (uintptr_t)m->scratch) & 7)
        return hh_epm_fail(fn, "run_return / ep_return / summary / totals / scratch must be 8-byte aligned");
    if (m->scratch_bytes < hh_wm_scratch(m->T, m->N, m->n_agents))
        return hh_epm_fail(fn, "scratch is smaller than hh_window_metrics_scratch_bytes(T, N, n_agents)");
    hipStream_t st = (hipStream_t)stream;
    switch (m->n_agents) {
    case 1: return hh_wm_launch<1>(*m, st);
    case 2: return hh_wm_launch<2>(*m, st);
    case 3: return hh_wm_launch<3>(*m, st);
    case 4: return hh_wm_launch<4>(*m, st);
    default: return hh_wm_launch<5>(*m, st);
    }
}

#endif /* HH_WINDOW_METRICS_H */
