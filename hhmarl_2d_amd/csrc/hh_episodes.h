/*
 * hh_episodes.h — whole-episode batches from consecutive fixed-length collects (batch_mode = "complete_episodes",
 * train_hetero.py:212 / train_hier.py:182): RLlib hands its learner only whole episodes, from the reset row to the done row, with
 * GAE over each episode and last_r = 0 at its end.  A collect fills [T, N, ...] windows; an episode that spans collects is held in a
 * per-arena carry on the device until its done row arrives, then all its rows go out together in one flat batch.
 *
 * Not tied to a world (like hh_gae.h): generic in n_agents and in the observation width D.  One call (hh_episodes_emit) = four
 * launches on one stream, no host synchronisation, no allocation, so it can be captured into the collect's graph:
 *   1. hh_k_ep_count  one lane per arena: last done tick, episodes ending in the window, rows to emit (carry + last_done + 1, or 0)
 *   2. hh_k_ep_scan   one 1024-thread workgroup: exclusive scan of those counts over the arenas -> output offsets (no atomics: the
 *                     order is arena-major, then episode, then time, whatever the scheduling)
 *   3. hh_k_ep_emit   one workgroup per arena: gather the finished episodes' rows (carry first, then the window) into the batch, then
 *                     (after a barrier, so the carry is read before it is rewritten in the same launch) move the trailing fragment
 *                     into the carry
 *   4. hh_k_ep_gae    one wave per episode, one lane per agent: the recursion of hh_k_gae_rllib over the whole episode with
 *                     last_r = 0, float64 delta and discounted sum in its operation order, float32 results
 */
#ifndef HH_EPISODES_H
#define HH_EPISODES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hh_abi.h"

#define HH_EP_MAX_T 4096   /* the emit kernel keeps three ints per tick of the window in LDS */

/* scratch rows ([5, N] i32) */
#define HH_EP_S_ROWS 0
#define HH_EP_S_EPS 1
#define HH_EP_S_LAST 2
#define HH_EP_S_ROW_OFF 3
#define HH_EP_S_EP_OFF 4

__global__ __launch_bounds__(256) void hh_k_ep_count(hh_episode_bufs b) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= b.N) return;
    int nd = 0, last = -1;
    for (int t0 = 0; t0 < b.T; t0 += 16) {   // lanes = consecutive arenas: every tick's read is one coalesced row of done; 16 in flight
        uint8_t d[16];
#pragma unroll
        for (int k = 0; k < 16; k++) d[k] = t0 + k < b.T ? b.done[(size_t)(t0 + k) * b.N + n] : 0;
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (d[k]) { nd++; last = t0 + k; }
    }
    int32_t *s = b.scratch;
    s[HH_EP_S_ROWS * b.N + n] = last >= 0 ? b.carried[n] + last + 1 : 0;
    s[HH_EP_S_EPS * b.N + n] = nd;
    s[HH_EP_S_LAST * b.N + n] = last;
}

/* one workgroup: thread i sums a contiguous run of arenas, the 1024 sums are scanned (wave shuffles, then the 16 wave totals), and
 * every thread writes the exclusive offsets of its run.  Totals fit in int: N (carry_cap + T) < 2^31 is checked at the entry point */
__global__ __launch_bounds__(1024) void hh_k_ep_scan(hh_episode_bufs b) {
    __shared__ int w_rows[16], w_eps[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = b.N;
    int32_t *s = b.scratch;
    const int per = (N + 1023) / 1024, n0 = tid * per < N ? tid * per : N, n1 = n0 + per < N ? n0 + per : N;
    int sr = 0, se = 0;
#pragma unroll 8
    for (int n = n0; n < n1; n++) { sr += s[HH_EP_S_ROWS * N + n]; se += s[HH_EP_S_EPS * N + n]; }
    int r = sr, e = se;
    for (int off = 1; off < 64; off <<= 1) {   // inclusive scan inside the wave
        const int r2 = __shfl_up(r, off), e2 = __shfl_up(e, off);
        if (lane >= off) { r += r2; e += e2; }
    }
    if (lane == 63) { w_rows[wave] = r; w_eps[wave] = e; }
    __syncthreads();
    int pre_r = r - sr, pre_e = e - se, tot_r = 0, tot_e = 0;
    for (int w = 0; w < 16; w++) {
        if (w < wave) { pre_r += w_rows[w]; pre_e += w_eps[w]; }
        tot_r += w_rows[w];
        tot_e += w_eps[w];
    }
#pragma unroll 8
    for (int n = n0; n < n1; n++) {
        s[HH_EP_S_ROW_OFF * N + n] = pre_r;
        s[HH_EP_S_EP_OFF * N + n] = pre_e;
        pre_r += s[HH_EP_S_ROWS * N + n];
        pre_e += s[HH_EP_S_EPS * N + n];
    }
    if (tid == 0) {
        b.counts[0] = tot_r < b.row_cap ? tot_r : (int)b.row_cap;
        b.counts[1] = tot_e < b.ep_cap ? tot_e : (int)b.ep_cap;
        if (tot_r > b.row_cap || tot_e > b.ep_cap) b.counts[2] = 1;   // sticky: never cleared by a kernel
    }
}

/* wave 0 of an arena's workgroup (lane = tid < 64): per tick t of the window, the episodes that ended strictly before t (l_seg), the last
 * done tick strictly before t (l_prev, -1: none) and the done flag (l_done) */
__device__ __forceinline__ void hh_ep_tick_tables(const uint8_t *done, int T, int N, int n, int lane, int *l_seg, int *l_prev, int *l_done) {
    int cnt = 0, prev = -1;
    for (int base = 0; base < T; base += 64) {
        const int t = base + lane;
        const bool d = t < T && done[(size_t)t * N + n] != 0;
        const unsigned long long m = __ballot(d);
        const unsigned long long below = m & ((1ull << lane) - 1ull);
        if (t < T) {
            l_seg[t] = cnt + __popcll(below);
            l_prev[t] = below ? base + 63 - __clzll((long long)below) : prev;
            l_done[t] = d;
        }
        cnt += __popcll(m);
        if (m) prev = base + 63 - __clzll((long long)m);
    }
}

/* rows [0, rows) of one arena's emission: row i < cl is carry slot i, row i >= cl is tick i - cl of the window */
template <typename U>
__device__ __forceinline__ void hh_ep_gather(U *out, const U *carry, const U *coll, int upr, int rows, int cl, size_t crow0, int N, int n, size_t orow0) {
    const int total = rows * upr;
    for (int k = threadIdx.x; k < total; k += blockDim.x) {
        const int i = k / upr, u = k - i * upr;
        out[(orow0 + i) * upr + u] = i < cl ? carry[(crow0 + i) * upr + u] : coll[((size_t)(i - cl) * N + n) * upr + u];
    }
}

/* ticks [t0, t0 + rows) of the window -> carry slots [c0, c0 + rows) of one arena */
template <typename U>
__device__ __forceinline__ void hh_ep_stash(U *carry, const U *coll, int upr, int rows, int t0, size_t crow0, int N, int n) {
    const int total = rows * upr;
    for (int k = threadIdx.x; k < total; k += blockDim.x) {
        const int j = k / upr, u = k - j * upr;
        carry[(crow0 + j) * upr + u] = coll[((size_t)(t0 + j) * N + n) * upr + u];
    }
}

__global__ __launch_bounds__(256) void hh_k_ep_emit(hh_episode_bufs b) {
    extern __shared__ int ep_lds[];
    int *l_seg = ep_lds;              // episodes of the window that ended strictly before tick t
    int *l_prev = ep_lds + b.T;       // last done tick strictly before t (-1: none)
    int *l_done = ep_lds + 2 * b.T;
    const int n = blockIdx.x, tid = threadIdx.x, N = b.N, nA = b.n_agents, cap = b.carry_cap;
    const int32_t *s = b.scratch;
    const int cl = b.carried[n];
    const int last = s[HH_EP_S_LAST * N + n], nd = s[HH_EP_S_EPS * N + n];
    const int ro = s[HH_EP_S_ROW_OFF * N + n], eo = s[HH_EP_S_EP_OFF * N + n];
    const int ep0 = b.episode[n];
    if (tid < 64) hh_ep_tick_tables(b.done, b.T, N, n, tid, l_seg, l_prev, l_done);
    __syncthreads();

    // 1. the finished episodes: carry slots [0, cl), then ticks [0, last]
    int emit = last >= 0 ? cl + last + 1 : 0;
    if (emit > 0 && (long long)ro + emit > b.row_cap) emit = ro < b.row_cap ? (int)(b.row_cap - ro) : 0;   // flagged by the scan
    const size_t crow0 = (size_t)n * cap, orow0 = (size_t)ro;
    if (emit > 0) {
        const int D = b.obs_dim;
        if ((nA * D) % 4 == 0)   // an obs row is 2 D floats = 16 B aligned for D = 26 | 30: dwordx4
            hh_ep_gather((float4 *)b.o_obs, (const float4 *)b.c_obs, (const float4 *)b.obs, nA * D / 4, emit, cl, crow0, N, n, orow0);
        else
            hh_ep_gather(b.o_obs, b.c_obs, b.obs, nA * D, emit, cl, crow0, N, n, orow0);
        hh_ep_gather((uint32_t *)b.o_actions, (const uint32_t *)b.c_actions, (const uint32_t *)b.actions, nA, emit, cl, crow0, N, n, orow0);
        hh_ep_gather(b.o_logp, b.c_logp, b.logp, nA, emit, cl, crow0, N, n, orow0);
        hh_ep_gather(b.o_vf, b.c_vf, b.vf, nA, emit, cl, crow0, N, n, orow0);
        hh_ep_gather(b.o_reward, b.c_reward, b.reward, nA, emit, cl, crow0, N, n, orow0);
        hh_ep_gather(b.o_valid, b.c_valid, b.valid, nA, emit, cl, crow0, N, n, orow0);
        for (int i = tid; i < emit; i += blockDim.x) {
            int k = 0, te = i, d = 0;           // carry rows: the running episode's first rows, never a done
            if (i >= cl) {
                const int t = i - cl, p = l_prev[t];
                k = l_seg[t];
                te = p < 0 ? cl + t : t - p - 1;
                d = l_done[t];
            }
            const size_t r = orow0 + i;
            b.o_done[r] = (uint8_t)d;
            b.o_arena[r] = n;
            b.o_episode[r] = ep0 + k;
            b.o_t[r] = te;
            const long long e = (long long)eo + k;
            if (e < b.ep_cap) {
                if (te == 0) { b.ep_start[e] = (int)r; b.ep_arena[e] = n; }
                if (d) b.ep_len[e] = te + 1;
            }
        }
    }
    __syncthreads();   // every read of the carry above happens before it is rewritten below

    // 2. the trailing fragment: ticks (last, T) replace the carry, or, with no done in the window, all T ticks extend it
    const int c0 = last >= 0 ? 0 : cl, t0 = last + 1;
    int keep = b.T - t0;
    if (c0 + keep > cap) keep = cap - c0 > 0 ? cap - c0 : 0;   // cannot happen under the horizon rule (an episode has <= horizon rows)
    if (keep > 0) {
        const size_t c = crow0 + c0;
        const int D = b.obs_dim;
        if ((nA * D) % 4 == 0)
            hh_ep_stash((float4 *)b.c_obs, (const float4 *)b.obs, nA * D / 4, keep, t0, c, N, n);
        else
            hh_ep_stash(b.c_obs, b.obs, nA * D, keep, t0, c, N, n);
        hh_ep_stash((uint32_t *)b.c_actions, (const uint32_t *)b.actions, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_logp, b.logp, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_vf, b.vf, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_reward, b.reward, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_valid, b.valid, nA, keep, t0, c, N, n);
    }
    if (tid == 0) {
        if (keep < b.T - t0) b.counts[2] = 1;
        b.carried[n] = c0 + keep;
        b.episode[n] = ep0 + nd;
    }
}

/* The whole-episode recursion, in hh_k_gae_rllib's float64 operation order, last_r = 0 after the done row.  One wave per episode (grid-stride
 * over the table): the episode's rows are contiguous in the batch, so its rewards / values are staged into LDS with coalesced loads, lane
 * a < n_agents walks agent a backwards on the LDS copy (the chain is sequential: bit-exactness fixes its order), and the results leave
 * with coalesced stores.  Episodes longer than a chunk are walked chunk by chunk from the end, the recursion carried in registers. */
#define HH_EP_GAE_LDS 512   /* floats per staged column */
__global__ __launch_bounds__(64) void hh_k_ep_gae(hh_episode_bufs b) {
    __shared__ float l_r[HH_EP_GAE_LDS], l_v[HH_EP_GAE_LDS];
    const int nA = b.n_agents, tid = threadIdx.x, chunk = HH_EP_GAE_LDS / nA;
    const int n_eps = b.counts[1];
    const double gamma = b.gamma, gl = b.gamma * b.lam;
    for (int e = blockIdx.x; e < n_eps; e += gridDim.x) {
        const int start = b.ep_start[e], len = b.ep_len[e];
        if (start < 0 || len <= 0 || (long long)start + len > b.row_cap) continue;   // only after an overflow (flagged)
        double a_next = 0.0;
        float v_next = 0.0f;
        bool last = true;
        for (int hi = len; hi > 0; hi -= chunk) {
            const int lo = hi - chunk > 0 ? hi - chunk : 0, m = (hi - lo) * nA;
            const size_t base = (size_t)(start + lo) * nA;
            for (int k = tid; k < m; k += 64) { l_r[k] = b.o_reward[base + k]; l_v[k] = b.o_vf[base + k]; }
            __syncthreads();
            if (tid < nA) {
                for (int i = hi - lo - 1; i >= 0; i--) {
                    const int x = i * nA + tid;
                    const float v = l_v[x];
                    const double delta = __dsub_rn(__dadd_rn((double)l_r[x], __dmul_rn(gamma, last ? 0.0 : (double)v_next)), (double)v);
                    const double ad = __dadd_rn(delta, __dmul_rn(gl, last ? 0.0 : a_next));
                    l_r[x] = (float)ad;                       // the slots now hold advantage / value target
                    l_v[x] = (float)__dadd_rn(ad, (double)v);
                    a_next = ad;
                    v_next = v;
                    last = false;
                }
            }
            __syncthreads();
            for (int k = tid; k < m; k += 64) { b.o_adv[base + k] = l_r[k]; b.o_target[base + k] = l_v[k]; }
            __syncthreads();   // before the next chunk overwrites the staging
        }
    }
}

#endif /* HH_EPISODES_H */
