/*
 * hh_commander_episodes.h — whole-episode GRU-sequence batches of the commander (hh_commander_episodes_emit, include/hh_commander.h):
 * hh_episodes.h's whole-episode batch for CommanderRollout's columns (1-byte actions, 3 agents x 34 observations), plus RLlib's cut of
 * every episode into sequences of at most L = max_seq_len steps, each carrying the GRU states (state_in_0 / state_in_1) of its first
 * step.  The carry holds, besides the running episode's rows, only the states at its sequence starts (ceil(carry_cap / L) per arena),
 * not a state per row.
 *
 * One call = six launches on one stream, no host synchronisation, no allocation (graph-capturable).  hh_episodes.h's count, scan and
 * GAE kernels run unchanged on an internal hh_episode_bufs view of these buffers (they read only done / carried / scratch, and the
 * batch's vf / reward columns with its tables); the sequence counts are scanned by the same scan kernel on a second view whose scratch
 * rows are the sequence rows:
 *   1. hh_k_ep_count       (episode view)  last done tick, episodes ending in the window, rows to emit
 *   2. hh_k_ep_scan        (episode view)  row / episode offsets per arena, counts[0..2]
 *   3. hh_k_cep_seq_count  one lane per arena: sequences of the episodes ending in the window (sum of ceil(E / L))
 *   4. hh_k_ep_scan        (sequence view) sequence offsets per arena
 *   5. hh_k_cep_emit       one workgroup per arena: rows (carry, then window), row metadata, episode and sequence tables, the states at
 *                          the sequence starts (window state_in or state carry); after a barrier, the trailing fragment's rows and its
 *                          sequence-start states into the carry
 *   6. hh_k_ep_gae         (episode view)  the whole-episode recursion, n_agents = 3
 * Every order (rows, episodes, sequences) is fixed by the scans and the arrangement, never by scheduling: graph and eager runs give
 * identical batches.
 */
#ifndef HH_COMMANDER_EPISODES_H
#define HH_COMMANDER_EPISODES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hh_commander.h"
#include "hh_episodes.h"

#define HH_CEP_OBS2 (HH_CMD_AGENTS * HH_CMD_OBS / 2)         /* float2 per observation row (408 B: 8-byte aligned rows) */
#define HH_CEP_STATE4 (HH_CMD_AGENTS * 2 * HH_CMD_HIDDEN / 4) /* float4 per arena row of GRU states (4800 B) */

/* scratch [10 N + 4]: rows 0..4 the episode view's (hh_episodes.h HH_EP_S_*), rows 5..9 the sequence view's (its "rows" = sequences per
 * arena, its "episodes" = 0, row 8 = the sequences' exclusive offsets), then the sequence view's counts [3] (sequences, 0, overflow) */
#define HH_CEP_S_SEQ 5
#define HH_CEP_S_SEQ_OFF 8
#define HH_CEP_S_COUNTS 10

/* dynamic LDS of hh_k_cep_emit, in ints: l_seg / l_prev / l_done / l_end [T], l_sq [T + 1], l_src [T + carry_cap / L] */
static inline int64_t hh_cep_lds_ints(int T, int carry_cap, int L) { return 5 * (int64_t)T + 1 + T + carry_cap / L; }

__global__ __launch_bounds__(256) void hh_k_cep_seq_count(hh_commander_episode_bufs b) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= b.N) return;
    const int L = b.max_seq_len;
    int prev = -1 - b.carried[n], ns = 0;   // the running episode's row 0 lies carried[n] rows before tick 0
    for (int t0 = 0; t0 < b.T; t0 += 16) {  // lanes = consecutive arenas: coalesced rows of done, 16 in flight
        uint8_t d[16];
#pragma unroll
        for (int k = 0; k < 16; k++) d[k] = t0 + k < b.T ? b.done[(size_t)(t0 + k) * b.N + n] : 0;
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (d[k]) {
                ns += (t0 + k - prev + L - 1) / L;
                prev = t0 + k;
            }
    }
    b.scratch[HH_CEP_S_SEQ * b.N + n] = ns;
    b.scratch[(HH_CEP_S_SEQ + 1) * b.N + n] = 0;
}

__global__ __launch_bounds__(256) void hh_k_cep_emit(hh_commander_episode_bufs b) {
    extern __shared__ int cep_lds[];
    const int T = b.T, N = b.N, L = b.max_seq_len, cap = b.carry_cap, Q = T + cap / L, SC = (cap + L - 1) / L;
    int *l_seg = cep_lds, *l_prev = l_seg + T, *l_done = l_prev + T;
    int *l_end = l_done + T;       // [k]: the window tick episode k of the window ends on
    int *l_sq = l_end + T;         // [k]: sequences of the episodes before k; [nd]: all of them
    int *l_src = l_sq + T + 1;     // [q]: where sequence q's first state is: window tick (>= 0) or carry slot -1 - src
    const int n = blockIdx.x, tid = threadIdx.x;
    const int32_t *s = b.scratch;
    const int cl = b.carried[n];
    const int last = s[HH_EP_S_LAST * N + n], nd = s[HH_EP_S_EPS * N + n];
    const int ro = s[HH_EP_S_ROW_OFF * N + n], eo = s[HH_EP_S_EP_OFF * N + n], so = s[HH_CEP_S_SEQ_OFF * N + n];
    const int ep0 = b.episode[n];
    if (tid < 64) hh_ep_tick_tables(b.done, T, N, n, tid, l_seg, l_prev, l_done);
    __syncthreads();
    for (int t = tid; t < T; t += blockDim.x)
        if (l_done[t]) l_end[l_seg[t]] = t;
    __syncthreads();
    if (tid < 64) {   // sequences per finished episode -> exclusive prefix (wave scan, 64 episodes at a time)
        int run = 0;
        for (int k0 = 0; k0 < nd; k0 += 64) {
            const int k = k0 + tid;
            int c = 0;
            if (k < nd) c = ((k == 0 ? cl + l_end[0] + 1 : l_end[k] - l_end[k - 1]) + L - 1) / L;
            int x = c;
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(x, off);
                if (tid >= off) x += y;
            }
            if (k < nd) l_sq[k] = run + x - c;
            run += __shfl(x, 63);
        }
        if (tid == 0) l_sq[nd] = run;
    }
    __syncthreads();
    int ns = l_sq[nd];
    if (ns > Q) ns = Q;   // cannot happen while carried <= carry_cap (sum ceil(E_k / L) <= nd + (rows - nd) / L); keeps l_src in bounds

    // 1. the sequence table and where each sequence's first state is
    for (int q = tid; q < ns; q += blockDim.x) {
        int lo = 0, hi = nd - 1;   // the episode of sequence q: the last k with l_sq[k] <= q
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (l_sq[mid] <= q) lo = mid; else hi = mid - 1;
        }
        const int k = lo, j = q - l_sq[k];
        const int i0 = k == 0 ? 0 : cl + l_end[k - 1] + 1, len = k == 0 ? cl + l_end[0] + 1 : l_end[k] - l_end[k - 1];
        const int i = i0 + j * L, rem = len - j * L;
        l_src[q] = i < cl ? -1 - j : i - cl;   // only the first episode reaches into the carry, whose slot j holds its step j L
        const long long e = (long long)so + q;
        if (e < b.seq_cap) {
            b.seq_start[e] = ro + i;
            b.seq_len[e] = rem < L ? rem : L;
            b.seq_ep[e] = eo + k;
        }
    }
    __syncthreads();

    // 2. the states at the sequence starts: 4800 B per sequence, dwordx4
    const float4 *__restrict__ sin4 = (const float4 *)b.state_in;
    float4 *__restrict__ cs4 = (float4 *)b.c_state;
    {
        const int nsw = (long long)so + ns <= b.seq_cap ? ns : (so < b.seq_cap ? (int)(b.seq_cap - so) : 0);   // flagged by the scan
        float4 *__restrict__ os4 = (float4 *)b.o_state_in + (size_t)so * HH_CEP_STATE4;
        const int units = nsw * HH_CEP_STATE4;
        for (int u = tid; u < units; u += blockDim.x) {
            const int q = u / HH_CEP_STATE4, w = u - q * HH_CEP_STATE4, src = l_src[q];
            os4[u] = src >= 0 ? sin4[((size_t)src * N + n) * HH_CEP_STATE4 + w] : cs4[((size_t)n * SC + (-1 - src)) * HH_CEP_STATE4 + w];
        }
    }

    // 3. the finished episodes' rows: carry slots [0, cl), then ticks [0, last]
    int emit = last >= 0 ? cl + last + 1 : 0;
    if (emit > 0 && (long long)ro + emit > b.row_cap) emit = ro < b.row_cap ? (int)(b.row_cap - ro) : 0;   // flagged by the scan
    const size_t crow0 = (size_t)n * cap, orow0 = (size_t)ro;
    const int nA = HH_CMD_AGENTS;
    if (emit > 0) {
        hh_ep_gather((float2 *)b.o_obs, (const float2 *)b.c_obs, (const float2 *)b.obs, HH_CEP_OBS2, emit, cl, crow0, N, n, orow0);
        hh_ep_gather((uint8_t *)b.o_actions, (const uint8_t *)b.c_actions, (const uint8_t *)b.actions, nA, emit, cl, crow0, N, n, orow0);
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
    __syncthreads();   // every read of the carry above (rows and states) happens before it is rewritten below

    // 4. the trailing fragment: ticks (last, T) replace the carry, or, with no done in the window, all T ticks extend it
    const int c0 = last >= 0 ? 0 : cl, t0 = last + 1;
    int keep = T - t0;
    if (c0 + keep > cap) keep = cap - c0 > 0 ? cap - c0 : 0;   // only if an episode outgrew carry_cap (flagged below)
    if (keep > 0) {
        const size_t c = crow0 + c0;
        hh_ep_stash((float2 *)b.c_obs, (const float2 *)b.obs, HH_CEP_OBS2, keep, t0, c, N, n);
        hh_ep_stash((uint8_t *)b.c_actions, (const uint8_t *)b.actions, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_logp, b.logp, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_vf, b.vf, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_reward, b.reward, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_valid, b.valid, nA, keep, t0, c, N, n);
        // the running episode's sequence starts among the new carry slots: steps j L in [c0, c0 + keep), window tick t0 + j L - c0
        const int j0 = (c0 + L - 1) / L, j1 = (c0 + keep + L - 1) / L;   // j1 <= SC: c0 + keep <= cap
        const int units = (j1 - j0) * HH_CEP_STATE4;
        for (int u = tid; u < units; u += blockDim.x) {
            const int q = u / HH_CEP_STATE4, w = u - q * HH_CEP_STATE4, j = j0 + q, t = t0 + j * L - c0;
            cs4[((size_t)n * SC + j) * HH_CEP_STATE4 + w] = sin4[((size_t)t * N + n) * HH_CEP_STATE4 + w];
        }
    }
    if (tid == 0) {
        if (keep < T - t0 || l_sq[nd] > Q) b.counts[2] = 1;
        b.carried[n] = c0 + keep;
        b.episode[n] = ep0 + nd;
        if (n == 0) {   // the sequence view's count and flag (written by launch 4, read here once)
            const int32_t *sc = b.scratch + (size_t)HH_CEP_S_COUNTS * N;
            b.counts[3] = sc[0];
            if (sc[2]) b.counts[2] = 1;
        }
    }
}

/* the internal hh_episode_bufs views: only the fields hh_k_ep_count / hh_k_ep_scan / hh_k_ep_gae read are set */
static hh_episode_bufs hh_cep_episode_view(const hh_commander_episode_bufs *b) {
    hh_episode_bufs v;
    memset(&v, 0, sizeof(v));
    v.T = b->T; v.N = b->N; v.n_agents = HH_CMD_AGENTS; v.obs_dim = HH_CMD_OBS; v.carry_cap = b->carry_cap;
    v.row_cap = b->row_cap; v.ep_cap = b->ep_cap; v.gamma = b->gamma; v.lam = b->lam;
    v.done = b->done; v.carried = b->carried; v.episode = b->episode; v.scratch = b->scratch; v.counts = b->counts;
    v.o_vf = b->o_vf; v.o_reward = b->o_reward; v.o_adv = b->o_adv; v.o_target = b->o_target;
    v.ep_start = b->ep_start; v.ep_len = b->ep_len; v.ep_arena = b->ep_arena;
    return v;
}

static hh_episode_bufs hh_cep_sequence_view(const hh_commander_episode_bufs *b) {
    hh_episode_bufs v;
    memset(&v, 0, sizeof(v));
    v.T = b->T; v.N = b->N; v.n_agents = HH_CMD_AGENTS; v.obs_dim = HH_CMD_OBS;
    v.row_cap = b->seq_cap; v.ep_cap = 1;   // its "episodes" row is all zero
    v.scratch = b->scratch + (size_t)HH_CEP_S_SEQ * b->N;
    v.counts = b->scratch + (size_t)HH_CEP_S_COUNTS * b->N;
    return v;
}

extern "C" int hh_commander_episodes_emit(const hh_commander_episode_bufs *b, void *stream) {
    if (!b || b->T <= 0 || b->N <= 0 || b->max_seq_len < 1 || b->carry_cap < 0) { g_err = "hh_commander_episodes_emit: bad sizes"; return HH_E_ARG; }
    if (b->T > HH_EP_MAX_T) { g_err = "hh_commander_episodes_emit: T > HH_EP_MAX_T"; return HH_E_ARG; }
    const int64_t N = b->N, T = b->T, cap = b->carry_cap, L = b->max_seq_len;
    if (N * (cap + T) > INT32_MAX || b->row_cap > INT32_MAX || b->ep_cap > INT32_MAX || b->seq_cap > INT32_MAX) {
        g_err = "hh_commander_episodes_emit: capacities must stay below 2^31"; return HH_E_ARG;
    }
    if (b->row_cap < N * (cap + T) || b->ep_cap < N * T || b->seq_cap < N * (T + cap / L)) {
        g_err = "hh_commander_episodes_emit: row_cap >= N (carry_cap + T), ep_cap >= N T and seq_cap >= N (T + carry_cap / max_seq_len) are required";
        return HH_E_ARG;
    }
    const int64_t lds = hh_cep_lds_ints((int)T, (int)cap, (int)L) * (int64_t)sizeof(int);
    if (lds > 65536) { g_err = "hh_commander_episodes_emit: T and carry_cap / max_seq_len too large for the emit kernel's LDS"; return HH_E_ARG; }
    const void *ptrs[] = {b->obs, b->actions, b->logp, b->vf, b->reward, b->valid, b->done, b->state_in, b->c_obs, b->c_actions, b->c_logp,
                          b->c_vf, b->c_reward, b->c_valid, b->c_state, b->carried, b->episode, b->scratch, b->o_obs, b->o_actions, b->o_logp,
                          b->o_vf, b->o_reward, b->o_valid, b->o_adv, b->o_target, b->o_done, b->o_arena, b->o_episode, b->o_t, b->ep_start,
                          b->ep_len, b->ep_arena, b->seq_start, b->seq_len, b->seq_ep, b->o_state_in, b->counts};
    for (const void *p : ptrs)
        if (!p) { g_err = "hh_commander_episodes_emit: null buffer"; return HH_E_ARG; }
    if (((uintptr_t)b->state_in | (uintptr_t)b->c_state | (uintptr_t)b->o_state_in) & 15) { g_err = "hh_commander_episodes_emit: state buffers must be 16-byte aligned"; return HH_E_ARG; }
    if (((uintptr_t)b->obs | (uintptr_t)b->c_obs | (uintptr_t)b->o_obs) & 7) { g_err = "hh_commander_episodes_emit: obs buffers must be 8-byte aligned"; return HH_E_ARG; }
    const hh_episode_bufs ev = hh_cep_episode_view(b), sv = hh_cep_sequence_view(b);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hh_k_ep_count, dim3((b->N + 255) / 256), dim3(256), 0, st, ev);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_ep_scan, dim3(1), dim3(1024), 0, st, ev);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_cep_seq_count, dim3((b->N + 255) / 256), dim3(256), 0, st, *b);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_ep_scan, dim3(1), dim3(1024), 0, st, sv);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_cep_emit, dim3(b->N), dim3(256), (size_t)lds, st, *b);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_ep_gae, dim3(b->ep_cap < 8192 ? (int)b->ep_cap : 8192), dim3(64), 0, st, ev);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

#endif /* HH_COMMANDER_EPISODES_H */
