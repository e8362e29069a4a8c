/*
 * hh_episodes.h — whole-episode batches from consecutive fixed-length collects (batch_mode = "complete_episodes",
 * train_hetero.py:212 / train_hier.py:182): RLlib hands its learner only whole episodes, from the reset row to the done row, with
 * GAE over each episode and last_r = 0 at its end.  A collect fills [T, N, ...] windows; an episode that spans collects is held in a
 * per-arena carry on the device until its done row arrives, then all its rows go out together in one flat batch.
 *
 * Two entry points share one path: hh_episodes_emit (include/hh_abi.h: PPORollout, generic in n_agents and the observation width D)
 * and hh_commander_episodes_emit (include/hh_commander.h: CommanderRollout's 3 x 34 rows), which adds one stage — RLlib's cut of every
 * episode into sequences of at most L = max_seq_len steps, each carrying the GRU states (state_in_0 / state_in_1) of its first step.
 * Its carry holds, besides the running episode's rows, only the states at its sequence starts (ceil(carry_cap / L) per arena).
 * Each entry point fills the internal descriptor hh_ep_desc from its own struct; the kernels below take only that.
 * hh_episodes_emit_aux / hh_commander_episodes_emit_aux are the same two with one optional per-agent float column (hh_episode_aux:
 * the rollouts' sampler logits) that moves with obs in the emit kernel's AUX instances; without it they are the entry points above.
 *
 * One call = four launches on one stream, no host synchronisation, no allocation, so it can be captured into the collect's graph:
 *   1. hh_k_ep_count  one lane per arena: last done tick, episodes ending in the window, rows to emit (carry + last_done + 1, or 0)
 *                     and, when sequences are cut, their sequences (sum of ceil(E / L))
 *   2. hh_k_ep_scan   one 1024-thread workgroup: exclusive scans of those counts over the arenas -> output offsets (no atomics: the
 *                     order is arena-major, then episode, then time, whatever the scheduling), counts[0..3]
 *   3. hh_k_ep_emit   one workgroup per arena: (sequences) the sequence table and the states at the sequence starts (window state_in
 *                     or state carry); gather the finished episodes' rows (carry first, then the window) into the batch with their
 *                     metadata and episode table; then (after a barrier, so the carry is read before it is rewritten in the same
 *                     launch) move the trailing fragment, (sequences) with its sequence-start states, into the carry
 *   4. hh_k_ep_gae    one wave per episode, one lane per agent: the recursion of hh_k_gae_rllib over the whole episode with
 *                     last_r = 0, float64 delta and discounted sum in its operation order, float32 results
 * Every order (rows, episodes, sequences) is fixed by the scans and the arrangement, never by scheduling: graph and eager runs give
 * identical batches.
 *
 * hh_episodes_emit_append / hh_commander_episodes_emit_append accumulate consecutive calls into one batch (RLlib's train_batch_size: whole
 * collects are concatenated until at least train_rows rows are there).  The same four launches; only the ACC instances of the scan and of
 * the GAE differ: the scan starts its three exclusive scans from the device-side bases acc[0] / acc[1] / acc[3] (0 when the previous
 * call completed a batch: acc[4]), so every offset the emit kernel reads — and with it ep_start, seq_start and seq_ep — is an absolute
 * position in the accumulated batch and hh_k_ep_emit runs unchanged; the GAE walks the episodes this call appended only.  The order is
 * collect-major, then arena, episode, time.
 *
 * Host part: needs g_err / HIPCHK of the including translation unit (hh_world.hip).
 */
#ifndef HH_EPISODES_H
#define HH_EPISODES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "hh_abi.h"
#include "hh_commander.h"

#define HH_EP_MAX_T 4096   /* the emit kernel keeps three ints per tick of the window in LDS (five or six with sequences) */

/* scratch rows ([5, N] i32; [7, N] with sequences) */
#define HH_EP_S_ROWS 0
#define HH_EP_S_EPS 1
#define HH_EP_S_LAST 2
#define HH_EP_S_ROW_OFF 3
#define HH_EP_S_EP_OFF 4
#define HH_EP_S_SEQ 5
#define HH_EP_S_SEQ_OFF 6

#define HH_EP_STATE4 (HH_CMD_AGENTS * 2 * HH_CMD_HIDDEN / 4) /* float4 per arena row of GRU states (4800 B) */

/* dynamic LDS of the sequence instance of hh_k_ep_emit, in ints: l_seg / l_prev / l_done / l_end [T], l_sq [T + 1], l_src [T + carry_cap / L] */
static inline int64_t hh_cep_lds_ints(int T, int carry_cap, int L) { return 5 * (int64_t)T + 1 + T + carry_cap / L; }

/* the buffers of one emission; max_seq_len, seq_cap, the state columns and the sequence table are the sequence instance's only */
struct hh_ep_desc {
    int32_t T, N, n_agents, obs_dim, carry_cap, max_seq_len;
    int64_t row_cap, ep_cap, seq_cap;
    double gamma, lam;
    const float *obs;
    const int8_t *actions;
    const float *logp, *vf, *reward;
    const uint8_t *valid, *done;
    const float *state_in;
    float *c_obs;
    int8_t *c_actions;
    float *c_logp, *c_vf, *c_reward;
    uint8_t *c_valid;
    float *c_state;
    int32_t *carried, *episode, *scratch;
    float *o_obs;
    int8_t *o_actions;
    float *o_logp, *o_vf, *o_reward;
    uint8_t *o_valid;
    float *o_adv, *o_target;
    uint8_t *o_done;
    int32_t *o_arena, *o_episode, *o_t, *ep_start, *ep_len, *ep_arena, *seq_start, *seq_len, *seq_ep;
    float *o_state_in;
    int32_t *counts;
    /* the optional per-agent float column of the _aux entry points ([.., n_agents, aux_dim]); read by the AUX instances of hh_k_ep_emit only */
    const float *aux;
    float *c_aux, *o_aux;
    int32_t aux_dim;
    /* the _append entry points' accumulator (i32 [HH_EP_ACC]), batch size in rows and optional running totals (i64 [2]); read by the ACC
       instances of hh_k_ep_scan / hh_k_ep_gae only */
    int32_t *acc;
    int64_t *totals;
    int64_t train_rows;
};

template <bool SEQ>
__global__ __launch_bounds__(256) void hh_k_ep_count(hh_ep_desc b) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= b.N) return;
    const int cl = b.carried[n], L = b.max_seq_len;
    int nd = 0, last = -1, ns = 0;
    for (int t0 = 0; t0 < b.T; t0 += 16) {   // lanes = consecutive arenas: every tick's read is one coalesced row of done; 16 in flight
        uint8_t d[16];
#pragma unroll
        for (int k = 0; k < 16; k++) d[k] = t0 + k < b.T ? b.done[(size_t)(t0 + k) * b.N + n] : 0;
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (d[k]) {
                // the episode ending here began after the previous done, or carried[n] rows before tick 0
                if constexpr (SEQ) ns += (t0 + k - (last >= 0 ? last : -1 - cl) + L - 1) / L;
                nd++;
                last = t0 + k;
            }
    }
    int32_t *s = b.scratch;
    s[HH_EP_S_ROWS * b.N + n] = last >= 0 ? cl + last + 1 : 0;
    s[HH_EP_S_EPS * b.N + n] = nd;
    s[HH_EP_S_LAST * b.N + n] = last;
    if constexpr (SEQ) s[HH_EP_S_SEQ * b.N + n] = ns;
}

/* one workgroup: thread i sums a contiguous run of arenas, the 1024 sums are scanned (wave shuffles, then the 16 wave totals), and
 * every thread writes the exclusive offsets of its run; rows, episodes and (SEQ) sequences side by side.  Totals fit in int:
 * N (carry_cap + T) < 2^31 is checked at the entry points (and bounds the sequences).
 * ACC (the _append entry points): the scans start from the accumulator's bases — thread 0 reads acc before the barrier and hands the bases
 * out through LDS (w_tot[q][16]), and rewrites acc after it, so no thread reads what thread 0 has already advanced.  A base is taken
 * into [0, capacity] whatever acc holds (acc is written clamped), so base + total stays below 2^32: the offsets are added as unsigned
 * and saturate at INT32_MAX — at or beyond every capacity, where the emit kernel writes nothing — and the sums that decide the
 * accumulator are taken in 64 bits */
template <bool SEQ, bool ACC = false>
__global__ __launch_bounds__(1024) void hh_k_ep_scan(hh_ep_desc b) {
    constexpr int Q = SEQ ? 3 : 2;
    constexpr int in[3] = {HH_EP_S_ROWS, HH_EP_S_EPS, HH_EP_S_SEQ}, out[3] = {HH_EP_S_ROW_OFF, HH_EP_S_EP_OFF, HH_EP_S_SEQ_OFF};
    constexpr int slot[3] = {0, 1, 3};
    __shared__ int w_tot[Q][ACC ? 17 : 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = b.N;
    int32_t *s = b.scratch;
    const int per = (N + 1023) / 1024, n0 = tid * per < N ? tid * per : N, n1 = n0 + per < N ? n0 + per : N;
    int sum[Q], x[Q], pre[Q], tot[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) sum[q] = 0;
#pragma unroll 8
    for (int n = n0; n < n1; n++)
#pragma unroll
        for (int q = 0; q < Q; q++) sum[q] += s[in[q] * N + n];
#pragma unroll
    for (int q = 0; q < Q; q++) x[q] = sum[q];
    for (int off = 1; off < 64; off <<= 1) {   // inclusive scan inside the wave
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int y = __shfl_up(x[q], off);
            if (lane >= off) x[q] += y;
        }
    }
    if (lane == 63)
#pragma unroll
        for (int q = 0; q < Q; q++) w_tot[q][wave] = x[q];
    bool fresh = false;   // (ACC, thread 0) the previous call completed a batch: this one starts the next
    if constexpr (ACC) {
        if (tid == 0) {
            fresh = b.acc[4] != 0;
            const int64_t cap[3] = {b.row_cap, b.ep_cap, b.seq_cap};
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int a = b.acc[slot[q]];
                w_tot[q][16] = fresh || a < 0 ? 0 : (a < cap[q] ? a : (int)cap[q]);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; q++) { pre[q] = x[q] - sum[q]; tot[q] = 0; }
#pragma unroll SEQ ? 4 : 16   // fully unrolled, the 48 totals of three scans would cost the sequence instance occupancy
    for (int w = 0; w < 16; w++)
#pragma unroll
        for (int q = 0; q < Q; q++) {
            if (w < wave) pre[q] += w_tot[q][w];
            tot[q] += w_tot[q][w];
        }
    if constexpr (!ACC) {
#pragma unroll 8
        for (int n = n0; n < n1; n++)
#pragma unroll
            for (int q = 0; q < Q; q++) {
                s[out[q] * N + n] = pre[q];
                pre[q] += s[in[q] * N + n];
            }
    } else {
        unsigned upre[Q];   // base + exclusive offset, below 2^32
#pragma unroll
        for (int q = 0; q < Q; q++) upre[q] = (unsigned)pre[q] + (unsigned)w_tot[q][16];
#pragma unroll 8
        for (int n = n0; n < n1; n++)
#pragma unroll
            for (int q = 0; q < Q; q++) {
                s[out[q] * N + n] = upre[q] < (unsigned)INT32_MAX ? (int)upre[q] : INT32_MAX;
                upre[q] += (unsigned)s[in[q] * N + n];
            }
    }
    if (tid == 0) {
        const int64_t cap[3] = {b.row_cap, b.ep_cap, b.seq_cap};
        if constexpr (!ACC) {
            bool over = false;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                b.counts[slot[q]] = tot[q] < cap[q] ? tot[q] : (int)cap[q];
                over |= tot[q] > cap[q];
            }
            if (over) b.counts[2] = 1;   // sticky: never cleared by a kernel
        } else {
            bool over = b.counts[2] != 0;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int base = w_tot[q][16];
                const int64_t end = (int64_t)base + tot[q], endc = end < cap[q] ? end : cap[q];
                b.acc[slot[q]] = (int)endc;
                b.counts[slot[q]] = (int)(endc - base);   // written by this call; base <= cap
                over |= end > cap[q];
            }
            if (over) { b.counts[2] = 1; b.acc[2] = 1; }   // both sticky
            b.acc[4] = b.acc[0] >= b.train_rows;
            b.acc[5] = (fresh ? 0 : b.acc[5]) + 1;
            if (fresh) b.acc[6] += 1;
            if (b.totals) {   // every episode and row once, whatever the metrics are taken over
                b.totals[0] += b.counts[1];
                b.totals[1] += b.counts[0];
            }
        }
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

/* OBS / ACT: the access units of the observation and action columns (an action row holds one ACT per agent); SEQ: cut sequences —
 * the commander's instance, whose row geometry (3 x 34) and states (3 x 2 x 200) are compile-time constants; AUX: floats per access
 * unit of the optional aux column (0: no such column — the instances of the entry points without it; 1: dword; 4: dwordx4, when a row
 * of n_agents aux_dim floats is a multiple of 16 B and the three bases are 16-byte aligned).  The column moves with obs: same passes,
 * same row order */
template <typename OBS, typename ACT, bool SEQ, int AUX = 0>
__global__ __launch_bounds__(256) void hh_k_ep_emit(hh_ep_desc b) {
    extern __shared__ int ep_lds[];
    const int T = b.T, N = b.N, nA = SEQ ? HH_CMD_AGENTS : b.n_agents, D = SEQ ? HH_CMD_OBS : b.obs_dim, cap = b.carry_cap, L = b.max_seq_len;
    int *l_seg = ep_lds;           // episodes of the window that ended strictly before tick t
    int *l_prev = l_seg + T;       // last done tick strictly before t (-1: none)
    int *l_done = l_prev + T;
    int *l_end = l_done + T;       // (SEQ) [k]: the window tick episode k of the window ends on
    int *l_sq = l_end + T;         // (SEQ) [k]: sequences of the episodes before k; [nd]: all of them
    int *l_src = l_sq + T + 1;     // (SEQ) [q]: where sequence q's first state is: window tick (>= 0) or carry slot -1 - src
    const int n = blockIdx.x, tid = threadIdx.x;
    const int32_t *s = b.scratch;
    const int cl = b.carried[n];
    const int last = s[HH_EP_S_LAST * N + n], nd = s[HH_EP_S_EPS * N + n];
    const int ro = s[HH_EP_S_ROW_OFF * N + n], eo = s[HH_EP_S_EP_OFF * N + n];
    const int ep0 = b.episode[n];
    if (tid < 64) hh_ep_tick_tables(b.done, T, N, n, tid, l_seg, l_prev, l_done);
    __syncthreads();

    // 1. (SEQ) the sequence table, and the states at the sequence starts: 4800 B per sequence, dwordx4 (ahead of the rows: in this
    //    order the commander's instance needs fewer registers)
    const int SC = SEQ ? (cap + L - 1) / L : 0;   // state carry slots per arena
    const float4 *__restrict__ sin4 = (const float4 *)b.state_in;
    float4 *__restrict__ cs4 = (float4 *)b.c_state;
    if constexpr (SEQ) {
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
        const int so = s[HH_EP_S_SEQ_OFF * N + n], Q = T + cap / L;
        int ns = l_sq[nd];
        if (ns > Q) ns = Q;   // cannot happen while carried <= carry_cap (sum ceil(E_k / L) <= nd + (rows - nd) / L); keeps l_src in bounds
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
        const int nsw = (long long)so + ns <= b.seq_cap ? ns : (so < b.seq_cap ? (int)(b.seq_cap - so) : 0);   // flagged by the scan
        float4 *__restrict__ os4 = (float4 *)b.o_state_in + (size_t)so * HH_EP_STATE4;
        const int units = nsw * HH_EP_STATE4;
        for (int u = tid; u < units; u += blockDim.x) {
            const int q = u / HH_EP_STATE4, w = u - q * HH_EP_STATE4, src = l_src[q];
            os4[u] = src >= 0 ? sin4[((size_t)src * N + n) * HH_EP_STATE4 + w] : cs4[((size_t)n * SC + (-1 - src)) * HH_EP_STATE4 + w];
        }
    }

    // 2. the finished episodes: carry slots [0, cl), then ticks [0, last]
    int emit = last >= 0 ? cl + last + 1 : 0;
    if (emit > 0 && (long long)ro + emit > b.row_cap) emit = ro < b.row_cap ? (int)(b.row_cap - ro) : 0;   // flagged by the scan
    const size_t crow0 = (size_t)n * cap, orow0 = (size_t)ro;
    const int obs_units = nA * D / (int)(sizeof(OBS) / sizeof(float));
    using AUXU = typename std::conditional<AUX == 4, float4, float>::type;
    const int aux_units = AUX ? nA * b.aux_dim / AUX : 0;
    if (emit > 0) {
        hh_ep_gather((OBS *)b.o_obs, (const OBS *)b.c_obs, (const OBS *)b.obs, obs_units, emit, cl, crow0, N, n, orow0);
        if constexpr (AUX != 0) hh_ep_gather((AUXU *)b.o_aux, (const AUXU *)b.c_aux, (const AUXU *)b.aux, aux_units, emit, cl, crow0, N, n, orow0);
        hh_ep_gather((ACT *)b.o_actions, (const ACT *)b.c_actions, (const ACT *)b.actions, nA, emit, cl, crow0, N, n, orow0);
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

    // 3. the trailing fragment: ticks (last, T) replace the carry, or, with no done in the window, all T ticks extend it
    const int c0 = last >= 0 ? 0 : cl, t0 = last + 1;
    int keep = T - t0;
    if (c0 + keep > cap) keep = cap - c0 > 0 ? cap - c0 : 0;   // only if an episode outgrew carry_cap (flagged below)
    if (keep > 0) {
        const size_t c = crow0 + c0;
        hh_ep_stash((OBS *)b.c_obs, (const OBS *)b.obs, obs_units, keep, t0, c, N, n);
        if constexpr (AUX != 0) hh_ep_stash((AUXU *)b.c_aux, (const AUXU *)b.aux, aux_units, keep, t0, c, N, n);
        hh_ep_stash((ACT *)b.c_actions, (const ACT *)b.actions, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_logp, b.logp, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_vf, b.vf, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_reward, b.reward, nA, keep, t0, c, N, n);
        hh_ep_stash(b.c_valid, b.valid, nA, keep, t0, c, N, n);
        if constexpr (SEQ) {
            // the running episode's sequence starts among the new carry slots: steps j L in [c0, c0 + keep), window tick t0 + j L - c0
            const int j0 = (c0 + L - 1) / L, j1 = (c0 + keep + L - 1) / L;   // j1 <= SC: c0 + keep <= cap
            const int units = (j1 - j0) * HH_EP_STATE4;
            for (int u = tid; u < units; u += blockDim.x) {
                const int q = u / HH_EP_STATE4, w = u - q * HH_EP_STATE4, j = j0 + q, t = t0 + j * L - c0;
                cs4[((size_t)n * SC + j) * HH_EP_STATE4 + w] = sin4[((size_t)t * N + n) * HH_EP_STATE4 + w];
            }
        }
    }
    if (tid == 0) {
        if (keep < T - t0 || (SEQ && l_sq[nd] > T + cap / L)) b.counts[2] = 1;
        b.carried[n] = c0 + keep;
        b.episode[n] = ep0 + nd;
    }
}

/* The whole-episode recursion, in hh_k_gae_rllib's float64 operation order, last_r = 0 after the done row.  One wave per episode (grid-stride
 * over the table): the episode's rows are contiguous in the batch, so its rewards / values are staged into LDS with coalesced loads, lane
 * a < n_agents walks agent a backwards on the LDS copy (the chain is sequential: bit-exactness fixes its order), and the results leave
 * with coalesced stores.  Episodes longer than a chunk are walked chunk by chunk from the end, the recursion carried in registers. */
#define HH_EP_GAE_LDS 512   /* floats per staged column */
/* ACC: the episodes this call appended, [acc[1] - counts[1], acc[1]) — the adv / target bytes of the batch's earlier episodes stay */
template <bool ACC = false>
__global__ __launch_bounds__(64) void hh_k_ep_gae(hh_ep_desc b) {
    __shared__ float l_r[HH_EP_GAE_LDS], l_v[HH_EP_GAE_LDS];
    const int nA = b.n_agents, tid = threadIdx.x, chunk = HH_EP_GAE_LDS / nA;
    const int n_eps = ACC ? b.acc[1] : b.counts[1], e0 = ACC ? n_eps - b.counts[1] : 0;
    const double gamma = b.gamma, gl = b.gamma * b.lam;
    for (int e = e0 + blockIdx.x; e < n_eps; e += gridDim.x) {
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

/* ---- host side ---- */

/* the fields both public structs name alike */
template <typename B>
static hh_ep_desc hh_ep_common(const B *b) {
    hh_ep_desc d = {};
    d.T = b->T; d.N = b->N; d.carry_cap = b->carry_cap; d.row_cap = b->row_cap; d.ep_cap = b->ep_cap; d.gamma = b->gamma; d.lam = b->lam;
    d.obs = b->obs; d.actions = b->actions; d.logp = b->logp; d.vf = b->vf; d.reward = b->reward; d.valid = b->valid; d.done = b->done;
    d.c_obs = b->c_obs; d.c_actions = b->c_actions; d.c_logp = b->c_logp; d.c_vf = b->c_vf; d.c_reward = b->c_reward; d.c_valid = b->c_valid;
    d.carried = b->carried; d.episode = b->episode; d.scratch = b->scratch;
    d.o_obs = b->o_obs; d.o_actions = b->o_actions; d.o_logp = b->o_logp; d.o_vf = b->o_vf; d.o_reward = b->o_reward; d.o_valid = b->o_valid;
    d.o_adv = b->o_adv; d.o_target = b->o_target; d.o_done = b->o_done; d.o_arena = b->o_arena; d.o_episode = b->o_episode; d.o_t = b->o_t;
    d.ep_start = b->ep_start; d.ep_len = b->ep_len; d.ep_arena = b->ep_arena; d.counts = b->counts;
    return d;
}

static int hh_ep_fail(const char *fn, const char *what) {
    g_err = std::string(fn) + ": " + what;
    return HH_E_ARG;
}

/* The checks both entry points make, in this order: sizes, T, capacities below 2^31.  own_* is the entry point's own condition of the
 * same step, reported with it (t_msg: the T step's message). */
static int hh_ep_check_sizes(const char *fn, const hh_ep_desc &d, bool own_sizes, bool own_t, const char *t_msg, bool own_caps) {
    if (d.T <= 0 || d.N <= 0 || d.carry_cap < 0 || own_sizes) return hh_ep_fail(fn, "bad sizes");
    if (d.T > HH_EP_MAX_T || own_t) return hh_ep_fail(fn, t_msg);
    if ((int64_t)d.N * ((int64_t)d.carry_cap + d.T) > INT32_MAX || d.row_cap > INT32_MAX || d.ep_cap > INT32_MAX || own_caps)
        return hh_ep_fail(fn, "capacities must stay below 2^31");
    return HH_OK;
}

/* the null-pointer sweep: every buffer of the descriptor (with sequences: the state columns and the sequence table as well) */
static int hh_ep_check_ptrs(const char *fn, const hh_ep_desc &d) {
    const void *ptrs[] = {d.obs, d.actions, d.logp, d.vf, d.reward, d.valid, d.done, d.c_obs, d.c_actions, d.c_logp, d.c_vf, d.c_reward,
                          d.c_valid, d.carried, d.episode, d.scratch, d.o_obs, d.o_actions, d.o_logp, d.o_vf, d.o_reward, d.o_valid,
                          d.o_adv, d.o_target, d.o_done, d.o_arena, d.o_episode, d.o_t, d.ep_start, d.ep_len, d.ep_arena, d.counts};
    const void *seq[] = {d.state_in, d.c_state, d.seq_start, d.seq_len, d.seq_ep, d.o_state_in};
    for (const void *p : ptrs)
        if (!p) return hh_ep_fail(fn, "null buffer");
    if (d.max_seq_len > 0)
        for (const void *p : seq)
            if (!p) return hh_ep_fail(fn, "null buffer");
    return HH_OK;
}

template <typename OBS, typename ACT, bool SEQ, int AUX = 0>
static int hh_ep_launch(const hh_ep_desc &d, size_t lds, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hh_k_ep_count<SEQ>, dim3((d.N + 255) / 256), dim3(256), 0, st, d);
    HIPCHK(hipGetLastError());
    if (d.acc) hipLaunchKernelGGL((hh_k_ep_scan<SEQ, true>), dim3(1), dim3(1024), 0, st, d);
    else hipLaunchKernelGGL((hh_k_ep_scan<SEQ, false>), dim3(1), dim3(1024), 0, st, d);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((hh_k_ep_emit<OBS, ACT, SEQ, AUX>), dim3(d.N), dim3(256), lds, st, d);
    HIPCHK(hipGetLastError());
    const dim3 gae_grid(d.ep_cap < 8192 ? (int)d.ep_cap : 8192);
    if (d.acc) hipLaunchKernelGGL(hh_k_ep_gae<true>, gae_grid, dim3(64), 0, st, d);
    else hipLaunchKernelGGL(hh_k_ep_gae<false>, gae_grid, dim3(64), 0, st, d);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

/* the aux column's instance: 0 without one, dwordx4 where a row's bytes and the three bases allow it, dword otherwise */
template <typename OBS, typename ACT, bool SEQ>
static int hh_ep_launch_aux(const hh_ep_desc &d, size_t lds, void *stream) {
    if (!d.aux) return hh_ep_launch<OBS, ACT, SEQ, 0>(d, lds, stream);
    const bool aux4 = (d.n_agents * d.aux_dim) % 4 == 0 && !(((uintptr_t)d.aux | (uintptr_t)d.c_aux | (uintptr_t)d.o_aux) & 15);
    return aux4 ? hh_ep_launch<OBS, ACT, SEQ, 4>(d, lds, stream) : hh_ep_launch<OBS, ACT, SEQ, 1>(d, lds, stream);
}

/* the _aux entry points' own argument checks (x != NULL), made after the struct's; fills the descriptor's aux fields */
static int hh_ep_check_aux(const char *fn, const hh_episode_aux *x, hh_ep_desc &d) {
    if (x->aux_dim < 1 || x->aux_dim > HH_EP_AUX_MAX_DIM) return hh_ep_fail(fn, "aux_dim must be 1 .. 32");
    if (x->reserved0 != 0) return hh_ep_fail(fn, "hh_episode_aux.reserved0 must be 0");
    if (!x->aux || !x->c_aux || !x->o_aux) return hh_ep_fail(fn, "null aux buffer");
    if (((uintptr_t)x->aux | (uintptr_t)x->c_aux | (uintptr_t)x->o_aux) & 3) return hh_ep_fail(fn, "aux buffers must be 4-byte aligned");
    d.aux = x->aux; d.c_aux = x->c_aux; d.o_aux = x->o_aux; d.aux_dim = x->aux_dim;
    return HH_OK;
}

/* the _append entry points' own argument checks, made after the struct's; fills the descriptor's accumulator fields */
struct hh_ep_append {
    int64_t train_rows;
    int32_t *acc;
    int64_t *totals;
};

static int hh_ep_check_append(const char *fn, const hh_ep_append *a, hh_ep_desc &d) {
    if (a->train_rows < 1) return hh_ep_fail(fn, "train_rows must be at least 1");
    if (!a->acc) return hh_ep_fail(fn, "null acc");
    if ((uintptr_t)a->acc & 3) return hh_ep_fail(fn, "acc must be 4-byte aligned");
    if ((uintptr_t)a->totals & 7) return hh_ep_fail(fn, "totals must be 8-byte aligned");
    d.acc = a->acc; d.totals = a->totals; d.train_rows = a->train_rows;
    return HH_OK;
}

static int hh_ep_emit_any(const char *fn, const hh_episode_bufs *b, const hh_episode_aux *x, void *stream, const hh_ep_append *a = NULL) {
    if (!b) return hh_ep_fail(fn, "bad sizes");
    hh_ep_desc d = hh_ep_common(b);
    d.n_agents = b->n_agents; d.obs_dim = b->obs_dim;
    int rc = hh_ep_check_sizes(fn, d, b->n_agents <= 0 || b->obs_dim <= 0 || b->reserved0 != 0, b->n_agents > 64,
                               "T > HH_EP_MAX_T or n_agents > 64", b->row_cap < 1 || b->ep_cap < 1);
    if (rc != HH_OK || (rc = hh_ep_check_ptrs(fn, d)) != HH_OK) return rc;
    const bool obs4 = (b->n_agents * b->obs_dim) % 4 == 0;   // an obs row is 2 D floats = 16 B aligned for D = 26 | 30: dwordx4
    if (obs4 && (((uintptr_t)b->obs | (uintptr_t)b->c_obs | (uintptr_t)b->o_obs) & 15)) return hh_ep_fail(fn, "obs buffers must be 16-byte aligned");
    if ((((uintptr_t)b->actions | (uintptr_t)b->c_actions | (uintptr_t)b->o_actions) & 3)) return hh_ep_fail(fn, "action buffers must be 4-byte aligned");
    if (a && (rc = hh_ep_check_append(fn, a, d)) != HH_OK) return rc;
    if (x && (rc = hh_ep_check_aux(fn, x, d)) != HH_OK) return rc;
    const size_t lds = 3 * (size_t)b->T * sizeof(int);
    return obs4 ? hh_ep_launch_aux<float4, uint32_t, false>(d, lds, stream) : hh_ep_launch_aux<float, uint32_t, false>(d, lds, stream);
}

extern "C" int hh_episodes_emit(const hh_episode_bufs *b, void *stream) { return hh_ep_emit_any("hh_episodes_emit", b, NULL, stream); }

extern "C" int hh_episodes_emit_aux(const hh_episode_bufs *b, const hh_episode_aux *x, void *stream) {
    return hh_ep_emit_any("hh_episodes_emit_aux", b, x, stream);
}

extern "C" int hh_episodes_emit_append(const hh_episode_bufs *b, const hh_episode_aux *x, int64_t train_rows, int32_t *acc, int64_t *totals,
                                       void *stream) {
    const hh_ep_append a = {train_rows, acc, totals};
    return hh_ep_emit_any("hh_episodes_emit_append", b, x, stream, &a);
}

static int hh_cep_emit_any(const char *fn, const hh_commander_episode_bufs *b, const hh_episode_aux *x, void *stream,
                           const hh_ep_append *a = NULL) {
    if (!b) return hh_ep_fail(fn, "bad sizes");
    hh_ep_desc d = hh_ep_common(b);
    d.n_agents = HH_CMD_AGENTS; d.obs_dim = HH_CMD_OBS; d.max_seq_len = b->max_seq_len; d.seq_cap = b->seq_cap;
    d.state_in = b->state_in; d.c_state = b->c_state; d.o_state_in = b->o_state_in;
    d.seq_start = b->seq_start; d.seq_len = b->seq_len; d.seq_ep = b->seq_ep;
    int rc = hh_ep_check_sizes(fn, d, b->max_seq_len < 1, false, "T > HH_EP_MAX_T", b->seq_cap > INT32_MAX);
    if (rc != HH_OK) return rc;
    const int64_t N = b->N, T = b->T, cap = b->carry_cap, L = b->max_seq_len;
    if (b->row_cap < N * (cap + T) || b->ep_cap < N * T || b->seq_cap < N * (T + cap / L))
        return hh_ep_fail(fn, "row_cap >= N (carry_cap + T), ep_cap >= N T and seq_cap >= N (T + carry_cap / max_seq_len) are required");
    const int64_t lds = hh_cep_lds_ints((int)T, (int)cap, (int)L) * (int64_t)sizeof(int);
    if (lds > 65536) return hh_ep_fail(fn, "T and carry_cap / max_seq_len too large for the emit kernel's LDS");
    if ((rc = hh_ep_check_ptrs(fn, d)) != HH_OK) return rc;
    if (((uintptr_t)b->state_in | (uintptr_t)b->c_state | (uintptr_t)b->o_state_in) & 15) return hh_ep_fail(fn, "state buffers must be 16-byte aligned");
    if (((uintptr_t)b->obs | (uintptr_t)b->c_obs | (uintptr_t)b->o_obs) & 7) return hh_ep_fail(fn, "obs buffers must be 8-byte aligned");
    if (a && (rc = hh_ep_check_append(fn, a, d)) != HH_OK) return rc;
    if (x && (rc = hh_ep_check_aux(fn, x, d)) != HH_OK) return rc;
    return hh_ep_launch_aux<float2, uint8_t, true>(d, (size_t)lds, stream);
}

extern "C" int hh_commander_episodes_emit(const hh_commander_episode_bufs *b, void *stream) {
    return hh_cep_emit_any("hh_commander_episodes_emit", b, NULL, stream);
}

extern "C" int hh_commander_episodes_emit_aux(const hh_commander_episode_bufs *b, const hh_episode_aux *x, void *stream) {
    return hh_cep_emit_any("hh_commander_episodes_emit_aux", b, x, stream);
}

extern "C" int hh_commander_episodes_emit_append(const hh_commander_episode_bufs *b, const hh_episode_aux *x, int64_t train_rows,
                                                 int32_t *acc, int64_t *totals, void *stream) {
    const hh_ep_append a = {train_rows, acc, totals};
    return hh_cep_emit_any("hh_commander_episodes_emit_append", b, x, stream, &a);
}

#endif /* HH_EPISODES_H */
