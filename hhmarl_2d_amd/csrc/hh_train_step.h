/*
 * hh_train_step.h — what turns the PPO learner's minibatch step into a fixed chain of launches that a HIP graph can replay (C ABI at the
 * end of include/hh_learner.h): the Adam step of a whole module on the device (hh_adam_step), the minibatch's columns copied into
 * fixed-address staging buffers by a schedule table and a cursor that live on the device (hh_minibatch_stage; through an order table,
 * for shuffled minibatches: hh_minibatch_stage_gather), and the step's bookkeeping (hh_train_commit).  Included from hh_world.hip (g_err, HIPCHK).
 *
 * The counter hazard.  Two device counters steer a replayed step: the CURSOR (which schedule row the stage reads, which row of the
 * statistics table the commit fills) and Adam's T (the number of steps taken, from which the bias corrections follow).  Both change once
 * per step, and no launch may read a counter that a thread of the same launch writes: workgroups of one launch run in no defined order, so
 * a late workgroup could see the next step's value.  Hence the counters are READ-ONLY in hh_k_minibatch_stage (cursor) and in
 * hh_k_adam_step (t), and they are written by hh_k_train_commit alone, a launch of ONE thread that the stream orders after the Adam
 * launch of the step and before the stage launch of the next one.  A step is stage -> forward -> loss -> backward -> adam -> commit.
 *
 * Both streaming kernels are memory-bound and move every byte once: 16-byte accesses where pointers and sizes allow, 256-thread
 * workgroups, grid-stride under a cap on the grid.  No atomics, no allocation, no host synchronisation.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hh_learner.h"

#define HTS_THREADS 256
#define HTS_ADAM_TILE (HTS_THREADS * 4 * 4)   /* elements of one tensor that one workgroup steps: four float4 per thread */
#define HTS_STAGE_MAX_BLOCKS 512              /* workgroups per column of the stage (grid-stride beyond) */

/* ------------------------------------------------------------------------------------------------------------------ Adam */
struct hts_adam_desc {
    float *p; const float *g; float *m; float *v;
    int64_t n;
    int32_t first_block;   /* the launch's workgroups [first_block, next first_block) step this tensor, HTS_ADAM_TILE elements each */
    int32_t vec;           /* 1: all four pointers are 16-byte aligned, the float4 body covers n / 4 * 4 elements; 0: every element is scalar */
};
struct hts_adam_args {
    hts_adam_desc t[HH_ADAM_MAX_TENSORS];
    int32_t n_tensors, n_blocks;
    double lr, beta1, beta2, eps;
};

struct hts_adam_coef { double omb1, omb2, step_size, bc2_sqrt, eps; };

/* One element, in float64 from float32 inputs, each stored value rounded to float32 ONCE: m and v are the correctly rounded moving averages
 * (half an ulp from the exact update of the stored state; float32 arithmetic rounds three to four times and carries the float32
 * coefficient's own error), and p moves by the float64 step computed from the stored m and v.  The kernel stays memory-bound: 28 bytes
 * move per element against a few dozen float64 operations. */
__device__ __forceinline__ void hts_adam_elem(const hts_adam_coef &c, float g, float &p, float &m, float &v) {
    const double gd = (double)g;
    m = (float)fma(c.omb1, gd - (double)m, (double)m);
    v = (float)fma(c.omb2, gd * gd - (double)v, (double)v);
    const double denom = sqrt((double)v) / c.bc2_sqrt + c.eps;
    p = (float)((double)p - c.step_size * ((double)m / denom));
}

__global__ __launch_bounds__(HTS_THREADS) void hh_k_adam_step(const hts_adam_args a, const int32_t *__restrict__ step) {
    __shared__ hts_adam_coef s_c;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        /* the bias corrections in float64, once per workgroup: t = steps taken so far + 1 */
        const double t = (double)(step[0] + 1);
        const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
        s_c.omb1 = 1.0 - a.beta1;
        s_c.omb2 = 1.0 - a.beta2;
        s_c.step_size = a.lr / bc1;
        s_c.bc2_sqrt = sqrt(bc2);
        s_c.eps = a.eps;
    }
    /* which tensor: first_block is ascending, at most HH_ADAM_MAX_TENSORS entries, uniform over the workgroup */
    int lo = 0, hi = a.n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.t[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const hts_adam_desc d = a.t[lo];
    __syncthreads();
    const hts_adam_coef c = s_c;
    const int64_t e0 = (int64_t)(b - d.first_block) * HTS_ADAM_TILE;
    const int64_t e1 = e0 + HTS_ADAM_TILE < d.n ? e0 + HTS_ADAM_TILE : d.n;
    const int64_t body = d.vec ? (d.n & ~(int64_t)3) : 0;          /* tiles start at multiples of 4, so the body of a tile ends at min(e1, body) */
    const int64_t v1 = e1 < body ? e1 : body;
    for (int64_t i = e0 + (int64_t)threadIdx.x * 4; i < v1; i += HTS_THREADS * 4) {
        const float4 g = *reinterpret_cast<const float4 *>(d.g + i);
        float4 p = *reinterpret_cast<float4 *>(d.p + i), m = *reinterpret_cast<float4 *>(d.m + i), v = *reinterpret_cast<float4 *>(d.v + i);
        hts_adam_elem(c, g.x, p.x, m.x, v.x);
        hts_adam_elem(c, g.y, p.y, m.y, v.y);
        hts_adam_elem(c, g.z, p.z, m.z, v.z);
        hts_adam_elem(c, g.w, p.w, m.w, v.w);
        *reinterpret_cast<float4 *>(d.p + i) = p;
        *reinterpret_cast<float4 *>(d.m + i) = m;
        *reinterpret_cast<float4 *>(d.v + i) = v;
    }
    /* the scalar tail: what the body leaves of this tile (n not a multiple of 4), or all of it (pointers only 4-byte aligned) */
    for (int64_t i = (v1 > e0 ? v1 : e0) + threadIdx.x; i < e1; i += HTS_THREADS) {
        float p = d.p[i], m = d.m[i], v = d.v[i];
        hts_adam_elem(c, d.g[i], p, m, v);
        d.p[i] = p; d.m[i] = m; d.v[i] = v;
    }
}

/* the host side of an Adam step: the arguments checked, then the list packed into launches of at most HH_ADAM_MAX_TENSORS descriptors;
 * launch(blocks, args) enqueues one of them (hh_k_adam_step here, hh_k_adam_step_clipped in hh_grad_clip.h) */
template <typename Launch>
static int hts_adam_run(int32_t n_tensors, const hh_adam_tensor *t, const int32_t *step, double lr, double beta1, double beta2, double eps, Launch launch) {
    if (n_tensors < 0 || !step || (n_tensors > 0 && !t)) { g_err = "hh_adam_step: null argument or negative count"; return HH_E_ARG; }
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) {
        g_err = "hh_adam_step: need lr >= 0, 0 <= beta < 1, eps >= 0"; return HH_E_ARG;
    }
    for (int32_t i = 0; i < n_tensors; i++) {
        if (t[i].n < 0 || (t[i].n > 0 && (!t[i].p || !t[i].g || !t[i].m || !t[i].v))) { g_err = "hh_adam_step: a tensor with a null pointer or a negative count"; return HH_E_ARG; }
        if (t[i].n > 0 && ((reinterpret_cast<uintptr_t>(t[i].p) | reinterpret_cast<uintptr_t>(t[i].g) | reinterpret_cast<uintptr_t>(t[i].m) |
                            reinterpret_cast<uintptr_t>(t[i].v)) & 3)) { g_err = "hh_adam_step: every tensor must be 4-byte aligned"; return HH_E_ARG; }
        if (t[i].n > ((int64_t)1 << 40)) { g_err = "hh_adam_step: a tensor of more than 2^40 elements"; return HH_E_ARG; }
    }
    int32_t i = 0;
    while (i < n_tensors) {
        hts_adam_args a;
        memset(&a, 0, sizeof(a));
        a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
        int64_t blocks = 0;
        int32_t k = 0;
        for (; i < n_tensors && k < HH_ADAM_MAX_TENSORS; i++) {
            if (t[i].n == 0) continue;
            const int64_t nb = (t[i].n + HTS_ADAM_TILE - 1) / HTS_ADAM_TILE;
            if (blocks + nb > 0x7fffffff) {
                if (k == 0) { g_err = "hh_adam_step: a tensor too large for one launch"; return HH_E_ARG; }
                break;   /* the next launch takes it */
            }
            hts_adam_desc &d = a.t[k++];
            d.p = t[i].p; d.g = t[i].g; d.m = t[i].m; d.v = t[i].v; d.n = t[i].n;
            d.first_block = (int32_t)blocks;
            d.vec = ((reinterpret_cast<uintptr_t>(d.p) | reinterpret_cast<uintptr_t>(d.g) | reinterpret_cast<uintptr_t>(d.m) |
                      reinterpret_cast<uintptr_t>(d.v)) & 15) == 0;
            blocks += nb;
        }
        if (k == 0) continue;
        a.n_tensors = k; a.n_blocks = (int32_t)blocks;
        launch((unsigned)blocks, a);
        HIPCHK(hipGetLastError());
    }
    return HH_OK;
}

extern "C" int hh_adam_step(int32_t n_tensors, const hh_adam_tensor *t, const int32_t *step, double lr, double beta1, double beta2, double eps,
                            void *stream) {
    return hts_adam_run(n_tensors, t, step, lr, beta1, beta2, eps, [=](unsigned blocks, const hts_adam_args &a) {
        hipLaunchKernelGGL(hh_k_adam_step, dim3(blocks), dim3(HTS_THREADS), 0, (hipStream_t)stream, a, step);
    });
}

/* ------------------------------------------------------------------------------------------------------------------ the stage */
struct hts_stage_col { const unsigned char *src; unsigned char *dst; int64_t chunk_bytes; int32_t unit_log2, pad; };
struct hts_stage_args {
    hts_stage_col c[HH_STAGE_MAX_COLS];
    int32_t cap, sched_rows;
    int64_t src_chunks;
};

template <typename T>
__device__ __forceinline__ void hts_copy_zero(const unsigned char *src, unsigned char *dst, int64_t n_copy, int64_t n_all) {
    /* units [0, n_copy) come from src, units [n_copy, n_all) become zero: ONE pass over the staging buffer */
    const T *s = reinterpret_cast<const T *>(src);
    T *d = reinterpret_cast<T *>(dst);
    const T zero{};
    const int64_t stride = (int64_t)gridDim.x * HTS_THREADS;
    const int64_t first = (int64_t)blockIdx.x * HTS_THREADS + threadIdx.x;
    int64_t i = first;
    for (; i + 3 * stride < n_copy; i += 4 * stride) {      /* four loads in flight per thread: one per trip leaves the copy latency-bound */
        const T a = s[i], b = s[i + stride], c = s[i + 2 * stride], e = s[i + 3 * stride];
        d[i] = a; d[i + stride] = b; d[i + 2 * stride] = c; d[i + 3 * stride] = e;
    }
    for (; i < n_copy; i += stride) d[i] = s[i];
    for (; i < n_all; i += stride) d[i] = zero;
}

__global__ __launch_bounds__(HTS_THREADS) void hh_k_minibatch_stage(const hts_stage_args a, const int32_t *__restrict__ schedule,
                                                                    const int32_t *__restrict__ cursor, int32_t *__restrict__ n_valid) {
    const int cur = cursor[0];
    int64_t s0 = 0, s1 = 0;
    int32_t nv = 0;
    if (cur >= 0 && cur < a.sched_rows) {       /* a cursor beyond the table stages an empty minibatch: zeros everywhere, n_valid = 0 */
        s0 = schedule[4 * cur]; s1 = schedule[4 * cur + 1]; nv = schedule[4 * cur + 2];
    }
    /* whatever the table holds, nothing outside the source or the staging buffers is touched */
    if (s0 < 0) s0 = 0;
    if (s1 > a.src_chunks) s1 = a.src_chunks;
    if (s1 < s0) s1 = s0;
    if (s1 - s0 > a.cap) s1 = s0 + a.cap;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) n_valid[0] = nv;
    const hts_stage_col c = a.c[blockIdx.y];
    const int64_t n_copy = ((s1 - s0) * c.chunk_bytes) >> c.unit_log2, n_all = ((int64_t)a.cap * c.chunk_bytes) >> c.unit_log2;
    const unsigned char *src = c.src + s0 * c.chunk_bytes;
    switch (c.unit_log2) {
        case 4: hts_copy_zero<uint4>(src, c.dst, n_copy, n_all); break;
        case 3: hts_copy_zero<uint2>(src, c.dst, n_copy, n_all); break;
        case 2: hts_copy_zero<uint32_t>(src, c.dst, n_copy, n_all); break;
        case 1: hts_copy_zero<uint16_t>(src, c.dst, n_copy, n_all); break;
        default: hts_copy_zero<unsigned char>(src, c.dst, n_copy, n_all); break;
    }
}

extern "C" int hh_minibatch_stage(int32_t n_cols, const hh_stage_col *cols, int32_t chunk_len, int32_t cap, int64_t src_chunks,
                                  const int32_t *schedule, int32_t sched_rows, const int32_t *cursor, int32_t *n_valid, void *stream) {
    if (n_cols < 0 || n_cols > HH_STAGE_MAX_COLS || cap < 1 || chunk_len < 1 || src_chunks < 0 || sched_rows < 0 || !schedule || !cursor || !n_valid ||
        (n_cols > 0 && !cols)) {
        g_err = "hh_minibatch_stage: need 0 <= n_cols <= 8, cap >= 1, chunk_len >= 1, src_chunks >= 0, sched_rows >= 0 and no null pointer"; return HH_E_ARG;
    }
    hts_stage_args a;
    memset(&a, 0, sizeof(a));
    a.cap = cap; a.sched_rows = sched_rows; a.src_chunks = src_chunks;
    int64_t most = 0;
    for (int32_t i = 0; i < n_cols; i++) {
        const int64_t cb = cols[i].chunk_bytes;
        if (!cols[i].src || !cols[i].dst || cb < 1 || cb % chunk_len || cb > ((int64_t)1 << 30)) {
            g_err = "hh_minibatch_stage: a column with a null pointer, or chunk_bytes that is not a positive multiple of chunk_len (at most 2^30)"; return HH_E_ARG;
        }
        const uintptr_t bits = reinterpret_cast<uintptr_t>(cols[i].src) | reinterpret_cast<uintptr_t>(cols[i].dst) | (uintptr_t)cb;
        int lg = 4;
        while (lg > 0 && (bits & (((uintptr_t)1 << lg) - 1))) lg--;
        a.c[i].src = (const unsigned char *)cols[i].src; a.c[i].dst = (unsigned char *)cols[i].dst; a.c[i].chunk_bytes = cb; a.c[i].unit_log2 = lg;
        const int64_t units = ((int64_t)cap * cb) >> lg;
        if (units > most) most = units;
    }
    if (n_cols == 0) return HH_OK;
    int64_t bx = (most + (int64_t)HTS_THREADS * 4 - 1) / ((int64_t)HTS_THREADS * 4);     /* about four units per thread */
    if (bx < 1) bx = 1;
    if (bx > HTS_STAGE_MAX_BLOCKS) bx = HTS_STAGE_MAX_BLOCKS;
    hipLaunchKernelGGL(hh_k_minibatch_stage, dim3((unsigned)bx, (unsigned)n_cols), dim3(HTS_THREADS), 0, (hipStream_t)stream, a, schedule, cursor, n_valid);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ the gather stage
 * hh_minibatch_stage with the chunks named by an order table: staged chunk i = source chunk order[o0 + i].  The unit of work is a SLOT (one
 * staged chunk), and a group of G = 2^grp_log2 neighbouring lanes (1 .. 64, so a group never leaves its wave) copies it: lane l of the group
 * moves units l, l + G, l + 2 G, ..  of the chunk, so the lanes of a group read and write consecutive units.  The host picks G per column so that a
 * lane moves about four units: G = 1 for the one-unit chunks of the escape kinds (a lane per row), G = 64 for the fight kinds' chunks of
 * hundreds of units (a wave per chunk).  Every lane of a group loads the slot's order entry itself — one address per group, once per slot,
 * not per unit — and no division is needed: slot and lane come from shifts of the thread index.  Slots stride over the grid. */
struct hts_gather_args {
    hts_stage_col c[HH_STAGE_MAX_COLS];       /* `pad` holds grp_log2 here */
    int32_t cap, sched_rows;
    int64_t src_chunks, order_len;
};

template <typename T>
__device__ __forceinline__ void hts_gather_slots(const hts_stage_col &c, const int32_t *__restrict__ order, int64_t o0, int32_t n, int32_t cap,
                                                 int64_t src_chunks) {
    const int g = c.pad;
    const int32_t G = 1 << g, lane = (int32_t)threadIdx.x & (G - 1);
    const int32_t upc = (int32_t)(c.chunk_bytes >> c.unit_log2);                     /* units per chunk: chunk_bytes <= 2^30 */
    const int64_t groups = ((int64_t)gridDim.x * HTS_THREADS) >> g;
    const T zero{};
    for (int64_t slot = ((int64_t)blockIdx.x * HTS_THREADS + threadIdx.x) >> g; slot < cap; slot += groups) {
        T *d = reinterpret_cast<T *>(c.dst + slot * c.chunk_bytes);
        int64_t chunk = -1;
        if (slot < n) chunk = order[o0 + slot];                                     /* o0 + slot < o1 <= order_len */
        int32_t u = lane;
        if (chunk >= 0 && chunk < src_chunks) {
            const T *s = reinterpret_cast<const T *>(c.src + chunk * c.chunk_bytes);
            for (; u + 3 * G < upc; u += 4 * G) {                                   /* four loads in flight per lane, as hts_copy_zero */
                const T a = s[u], b = s[u + G], e = s[u + 2 * G], f = s[u + 3 * G];
                d[u] = a; d[u + G] = b; d[u + 2 * G] = e; d[u + 3 * G] = f;
            }
            for (; u < upc; u += G) d[u] = s[u];
        } else {
            for (; u < upc; u += G) d[u] = zero;                                    /* behind the minibatch, or an entry that names no chunk */
        }
    }
}

__global__ __launch_bounds__(HTS_THREADS) void hh_k_minibatch_stage_gather(const hts_gather_args a, const int32_t *__restrict__ order,
                                                                           const int32_t *__restrict__ schedule,
                                                                           const int32_t *__restrict__ cursor, int32_t *__restrict__ n_valid) {
    const int cur = cursor[0];
    int64_t o0 = 0, o1 = 0;
    int32_t nv = 0;
    if (cur >= 0 && cur < a.sched_rows) {       /* a cursor beyond the table stages an empty minibatch: zeros everywhere, n_valid = 0 */
        o0 = schedule[4 * (int64_t)cur]; o1 = schedule[4 * (int64_t)cur + 1]; nv = schedule[4 * (int64_t)cur + 2];
    }
    /* whatever the tables hold, nothing outside the order table, the source or the staging buffers is touched */
    if (o0 < 0) o0 = 0;
    if (o1 > a.order_len) o1 = a.order_len;
    if (o1 < o0) o1 = o0;
    if (o1 - o0 > a.cap) o1 = o0 + a.cap;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) n_valid[0] = nv;
    const hts_stage_col c = a.c[blockIdx.y];
    const int32_t n = (int32_t)(o1 - o0);
    switch (c.unit_log2) {
        case 4: hts_gather_slots<uint4>(c, order, o0, n, a.cap, a.src_chunks); break;
        case 3: hts_gather_slots<uint2>(c, order, o0, n, a.cap, a.src_chunks); break;
        case 2: hts_gather_slots<uint32_t>(c, order, o0, n, a.cap, a.src_chunks); break;
        case 1: hts_gather_slots<uint16_t>(c, order, o0, n, a.cap, a.src_chunks); break;
        default: hts_gather_slots<unsigned char>(c, order, o0, n, a.cap, a.src_chunks); break;
    }
}

extern "C" int hh_minibatch_stage_gather(int32_t n_cols, const hh_stage_col *cols, int32_t chunk_len, int32_t cap, int64_t src_chunks,
                                         const int32_t *order, int64_t order_len, const int32_t *schedule, int32_t sched_rows,
                                         const int32_t *cursor, int32_t *n_valid, void *stream) {
    if (n_cols < 0 || n_cols > HH_STAGE_MAX_COLS || cap < 1 || chunk_len < 1 || src_chunks < 0 || sched_rows < 0 || order_len < 0 || !order ||
        !schedule || !cursor || !n_valid || (n_cols > 0 && !cols)) {
        g_err = "hh_minibatch_stage_gather: need 0 <= n_cols <= 8, cap >= 1, chunk_len >= 1, src_chunks >= 0, sched_rows >= 0, order_len >= 0 and no null pointer";
        return HH_E_ARG;
    }
    hts_gather_args a;
    memset(&a, 0, sizeof(a));
    a.cap = cap; a.sched_rows = sched_rows; a.src_chunks = src_chunks; a.order_len = order_len;
    int64_t most = 0;
    for (int32_t i = 0; i < n_cols; i++) {
        const int64_t cb = cols[i].chunk_bytes;
        if (!cols[i].src || !cols[i].dst || cb < 1 || cb % chunk_len || cb > ((int64_t)1 << 30)) {
            g_err = "hh_minibatch_stage_gather: a column with a null pointer, or chunk_bytes that is not a positive multiple of chunk_len (at most 2^30)"; return HH_E_ARG;
        }
        const uintptr_t bits = reinterpret_cast<uintptr_t>(cols[i].src) | reinterpret_cast<uintptr_t>(cols[i].dst) | (uintptr_t)cb;
        int lg = 4;
        while (lg > 0 && (bits & (((uintptr_t)1 << lg) - 1))) lg--;
        const int64_t upc = cb >> lg;
        int g = 0;
        while (g < 6 && ((int64_t)4 << g) < upc) g++;          /* the smallest group, up to a wave, whose lanes move at most four units each */
        a.c[i].src = (const unsigned char *)cols[i].src; a.c[i].dst = (unsigned char *)cols[i].dst; a.c[i].chunk_bytes = cb; a.c[i].unit_log2 = lg;
        a.c[i].pad = g;
        const int64_t threads = (int64_t)cap << g;
        if (threads > most) most = threads;
    }
    if (n_cols == 0) return HH_OK;
    int64_t bx = (most + HTS_THREADS - 1) / HTS_THREADS;        /* a group per slot of the widest column, grid-stride beyond the cap */
    if (bx < 1) bx = 1;
    if (bx > HTS_STAGE_MAX_BLOCKS) bx = HTS_STAGE_MAX_BLOCKS;
    hipLaunchKernelGGL(hh_k_minibatch_stage_gather, dim3((unsigned)bx, (unsigned)n_cols), dim3(HTS_THREADS), 0, (hipStream_t)stream, a, order, schedule,
                       cursor, n_valid);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ the commit */
__global__ void hh_k_train_commit(const double *__restrict__ stats, double *__restrict__ table, int32_t table_rows, int32_t *cursor, int32_t *step) {
    const int32_t cur = cursor[0];
    if (cur >= 0 && cur < table_rows)
        for (int k = 0; k < HH_PPO_STATS; k++) table[(int64_t)cur * HH_PPO_STATS + k] = stats[k];
    cursor[0] = cur + 1;
    step[0] = step[0] + 1;
}

extern "C" int hh_train_commit(const double *stats, double *table, int32_t table_rows, int32_t *cursor, int32_t *step, void *stream) {
    if (!stats || !table || !cursor || !step || table_rows < 0) { g_err = "hh_train_commit: null argument or negative count"; return HH_E_ARG; }
    hipLaunchKernelGGL(hh_k_train_commit, dim3(1), dim3(1), 0, (hipStream_t)stream, stats, table, table_rows, cursor, step);
    HIPCHK(hipGetLastError());
    return HH_OK;
}
