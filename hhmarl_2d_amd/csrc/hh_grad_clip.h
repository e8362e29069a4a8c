/*
 * hh_grad_clip.h — gradient clipping by global L2 norm inside the replayable minibatch step (C ABI in include/hh_learner.h, in the section
 * of hh_adam_step): the norm of all gradients of one optimizer and the clip coefficient computed on the device (hh_grad_norm), and the
 * Adam step that scales every gradient it reads by that coefficient (hh_adam_step_clipped).  Included from hh_world.hip after
 * hh_train_step.h (hts_adam_args, hts_adam_elem, hts_adam_run, HTS_THREADS, HTS_ADAM_TILE, g_err, HIPCHK).
 *
 * A step with clipping is stage -> forward -> loss -> backward -> norm (partials, final) -> clipped Adam -> commit: two launches more than
 * without (one more partial launch per further HH_ADAM_MAX_TENSORS tensors).  The counter hazard of hh_train_step.h holds: the final
 * launch only READS the cursor, hh_k_train_commit stays its only writer.
 *
 * The reduction has a fixed order and no atomics, so the same inputs give the same bytes on every run, whatever the alignment of g:
 *   1. a workgroup sums one HTS_ADAM_TILE-element tile of one tensor: thread k takes elements 4k .. 4k+3 of each 1024-element row of the tile
 *      in ascending order (one float4 load where g is 16-byte aligned, four float loads otherwise: the same elements, the same order), adds
 *      their float64 squares to its accumulator, a 64-lane shuffle tree (offsets 32, 16, .. 1) folds the wave, and thread 0 adds the four
 *      waves' sums in wave order through LDS -> ONE float64 per tile in scratch, tiles in list order;
 *   2. ONE workgroup sums the slots the same way (thread k takes slots k, k + 256, ..) and writes clip and the table row.
 * (double)g * (double)g is exact (24 + 24 significant bits), so only the additions round.
 */
#pragma once

#include "hh_train_step.h"

struct hgc_norm_desc {
    const float *g;
    int64_t n;
    int32_t first_block;   /* the launch's workgroups [first_block, next first_block) sum this tensor, HTS_ADAM_TILE elements each */
    int32_t vec;           /* 1: g is 16-byte aligned, whole groups of four are one float4 load */
};
struct hgc_norm_args {
    hgc_norm_desc t[HH_ADAM_MAX_TENSORS];
    int32_t n_tensors, n_blocks;
    int64_t first_slot;    /* workgroup b writes scratch[first_slot + b] */
};

/* the workgroup's sum of one float64 per thread, in a fixed order; the result is valid in thread 0 */
__device__ __forceinline__ double hgc_block_sum(double acc) {
    __shared__ double s_w[HTS_THREADS / 64];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    double sum = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < HTS_THREADS / 64; w++) sum += s_w[w];
    return sum;
}

__global__ __launch_bounds__(HTS_THREADS) void hh_k_grad_norm_partial(const hgc_norm_args a, double *__restrict__ scratch) {
    const int b = blockIdx.x;
    int lo = 0, hi = a.n_tensors - 1;      /* which tensor: first_block is ascending, uniform over the workgroup */
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.t[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const hgc_norm_desc d = a.t[lo];
    const int64_t e0 = (int64_t)(b - d.first_block) * HTS_ADAM_TILE;
    const int64_t e1 = e0 + HTS_ADAM_TILE < d.n ? e0 + HTS_ADAM_TILE : d.n;
    double acc = 0.0;
    for (int64_t i = e0 + (int64_t)threadIdx.x * 4; i < e1; i += HTS_THREADS * 4) {
        if (i + 4 <= e1) {
            float4 g;
            if (d.vec) g = *reinterpret_cast<const float4 *>(d.g + i);       /* tiles start at multiples of 4 */
            else g = make_float4(d.g[i], d.g[i + 1], d.g[i + 2], d.g[i + 3]);
            acc += (double)g.x * (double)g.x;
            acc += (double)g.y * (double)g.y;
            acc += (double)g.z * (double)g.z;
            acc += (double)g.w * (double)g.w;
        } else {
            for (int64_t j = i; j < e1; j++) acc += (double)d.g[j] * (double)d.g[j];     /* the last n % 4 elements of the tensor */
        }
    }
    const double sum = hgc_block_sum(acc);
    if (threadIdx.x == 0) scratch[a.first_slot + b] = sum;
}

__global__ __launch_bounds__(HTS_THREADS) void hh_k_grad_norm_final(const double *__restrict__ scratch, int64_t n_slots, double max_norm,
                                                                    double *__restrict__ clip, const int32_t *__restrict__ cursor,
                                                                    double *__restrict__ table, int32_t table_rows) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n_slots; i += HTS_THREADS) acc += scratch[i];
    const double sum = hgc_block_sum(acc);
    if (threadIdx.x == 0) {
        const double norm = sqrt(sum);
        const double coef = fmin(1.0, max_norm / (norm + 1e-6));     /* torch.nn.utils.clip_grad_norm_'s coefficient */
        clip[0] = norm;
        clip[1] = coef;
        if (cursor) {
            const int32_t cur = cursor[0];
            if (cur >= 0 && cur < table_rows) table[cur] = norm;
        }
    }
}

/* the tiles of the list, or -1 for a bad tensor (g_err set) */
static int64_t hgc_tiles(const char *who, int32_t n_tensors, const hh_adam_tensor *t) {
    if (n_tensors < 0 || (n_tensors > 0 && !t)) { g_err = std::string(who) + ": null argument or negative count"; return -1; }
    int64_t tiles = 0;
    for (int32_t i = 0; i < n_tensors; i++) {
        if (t[i].n < 0 || (t[i].n > 0 && !t[i].g)) { g_err = std::string(who) + ": a tensor with a null gradient or a negative count"; return -1; }
        if (t[i].n > 0 && (reinterpret_cast<uintptr_t>(t[i].g) & 3)) { g_err = std::string(who) + ": every gradient must be 4-byte aligned"; return -1; }
        if (t[i].n > ((int64_t)1 << 40)) { g_err = std::string(who) + ": a tensor of more than 2^40 elements"; return -1; }
        tiles += (t[i].n + HTS_ADAM_TILE - 1) / HTS_ADAM_TILE;
    }
    return tiles;
}

extern "C" int hh_grad_norm_scratch_bytes(int32_t n_tensors, const hh_adam_tensor *t, int64_t *bytes) {
    if (!bytes) { g_err = "hh_grad_norm_scratch_bytes: null argument"; return HH_E_ARG; }
    const int64_t tiles = hgc_tiles("hh_grad_norm_scratch_bytes", n_tensors, t);
    if (tiles < 0) return HH_E_ARG;
    *bytes = 8 * tiles;
    return HH_OK;
}

extern "C" int hh_grad_norm(int32_t n_tensors, const hh_adam_tensor *t, double max_norm, double *clip, const int32_t *cursor, double *table,
                            int32_t table_rows, void *scratch, int64_t scratch_bytes, void *stream) {
    const int64_t tiles = hgc_tiles("hh_grad_norm", n_tensors, t);
    if (tiles < 0) return HH_E_ARG;
    if (!clip || !(max_norm > 0.0) || !isfinite(max_norm)) { g_err = "hh_grad_norm: need clip and a finite max_norm > 0"; return HH_E_ARG; }
    if ((cursor == nullptr) != (table == nullptr) || table_rows < 0) { g_err = "hh_grad_norm: cursor and table come together, table_rows >= 0"; return HH_E_ARG; }
    if (scratch_bytes < 8 * tiles || (tiles > 0 && !scratch) || (tiles > 0 && (reinterpret_cast<uintptr_t>(scratch) & 7))) {
        g_err = "hh_grad_norm: scratch is smaller than hh_grad_norm_scratch_bytes or not 8-byte aligned"; return HH_E_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    int64_t slot = 0;
    int32_t i = 0;
    while (i < n_tensors) {
        hgc_norm_args a;
        memset(&a, 0, sizeof(a));
        a.first_slot = slot;
        int64_t blocks = 0;
        int32_t k = 0;
        for (; i < n_tensors && k < HH_ADAM_MAX_TENSORS; i++) {
            if (t[i].n == 0) continue;
            const int64_t nb = (t[i].n + HTS_ADAM_TILE - 1) / HTS_ADAM_TILE;
            if (blocks + nb > 0x7fffffff) {
                if (k == 0) { g_err = "hh_grad_norm: a tensor too large for one launch"; return HH_E_ARG; }   /* n <= 2^40 has at most 2^28 tiles: not reached */
                break;   /* the next launch takes it */
            }
            hgc_norm_desc &d = a.t[k++];
            d.g = t[i].g; d.n = t[i].n;
            d.first_block = (int32_t)blocks;
            d.vec = (reinterpret_cast<uintptr_t>(d.g) & 15) == 0;
            blocks += nb;
        }
        if (k == 0) continue;
        a.n_tensors = k; a.n_blocks = (int32_t)blocks;
        hipLaunchKernelGGL(hh_k_grad_norm_partial, dim3((unsigned)blocks), dim3(HTS_THREADS), 0, st, a, (double *)scratch);
        HIPCHK(hipGetLastError());
        slot += blocks;
    }
    /* ONE final launch over all slots, also for an empty list: clip = (0, min(1, max_norm / 1e-6)) */
    hipLaunchKernelGGL(hh_k_grad_norm_final, dim3(1), dim3(HTS_THREADS), 0, st, (const double *)scratch, slot, max_norm, clip, cursor, table, table_rows);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ the clipped Adam step */
/* hh_k_adam_step with every gradient read as (float)((double)g * clip[1]): one rounding to float32, then hts_adam_elem as it stands, so a
 * coefficient of 1.0 leaves hh_k_adam_step's bytes.  The coefficient is read once per workgroup, next to the bias corrections. */
__device__ __forceinline__ float hgc_scaled(float g, double coef) { return (float)((double)g * coef); }

__global__ __launch_bounds__(HTS_THREADS) void hh_k_adam_step_clipped(const hts_adam_args a, const int32_t *__restrict__ step, const double *__restrict__ clip) {
    __shared__ hts_adam_coef s_c;
    __shared__ double s_coef;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        const double t = (double)(step[0] + 1);
        const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
        s_c.omb1 = 1.0 - a.beta1;
        s_c.omb2 = 1.0 - a.beta2;
        s_c.step_size = a.lr / bc1;
        s_c.bc2_sqrt = sqrt(bc2);
        s_c.eps = a.eps;
        s_coef = clip[1];
    }
    int lo = 0, hi = a.n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.t[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const hts_adam_desc d = a.t[lo];
    __syncthreads();
    const hts_adam_coef c = s_c;
    const double coef = s_coef;
    const int64_t e0 = (int64_t)(b - d.first_block) * HTS_ADAM_TILE;
    const int64_t e1 = e0 + HTS_ADAM_TILE < d.n ? e0 + HTS_ADAM_TILE : d.n;
    const int64_t body = d.vec ? (d.n & ~(int64_t)3) : 0;
    const int64_t v1 = e1 < body ? e1 : body;
    for (int64_t i = e0 + (int64_t)threadIdx.x * 4; i < v1; i += HTS_THREADS * 4) {
        const float4 g = *reinterpret_cast<const float4 *>(d.g + i);
        float4 p = *reinterpret_cast<float4 *>(d.p + i), m = *reinterpret_cast<float4 *>(d.m + i), v = *reinterpret_cast<float4 *>(d.v + i);
        hts_adam_elem(c, hgc_scaled(g.x, coef), p.x, m.x, v.x);
        hts_adam_elem(c, hgc_scaled(g.y, coef), p.y, m.y, v.y);
        hts_adam_elem(c, hgc_scaled(g.z, coef), p.z, m.z, v.z);
        hts_adam_elem(c, hgc_scaled(g.w, coef), p.w, m.w, v.w);
        *reinterpret_cast<float4 *>(d.p + i) = p;
        *reinterpret_cast<float4 *>(d.m + i) = m;
        *reinterpret_cast<float4 *>(d.v + i) = v;
    }
    for (int64_t i = (v1 > e0 ? v1 : e0) + threadIdx.x; i < e1; i += HTS_THREADS) {
        float p = d.p[i], m = d.m[i], v = d.v[i];
        hts_adam_elem(c, hgc_scaled(d.g[i], coef), p, m, v);
        d.p[i] = p; d.m[i] = m; d.v[i] = v;
    }
}

extern "C" int hh_adam_step_clipped(int32_t n_tensors, const hh_adam_tensor *t, const int32_t *step, const double *clip, double lr, double beta1,
                                    double beta2, double eps, void *stream) {
    if (!clip) { g_err = "hh_adam_step_clipped: null clip"; return HH_E_ARG; }
    return hts_adam_run(n_tensors, t, step, lr, beta1, beta2, eps, [=](unsigned blocks, const hts_adam_args &a) {
        hipLaunchKernelGGL(hh_k_adam_step_clipped, dim3(blocks), dim3(HTS_THREADS), 0, (hipStream_t)stream, a, step, clip);
    });
}
