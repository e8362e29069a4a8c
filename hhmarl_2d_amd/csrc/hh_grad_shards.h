/*
 * hh_grad_shards.h — the two launches that make a data-parallel minibatch step of W shards give the bytes of ONE process that holds the W
 * shards (C ABI at the end of include/hh_learner.h): hh_grad_pack copies a module's gradients into one flat bucket (the block an
 * all-gather moves), hh_grad_combine turns the W gathered buckets back into the gradients as a weighted sum whose order of additions is
 * the shard order, whatever W is and whichever rank computes it.  Included from hh_world.hip (g_err, HIPCHK) after hh_train_step.h, whose
 * launch shape they share: descriptors by value, at most HH_ADAM_MAX_TENSORS per launch, a workgroup finds its tensor by binary search
 * over first_block and moves one tile of HTS_ADAM_TILE elements.
 *
 * Both are memory-bound and move every byte once.  The bucket side is always float4: the bucket is 16-byte aligned and every offset a
 * multiple of 4 elements.  The gradient side is float4 where its pointer is 16-byte aligned and scalar otherwise — the same values.
 * No atomics, no scratch, no allocation, no host synchronisation.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hh_learner.h"

/* ------------------------------------------------------------------------------------------------------------------ pack */
struct hgs_pack_desc {
    const float *g;        /* NULL: the whole span becomes +0.0f */
    int64_t n;             /* elements copied (0 for a NULL g) */
    int64_t off;           /* the span's first element of the bucket, a multiple of 4 */
    int64_t span;          /* elements of the bucket this tensor's workgroups write: up to the next tensor's off (the last: bucket_elems); a multiple of 4 */
    int32_t first_block;
    int32_t vec;           /* 1: g is 16-byte aligned */
};
struct hgs_pack_args {
    hgs_pack_desc t[HH_ADAM_MAX_TENSORS];
    int32_t n_tensors, n_blocks;
};

__global__ __launch_bounds__(HTS_THREADS) void hh_k_grad_pack(const hgs_pack_args a, float *__restrict__ bucket) {
    const int b = blockIdx.x;
    int lo = 0, hi = a.n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.t[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const hgs_pack_desc d = a.t[lo];
    const int64_t e0 = (int64_t)(b - d.first_block) * HTS_ADAM_TILE;
    const int64_t e1 = e0 + HTS_ADAM_TILE < d.span ? e0 + HTS_ADAM_TILE : d.span;
    float *dst = bucket + d.off;
    /* e0, e1 and the stride are multiples of 4: every trip writes one whole float4 inside the span */
    for (int64_t i = e0 + (int64_t)threadIdx.x * 4; i < e1; i += HTS_THREADS * 4) {
        float4 v;
        if (d.vec && i + 4 <= d.n) {
            v = *reinterpret_cast<const float4 *>(d.g + i);
        } else {                                   /* a 4-byte-aligned gradient, the tensor's last elements, the padding behind them */
            v.x = i     < d.n ? d.g[i]     : 0.0f;
            v.y = i + 1 < d.n ? d.g[i + 1] : 0.0f;
            v.z = i + 2 < d.n ? d.g[i + 2] : 0.0f;
            v.w = i + 3 < d.n ? d.g[i + 3] : 0.0f;
        }
        *reinterpret_cast<float4 *>(dst + i) = v;
    }
}

static int hgs_check_bucket(const char *who, const void *bucket, int64_t bucket_elems) {
    if (!bucket || (reinterpret_cast<uintptr_t>(bucket) & 15) || bucket_elems < 0 || (bucket_elems & 3) || bucket_elems > ((int64_t)1 << 40)) {
        g_err = std::string(who) + ": the bucket is a 16-byte aligned pointer and bucket_elems a multiple of 4 in 0 .. 2^40"; return HH_E_ARG;
    }
    return HH_OK;
}

extern "C" int hh_grad_pack(int32_t n_tensors, const hh_grad_tensor *t, float *bucket, int64_t bucket_elems, void *stream) {
    if (n_tensors < 1 || !t) { g_err = "hh_grad_pack: need at least one tensor (a module without parameters has no bucket)"; return HH_E_ARG; }
    if (hgs_check_bucket("hh_grad_pack", bucket, bucket_elems) != HH_OK) return HH_E_ARG;
    if (t[0].off != 0) { g_err = "hh_grad_pack: the first tensor starts the bucket (off = 0)"; return HH_E_ARG; }
    for (int32_t i = 0; i < n_tensors; i++) {
        const int64_t end = i + 1 < n_tensors ? t[i + 1].off : bucket_elems;
        if (t[i].n < 0 || t[i].off < 0 || (t[i].off & 3) || t[i].off > bucket_elems || t[i].n > bucket_elems - t[i].off || t[i].off + t[i].n > end) {
            g_err = "hh_grad_pack: every tensor needs n >= 0 and an off that is a multiple of 4, ascending, with [off, off + n) inside the bucket and in front of the next tensor";
            return HH_E_ARG;
        }
        if (t[i].g && (reinterpret_cast<uintptr_t>(t[i].g) & 3)) { g_err = "hh_grad_pack: every gradient must be 4-byte aligned"; return HH_E_ARG; }
    }
    int32_t i = 0;
    while (i < n_tensors) {
        hgs_pack_args a;
        memset(&a, 0, sizeof(a));
        int64_t blocks = 0;
        int32_t k = 0;
        for (; i < n_tensors && k < HH_ADAM_MAX_TENSORS; i++) {
            const int64_t span = (i + 1 < n_tensors ? t[i + 1].off : bucket_elems) - t[i].off;
            if (span == 0) continue;
            const int64_t nb = (span + HTS_ADAM_TILE - 1) / HTS_ADAM_TILE;
            if (blocks + nb > 0x7fffffff) {
                if (k == 0) { g_err = "hh_grad_pack: a tensor too large for one launch"; return HH_E_ARG; }
                break;   /* the next launch takes it */
            }
            hgs_pack_desc &d = a.t[k++];
            d.g = t[i].g; d.n = t[i].g ? t[i].n : 0; d.off = t[i].off; d.span = span;
            d.first_block = (int32_t)blocks;
            d.vec = t[i].g && (reinterpret_cast<uintptr_t>(t[i].g) & 15) == 0;
            blocks += nb;
        }
        if (k == 0) continue;
        a.n_tensors = k; a.n_blocks = (int32_t)blocks;
        hipLaunchKernelGGL(hh_k_grad_pack, dim3((unsigned)blocks), dim3(HTS_THREADS), 0, (hipStream_t)stream, a, bucket);
        HIPCHK(hipGetLastError());
    }
    return HH_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ combine */
struct hgs_comb_desc {
    float *g;
    int64_t n, off;
    int32_t first_block;
    int32_t vec;           /* 1: g is 16-byte aligned, the float4 body covers n / 4 * 4 elements */
};
struct hgs_comb_args {
    hgs_comb_desc t[HH_ADAM_MAX_TENSORS];
    double weight[HH_GRAD_MAX_SHARDS];
    int64_t bucket_elems;
    int32_t n_tensors, n_shards;
};

/* the product and the sum are two roundings, whatever the translation unit's contraction mode is */
__device__ __forceinline__ double hgs_first(float b, double w) {
#pragma clang fp contract(off)
    return (double)b * w;
}
__device__ __forceinline__ double hgs_next(double acc, float b, double w) {
#pragma clang fp contract(off)
    const double p = (double)b * w;
    return acc + p;
}

__global__ __launch_bounds__(HTS_THREADS) void hh_k_grad_combine(const hgs_comb_args a, const float *__restrict__ buckets) {
    const int b = blockIdx.x;
    int lo = 0, hi = a.n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.t[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const hgs_comb_desc d = a.t[lo];
    const int W = a.n_shards;
    const int64_t E = a.bucket_elems;
    const float *src = buckets + d.off;          /* shard r's copy of this tensor: src + r E, 16-byte aligned */
    const int64_t e0 = (int64_t)(b - d.first_block) * HTS_ADAM_TILE;
    const int64_t e1 = e0 + HTS_ADAM_TILE < d.n ? e0 + HTS_ADAM_TILE : d.n;
    const int64_t body = d.vec ? (d.n & ~(int64_t)3) : 0;
    const int64_t v1 = e1 < body ? e1 : body;
    for (int64_t i = e0 + (int64_t)threadIdx.x * 4; i < v1; i += HTS_THREADS * 4) {
        const float4 x0 = *reinterpret_cast<const float4 *>(src + i);
        const double w0 = a.weight[0];
        double ax = hgs_first(x0.x, w0), ay = hgs_first(x0.y, w0), az = hgs_first(x0.z, w0), aw = hgs_first(x0.w, w0);
        for (int r = 1; r < W; r++) {
            const float4 x = *reinterpret_cast<const float4 *>(src + (int64_t)r * E + i);
            const double w = a.weight[r];
            ax = hgs_next(ax, x.x, w); ay = hgs_next(ay, x.y, w); az = hgs_next(az, x.z, w); aw = hgs_next(aw, x.w, w);
        }
        float4 o;
        o.x = (float)ax; o.y = (float)ay; o.z = (float)az; o.w = (float)aw;
        *reinterpret_cast<float4 *>(d.g + i) = o;
    }
    /* the scalar tail: what the body leaves of this tile (n not a multiple of 4), or all of it (g only 4-byte aligned) */
    for (int64_t i = (v1 > e0 ? v1 : e0) + threadIdx.x; i < e1; i += HTS_THREADS) {
        double acc = hgs_first(src[i], a.weight[0]);
        for (int r = 1; r < W; r++) acc = hgs_next(acc, src[(int64_t)r * E + i], a.weight[r]);
        d.g[i] = (float)acc;
    }
}

extern "C" int hh_grad_combine(int32_t n_tensors, const hh_grad_tensor *t, const float *buckets, int64_t bucket_elems, int32_t n_shards,
                               const double *weight, void *stream) {
    if (n_tensors < 0 || (n_tensors > 0 && !t) || !weight || n_shards < 1 || n_shards > HH_GRAD_MAX_SHARDS) {
        g_err = "hh_grad_combine: a null argument, a negative count, or n_shards outside 1 .. 64"; return HH_E_ARG;
    }
    if (hgs_check_bucket("hh_grad_combine", buckets, bucket_elems) != HH_OK) return HH_E_ARG;
    for (int32_t i = 0; i < n_tensors; i++) {
        if (t[i].n < 0 || t[i].off < 0 || (t[i].off & 3) || t[i].off > bucket_elems || t[i].n > bucket_elems - t[i].off) {
            g_err = "hh_grad_combine: every tensor needs n >= 0 and an off that is a multiple of 4 with [off, off + n) inside the bucket"; return HH_E_ARG;
        }
        if (t[i].g && (reinterpret_cast<uintptr_t>(t[i].g) & 3)) { g_err = "hh_grad_combine: every gradient must be 4-byte aligned"; return HH_E_ARG; }
    }
    int32_t i = 0;
    while (i < n_tensors) {
        hgs_comb_args a;
        memset(&a, 0, sizeof(a));
        a.bucket_elems = bucket_elems; a.n_shards = n_shards;
        for (int32_t r = 0; r < n_shards; r++) a.weight[r] = weight[r];
        int64_t blocks = 0;
        int32_t k = 0;
        for (; i < n_tensors && k < HH_ADAM_MAX_TENSORS; i++) {
            if (t[i].n == 0 || !t[i].g) continue;          /* a parameter without a gradient receives nothing */
            const int64_t nb = (t[i].n + HTS_ADAM_TILE - 1) / HTS_ADAM_TILE;
            if (blocks + nb > 0x7fffffff) {
                if (k == 0) { g_err = "hh_grad_combine: a tensor too large for one launch"; return HH_E_ARG; }
                break;   /* the next launch takes it */
            }
            hgs_comb_desc &d = a.t[k++];
            d.g = t[i].g; d.n = t[i].n; d.off = t[i].off;
            d.first_block = (int32_t)blocks;
            d.vec = (reinterpret_cast<uintptr_t>(t[i].g) & 15) == 0;
            blocks += nb;
        }
        if (k == 0) continue;
        a.n_tensors = k;
        hipLaunchKernelGGL(hh_k_grad_combine, dim3((unsigned)blocks), dim3(HTS_THREADS), 0, (hipStream_t)stream, a, buckets);
        HIPCHK(hipGetLastError());
    }
    return HH_OK;
}
