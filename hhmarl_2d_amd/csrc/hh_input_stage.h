/*
 * hh_input_stage.h — what the five trainable networks do in front of shared_layer, for the learners (learner.input_stage; C ABI and the
 * formulas: include/hh_learner.h): G <= 4 layers y_g = tanh(W_g gather_g(src) + b_g) from ONE source matrix, each written straight into
 * its columns of a concatenated output, and their weight and bias gradients.  There is no input gradient.
 *
 * Forward, one launch.  A workgroup of 512 lanes walks the row tiles (32 rows) grid-stride.  Per tile it stages the gathered inputs of
 * all groups once in LDS, k-major ([sum K][32 rows], row stride 36 words: a lane reads four rows of one input with one 16-byte read that
 * the lanes of a group share), by 4-byte loads — source rows are 26 / 57 / 66 / 105 floats, nothing wider is aligned.  Lane t owns
 * output column t of the concatenation (sum n_out <= 500): 32 accumulators, one per row, its weight row read k by k from global memory
 * (a stride of K floats from lane to lane, again for every tile; the whole set of a call is at most 224 KB), plain fmaf in k order,
 * tanhf, and 32 stores, each of which writes consecutive floats of one row from consecutive lanes.
 *
 * Backward, two launches.  Pass 1: grid (parts, column blocks of 64).  Lane = column, the four waves of a workgroup take the inputs
 * k = wave, wave + 4, ...: at most 28 accumulators per lane that live in registers over the whole grid-stride walk of the workgroup's
 * row tiles.  Per tile d_pre = d_y (1 - y^2) of the 64 columns goes through LDS once (each wave computes 8 of the 32 rows); wave 0 also
 * sums it for d_b, in float64: that is one long sum per column.  The workgroup's sums go to its slot of `scratch` as float32.
 * Pass 2: one lane per element of d_w | d_b adds the `parts` slots in slot order, in float64, and rounds once.
 * parts = min(HH_INSTAGE_MAX_PARTS, row tiles): no atomics, the same bytes on every run, and the scratch stops growing at
 * HH_INSTAGE_MAX_PARTS * 32 rows.
 */
#ifndef HH_INPUT_STAGE_H
#define HH_INPUT_STAGE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hh_learner.h"

#define HIS_FWD_THREADS 512
#define HIS_BWD_THREADS 256
#define HIS_TR 32                      /* rows per tile */
#define HIS_TRP 36                     /* row stride of the staged inputs: 16-byte aligned rows */
#define HIS_FWD_MAX_GRID 2048          /* forward workgroups: beyond this many tiles they walk grid-stride */
#define HIS_COLS 64                    /* backward: columns per workgroup, one per lane of a wave */
#define HIS_KW (HIS_BWD_THREADS / 64)  /* backward: waves per workgroup, wave q takes k = q (mod HIS_KW) */
#define HIS_KACC ((HH_INSTAGE_MAX_K + HIS_KW - 1) / HIS_KW)

static_assert(HH_INSTAGE_MAX_OUT <= HIS_FWD_THREADS, "one forward lane per output column");
static_assert(HIS_TR == 8 * HIS_KW, "each backward wave computes 8 rows of d_pre per tile");

struct his_group {
    int32_t n_out, k, k_off, n_off, w_off; /* K; first staged input; first column of the concatenation; first element in a scratch slot */
    int32_t n_seg;
    int16_t seg_col[HH_INSTAGE_MAX_SEGS], seg_len[HH_INSTAGE_MAX_SEGS];
    const float *w, *b, *y_in, *d_y;
    float *y, *d_w, *d_b;
    int64_t y_ld, d_y_ld;
};

struct his_args {
    int32_t n_groups, k_total, n_total, w_total; /* sums over the groups of K, n_out, n_out * K */
    his_group g[HH_INSTAGE_MAX_GROUPS];
};

/* the group that holds column n of the concatenation, picked with selects (no indexing of the kernel arguments by a register) */
#define HIS_PICK(a, n, field) \
    ((a).n_groups > 3 && (n) >= (a).g[3].n_off ? (a).g[3].field : (a).n_groups > 2 && (n) >= (a).g[2].n_off ? (a).g[2].field : \
     (a).n_groups > 1 && (n) >= (a).g[1].n_off ? (a).g[1].field : (a).g[0].field)

/* colmap[kk] = the source column of staged input kk */
__device__ __forceinline__ void his_build_colmap(const his_args &a, int *colmap, int t, int nt) {
    for (int kk = t; kk < a.k_total; kk += nt) {
        int col = 0;
#pragma unroll
        for (int gi = 0; gi < HH_INSTAGE_MAX_GROUPS; gi++) {
            if (gi < a.n_groups && kk >= a.g[gi].k_off && kk < a.g[gi].k_off + a.g[gi].k) {
                int rest = kk - a.g[gi].k_off;
                bool found = false;
#pragma unroll
                for (int s = 0; s < HH_INSTAGE_MAX_SEGS; s++) {
                    if (s < a.g[gi].n_seg && !found) {
                        const int len = a.g[gi].seg_len[s];
                        if (rest < len) {
                            col = a.g[gi].seg_col[s] + rest;
                            found = true;
                        } else {
                            rest -= len;
                        }
                    }
                }
            }
        }
        colmap[kk] = col;
    }
}

/* xs[kk][r] = src[row0 + r][colmap[kk]], 0 in the rows beyond the last one; consecutive lanes read consecutive inputs of one row */
__device__ __forceinline__ void his_stage(float *__restrict__ xs, const int *__restrict__ colmap, const float *__restrict__ src, int64_t src_ld,
                                          int64_t row0, int rows, int k_total, int t, int nt) {
    const int n = HIS_TR * k_total;
    for (int e = t; e < n; e += nt) {
        const int r = e / k_total, kk = e - r * k_total;
        xs[kk * HIS_TRP + r] = r < rows ? src[(row0 + r) * src_ld + colmap[kk]] : 0.0f;
    }
}

__global__ __launch_bounds__(HIS_FWD_THREADS) void hh_k_input_stage_fwd(his_args a, int64_t n_rows, const float *__restrict__ src, int64_t src_ld) {
    extern __shared__ float4 his_lds_fwd[];
    float *xs = reinterpret_cast<float *>(his_lds_fwd);
    int *colmap = reinterpret_cast<int *>(xs + a.k_total * HIS_TRP);
    const int t = threadIdx.x;
    his_build_colmap(a, colmap, t, HIS_FWD_THREADS);
    const bool on = t < a.n_total;
    const int n = on ? t : 0;
    const int j = n - HIS_PICK(a, n, n_off), K = HIS_PICK(a, n, k);
    const float *wr = HIS_PICK(a, n, w) + (int64_t)j * K;
    const float bias = on ? HIS_PICK(a, n, b)[j] : 0.0f;
    const float *xk = xs + HIS_PICK(a, n, k_off) * HIS_TRP;
    float *yc = HIS_PICK(a, n, y) + j;
    const int64_t y_ld = HIS_PICK(a, n, y_ld);
    __syncthreads();
    const int64_t n_tiles = (n_rows + HIS_TR - 1) / HIS_TR;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * HIS_TR;
        const int rows = (int)(n_rows - row0 < HIS_TR ? n_rows - row0 : HIS_TR);
        his_stage(xs, colmap, src, src_ld, row0, rows, a.k_total, t, HIS_FWD_THREADS);
        __syncthreads();
        if (on) {
            float acc[HIS_TR];
#pragma unroll
            for (int r = 0; r < HIS_TR; r++) acc[r] = bias;
#pragma unroll 2
            for (int k = 0; k < K; k++) {
                const float wv = wr[k];
                const float4 *xr = reinterpret_cast<const float4 *>(xk + k * HIS_TRP);
#pragma unroll
                for (int r4 = 0; r4 < HIS_TR / 4; r4++) {
                    const float4 x = xr[r4];
                    acc[4 * r4 + 0] = fmaf(wv, x.x, acc[4 * r4 + 0]);
                    acc[4 * r4 + 1] = fmaf(wv, x.y, acc[4 * r4 + 1]);
                    acc[4 * r4 + 2] = fmaf(wv, x.z, acc[4 * r4 + 2]);
                    acc[4 * r4 + 3] = fmaf(wv, x.w, acc[4 * r4 + 3]);
                }
            }
            float *yo = yc + row0 * y_ld;
#pragma unroll
            for (int r = 0; r < HIS_TR; r++)
                if (r < rows) yo[r * y_ld] = tanhf(acc[r]);
        }
        __syncthreads();
    }
}

/* pass 1 of the backward: slot blockIdx.x of `part` ([parts][w_total + n_total]) = this workgroup's sums over its row tiles */
__global__ __launch_bounds__(HIS_BWD_THREADS) void hh_k_input_stage_bwd(his_args a, int64_t n_rows, const float *__restrict__ src, int64_t src_ld,
                                                                        float *__restrict__ part) {
    extern __shared__ float4 his_lds_bwd[];
    float *dps = reinterpret_cast<float *>(his_lds_bwd);            /* d_pre [32 rows][64 columns] */
    float *xs = dps + HIS_TR * HIS_COLS;
    int *colmap = reinterpret_cast<int *>(xs + a.k_total * HIS_TRP);
    const int t = threadIdx.x, lane = t & 63, q = t >> 6;
    his_build_colmap(a, colmap, t, HIS_BWD_THREADS);
    const int col = blockIdx.y * HIS_COLS + lane;
    const bool on = col < a.n_total;
    const int n = on ? col : 0;
    const int j = n - HIS_PICK(a, n, n_off), K = on ? HIS_PICK(a, n, k) : 0;
    const float *xk = xs + HIS_PICK(a, n, k_off) * HIS_TRP;
    const float *yc = HIS_PICK(a, n, y_in) + j, *gc = HIS_PICK(a, n, d_y) + j;
    const int64_t y_ld = HIS_PICK(a, n, y_ld), g_ld = HIS_PICK(a, n, d_y_ld);
    float acc[HIS_KACC];
    double accb = 0.0;      /* d_b is one sum of all rows per column: float64 here and in pass 2 keeps it as exact as a tree sum */
#pragma unroll
    for (int i = 0; i < HIS_KACC; i++) acc[i] = 0.0f;
    __syncthreads();
    const int64_t n_tiles = (n_rows + HIS_TR - 1) / HIS_TR;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * HIS_TR;
        const int rows = (int)(n_rows - row0 < HIS_TR ? n_rows - row0 : HIS_TR);
        his_stage(xs, colmap, src, src_ld, row0, rows, a.k_total, t, HIS_BWD_THREADS);
#pragma unroll
        for (int u = 0; u < HIS_TR / HIS_KW; u++) {
            const int r = q * (HIS_TR / HIS_KW) + u;
            float dp = 0.0f;
            if (on && r < rows) {
                const float yv = yc[(row0 + r) * y_ld], gv = gc[(row0 + r) * g_ld];
                dp = gv * (1.0f - yv * yv);
            }
            dps[r * HIS_COLS + lane] = dp;
        }
        __syncthreads();
#pragma unroll 1
        for (int r4 = 0; r4 < HIS_TR / 4; r4++) {
            const float d0 = dps[(4 * r4 + 0) * HIS_COLS + lane], d1 = dps[(4 * r4 + 1) * HIS_COLS + lane];
            const float d2 = dps[(4 * r4 + 2) * HIS_COLS + lane], d3 = dps[(4 * r4 + 3) * HIS_COLS + lane];
            accb += (double)((d0 + d1) + (d2 + d3));
#pragma unroll
            for (int i = 0; i < HIS_KACC; i++) {
                const int k = q + HIS_KW * i;
                if (k < K) {
                    const float4 x = *reinterpret_cast<const float4 *>(xk + k * HIS_TRP + 4 * r4);
                    acc[i] = fmaf(d3, x.w, fmaf(d2, x.z, fmaf(d1, x.y, fmaf(d0, x.x, acc[i]))));
                }
            }
        }
        __syncthreads();
    }
    if (on) {
        float *slot = part + (int64_t)blockIdx.x * (a.w_total + a.n_total);
        float *wo = slot + HIS_PICK(a, n, w_off) + (int64_t)j * K;
#pragma unroll
        for (int i = 0; i < HIS_KACC; i++) {
            const int k = q + HIS_KW * i;
            if (k < K) wo[k] = acc[i];
        }
        if (q == 0) slot[a.w_total + n] = (float)accb;
    }
}

/* pass 2: element e of [d_w of group 0 | ... | d_b of all columns] = the sum of the slots in slot order */
__global__ __launch_bounds__(HIS_BWD_THREADS) void hh_k_input_stage_reduce(his_args a, int parts, const float *__restrict__ part) {
    const int entries = a.w_total + a.n_total;
    const int e = blockIdx.x * HIS_BWD_THREADS + threadIdx.x;
    if (e >= entries) return;
    double sum = part[e];
    for (int p = 1; p < parts; p++) sum += (double)part[(int64_t)p * entries + e];
    const float s = (float)sum;
    if (e >= a.w_total) {
        const int n = e - a.w_total;
        HIS_PICK(a, n, d_b)[n - HIS_PICK(a, n, n_off)] = s;
    } else {
        /* the groups' weight blocks follow one another as their columns do: pick by w_off */
        float *dst = a.g[0].d_w;
        int off = 0;
#pragma unroll
        for (int gi = 1; gi < HH_INSTAGE_MAX_GROUPS; gi++)
            if (gi < a.n_groups && e >= a.g[gi].w_off) { dst = a.g[gi].d_w; off = a.g[gi].w_off; }
        dst[e - off] = s;
    }
}

/* ---- the C ABI ---- */
/* four layers of HH_INSTAGE_MAX_K inputs stage 66 KB; the networks' own stages need at most 31 KB */
template <typename F>
static int his_allow_lds(F kernel, size_t lds) {
    if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return HH_OK;
}

static int64_t his_parts(int64_t n_rows) {
    const int64_t tiles = (n_rows + HIS_TR - 1) / HIS_TR;
    return tiles < HH_INSTAGE_MAX_PARTS ? tiles : HH_INSTAGE_MAX_PARTS;
}

/* the shape checks both passes share; fills `a` */
static int his_check(const char *who, int64_t n_rows, int64_t src_ld, int32_t src_width, int32_t n_groups, const hh_input_group *g, bool io, his_args *a) {
    const std::string w(who);
    if (n_groups < 1 || n_groups > HH_INSTAGE_MAX_GROUPS || !g) { g_err = w + ": 1 .. 4 groups"; return HH_E_ARG; }
    if (n_rows < 0 || src_width < 1 || src_ld < src_width) { g_err = w + ": need n_rows >= 0 and src_ld >= src_width >= 1"; return HH_E_ARG; }
    memset(a, 0, sizeof(*a));
    a->n_groups = n_groups;
    for (int gi = 0; gi < n_groups; gi++) {
        const hh_input_group &in = g[gi];
        his_group &o = a->g[gi];
        if (in.n_out < 1 || in.n_seg < 1 || in.n_seg > HH_INSTAGE_MAX_SEGS) { g_err = w + ": a group needs n_out >= 1 and 1 .. 6 segments"; return HH_E_ARG; }
        int k = 0;
        for (int s = 0; s < in.n_seg; s++) {
            if (in.seg_col[s] < 0 || in.seg_len[s] < 1 || (int)in.seg_col[s] + (int)in.seg_len[s] > src_width) {
                g_err = w + ": a segment is empty or reaches outside the source row";
                return HH_E_ARG;
            }
            o.seg_col[s] = in.seg_col[s];
            o.seg_len[s] = in.seg_len[s];
            k += in.seg_len[s];
        }
        if (k > HH_INSTAGE_MAX_K) { g_err = w + ": a layer has more than HH_INSTAGE_MAX_K inputs"; return HH_E_ARG; }
        o.n_out = in.n_out; o.k = k; o.n_seg = in.n_seg;
        o.k_off = a->k_total; o.n_off = a->n_total; o.w_off = a->w_total;
        a->k_total += k;
        a->w_total += in.n_out * k;
        if ((int64_t)a->n_total + in.n_out > HH_INSTAGE_MAX_OUT) { g_err = w + ": more than HH_INSTAGE_MAX_OUT outputs in one call"; return HH_E_ARG; }
        a->n_total += in.n_out;
        if (io && in.y_ld < in.n_out) { g_err = w + ": y_ld < n_out"; return HH_E_ARG; }
        o.w = in.w; o.b = in.b; o.y = in.y; o.y_in = in.y; o.d_y = in.d_y; o.d_w = in.d_w; o.d_b = in.d_b;
        o.y_ld = in.y_ld; o.d_y_ld = in.d_y_ld;
    }
    return HH_OK;
}

extern "C" int hh_input_stage_scratch_bytes(int32_t n_groups, const hh_input_group *g, int64_t n_rows, int64_t *bytes) {
    his_args a;
    if (!bytes) { g_err = "hh_input_stage_scratch_bytes: null argument"; return HH_E_ARG; }
    /* the widths alone decide the size: a source as wide as the widest segment end passes the segment check */
    int32_t width = 1;
    if (g && n_groups >= 1 && n_groups <= HH_INSTAGE_MAX_GROUPS)
        for (int gi = 0; gi < n_groups; gi++)
            for (int s = 0; s < g[gi].n_seg && s < HH_INSTAGE_MAX_SEGS; s++)
                if ((int)g[gi].seg_col[s] + (int)g[gi].seg_len[s] > width) width = (int)g[gi].seg_col[s] + (int)g[gi].seg_len[s];
    if (int rc = his_check("hh_input_stage_scratch_bytes", n_rows, width, width, n_groups, g, false, &a)) return rc;
    const int64_t parts = his_parts(n_rows);
    *bytes = (parts < 1 ? 1 : parts) * (int64_t)(a.w_total + a.n_total) * 4;
    return HH_OK;
}

extern "C" int hh_input_stage_forward(int64_t n_rows, const float *src, int64_t src_ld, int32_t src_width, int32_t n_groups,
                                      const hh_input_group *g, void *stream) {
    his_args a;
    if (int rc = his_check("hh_input_stage_forward", n_rows, src_ld, src_width, n_groups, g, true, &a)) return rc;
    if (n_rows == 0) return HH_OK;
    bool null = !src;
    for (int gi = 0; gi < n_groups; gi++) null = null || !g[gi].w || !g[gi].b || !g[gi].y;
    if (null) { g_err = "hh_input_stage_forward: null argument"; return HH_E_ARG; }
    const int64_t tiles = (n_rows + HIS_TR - 1) / HIS_TR;
    const dim3 grid((unsigned)(tiles < HIS_FWD_MAX_GRID ? tiles : HIS_FWD_MAX_GRID));
    const size_t lds = (size_t)a.k_total * (HIS_TRP + 1) * 4;
    if (int rc = his_allow_lds(hh_k_input_stage_fwd, lds)) return rc;
    hipLaunchKernelGGL(hh_k_input_stage_fwd, grid, dim3(HIS_FWD_THREADS), lds, (hipStream_t)stream, a, n_rows, src, src_ld);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_input_stage_backward(int64_t n_rows, const float *src, int64_t src_ld, int32_t src_width, int32_t n_groups,
                                       const hh_input_group *g, void *scratch, int64_t scratch_bytes, void *stream) {
    his_args a;
    if (int rc = his_check("hh_input_stage_backward", n_rows, src_ld, src_width, n_groups, g, true, &a)) return rc;
    if (n_rows == 0) return HH_OK;
    bool null = !src || !scratch;
    for (int gi = 0; gi < n_groups; gi++) {
        null = null || !g[gi].y || !g[gi].d_y || !g[gi].d_w || !g[gi].d_b;
        if (g[gi].d_y_ld < g[gi].n_out) { g_err = "hh_input_stage_backward: d_y_ld < n_out"; return HH_E_ARG; }
    }
    if (null) { g_err = "hh_input_stage_backward: null argument"; return HH_E_ARG; }
    const int64_t parts = his_parts(n_rows), entries = a.w_total + a.n_total;
    if (scratch_bytes < parts * entries * 4) { g_err = "hh_input_stage_backward: scratch too small (hh_input_stage_scratch_bytes)"; return HH_E_ARG; }
    hipStream_t st = (hipStream_t)stream;
    float *part = static_cast<float *>(scratch);
    const size_t lds = (size_t)(HIS_TR * HIS_COLS + a.k_total * (HIS_TRP + 1)) * 4;
    const dim3 grid((unsigned)parts, (unsigned)((a.n_total + HIS_COLS - 1) / HIS_COLS));
    if (int rc = his_allow_lds(hh_k_input_stage_bwd, lds)) return rc;
    hipLaunchKernelGGL(hh_k_input_stage_bwd, grid, dim3(HIS_BWD_THREADS), lds, st, a, n_rows, src, src_ld, part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hh_k_input_stage_reduce, dim3((unsigned)((entries + HIS_BWD_THREADS - 1) / HIS_BWD_THREADS)), dim3(HIS_BWD_THREADS), 0, st,
                       a, (int)parts, part);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

#endif /* HH_INPUT_STAGE_H */
