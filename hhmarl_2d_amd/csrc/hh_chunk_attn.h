/*
 * hh_chunk_attn.h — the parts of Fight1 / Fight2's two self-attention blocks that are not proper GEMMs, for the 2-vs-2 learner
 * (learner.TrainableNet(attention="fused"); C ABI and the formulas: include/hh_learner.h): the attention core between the in- and the
 * out-projection, forward and backward, and normalize(x + att), forward and backward.  The projections stay rocBLAS GEMMs.
 *
 * Core.  One workgroup of 256 lanes owns one (sequence, head) unit: Q, K, V (backward: and dO) of the unit, len <= 32 rows of d = 50 | 75
 * floats each, are staged in LDS with a row stride of d | 1 words (51 | 75: odd, so the column reads of Q K^T, where neighbouring lanes
 * read neighbouring rows, fall on distinct banks), by 4-byte loads — a 75-float head slice starts 300 B into a 600 B row, so nothing wider
 * is aligned.  LDS is sized by len at launch: 20.4 KB forward / 31.9 KB backward at len = 20, d = 75, at most 51 KB.
 *   scores   lane (i = t / 8, part = t % 8) owns S[i][part + 8 jj], jj < 4: one Q read per four K reads and four fmaf; the row maximum, the
 *            row sum and (backward) rowsum(P o dP) are xor-shuffles over the 8 lanes of a row.  expf is the device library's.
 *   products every output tile is 4 rows x 1 column per lane (consecutive lanes: consecutive columns, so V / K / Q / dO reads are
 *            conflict-free and the stores coalesce), the 4 probabilities one 16-byte LDS read that the whole wave shares.  P is kept
 *            transposed ([j][i]) for P V and dS K, as it is ([i][j]) for P^T dO and dS^T Q; row stride 36 words.
 * The sums over the keys and over the queries of a sequence run inside one workgroup in index order: no atomics, no second pass,
 * the same bytes on every run.  Rows of the P tiles beyond len are never read into a stored result.
 *
 * Normalize.  One row per 32 lanes, 8-byte accesses (a width-150 row is 600 B: 8-byte aligned, not 16), the two row sums by xor-shuffle.
 */
#ifndef HH_CHUNK_ATTN_H
#define HH_CHUNK_ATTN_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hh_learner.h"

#define HCA_THREADS 256
#define HCA_PS 36        /* row stride of the probability tiles: HH_ATTN_MAX_LEN + 4, rows 16-byte aligned */
#define HCA_JJ 4         /* keys per lane: HH_ATTN_MAX_LEN / 8 */
#define HCA_ROWS 8       /* normalize: rows per workgroup, 32 lanes each */
#define HCA_EPS 1e-12f   /* F.normalize's eps */

static_assert(HH_ATTN_HEADS == 2 && HH_ATTN_MAX_LEN == 32, "the lane maps below are written for 2 heads and at most 32 steps");

/* NP slices of D floats per row (E = 2 D floats apart in the row, rows `ld` floats apart) -> NP tiles [len][D | 1], one after the other */
template <int D, int NP>
__device__ __forceinline__ void hca_stage(float *__restrict__ dst, const float *__restrict__ src, int len, int ld, int t) {
    constexpr int DP = D | 1;
    const int n = len * D;
    for (int e0 = t; e0 < n; e0 += 2 * HCA_THREADS) {
        float val[2][NP];
        int at[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int e = e0 + u * HCA_THREADS;
            const bool on = e < n;
            const int r = on ? e / D : 0, c = on ? e - r * D : 0;
            at[u] = on ? r * DP + c : -1;
#pragma unroll
            for (int p = 0; p < NP; p++) val[u][p] = on ? src[(int64_t)r * ld + p * (2 * D) + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 2; u++)
            if (at[u] >= 0) {
#pragma unroll
                for (int p = 0; p < NP; p++) dst[p * len * DP + at[u]] = val[u][p];
            }
    }
}

/* softmax(Q K^T / sqrt(D)) of row i for the lane's keys j = part + 8 jj (0 where j >= len); BWD: dp = (dO V^T)[i][j] too */
template <int D, bool BWD>
__device__ __forceinline__ void hca_scores(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                           const float *__restrict__ dO, int len, int ic, int part, float p[HCA_JJ], float dp[HCA_JJ]) {
    constexpr int DP = D | 1;
    const float scale = (float)(1.0 / sqrt((double)D));
    int jo[HCA_JJ];
    float acc[HCA_JJ];
#pragma unroll
    for (int jj = 0; jj < HCA_JJ; jj++) {
        const int j = part + 8 * jj;
        jo[jj] = (j < len ? j : 0) * DP;
        acc[jj] = 0.0f;
        dp[jj] = 0.0f;
    }
    const float *qi = q + ic * DP, *di = dO + ic * DP;
#pragma unroll 5
    for (int c = 0; c < D; c++) {
        const float qv = qi[c];
        const float dv = BWD ? di[c] : 0.0f;
#pragma unroll
        for (int jj = 0; jj < HCA_JJ; jj++) {
            if (8 * jj < len) {
                acc[jj] = fmaf(qv, k[jo[jj] + c], acc[jj]);
                if (BWD) dp[jj] = fmaf(dv, v[jo[jj] + c], dp[jj]);
            }
        }
    }
    float m = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < HCA_JJ; jj++) {
        acc[jj] = part + 8 * jj < len ? acc[jj] * scale : -INFINITY;
        m = fmaxf(m, acc[jj]);
    }
    m = fmaxf(m, __shfl_xor(m, 1));
    m = fmaxf(m, __shfl_xor(m, 2));
    m = fmaxf(m, __shfl_xor(m, 4));
    float sum = 0.0f;
#pragma unroll
    for (int jj = 0; jj < HCA_JJ; jj++) {
        p[jj] = expf(acc[jj] - m);      /* expf(-inf) = 0 for the keys beyond len; the maximum itself gives exactly 1 */
        sum += p[jj];
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 4);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int jj = 0; jj < HCA_JJ; jj++) p[jj] *= inv;
}

template <int D>
__global__ __launch_bounds__(HCA_THREADS) void hh_k_chunk_attn_fwd(int len, const float *__restrict__ qkv, float *__restrict__ ctx) {
    constexpr int E = 2 * D, DP = D | 1;
    extern __shared__ float4 hca_lds_fwd[];
    float *pt = reinterpret_cast<float *>(hca_lds_fwd);       /* P^T[j][i] */
    float *q = pt + len * HCA_PS, *k = q + len * DP, *v = k + len * DP;
    const int t = threadIdx.x, h = blockIdx.x & 1;
    const int64_t row0 = (int64_t)(blockIdx.x >> 1) * len;
    hca_stage<D, 3>(q, qkv + row0 * (3 * E) + h * D, len, 3 * E, t);
    __syncthreads();
    const int i = t >> 3, part = t & 7;
    float p[HCA_JJ], unused[HCA_JJ];
    hca_scores<D, false>(q, k, v, q, len, i < len ? i : 0, part, p, unused);
    if (i < len) {
#pragma unroll
        for (int jj = 0; jj < HCA_JJ; jj++) {
            const int j = part + 8 * jj;
            if (j < len) pt[j * HCA_PS + i] = p[jj];
        }
    }
    __syncthreads();
    const int n = ((len + 3) >> 2) * D;
    for (int e = t; e < n; e += HCA_THREADS) {
        const int b = e / D, c = e - b * D, i0 = 4 * b;
        float4 pr = *reinterpret_cast<const float4 *>(pt + i0);
        float vv = v[c];
        float a0 = pr.x * vv, a1 = pr.y * vv, a2 = pr.z * vv, a3 = pr.w * vv;     /* one key: 1.0f x v, the v columns bit for bit */
        for (int j = 1; j < len; j++) {
            pr = *reinterpret_cast<const float4 *>(pt + j * HCA_PS + i0);
            vv = v[j * DP + c];
            a0 = fmaf(pr.x, vv, a0); a1 = fmaf(pr.y, vv, a1); a2 = fmaf(pr.z, vv, a2); a3 = fmaf(pr.w, vv, a3);
        }
        float *o = ctx + (row0 + i0) * E + h * D + c;
        o[0] = a0;
        if (i0 + 1 < len) o[E] = a1;
        if (i0 + 2 < len) o[2 * E] = a2;
        if (i0 + 3 < len) o[3 * E] = a3;
    }
}

template <int D>
__global__ __launch_bounds__(HCA_THREADS) void hh_k_chunk_attn_bwd(int len, const float *__restrict__ qkv, const float *__restrict__ d_ctx,
                                                                   float *__restrict__ d_qkv) {
    constexpr int E = 2 * D, DP = D | 1;
    extern __shared__ float4 hca_lds_bwd[];
    float *pn = reinterpret_cast<float *>(hca_lds_bwd);       /* P[i][j] */
    float *sn = pn + len * HCA_PS, *st = sn + len * HCA_PS;   /* dS[i][j] / sqrt(D) and its transpose */
    float *q = st + len * HCA_PS, *k = q + len * DP, *v = k + len * DP, *dO = v + len * DP;
    const int t = threadIdx.x, h = blockIdx.x & 1;
    const int64_t row0 = (int64_t)(blockIdx.x >> 1) * len;
    hca_stage<D, 3>(q, qkv + row0 * (3 * E) + h * D, len, 3 * E, t);
    hca_stage<D, 1>(dO, d_ctx + row0 * E + h * D, len, E, t);
    __syncthreads();
    const int i = t >> 3, part = t & 7;
    float p[HCA_JJ], dp[HCA_JJ];
    hca_scores<D, true>(q, k, v, dO, len, i < len ? i : 0, part, p, dp);
    float rs = 0.0f;
#pragma unroll
    for (int jj = 0; jj < HCA_JJ; jj++) rs = fmaf(p[jj], dp[jj], rs);
    rs += __shfl_xor(rs, 1);
    rs += __shfl_xor(rs, 2);
    rs += __shfl_xor(rs, 4);
    if (i < len) {
        const float scale = (float)(1.0 / sqrt((double)D));
#pragma unroll
        for (int jj = 0; jj < HCA_JJ; jj++) {
            const int j = part + 8 * jj;
            if (j < len) {
                const float ds = p[jj] * (dp[jj] - rs) * scale;
                pn[i * HCA_PS + j] = p[jj];
                sn[i * HCA_PS + j] = ds;
                st[j * HCA_PS + i] = ds;
            }
        }
    }
    __syncthreads();
    const int n = ((len + 3) >> 2) * D;
    float *out = d_qkv + row0 * (3 * E) + h * D;
    for (int e = t; e < n; e += HCA_THREADS) {
        const int b = e / D, c = e - b * D, r0 = 4 * b;
        /* dK = dS^T Q and dV = P^T dO for keys r0 .. r0 + 3, summed over the queries in order */
        float4 ps = *reinterpret_cast<const float4 *>(pn + r0), ss = *reinterpret_cast<const float4 *>(sn + r0);
        float ov = dO[c], qv = q[c];
        float v0 = ps.x * ov, v1 = ps.y * ov, v2 = ps.z * ov, v3 = ps.w * ov;
        float k0 = ss.x * qv, k1 = ss.y * qv, k2 = ss.z * qv, k3 = ss.w * qv;
        for (int r = 1; r < len; r++) {
            ps = *reinterpret_cast<const float4 *>(pn + r * HCA_PS + r0);
            ss = *reinterpret_cast<const float4 *>(sn + r * HCA_PS + r0);
            ov = dO[r * DP + c];
            qv = q[r * DP + c];
            v0 = fmaf(ps.x, ov, v0); v1 = fmaf(ps.y, ov, v1); v2 = fmaf(ps.z, ov, v2); v3 = fmaf(ps.w, ov, v3);
            k0 = fmaf(ss.x, qv, k0); k1 = fmaf(ss.y, qv, k1); k2 = fmaf(ss.z, qv, k2); k3 = fmaf(ss.w, qv, k3);
        }
        /* dQ = dS K for queries r0 .. r0 + 3, summed over the keys in order */
        float4 ts = *reinterpret_cast<const float4 *>(st + r0);
        float kv = k[c];
        float q0 = ts.x * kv, q1 = ts.y * kv, q2 = ts.z * kv, q3 = ts.w * kv;
        for (int r = 1; r < len; r++) {
            ts = *reinterpret_cast<const float4 *>(st + r * HCA_PS + r0);
            kv = k[r * DP + c];
            q0 = fmaf(ts.x, kv, q0); q1 = fmaf(ts.y, kv, q1); q2 = fmaf(ts.z, kv, q2); q3 = fmaf(ts.w, kv, q3);
        }
        float *o = out + (int64_t)r0 * (3 * E) + c;
        o[0] = q0; o[E] = k0; o[2 * E] = v0;
        if (r0 + 1 < len) { o += 3 * E; o[0] = q1; o[E] = k1; o[2 * E] = v1; }
        if (r0 + 2 < len) { o += 3 * E; o[0] = q2; o[E] = k2; o[2 * E] = v2; }
        if (r0 + 3 < len) { o += 3 * E; o[0] = q3; o[E] = k3; o[2 * E] = v3; }
    }
}

/* ---- normalize(x + a) ---- */
template <int W>
__global__ __launch_bounds__(32 * HCA_ROWS) void hh_k_resnorm_fwd(int64_t n_rows, const float2 *__restrict__ x, const float2 *__restrict__ a,
                                                                  float2 *__restrict__ y, float *__restrict__ norm) {
    constexpr int W2 = W / 2, NV = (W2 + 31) / 32;
    const int lane = threadIdx.x & 31;
    const int64_t row = (int64_t)blockIdx.x * HCA_ROWS + (threadIdx.x >> 5);
    const bool on = row < n_rows;
    const int64_t base = (on ? row : 0) * W2;       /* a lane beyond the last row reads row 0 and stores nothing: every lane shuffles */
    float2 s[NV];
    float ss = 0.0f;
#pragma unroll
    for (int u = 0; u < NV; u++) {
        const int c = lane + 32 * u;
        s[u] = make_float2(0.0f, 0.0f);
        if (c < W2) {
            const float2 xv = x[base + c], av = a[base + c];
            s[u] = make_float2(xv.x + av.x, xv.y + av.y);
        }
        ss = fmaf(s[u].x, s[u].x, ss);
        ss = fmaf(s[u].y, s[u].y, ss);
    }
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) ss += __shfl_xor(ss, m);
    const float nrm = sqrtf(ss);
    const float den = fmaxf(nrm, HCA_EPS);
    if (on) {
#pragma unroll
        for (int u = 0; u < NV; u++) {
            const int c = lane + 32 * u;
            if (c < W2) y[base + c] = make_float2(s[u].x / den, s[u].y / den);
        }
        if (lane == 0) norm[row] = nrm;
    }
}

template <int W>
__global__ __launch_bounds__(32 * HCA_ROWS) void hh_k_resnorm_bwd(int64_t n_rows, const float2 *__restrict__ y, const float *__restrict__ norm,
                                                                  const float2 *__restrict__ d_y, float2 *__restrict__ d_s) {
    constexpr int W2 = W / 2, NV = (W2 + 31) / 32;
    const int lane = threadIdx.x & 31;
    const int64_t row = (int64_t)blockIdx.x * HCA_ROWS + (threadIdx.x >> 5);
    const bool on = row < n_rows;
    const int64_t base = (on ? row : 0) * W2;
    float2 yv[NV], gv[NV];
    float dot = 0.0f;
#pragma unroll
    for (int u = 0; u < NV; u++) {
        const int c = lane + 32 * u;
        yv[u] = gv[u] = make_float2(0.0f, 0.0f);
        if (c < W2) {
            yv[u] = y[base + c];
            gv[u] = d_y[base + c];
        }
        dot = fmaf(yv[u].x, gv[u].x, dot);
        dot = fmaf(yv[u].y, gv[u].y, dot);
    }
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) dot += __shfl_xor(dot, m);
    const float nrm = norm[on ? row : 0];
    if (on) {
#pragma unroll
        for (int u = 0; u < NV; u++) {
            const int c = lane + 32 * u;
            if (c < W2) {
                float2 o;
                if (nrm >= HCA_EPS) {
                    o.x = (gv[u].x - yv[u].x * dot) / nrm;
                    o.y = (gv[u].y - yv[u].y * dot) / nrm;
                } else {        /* the clamp holds the denominator at eps, and the norm's own gradient at 0 is 0 */
                    o.x = gv[u].x / HCA_EPS;
                    o.y = gv[u].y / HCA_EPS;
                }
                d_s[base + c] = o;
            }
        }
    }
}

/* ---- the C ABI ---- */
struct hca_span { const void *p; int64_t bytes; bool out; };

/* every pointer non-null and `align`-byte aligned; no output range meets an input or another output */
static int hca_check_spans(const char *who, const hca_span *sp, int n, int align) {
    for (int i = 0; i < n; i++) {
        if (!sp[i].p) { g_err = std::string(who) + ": null argument"; return HH_E_ARG; }
        if (reinterpret_cast<uintptr_t>(sp[i].p) & (uintptr_t)(align - 1)) {
            g_err = std::string(who) + ": every tensor must be " + std::to_string(align) + "-byte aligned";
            return HH_E_ARG;
        }
    }
    for (int i = 0; i < n; i++)
        for (int k = i + 1; k < n; k++) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(sp[i].p), b = reinterpret_cast<uintptr_t>(sp[k].p);
            if ((sp[i].out || sp[k].out) && a < b + (uintptr_t)sp[k].bytes && b < a + (uintptr_t)sp[i].bytes) {
                g_err = std::string(who) + ": an output overlaps another tensor of the call";
                return HH_E_ARG;
            }
        }
    return HH_OK;
}

static int hca_check_core(const char *who, int64_t n_seq, int32_t len, int32_t embed) {
    if ((embed != 100 && embed != 150) || len < 1 || len > HH_ATTN_MAX_LEN || n_seq < 0 || n_seq > ((int64_t)1 << 24)) {
        g_err = std::string(who) + ": need embed = 100 | 150, 1 <= len <= 32, 0 <= n_seq <= 2^24";
        return HH_E_ARG;
    }
    return HH_OK;
}

static int hca_check_rows(const char *who, int64_t n_rows, int32_t width) {
    if ((width != 100 && width != 150) || n_rows < 0 || n_rows > ((int64_t)1 << 32)) {
        g_err = std::string(who) + ": need width = 100 | 150, 0 <= n_rows <= 2^32";
        return HH_E_ARG;
    }
    return HH_OK;
}

extern "C" int hh_chunk_attn_forward(int64_t n_seq, int32_t len, int32_t embed, const float *qkv, float *ctx, void *stream) {
    if (int rc = hca_check_core("hh_chunk_attn_forward", n_seq, len, embed)) return rc;
    if (n_seq == 0) return HH_OK;
    const int64_t rows = n_seq * len;
    const hca_span sp[2] = {{qkv, rows * 3 * embed * 4, false}, {ctx, rows * embed * 4, true}};
    if (int rc = hca_check_spans("hh_chunk_attn_forward", sp, 2, 4)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int d = embed / HH_ATTN_HEADS;
    const size_t lds = (size_t)len * (HCA_PS + 3 * (d | 1)) * sizeof(float);
    const dim3 grid((unsigned)(n_seq * HH_ATTN_HEADS));
    if (embed == 100) hipLaunchKernelGGL(hh_k_chunk_attn_fwd<50>, grid, dim3(HCA_THREADS), lds, st, (int)len, qkv, ctx);
    else hipLaunchKernelGGL(hh_k_chunk_attn_fwd<75>, grid, dim3(HCA_THREADS), lds, st, (int)len, qkv, ctx);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_chunk_attn_backward(int64_t n_seq, int32_t len, int32_t embed, const float *qkv, const float *d_ctx, float *d_qkv, void *stream) {
    if (int rc = hca_check_core("hh_chunk_attn_backward", n_seq, len, embed)) return rc;
    if (n_seq == 0) return HH_OK;
    const int64_t rows = n_seq * len;
    const hca_span sp[3] = {{qkv, rows * 3 * embed * 4, false}, {d_ctx, rows * embed * 4, false}, {d_qkv, rows * 3 * embed * 4, true}};
    if (int rc = hca_check_spans("hh_chunk_attn_backward", sp, 3, 4)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int d = embed / HH_ATTN_HEADS;
    const size_t lds = (size_t)len * (3 * HCA_PS + 4 * (d | 1)) * sizeof(float);
    const dim3 grid((unsigned)(n_seq * HH_ATTN_HEADS));
    if (embed == 100) hipLaunchKernelGGL(hh_k_chunk_attn_bwd<50>, grid, dim3(HCA_THREADS), lds, st, (int)len, qkv, d_ctx, d_qkv);
    else hipLaunchKernelGGL(hh_k_chunk_attn_bwd<75>, grid, dim3(HCA_THREADS), lds, st, (int)len, qkv, d_ctx, d_qkv);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_residual_normalize_forward(int64_t n_rows, int32_t width, const float *x, const float *a, float *y, float *norm, void *stream) {
    if (int rc = hca_check_rows("hh_residual_normalize_forward", n_rows, width)) return rc;
    if (n_rows == 0) return HH_OK;
    const int64_t bytes = n_rows * width * 4;
    const hca_span sp[4] = {{x, bytes, false}, {a, bytes, false}, {y, bytes, true}, {norm, n_rows * 4, true}};
    if (int rc = hca_check_spans("hh_residual_normalize_forward", sp, 3, 8)) return rc;
    if (int rc = hca_check_spans("hh_residual_normalize_forward", sp, 4, 4)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((n_rows + HCA_ROWS - 1) / HCA_ROWS));
    const float2 *x2 = reinterpret_cast<const float2 *>(x), *a2 = reinterpret_cast<const float2 *>(a);
    float2 *y2 = reinterpret_cast<float2 *>(y);
    if (width == 100) hipLaunchKernelGGL(hh_k_resnorm_fwd<100>, grid, dim3(32 * HCA_ROWS), 0, st, n_rows, x2, a2, y2, norm);
    else hipLaunchKernelGGL(hh_k_resnorm_fwd<150>, grid, dim3(32 * HCA_ROWS), 0, st, n_rows, x2, a2, y2, norm);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_residual_normalize_backward(int64_t n_rows, int32_t width, const float *y, const float *norm, const float *d_y, float *d_s,
                                              void *stream) {
    if (int rc = hca_check_rows("hh_residual_normalize_backward", n_rows, width)) return rc;
    if (n_rows == 0) return HH_OK;
    const int64_t bytes = n_rows * width * 4;
    const hca_span sp[4] = {{y, bytes, false}, {d_y, bytes, false}, {d_s, bytes, true}, {norm, n_rows * 4, false}};
    if (int rc = hca_check_spans("hh_residual_normalize_backward", sp, 3, 8)) return rc;
    if (int rc = hca_check_spans("hh_residual_normalize_backward", sp, 4, 4)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((n_rows + HCA_ROWS - 1) / HCA_ROWS));
    const float2 *y2 = reinterpret_cast<const float2 *>(y), *g2 = reinterpret_cast<const float2 *>(d_y);
    float2 *o2 = reinterpret_cast<float2 *>(d_s);
    if (width == 100) hipLaunchKernelGGL(hh_k_resnorm_bwd<100>, grid, dim3(32 * HCA_ROWS), 0, st, n_rows, y2, norm, g2, o2);
    else hipLaunchKernelGGL(hh_k_resnorm_bwd<150>, grid, dim3(32 * HCA_ROWS), 0, st, n_rows, y2, norm, g2, o2);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

#endif /* HH_CHUNK_ATTN_H */
