/*
 * hh_commander_kernel.h — the trainable commander of train_hier.py (models/ac_models_hier.py:70-112 CommanderGru) as one fused
 * gfx950 kernel: actor, value branch, both GRU cells, the Categorical draw and its log-probability (C ABI: include/hh_commander.h).
 *
 * Arithmetic: the split-fp16 scheme of hh_policy_kernel_h16.h (hi / lo fp16 operands, hi hi + lo hi + hi lo by three
 * v_mfma_f32_32x32x16_f16 per 16 k-steps, fp32 accumulate) through its contraction (hhp_gemm_h) and C-tile store (hhp_store_tile_t);
 * sigmoid, tanh, the GRU update and the L2 normalisation in fp32 in the epilogues.
 *
 * Structure: a workgroup of 512 threads (eight waves) runs ONE 32-row tile of ONE branch: blockIdx.x = 2 tile + kind, kind 0 = the
 * actor (state 0), kind 1 = the value branch (state 1).  Both branches have the same shape, so one tile body serves both:
 *   L1      input X (actor: obs 34 -> K 48; critic: [obs_own|act_own|obs_o1|act_o1|obs_o2|act_o2] 105 -> K 112) -> 512 columns, one
 *           block-diagonal matrix holding the three narrow FCs AND the fourth: [e (300) | 0 (4) | f (200) | 0 (8)], tanh
 *   GRU     [f | 0 | h | 0] (K 416, f from L1's output in place, h loaded from h_in) -> per 32 hidden units one 128-column group
 *           [r | z | W_in f | W_hn h]: r and z contract over all 416, the n gate's two halves over their own 208 each; h' in fp32,
 *           h_out written, f + h' normalised over the row (cross-wave sum of squares in LDS) and stored back where f was
 *   shared  S = [e | 0 | normalize(f + h') | 0] (K 512, the shared layer's input rows permuted to this order on the host) -> 512, tanh
 *   out     act_out (3) / val_out (1) contracted in fp32 straight from the shared layer's C tiles in registers, partials in LDS
 * The activation tile lives in one LDS buffer of 720 k-columns (hi and lo planes, 90 KB): S at 0..511, h at 512..719, the input X
 * aliases the h region before h is loaded.  One workgroup per CU.  The stages are device functions (hhc_l1, hhc_gru, hhc_normalize,
 * hhc_shared_out, hhc_out_sum, hhc_first_max) that hh_k_commander_chain (hh_commander_chain.h) runs too.
 */
#ifndef HH_COMMANDER_KERNEL_H
#define HH_COMMANDER_KERNEL_H

#include "hh_commander.h"

#define HHC_R 32                                   /* rows per tile */
#define HHC_THREADS 512                            /* eight waves */
#define HHC_KS 512                                 /* shared layer K (S columns 0..511) */
#define HHC_FOFF 304                               /* column of f / normalize(f + h') in S */
#define HHC_HOFF 512                               /* column of h (and of the input X before h is loaded) */
#define HHC_KCOLS 720                              /* k-columns of the LDS activation buffer */
#define HHC_KG 416                                 /* GRU contraction: [f (200) | 0 (8) | h (200) | 0 (8)] */
#define HHC_JG 896                                 /* GRU output columns: 7 x [r | z | in | hn] (32 each) */
#define HHC_HT 7                                   /* 32-wide hidden tiles */
#define HHC_PLANE_BYTES (HHC_KCOLS * HHC_R * 2)    /* one of the hi / lo planes: 46080 */
#define HHC_OFF_NP (2 * HHC_PLANE_BYTES)           /* [8][32] f32 sum-of-squares partials */
#define HHC_OFF_OP (HHC_OFF_NP + 8 * HHC_R * 4)    /* [8][32][3] f32 output-layer partials */
#define HHC_LDS_BYTES (HHC_OFF_OP + 8 * HHC_R * 3 * 4)

struct HhcBranch {
    const float4 *w1h, *w1l; /* [K1 x 512] fragments (hhp_hidx), K1 = 48 | 112 */
    const float4 *wgh, *wgl; /* [416 x 896] */
    const float *b1;         /* [512] */
    const float *bg;         /* [4][224]: b_ir + b_hr | b_iz + b_hz | b_in | b_hn */
    const float *wo;         /* [3][512] (actor) | [1][512] (critic), fp32 */
    const float *bo;         /* [3] | [1] */
    int k1;
};
struct HhcNet {
    HhcBranch br[2];
    const float4 *wsh, *wsl; /* [512 x 512], input rows in S order */
    const float *bs;         /* [512] */
};
struct HhcArgs {
    const float *obs;
    float *h_in, *h_out;
    const uint8_t *fresh;
    const double *uniforms;
    const int4 *ar_pack;
    unsigned long long seed, arena_offset;
    const float *crit_act;
    int greedy, rows;
    int8_t *actions;
    float *logp, *vf, *logits;
};

__device__ __forceinline__ float hhc_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

/* ---- the stages of one 32-row tile of one branch, shared by hh_k_commander and hh_k_commander_chain (hh_commander_chain.h): the same
 * contractions in the same order, so both kernels give the same bits for the same row and state */
struct HhcLds {
    _Float16 *Sh, *Sl;
    const float4 *Sh4, *Sl4;
    float *npart, *opart;
};
__device__ __forceinline__ HhcLds hhc_lds(unsigned char *ldsb) {
    HhcLds s;
    s.Sh = reinterpret_cast<_Float16 *>(ldsb);
    s.Sl = reinterpret_cast<_Float16 *>(ldsb + HHC_PLANE_BYTES);
    s.Sh4 = reinterpret_cast<const float4 *>(s.Sh); s.Sl4 = reinterpret_cast<const float4 *>(s.Sl);
    s.npart = reinterpret_cast<float *>(ldsb + HHC_OFF_NP);
    s.opart = reinterpret_cast<float *>(ldsb + HHC_OFF_OP);
    return s;
}

/* L1 on the input X at columns HHC_HOFF ..: 16 column tiles, two per wave: tanh -> S */
__device__ __forceinline__ void hhc_l1(const HhcLds &s, const HhcBranch &B, int K1, int wave, int lane, int ci, int g) {
    hh_f32x16 acc[1][2];
#pragma unroll
    for (int t = 0; t < 2; t++) acc[0][t] = (hh_f32x16)(0.0f);
    hhp_gemm_h<2, 1>(s.Sh4, s.Sl4, HHC_HOFF / 16, K1 / 16, B.w1h, B.w1l, 0, HHC_KS, 64 * wave, lane, acc);
#pragma unroll
    for (int t = 0; t < 2; t++)
        hhp_store_tile_t<HHC_R>(s.Sh, s.Sl, 64 * wave + 32 * t, ci, g, acc[0][t], B.b1, [](hh_f2 x) { return hhp_tanh2(x); });
}

/* GRU on [f | 0 | h | 0] (h split into columns HHC_HOFF ..): wave w < 7 owns hidden units 32 w .. 32 w + 31 of row ci.  h_of(u) = the
 * fp32 state the forward used, put(u, h') stores the new one; vsum <- f + h' and the wave's sum of squares -> npart */
template <class HOf, class Put>
__device__ __forceinline__ void hhc_gru(const HhcLds &s, const HhcBranch &B, int wave, int lane, int ci, int g, HOf h_of, Put put,
                                        float (&vsum)[16]) {
    float ss = 0.0f;
    if (wave < HHC_HT) {
        hh_f32x16 rz[1][2], an[1][1], ah[1][1];
        rz[0][0] = (hh_f32x16)(0.0f); rz[0][1] = (hh_f32x16)(0.0f); an[0][0] = (hh_f32x16)(0.0f); ah[0][0] = (hh_f32x16)(0.0f);
        const int j0 = 128 * wave;
        hhp_gemm_h<2, 1>(s.Sh4, s.Sl4, HHC_FOFF / 16, HHC_KG / 16, B.wgh, B.wgl, 0, HHC_JG, j0, lane, rz);
        hhp_gemm_h<1, 1>(s.Sh4, s.Sl4, HHC_FOFF / 16, HHC_KG / 32, B.wgh, B.wgl, 0, HHC_JG, j0 + 64, lane, an);
        hhp_gemm_h<1, 1>(s.Sh4, s.Sl4, HHC_HOFF / 16, HHC_KG / 32, B.wgh, B.wgl, HHC_KG / 32, HHC_JG, j0 + 96, lane, ah);
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int reg = 4 * q + e, u = 32 * wave + 8 * q + 4 * g + e;
                float v = 0.0f;
                if (u < HH_CMD_HIDDEN) {
                    const float rr = hhc_sigmoid(rz[0][0][reg] + B.bg[u]);
                    const float zz = hhc_sigmoid(rz[0][1][reg] + B.bg[224 + u]);
                    const float nn = tanhf(an[0][0][reg] + B.bg[448 + u] + rr * (ah[0][0][reg] + B.bg[672 + u]));
                    const float h = h_of(u);
                    const float hn = (1.0f - zz) * nn + zz * h;
                    put(u, hn);
                    const int fi = hhp_haidx<HHC_R>(HHC_FOFF + u, ci);
                    const float f = (float)s.Sh[fi] + (float)s.Sl[fi];
                    v = f + hn;
                }
                vsum[reg] = v;
                ss += v * v;
            }
        }
        ss += __shfl_xor(ss, 32);
        if (g == 0) s.npart[wave * HHC_R + ci] = ss;
    }
}

/* normalize(f + h') over the row (the waves' partial sums in npart) -> S columns HHC_FOFF .. */
__device__ __forceinline__ void hhc_normalize(const HhcLds &s, int wave, int ci, int g, const float (&vsum)[16]) {
    if (wave < HHC_HT) {
        float nn = 0.0f;
#pragma unroll
        for (int w = 0; w < HHC_HT; w++) nn += s.npart[w * HHC_R + ci];
        const float den = fmaxf(sqrtf(nn), 1e-12f);
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int u = 32 * wave + 8 * q + 4 * g + e;
                if (u < 208) hhp_split_store<HHC_R>(s.Sh, s.Sl, hhp_haidx<HHC_R>(HHC_FOFF + u, ci), u < HH_CMD_HIDDEN ? vsum[4 * q + e] / den : 0.0f);
            }
        }
    }
}

/* shared layer (16 column tiles, two per wave), tanh, and the output layer (3 columns for the actor, kind 0; 1 for the value branch)
 * from registers: the waves' partials -> opart */
__device__ __forceinline__ void hhc_shared_out(const HhcLds &s, const HhcNet &net, const HhcBranch &B, int kind, int wave, int lane, int ci,
                                               int g) {
    hh_f32x16 acc[1][2];
#pragma unroll
    for (int t = 0; t < 2; t++) acc[0][t] = (hh_f32x16)(0.0f);
    hhp_gemm_h<2, 1>(s.Sh4, s.Sl4, 0, HHC_KS / 16, net.wsh, net.wsl, 0, HHC_KS, 64 * wave, lane, acc);
    float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
#pragma unroll
    for (int t = 0; t < 2; t++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int col = 64 * wave + 32 * t + 8 * q + 4 * g + e;
                const float y = tanhf(acc[0][t][4 * q + e] + net.bs[col]);
                p0 += y * B.wo[col];
                if (kind == 0) { p1 += y * B.wo[512 + col]; p2 += y * B.wo[1024 + col]; }
            }
        }
    }
    p0 += __shfl_xor(p0, 32); p1 += __shfl_xor(p1, 32); p2 += __shfl_xor(p2, 32);
    if (g == 0) {
        float *op = s.opart + (wave * HHC_R + ci) * 3;
        op[0] = p0; op[1] = p1; op[2] = p2;
    }
}

/* row `row`'s three output sums over the eight waves' partials, in wave order */
__device__ __forceinline__ void hhc_out_sum(const float *opart, int row, float (&l)[3]) {
    l[0] = 0.0f; l[1] = 0.0f; l[2] = 0.0f;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const float *op = opart + (w * HHC_R + row) * 3;
        l[0] += op[0]; l[1] += op[1]; l[2] += op[2];
    }
}

/* the first arg-max of the three logits (explore = False); m <- its logit */
__device__ __forceinline__ int hhc_first_max(const float (&l)[3], float &m) {
    m = l[0];
    int best = 0;
    if (l[1] > m) { m = l[1]; best = 1; }
    if (l[2] > m) { m = l[2]; best = 2; }
    return best;
}

__global__ __launch_bounds__(HHC_THREADS, 1) void hh_k_commander(HhcNet net, HhcArgs a) {
    extern __shared__ __align__(16) unsigned char ldsb[];
    const HhcLds s = hhc_lds(ldsb);
    const int kind = (int)blockIdx.x & 1, row0 = ((int)blockIdx.x >> 1) * HHC_R;
    const HhcBranch B = kind ? net.br[1] : net.br[0];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ci = lane & 31, g = lane >> 5;
    const int K1 = B.k1;

    /* ---- input X into the h region (columns 512 .. 512 + K1) */
    for (int e = tid; e < HHC_R * K1; e += HHC_THREADS) {
        const int i = e / K1, c = e - i * K1, r = row0 + i;
        float v = 0.0f;
        if (r < a.rows) {
            if (kind == 0) {
                if (c < HH_CMD_OBS) v = a.obs[(size_t)r * HH_CMD_OBS + c];
            } else if (c < 3 * (HH_CMD_OBS + 1)) {
                const int n = r / 3, s = r - 3 * n, blk = c / (HH_CMD_OBS + 1), j = c - blk * (HH_CMD_OBS + 1);
                /* own agent, then the other two in ascending id (central_critic_observer) */
                const int slot = blk == 0 ? s : (blk == 1 ? (s == 0 ? 1 : 0) : (s == 2 ? 1 : 2));
                if (j < HH_CMD_OBS) v = a.obs[((size_t)n * 3 + slot) * HH_CMD_OBS + j];
                else if (a.crit_act) v = a.crit_act[(size_t)n * 3 + slot];
            }
        }
        hhp_split_store<HHC_R>(s.Sh, s.Sl, hhp_haidx<HHC_R>(HHC_HOFF + c, i), v);
    }
    __syncthreads();

    /* ---- L1 */
    hhc_l1(s, B, K1, wave, lane, ci, g);
    __syncthreads();

    /* ---- h (zeros for fresh arenas, which are also written back into h_in) into columns 512 .. 719 */
    for (int e = tid; e < HHC_R * 208; e += HHC_THREADS) {
        const int i = e / 208, c = e - i * 208, r = row0 + i;
        float v = 0.0f;
        if (r < a.rows && c < HH_CMD_HIDDEN) {
            float *hp = a.h_in + ((size_t)r * 2 + kind) * HH_CMD_HIDDEN + c;
            if (a.fresh && a.fresh[r / 3]) *hp = 0.0f;
            else v = *hp;
        }
        hhp_split_store<HHC_R>(s.Sh, s.Sl, hhp_haidx<HHC_R>(HHC_HOFF + c, i), v);
    }
    __syncthreads();

    /* ---- GRU: h from h_in (zero for fresh rows), h' to h_out */
    const int r_me = row0 + ci;
    const bool row_ok = r_me < a.rows;
    const bool row_fresh = row_ok && a.fresh && a.fresh[r_me / 3];
    float vsum[16];
    hhc_gru(s, B, wave, lane, ci, g,
            [&](int u) { return (row_ok && !row_fresh) ? a.h_in[((size_t)r_me * 2 + kind) * HH_CMD_HIDDEN + u] : 0.0f; },
            [&](int u, float hn) { if (row_ok) a.h_out[((size_t)r_me * 2 + kind) * HH_CMD_HIDDEN + u] = hn; }, vsum);
    __syncthreads();
    hhc_normalize(s, wave, ci, g, vsum);
    __syncthreads();

    /* ---- shared layer and the output layer */
    hhc_shared_out(s, net, B, kind, wave, lane, ci, g);
    __syncthreads();

    /* ---- per row: logits -> draw, or the value */
    if (tid < HHC_R && row0 + tid < a.rows) {
        const int r = row0 + tid;
        float l[3];
        hhc_out_sum(s.opart, tid, l);
        if (kind == 1) {
            if (a.vf) a.vf[r] = l[0] + B.bo[0];
        } else {
            l[0] += B.bo[0]; l[1] += B.bo[1]; l[2] += B.bo[2];
            float m;
            const int best = hhc_first_max(l, m);
            const float e0 = expf(l[0] - m), e1 = expf(l[1] - m), e2 = expf(l[2] - m);
            const float S = e0 + e1 + e2;
            int act = best;
            if (!a.greedy) {
                double u;
                if (a.uniforms) u = a.uniforms[r];
                else {
                    const int n = r / 3, s = r - 3 * n;
                    const int4 ap = a.ar_pack[n];
                    u = hh_rng_u01(hh_rng_tick_key(hh_rng_arena_key(a.seed, a.arena_offset + (unsigned long long)n), (uint32_t)ap.y, (uint32_t)ap.x),
                                   (uint32_t)(s + 1), HH_SITE_COMMANDER_SAMPLE, 0u);
                }
                const float t = (float)u * S;
                float cum = e0;
                act = 2;
                if (cum > t) act = 0;
                else {
                    cum += e1;
                    if (cum > t) act = 1;
                }
            }
            a.actions[r] = (int8_t)act;
            a.logp[r] = (l[act] - m) - logf(S);
            if (a.logits) { /* scalar stores: the caller's buffer need not be 16-byte aligned */
                float *o = a.logits + (size_t)r * HH_CMD_LOGITS;
                o[0] = l[0]; o[1] = l[1]; o[2] = l[2]; o[3] = 0.0f;
            }
        }
    }
}

/* ===================================================================== host side */
struct hh_commander {
    int device, max_rows, loaded;
    HhcNet net;
    char *blob;
};

static hipError_t hhc_chain_set_lds(); /* hh_commander_chain.h: the chain kernel's LDS attribute */

extern "C" int hh_commander_create(int device, int32_t max_rows, hh_commander **out) {
    if (!out || max_rows <= 0) { g_err = "hh_commander_create: bad argument"; return HH_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device"; return HH_E_NODEV; }
    if (device < 0 || device >= ndev) { g_err = "bad device index"; return HH_E_ARG; }
    DeviceGuard guard_(device);
    if (!guard_.ok) { g_err = "hipSetDevice failed"; return HH_E_HIP; }
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(hh_k_commander), hipFuncAttributeMaxDynamicSharedMemorySize, HHC_LDS_BYTES));
    HIPCHK(hhc_chain_set_lds());
    hh_commander *c = new (std::nothrow) hh_commander();
    if (!c) { g_err = "hh_commander_create: out of host memory"; return HH_E_HIP; }
    c->device = device; c->max_rows = max_rows; c->loaded = 0; c->blob = nullptr;
    memset(&c->net, 0, sizeof(c->net));
    *out = c;
    return HH_OK;
}

extern "C" int hh_commander_destroy(hh_commander *c) {
    if (!c) return HH_E_ARG;
    DeviceGuard guard_(c->device);
    if (c->blob) (void)hipFree(c->blob);
    delete c;
    return HH_OK;
}

/* the first layer's blocks (the packer and hh_commander_set_weights, hh_weight_refresh.h): first input column, last + 1 | width, output
 * width and first output column in S order [e (300) | 0 | f (200) | 0] — actor inp1..inp4 on the observation, critic v1..v4 on
 * [obs_own|act_own|obs_o1|act_o1|obs_o2|act_o2] */
static const int HHC_L1A_C0[4] = {0, 4, 24, 0}, HHC_L1A_C1[4] = {4, 24, 34, 34}, HHC_L1A_WD[4] = {50, 200, 50, 200}, HHC_L1A_OUT0[4] = {0, 50, 250, HHC_FOFF};
static const int HHC_L1V_C0[4] = {0, 35, 70, 0}, HHC_L1V_IN[4] = {35, 35, 35, 105}, HHC_L1V_WD[4] = {100, 100, 100, 200}, HHC_L1V_OUT0[4] = {0, 100, 200, HHC_FOFF};

extern "C" int hh_commander_sample(hh_commander *c, const float *obs, int32_t n_arenas, float *h_in, float *h_out, const uint8_t *fresh,
                                   hh_world *w, const double *uniforms, const float *crit_act, int32_t greedy, int8_t *actions, float *logp,
                                   float *vf, float *logits, void *stream) {
    if (!c || !obs || !h_in || !h_out || !actions || !logp || n_arenas <= 0) { g_err = "hh_commander_sample: bad argument"; return HH_E_ARG; }
    const long long rows = 3LL * n_arenas;
    { /* the two state buffers must not overlap anywhere: fresh rows zero h_in while other workgroups write h_out */
        const uintptr_t i0 = (uintptr_t)h_in, o0 = (uintptr_t)h_out, nb = (uintptr_t)rows * 2 * HH_CMD_HIDDEN * sizeof(float);
        if (i0 < o0 + nb && o0 < i0 + nb) { g_err = "hh_commander_sample: h_in and h_out must not alias (overlapping ranges)"; return HH_E_ARG; }
    }
    if (rows > c->max_rows) { g_err = "hh_commander_sample: 3 x n_arenas exceeds max_rows of hh_commander_create"; return HH_E_ARG; }
    if (!c->loaded) { g_err = "hh_commander_sample: no weights loaded"; return HH_E_ARG; }
    if (!greedy && (uniforms != nullptr) == (w != nullptr)) { g_err = "hh_commander_sample: a draw needs exactly one of the world (keyed RNG) and explicit uniforms"; return HH_E_ARG; }
    HhcArgs a;
    memset(&a, 0, sizeof(a));
    a.obs = obs; a.h_in = h_in; a.h_out = h_out; a.fresh = fresh; a.crit_act = crit_act; a.greedy = greedy ? 1 : 0; a.rows = (int)rows;
    a.actions = actions; a.logp = logp; a.vf = vf; a.logits = logits;
    if (!greedy) {
        if (uniforms) a.uniforms = uniforms;
        else {
            if (w->device != c->device) { g_err = "hh_commander_sample: world and commander live on different devices"; return HH_E_ARG; }
            if (w->dc.N != n_arenas) { g_err = "hh_commander_sample: n_arenas differs from the world's arena count"; return HH_E_ARG; }
            a.ar_pack = w->P.ar_pack; a.seed = w->dc.seed; a.arena_offset = w->dc.arena_offset;
        }
    }
    HH_GUARD(c);
    const int tiles = (int)((rows + HHC_R - 1) / HHC_R);
    hipLaunchKernelGGL(hh_k_commander, dim3(2 * tiles), dim3(HHC_THREADS), HHC_LDS_BYTES, (hipStream_t)stream, c->net, a);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_commander_kernel_name(hh_commander *c, int32_t n_arenas, char *buf, int32_t len) {
    if (!c || !buf || len <= 0 || n_arenas <= 0) { g_err = "hh_commander_kernel_name: bad argument"; return HH_E_ARG; }
    snprintf(buf, (size_t)len, "%s", "hh_k_commander");
    return HH_OK;
}

#endif /* HH_COMMANDER_KERNEL_H */
