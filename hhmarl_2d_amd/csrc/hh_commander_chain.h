/*
 * hh_commander_chain.h — the commander as evaluation.py runs it (evaluation.py:40-48; C ABI: hh_commander_act_chain in
 * include/hh_commander.h).  Per commander step every agent id in order gets compute_single_action(explore=False) with
 * states = [zeros(200), zeros(200)] reset at the start of the step and each agent's state_out fed to the next agent as its state_in:
 * only the actor (rnn_act) decides the action, so the value branch is not computed, and the GRU state runs through the agent slots
 * of ONE step instead of through time.
 *
 * Structure: a workgroup of 512 threads (eight waves) owns 32 ARENAS and runs hh_k_commander's actor tile (kind 0) once per agent
 * slot, in slot order, through the same stages (hhc_l1, hhc_gru, hhc_normalize, hhc_shared_out, hhc_first_max of
 * hh_commander_kernel.h) on the same packed weights, so every link's logits are the bits hh_commander_sample gives for that row
 * and that h_in.  What the sampler reads from h_in in global memory the chain keeps in LDS: h' of link k goes to an fp32 copy
 * [32][208] beside the activation buffer (the input X of link k + 1 aliases the h columns of the split planes, so h' must live
 * elsewhere), and link k + 1 splits it into the hi / lo planes as its h operand.  Link 0 is the sampler's zero-state (fresh) path.
 * LDS: 96256 B of hh_k_commander + 26624 B = 122880 B, under gfx950's 160 KB per workgroup; one workgroup per CU.
 */
#ifndef HH_COMMANDER_CHAIN_H
#define HH_COMMANDER_CHAIN_H

#include "hh_commander_kernel.h"

#define HHC_CHAIN_MAX_AGENTS 5                                /* evaluation.py's n-vs-m worlds: 1..5 agents */
#define HHC_HC_STRIDE 208                                     /* floats per row of the carried fp32 state */
#define HHC_OFF_HC HHC_LDS_BYTES                              /* [32][208] f32 rnn_act state carried from link to link */
#define HHC_CHAIN_LDS_BYTES (HHC_OFF_HC + HHC_R * HHC_HC_STRIDE * 4)
static_assert(HHC_CHAIN_LDS_BYTES <= 160 * 1024, "hh_k_commander_chain: LDS above gfx950's 160 KB per workgroup");

struct HhcChainArgs {
    const float *obs;  /* [N, n_agents, 34] */
    int n_arenas, n_agents;
    int8_t *actions;   /* [N, n_agents] */
    float *h_out;      /* [N, n_agents, 200] or NULL */
    float *logits;     /* [N, n_agents, 4] or NULL */
};

__global__ __launch_bounds__(HHC_THREADS, 1) void hh_k_commander_chain(HhcNet net, HhcChainArgs a) {
    extern __shared__ __align__(16) unsigned char ldsb[];
    const HhcLds s = hhc_lds(ldsb);
    float *hc = reinterpret_cast<float *>(ldsb + HHC_OFF_HC);
    const HhcBranch &B = net.br[0];
    const int n0 = (int)blockIdx.x * HHC_R, nA = a.n_agents;
    const int K1 = B.k1;

    for (int k = 0; k < nA; k++) {
        /* the thread's coordinates per link, through an empty asm: otherwise LICM hoists every lane's LDS fragment addresses of all the
         * stages out of the agent loop, where they stay live across the whole body (256 VGPRs, 104 of them spilled); recomputed per
         * link they cost a few VALU instructions */
        int tid = (int)threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int ci = lane & 31, g = lane >> 5;
        const int n_me = n0 + ci;
        const bool row_ok = n_me < a.n_arenas;

        /* ---- input X = the observation of agent slot k into the h region (columns 512 .. 512 + K1).  The last readers of these
         * columns were link k - 1's GRU contractions, two barriers ago; the decode after the last barrier reads opart only. */
        for (int e = tid; e < HHC_R * K1; e += HHC_THREADS) {
            const int i = e / K1, c = e - i * K1, n = n0 + i;
            float v = 0.0f;
            if (n < a.n_arenas && c < HH_CMD_OBS) v = a.obs[((size_t)n * nA + k) * HH_CMD_OBS + c];
            hhp_split_store<HHC_R>(s.Sh, s.Sl, hhp_haidx<HHC_R>(HHC_HOFF + c, i), v);
        }
        __syncthreads();

        /* ---- L1 */
        hhc_l1(s, B, K1, wave, lane, ci, g);
        __syncthreads();

        /* ---- h: zeros for link 0 (evaluation.py's states = [zeros(200), zeros(200)]), else link k - 1's h' from the fp32 copy */
        for (int e = tid; e < HHC_R * 208; e += HHC_THREADS) {
            const int i = e / 208, c = e - i * 208;
            const float v = (k > 0 && c < HH_CMD_HIDDEN) ? hc[i * HHC_HC_STRIDE + c] : 0.0f;
            hhp_split_store<HHC_R>(s.Sh, s.Sl, hhp_haidx<HHC_R>(HHC_HOFF + c, i), v);
        }
        __syncthreads();

        /* ---- GRU: the same thread reads its (row, unit) of the copy and overwrites it with h'; the split above read it before the barrier */
        float vsum[16];
        hhc_gru(s, B, wave, lane, ci, g,
                [&](int u) { return k > 0 ? hc[ci * HHC_HC_STRIDE + u] : 0.0f; },
                [&](int u, float hn) {
                    hc[ci * HHC_HC_STRIDE + u] = hn;
                    if (row_ok && a.h_out) a.h_out[((size_t)n_me * nA + k) * HH_CMD_HIDDEN + u] = hn;
                }, vsum);
        __syncthreads();
        hhc_normalize(s, wave, ci, g, vsum);
        __syncthreads();

        /* ---- shared layer and act_out */
        hhc_shared_out(s, net, B, 0, wave, lane, ci, g);
        __syncthreads();

        /* ---- greedy decode: the first arg-max */
        if (tid < HHC_R && n0 + tid < a.n_arenas) {
            const size_t r = (size_t)(n0 + tid) * nA + k;
            float l[3];
            hhc_out_sum(s.opart, tid, l);
            l[0] += B.bo[0]; l[1] += B.bo[1]; l[2] += B.bo[2];
            float m;
            a.actions[r] = (int8_t)hhc_first_max(l, m);
            if (a.logits) { /* scalar stores, as hh_commander_sample's */
                float *o = a.logits + r * HH_CMD_LOGITS;
                o[0] = l[0]; o[1] = l[1]; o[2] = l[2]; o[3] = 0.0f;
            }
        }
    }
}

/* ===================================================================== host side */
static hipError_t hhc_chain_set_lds() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(hh_k_commander_chain), hipFuncAttributeMaxDynamicSharedMemorySize, HHC_CHAIN_LDS_BYTES);
}

extern "C" int hh_commander_act_chain(hh_commander *c, const float *obs, int32_t n_arenas, int32_t n_agents, int8_t *actions, float *h_out,
                                      float *logits, void *stream) {
    if (!c || !obs || !actions || n_arenas <= 0) { g_err = "hh_commander_act_chain: bad argument"; return HH_E_ARG; }
    if (n_agents < 1 || n_agents > HHC_CHAIN_MAX_AGENTS) { g_err = "hh_commander_act_chain: n_agents must be 1..5"; return HH_E_ARG; }
    if ((long long)n_arenas * n_agents > c->max_rows) { g_err = "hh_commander_act_chain: n_arenas x n_agents exceeds max_rows of hh_commander_create"; return HH_E_ARG; }
    if (!c->loaded) { g_err = "hh_commander_act_chain: no weights loaded"; return HH_E_ARG; }
    HhcChainArgs a;
    a.obs = obs; a.n_arenas = n_arenas; a.n_agents = n_agents; a.actions = actions; a.h_out = h_out; a.logits = logits;
    HH_GUARD(c);
    const int tiles = (n_arenas + HHC_R - 1) / HHC_R;
    hipLaunchKernelGGL(hh_k_commander_chain, dim3(tiles), dim3(HHC_THREADS), HHC_CHAIN_LDS_BYTES, (hipStream_t)stream, c->net, a);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_commander_chain_kernel_name(hh_commander *c, int32_t n_arenas, int32_t n_agents, char *buf, int32_t len) {
    if (!c || !buf || len <= 0 || n_arenas <= 0 || n_agents < 1 || n_agents > HHC_CHAIN_MAX_AGENTS) {
        g_err = "hh_commander_chain_kernel_name: bad argument";
        return HH_E_ARG;
    }
    snprintf(buf, (size_t)len, "%s", "hh_k_commander_chain");
    return HH_OK;
}

#endif /* HH_COMMANDER_CHAIN_H */
