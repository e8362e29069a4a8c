/*
 * hh_weight_refresh.h — THE packer of the samplers' weights: the only place where a weight element's packed destinations are computed
 * (C ABI: hh_policy_set_net / hh_policy_set_critic / hh_policy_refresh / hh_policy_copy_packed in include/hh_policy.h,
 * hh_commander_set_weights / hh_commander_refresh_weights / hh_commander_copy_packed in include/hh_commander.h).
 *
 * The kernels here read fp32 DEVICE tensors (the reference's state_dict layout) and write, in place and ordered on the caller's stream,
 * every packed form the forward kernels read: the fp32 blob, the (hi, lo) fp16 fragment planes, the 1 KB fragment streams and, for
 * Fight1 / Fight2, the folded attention (Wov = Wo Wv, bov = Wo bv + bo in fp64, m = 0, 1, ... in order, multiply and add rounded
 * separately).  One thread per SOURCE element (and one per bias row): it computes the destination of every packed form the element
 * feeds through the index maps the forward kernels read by (hhp_pidx, hhp_hidx, hhp_hidx_t, hhx_at / hhw16_korder) and splits with
 * hhp_f2h / hhp_h2f.  The sections' addresses are the bank's own (HhpNet, HhpNetH, HhpBankX, HhpCrit, HhpCritX, HhcNet), i.e. exactly
 * where the forward kernels read.  Padding is never written.
 *
 * Both ways in run these kernels.  A REFRESH (hh_policy_refresh, hh_commander_refresh_weights: the learner's device tensors into a
 * loaded slot) is the launch alone — no allocation, no memset, no host synchronisation, no scratch: capturable into a HIP graph; the
 * kind, hence the layout and the zero padding, stays.  A LOAD (the set_* calls: host arrays, possibly another kind than the slot held)
 * lays the sections out and allocates what is missing, stages the host arrays in one temporary device buffer (HhrStage), zeroes the
 * whole destination, launches the same kernel on the default stream and waits for it.
 */
#ifndef HH_WEIGHT_REFRESH_H
#define HH_WEIGHT_REFRESH_H

#define HHR_THREADS 256

__device__ __forceinline__ void hhr_split(uint16_t *hi, uint16_t *lo, size_t at, float v) {
    const uint16_t h = hhp_f2h(v);
    hi[at] = h;
    lo[at] = hhp_f2h(v - hhp_h2f(h));
}
/* element (k, col) into fragment piece `piece_hi` of a stream (its lo half is the next piece) */
__device__ __forceinline__ void hhr_xput(uint16_t *S, size_t piece_hi, int k, int col, bool nat, float v) {
    hhr_split(S + piece_hi * (HHW_PIECE / 2), S + (piece_hi + 1) * (HHW_PIECE / 2), hhx_at(k, col, nat), v);
}
/* the attention fold: s = 0; s += Wo[j][m] Wv[m][k] for m = 0 .. n - 1 in fp64 (the bias: s = bo[j]; s += Wo[j][m] bv[m]) */
__device__ __forceinline__ float hhr_fold(const float *wo, const float *wv, int j, int k, int n) {
    double s = 0.0;
    for (int m = 0; m < n; m++) s = __dadd_rn(s, __dmul_rn((double)wo[(size_t)j * n + m], (double)wv[(size_t)m * n + k]));
    return (float)s;
}
__device__ __forceinline__ float hhr_fold_bias(const float *wo, const float *bo, const float *bv, int j, int n) {
    double s = (double)bo[j];
    for (int m = 0; m < n; m++) s = __dadd_rn(s, __dmul_rn((double)wo[(size_t)j * n + m], (double)bv[m]));
    return (float)s;
}

/* ---- actor: the four forms (blob, planes, stream, folded attention).  Sections (flat thread index, cumulative ends): inp1..inp3 as [wd][nc + 1] (column nc = the
 * bias), shared_layer [500][501], act_out [n_out][501], the attention fold [100][101] (fight nets; column 100 = bov) */
struct HhrActorArgs {
    hh_net_weights w;                                                   /* [dev] sources */
    float *B_w1, *B_b1, *B_wov, *B_bov, *B_ws, *B_bs, *B_wa, *B_ba;    /* fp32 blob sections (HhpNet) */
    uint16_t *h_w1, *l_w1, *h_wov, *l_wov, *h_ws, *l_ws, *h_wa, *l_wa; /* fp16 planes (HhpNetH) */
    uint16_t *X;                                                        /* fragment stream (HhpBankX) */
    int c0[3], nc[3], wd[3];                                            /* HHP_INPUTS of the kind */
    int end[6];
};
__device__ __forceinline__ void hhr_actor_l1(const HhrActorArgs &a, const float *W, const float *b, int c0, int nc, int off, int i) {
    const int o = i / (nc + 1), cc = i - o * (nc + 1), col = off + o;
    if (cc == nc) { a.B_b1[col] = b[o]; return; }
    const int c = c0 + cc;
    const float v = W[(size_t)o * nc + cc];
    a.B_w1[hhp_pidx(c, col, HHP_H)] = v;
    hhr_split(a.h_w1, a.l_w1, hhp_hidx(c, col, HHP_H), v);
    hhr_xput(a.X, (size_t)(col >> 4) * 2, c, col, true, v);
}
__global__ __launch_bounds__(HHR_THREADS) void hh_k_refresh_actor(HhrActorArgs a) {
    const int i = (int)blockIdx.x * HHR_THREADS + (int)threadIdx.x;
    if (i < a.end[0]) hhr_actor_l1(a, a.w.inp_w[0], a.w.inp_b[0], a.c0[0], a.nc[0], 0, i);
    else if (i < a.end[1]) hhr_actor_l1(a, a.w.inp_w[1], a.w.inp_b[1], a.c0[1], a.nc[1], a.wd[0], i - a.end[0]);
    else if (i < a.end[2]) hhr_actor_l1(a, a.w.inp_w[2], a.w.inp_b[2], a.c0[2], a.nc[2], a.wd[0] + a.wd[1], i - a.end[1]);
    else if (i < a.end[3]) { /* shared layer: output j, input k */
        const int r = i - a.end[2], j = r / 501, k = r - j * 501;
        if (k == 500) { a.B_bs[j] = a.w.shared_b[j]; return; }
        const float v = a.w.shared_w[(size_t)j * 500 + k];
        a.B_ws[hhp_pidx(k, j, HHP_H)] = v;
        hhr_split(a.h_ws, a.l_ws, hhp_hidx(k, j, HHP_H), v);
        hhr_xput(a.X, (size_t)HHX_L1_PIECES + HHX_ATT_PIECES + (size_t)((((j >> 6) * 4 + (k >> 7)) * 16 + ((k >> 5) & 3) * 4 + ((j >> 4) & 3)) * 2),
                 k, j, false, v);
    } else if (i < a.end[4]) { /* act_out */
        const int r = i - a.end[3], j = r / 501, k = r - j * 501;
        if (k == 500) { a.B_ba[j] = a.w.out_b[j]; return; }
        const float v = a.w.out_w[(size_t)j * 500 + k];
        a.B_wa[hhp_pidx(k, j, HHP_OUT)] = v;
        hhr_split(a.h_wa, a.l_wa, hhp_hidx_t(k, j, HHP_OUT), v);
        hhr_xput(a.X, (size_t)HHX_L1_PIECES + HHX_ATT_PIECES + HHX_L2_PIECES + (size_t)(((k >> 5) * 2 + (j >> 4)) * 2), k, j, false, v);
    } else if (i < a.end[5]) { /* out_proj(v_proj(x)) folded: Wov [j][k], bov [j] */
        const int r = i - a.end[4], j = r / 101, k = r - j * 101;
        if (k == 100) { a.B_bov[j] = hhr_fold_bias(a.w.att_out_w, a.w.att_out_b, a.w.att_in_proj_b + 200, j, 100); return; }
        const float f = hhr_fold(a.w.att_out_w, a.w.att_in_proj_w + (size_t)200 * 100, j, k, 100);
        a.B_wov[hhp_pidx(k, j, HHP_ATT_J)] = f;
        hhr_split(a.h_wov, a.l_wov, hhp_hidx(k, j, HHP_ATT_J), f);
        /* the stream's attention block sits at hidden columns 384 + 32 kb + wq = 400 + k */
        hhr_xput(a.X, (size_t)HHX_L1_PIECES + (size_t)(((j >> 4) * 4 + ((k + 16) >> 5)) * 2), k + 16, j, false, f);
    }
}

/* ---- value branch: the planes + biases of hh_k_policy_ppo and the hh_k_policy_w16_ppo stream (with the branch's own copy of the shared layer).
 * Sections: the input FCs as [wd][nin + 1] (three for fight nets, one for escape nets; column nin = the bias), shared_layer [500][501],
 * val_out [501], the att_val fold [150][151] (fight nets) */
struct HhrCriticArgs {
    hh_critic_weights w;                                                /* [dev] sources */
    uint16_t *h_w1, *l_w1, *h_wov, *l_wov, *h_ws, *l_ws, *h_wa, *l_wa; /* fp16 planes (HhpCrit) */
    float *b1, *bs, *bov, *ba;                                          /* biases (HhpCrit) */
    float *xb1, *xbs, *xbov, *xba;                                      /* the same behind the stream (HhpCritX) */
    uint16_t *X;                                                        /* fragment stream (HhpCritX) */
    int in0[3], nin[3], out0[3], att;
    int end[6];
};
__device__ __forceinline__ void hhr_critic_l1(const HhrCriticArgs &a, const float *W, const float *b, int in0, int nin, int out0, int i) {
    const int o = i / (nin + 1), cc = i - o * (nin + 1), col = hhc_hcol(a.att != 0, out0 + o);
    if (cc == nin) { a.b1[col] = b[o]; a.xb1[col] = b[o]; return; }
    const int c = in0 + cc;
    const float v = W[(size_t)o * nin + cc];
    hhr_split(a.h_w1, a.l_w1, hhp_hidx(c, col, HHP_H), v);
    hhr_xput(a.X, (size_t)((col >> 4) * 3 + (c >> 5)) * 2, c, col, true, v);
}
__global__ __launch_bounds__(HHR_THREADS) void hh_k_refresh_critic(HhrCriticArgs a) {
    const int i = (int)blockIdx.x * HHR_THREADS + (int)threadIdx.x;
    if (i < a.end[0]) hhr_critic_l1(a, a.w.v_w[0], a.w.v_b[0], a.in0[0], a.nin[0], a.out0[0], i);
    else if (i < a.end[1]) hhr_critic_l1(a, a.w.v_w[1], a.w.v_b[1], a.in0[1], a.nin[1], a.out0[1], i - a.end[0]);
    else if (i < a.end[2]) hhr_critic_l1(a, a.w.v_w[2], a.w.v_b[2], a.in0[2], a.nin[2], a.out0[2], i - a.end[1]);
    else if (i < a.end[3]) { /* shared layer, input rows in the branch's hidden order */
        const int r = i - a.end[2], j = r / 501, k = r - j * 501;
        if (k == 500) { a.bs[j] = a.w.shared_b[j]; a.xbs[j] = a.w.shared_b[j]; return; }
        const float v = a.w.shared_w[(size_t)j * 500 + k];
        const int K = hhc_hcol(a.att != 0, k);
        hhr_split(a.h_ws, a.l_ws, hhp_hidx(K, j, HHP_H), v);
        hhr_xput(a.X, (size_t)HHXC_L1_PIECES + HHXC_ATT_PIECES + (size_t)((((j >> 6) * 4 + (K >> 7)) * 16 + ((K >> 5) & 3) * 4 + ((j >> 4) & 3)) * 2),
                 K, j, false, v);
    } else if (i < a.end[4]) { /* val_out: k = 500 the bias */
        const int k = i - a.end[3];
        if (k == 500) { a.ba[0] = a.w.val_b[0]; a.xba[0] = a.w.val_b[0]; return; }
        const float v = a.w.val_w[k];
        hhr_split(a.h_wa, a.l_wa, hhp_hidx_t(k, 0, HHP_OUT), v);
        hhr_xput(a.X, (size_t)HHXC_L1_PIECES + HHXC_ATT_PIECES + HHX_L2_PIECES + (size_t)(k >> 5) * 2, k, 0, false, v);
    } else if (i < a.end[5]) { /* att_val folded: Wov [j][k], bov [j] */
        const int r = i - a.end[4], j = r / 151, k = r - j * 151;
        if (k == 150) {
            const float f = hhr_fold_bias(a.w.att_out_w, a.w.att_out_b, a.w.att_in_proj_b + 300, j, 150);
            a.bov[j] = f; a.xbov[j] = f;
            return;
        }
        const float f = hhr_fold(a.w.att_out_w, a.w.att_in_proj_w + (size_t)300 * 150, j, k, 150);
        hhr_split(a.h_wov, a.l_wov, hhp_hidx(k, j, HHC_ATT_J), f);
        hhr_xput(a.X, (size_t)HHXC_L1_PIECES + (size_t)((j >> 4) * 5 + (k >> 5)) * 2, k, j, false, f);
    }
}

/* ---- commander: the planes and the fp32 section.  Sections: the eight first-layer blocks (actor inp1..inp4, critic v1..v4) as
 * [wd][nc + 1], the two GRUs as [200][201] (column 200: the gate biases), shared_layer [500][501] (column 500: its bias and the output
 * layers' column o) */
struct HhrCommanderArgs {
    hh_commander_weights w;                                        /* [dev] sources */
    uint16_t *h_w1[2], *l_w1[2], *h_wg[2], *l_wg[2], *h_ws, *l_ws; /* fp16 planes (HhcNet) */
    float *b1[2], *bg[2], *wo[2], *bo[2], *bs;                     /* fp32 section */
    int c0[8], nc[8], out0[8];                                     /* HHC_L1A_* / HHC_L1V_* of the eight blocks */
    int end[11];
};
__device__ __forceinline__ void hhr_cmd_l1(uint16_t *h, uint16_t *l, float *b1, const float *W, const float *b, int c0, int nc, int out0, int i) {
    const int o = i / (nc + 1), cc = i - o * (nc + 1);
    if (cc == nc) { b1[out0 + o] = b[o]; return; }
    hhr_split(h, l, hhp_hidx(c0 + cc, out0 + o, 512), W[(size_t)o * nc + cc]);
}
__device__ __forceinline__ void hhr_cmd_gru(uint16_t *h, uint16_t *l, float *bg, const float *wih, const float *whh, const float *bih,
                                            const float *bhh, int i) {
    const int u = i / (HH_CMD_HIDDEN + 1), k = i - u * (HH_CMD_HIDDEN + 1);
    if (k == HH_CMD_HIDDEN) {
        bg[u] = __fadd_rn(bih[u], bhh[u]);
        bg[224 + u] = __fadd_rn(bih[200 + u], bhh[200 + u]);
        bg[448 + u] = bih[400 + u];
        bg[672 + u] = bhh[400 + u];
        return;
    }
    const int col = 128 * (u >> 5) + (u & 31);
    hhr_split(h, l, hhp_hidx(k, col, HHC_JG), wih[(size_t)u * 200 + k]);                    /* r */
    hhr_split(h, l, hhp_hidx(208 + k, col, HHC_JG), whh[(size_t)u * 200 + k]);
    hhr_split(h, l, hhp_hidx(k, col + 32, HHC_JG), wih[(size_t)(200 + u) * 200 + k]);       /* z */
    hhr_split(h, l, hhp_hidx(208 + k, col + 32, HHC_JG), whh[(size_t)(200 + u) * 200 + k]);
    hhr_split(h, l, hhp_hidx(k, col + 64, HHC_JG), wih[(size_t)(400 + u) * 200 + k]);       /* W_in */
    hhr_split(h, l, hhp_hidx(208 + k, col + 96, HHC_JG), whh[(size_t)(400 + u) * 200 + k]); /* W_hn */
}
__global__ __launch_bounds__(HHR_THREADS) void hh_k_refresh_commander(HhrCommanderArgs a) {
    const int i = (int)blockIdx.x * HHR_THREADS + (int)threadIdx.x;
#pragma unroll
    for (int q = 0; q < 8; q++) { /* q < 4: actor inp{q+1}; q >= 4: critic v{q-3} */
        const int lo = q ? a.end[q - 1] : 0;
        if (i >= lo && i < a.end[q])
            hhr_cmd_l1(a.h_w1[q >> 2], a.l_w1[q >> 2], a.b1[q >> 2], q < 4 ? a.w.inp_w[q & 3] : a.w.v_w[q & 3],
                       q < 4 ? a.w.inp_b[q & 3] : a.w.v_b[q & 3], a.c0[q], a.nc[q], a.out0[q], i - lo);
    }
    if (i >= a.end[7] && i < a.end[8]) hhr_cmd_gru(a.h_wg[0], a.l_wg[0], a.bg[0], a.w.act_w_ih, a.w.act_w_hh, a.w.act_b_ih, a.w.act_b_hh, i - a.end[7]);
    else if (i >= a.end[8] && i < a.end[9]) hhr_cmd_gru(a.h_wg[1], a.l_wg[1], a.bg[1], a.w.val_w_ih, a.w.val_w_hh, a.w.val_b_ih, a.w.val_b_hh, i - a.end[8]);
    else if (i >= a.end[9] && i < a.end[10]) { /* shared layer: output o, reference input column src -> S row [e (300) | 0 | f (200) | 0] */
        const int r = i - a.end[9], o = r / 501, src = r - o * 501;
        if (src == 500) {
            a.bs[o] = a.w.shared_b[o];
            for (int j = 0; j < 3; j++) a.wo[0][(size_t)j * 512 + o] = a.w.act_out_w[(size_t)j * 500 + o];
            a.wo[1][o] = a.w.val_out_w[o];
            if (o < 3) a.bo[0][o] = a.w.act_out_b[o];
            if (o == 0) a.bo[1][0] = a.w.val_out_b[0];
            return;
        }
        const int k = src < 300 ? src : HHC_FOFF + (src - 300);
        hhr_split(a.h_ws, a.l_ws, hhp_hidx(k, o, HHC_KS), a.w.shared_w[(size_t)o * 500 + src]);
    }
}

/* ===================================================================== host side */
static bool hhr_actor_complete(const hh_net_weights *w, bool att) {
    for (int k = 0; k < 3; k++) if (!w->inp_w[k] || !w->inp_b[k]) return false;
    return w->shared_w && w->shared_b && w->out_w && w->out_b && (!att || (w->att_in_proj_w && w->att_in_proj_b && w->att_out_w && w->att_out_b));
}
static bool hhr_critic_complete(const hh_critic_weights *w, bool att) {
    if (!w->v_w[0] || !w->v_b[0] || !w->shared_w || !w->shared_b || !w->val_w || !w->val_b) return false;
    return !att || (w->v_w[1] && w->v_b[1] && w->v_w[2] && w->v_b[2] && w->att_in_proj_w && w->att_in_proj_b && w->att_out_w && w->att_out_b);
}
static uint16_t *hhr_h16(const float4 *q) { return reinterpret_cast<uint16_t *>(const_cast<float4 *>(q)); }

/* A load's sources: `at` = a pointer member of the load's own copy of the weights struct, holding the caller's HOST array of n floats.
 * upload() copies them back to back into ONE temporary device buffer and rewrites every member to its device copy, which turns the
 * struct into what the kernels take.  The buffer goes with the HhrStage, i.e. after the load has waited for its kernel. */
struct HhrSrc { const float **at; size_t n; };
struct HhrStage {
    float *buf = nullptr;
    ~HhrStage() { if (buf) (void)hipFree(buf); }
    hipError_t upload(const HhrSrc *src, int n_src) {
        size_t total = 0;
        for (int i = 0; i < n_src; i++) total += (src[i].n + 3) & ~(size_t)3; /* every array 16-byte aligned */
        hipError_t e = hipMalloc(&buf, total * sizeof(float));
        float *d = buf;
        for (int i = 0; i < n_src && e == hipSuccess; i++) {
            e = hipMemcpy(d, *src[i].at, src[i].n * sizeof(float), hipMemcpyHostToDevice);
            *src[i].at = d;
            d += (src[i].n + 3) & ~(size_t)3;
        }
        return e;
    }
};
/* the end of a load: its kernel has run when the call returns, so the caller's arrays are free and a launch on any stream sees the weights */
static int hhr_finish_load() {
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    return HH_OK;
}

/* the actor of a laid-out slot from [dev] sources: one launch on st */
static void hhr_launch_actor(hh_policy *p, int slot, const hh_net_weights &w, hipStream_t st) {
    const HhpNet &N = p->bank.net[slot];
    HhrActorArgs a;
    memset(&a, 0, sizeof(a));
    a.w = w;
    a.B_w1 = const_cast<float *>(N.w1p); a.B_b1 = const_cast<float *>(N.b1); a.B_wov = const_cast<float *>(N.wovp); a.B_bov = const_cast<float *>(N.bov);
    a.B_ws = const_cast<float *>(N.wsp); a.B_bs = const_cast<float *>(N.bs); a.B_wa = const_cast<float *>(N.wap); a.B_ba = const_cast<float *>(N.ba);
    const HhpNetH &H = p->bankh.net[slot];
    a.h_w1 = hhr_h16(H.w1h); a.l_w1 = hhr_h16(H.w1l); a.h_wov = hhr_h16(H.wovh); a.l_wov = hhr_h16(H.wovl);
    a.h_ws = hhr_h16(H.wsh); a.l_ws = hhr_h16(H.wsl); a.h_wa = hhr_h16(H.wah); a.l_wa = hhr_h16(H.wal);
    a.X = reinterpret_cast<uint16_t *>(p->xblob[slot]);
    int e = 0;
    for (int k = 0; k < 3; k++) {
        a.c0[k] = HHP_INPUTS[N.kind][k][0]; a.nc[k] = HHP_INPUTS[N.kind][k][1] - a.c0[k]; a.wd[k] = HHP_INPUTS[N.kind][k][2];
        a.end[k] = e += a.wd[k] * (a.nc[k] + 1);
    }
    a.end[3] = e += 500 * 501;
    a.end[4] = e += N.n_out * 501;
    a.end[5] = e += N.has_att ? 100 * 101 : 0;
    hipLaunchKernelGGL(hh_k_refresh_actor, dim3((e + HHR_THREADS - 1) / HHR_THREADS), dim3(HHR_THREADS), 0, st, a);
}

/* the value branch's input FCs -> their number.  Fight nets: v1 [own obs | own act], v2 [other obs | other act], v3 [all] at columns 0,
 * 175, 350 of cat(v1, v2, y3); escape nets: inp1_val [all] -> 500 */
static int hhr_critic_blocks(int kind, int in0[3], int nin[3], int wd[3], int out0[3]) {
    const int own = HHC_DIMS[kind][0] + HHC_DIMS[kind][1], n_in = own + HHC_DIMS[kind][2] + HHC_DIMS[kind][3];
    if (kind > HH_NET_FIGHT2) { in0[0] = 0; nin[0] = n_in; wd[0] = 500; out0[0] = 0; return 1; }
    in0[0] = 0; nin[0] = own; wd[0] = 175; out0[0] = 0;
    in0[1] = own; nin[1] = n_in - own; wd[1] = 175; out0[1] = 175;
    in0[2] = 0; nin[2] = n_in; wd[2] = 150; out0[2] = 350;
    return 3;
}
/* the value branch of a laid-out slot from [dev] sources: one launch on st */
static void hhr_launch_critic(hh_policy *p, int slot, const hh_critic_weights &w, hipStream_t st) {
    const HhpCrit &Cn = p->cbank.c[slot];
    const HhpCritX &Cx = p->cbankx.c[slot];
    HhrCriticArgs a;
    memset(&a, 0, sizeof(a));
    a.w = w;
    a.h_w1 = hhr_h16(Cn.w1h); a.l_w1 = hhr_h16(Cn.w1l); a.h_wov = hhr_h16(Cn.wovh); a.l_wov = hhr_h16(Cn.wovl);
    a.h_ws = hhr_h16(Cn.wsh); a.l_ws = hhr_h16(Cn.wsl); a.h_wa = hhr_h16(Cn.wah); a.l_wa = hhr_h16(Cn.wal);
    a.b1 = const_cast<float *>(Cn.b1); a.bs = const_cast<float *>(Cn.bs); a.bov = const_cast<float *>(Cn.bov); a.ba = const_cast<float *>(Cn.ba);
    a.xb1 = const_cast<float *>(Cx.b1); a.xbs = const_cast<float *>(Cx.bs); a.xbov = const_cast<float *>(Cx.bov); a.xba = const_cast<float *>(Cx.ba);
    a.X = reinterpret_cast<uint16_t *>(p->cxblob[slot]);
    a.att = Cn.has_att;
    int wd[3], e = 0;
    const int nb = hhr_critic_blocks(p->bank.net[slot].kind, a.in0, a.nin, wd, a.out0);
    for (int b = 0; b < 3; b++) a.end[b] = e += b < nb ? wd[b] * (a.nin[b] + 1) : 0;
    a.end[3] = e += 500 * 501;
    a.end[4] = e += 501;
    a.end[5] = e += a.att ? 150 * 151 : 0;
    hipLaunchKernelGGL(hh_k_refresh_critic, dim3((e + HHR_THREADS - 1) / HHR_THREADS), dim3(HHR_THREADS), 0, st, a);
}

extern "C" int hh_policy_set_net(hh_policy *p, int32_t slot, const hh_net_weights *w) {
    if (!p || !w || slot < 0 || slot >= HH_POLICY_MAX_NETS || w->kind < 0 || w->kind > 3) { g_err = "bad argument"; return HH_E_ARG; }
    const bool att = w->kind <= HH_NET_FIGHT2;
    if (!w->shared_w || !w->shared_b || !w->out_w || !w->out_b || (att && (!w->att_in_proj_w || !w->att_in_proj_b || !w->att_out_w || !w->att_out_b))) {
        g_err = "hh_policy_set_net: missing weight pointer"; return HH_E_ARG;
    }
    for (int k = 0; k < 3; k++) if (!w->inp_w[k] || !w->inp_b[k]) { g_err = "hh_policy_set_net: missing input layer"; return HH_E_ARG; }
    HH_GUARD(p);
    const int n_out = (w->kind == HH_NET_FIGHT1 || w->kind == HH_NET_ESC1) ? 26 : 24;
    hh_net_weights d = *w;
    if (!att) d.att_in_proj_w = d.att_in_proj_b = d.att_out_w = d.att_out_b = nullptr;
    HhrSrc src[14];
    int n = 0, obs_dim = 0;
    for (int k = 0; k < 3; k++) {
        const int c0 = HHP_INPUTS[w->kind][k][0], c1 = HHP_INPUTS[w->kind][k][1], wd = HHP_INPUTS[w->kind][k][2];
        src[n++] = {&d.inp_w[k], (size_t)wd * (c1 - c0)}; src[n++] = {&d.inp_b[k], (size_t)wd};
        if (c1 > obs_dim) obs_dim = c1;
    }
    if (att) { src[n++] = {&d.att_in_proj_w, 300 * 100}; src[n++] = {&d.att_in_proj_b, 300}; src[n++] = {&d.att_out_w, 100 * 100}; src[n++] = {&d.att_out_b, 100}; }
    src[n++] = {&d.shared_w, 500 * 500}; src[n++] = {&d.shared_b, 500}; src[n++] = {&d.out_w, (size_t)n_out * 500}; src[n++] = {&d.out_b, (size_t)n_out};
    HhrStage stage;
    HIPCHK(stage.upload(src, n));
    /* the slot's value branch holds its own permuted copy of the shared layer and the input widths of the kind it was loaded for: a new
     * actor makes both stale.  hh_policy_sample refuses vf for the slot until hh_policy_set_critic is called again (set_net + set_critic
     * are a pair; the old copy stays allocated and is simply never read) */
    p->cbank.c[slot].loaded = 0;
    p->cbankx.c[slot].loaded = 0;
    /* blob: w1p | b1 | wovp | bov | wsp | bs | wap | ba   (float counts; every section 16-byte aligned) */
    const size_t n_w1 = 4 * 2 * HHP_H * 4, n_wov = 13 * 2 * HHP_ATT_J * 4, n_ws = 64 * 2 * HHP_H * 4, n_wa = 64 * 2 * HHP_OUT * 4;
    const size_t o_w1 = 0, o_b1 = o_w1 + n_w1, o_wov = o_b1 + HHP_H, o_bov = o_wov + n_wov, o_ws = o_bov + HHP_ATT_J, o_bs = o_ws + n_ws,
                 o_wa = o_bs + HHP_H, o_ba = o_wa + n_wa, total = o_ba + HHP_OUT;
    /* the same four matrices as (hi, lo) fp16 fragment planes for hh_k_policy_h: w1 | wov | ws | wa, each [K/16][2][J][8] */
    const size_t h_w1 = 0, h_wov = h_w1 + (size_t)2 * 2 * HHP_H * 8, h_ws = h_wov + (size_t)7 * 2 * HHP_ATT_J * 8, h_wa = h_ws + (size_t)32 * 2 * HHP_H * 8,
                 h_total = h_wa + (size_t)32 * 2 * HHP_OUT * 8;
    static_assert(HHP_SLOT_BYTES >= (size_t)2 * 1024 * 1024 + 2 * 309248 * 2, "slot too small");
    if (total * sizeof(float) > (size_t)2 * 1024 * 1024 || 2 * h_total * sizeof(uint16_t) > HHP_SLOT_BYTES - (size_t)2 * 1024 * 1024) { g_err = "internal: blob exceeds its slot"; return HH_E_ARG; }
    /* ... and as ONE linear stream of 1 KB fragments in consumption order (hh_policy_kernel_w16.h) */
    const size_t xbytes = (size_t)HHX_STREAM_PIECES * HHW_PIECE;
    if (!p->xblob[slot]) HIPCHK(hipMalloc(&p->xblob[slot], xbytes));
    p->bankx.stream[slot] = p->xblob[slot];
    p->blob[slot] = reinterpret_cast<float *>(p->slab + (size_t)slot * HHP_SLOT_BYTES);                                   /* first 2 MB of the slot */
    p->blobh[slot] = reinterpret_cast<uint16_t *>(p->slab + (size_t)slot * HHP_SLOT_BYTES + (size_t)2 * 1024 * 1024);      /* second 2 MB */
    {
        HhpNetH &Hn = p->bankh.net[slot];
        const uint16_t *bh = p->blobh[slot], *bl = p->blobh[slot] + h_total;
        Hn.w1h = reinterpret_cast<const float4 *>(bh + h_w1); Hn.w1l = reinterpret_cast<const float4 *>(bl + h_w1);
        Hn.wovh = reinterpret_cast<const float4 *>(bh + h_wov); Hn.wovl = reinterpret_cast<const float4 *>(bl + h_wov);
        Hn.wsh = reinterpret_cast<const float4 *>(bh + h_ws); Hn.wsl = reinterpret_cast<const float4 *>(bl + h_ws);
        Hn.wah = reinterpret_cast<const float4 *>(bh + h_wa); Hn.wal = reinterpret_cast<const float4 *>(bl + h_wa);
    }
    HhpNet &N = p->bank.net[slot];
    float *b = p->blob[slot];
    N.w1p = b + o_w1; N.b1 = b + o_b1; N.wovp = b + o_wov; N.bov = b + o_bov; N.wsp = b + o_ws; N.bs = b + o_bs; N.wap = b + o_wa; N.ba = b + o_ba;
    N.kind = w->kind; N.n_out = n_out; N.obs_dim = obs_dim; N.has_att = att ? 1 : 0;
    if (slot + 1 > p->n_nets) p->n_nets = slot + 1;
    /* the kernel writes no padding, and the slot may have held another kind: all of it to zero first */
    HIPCHK(hipMemsetAsync(p->blob[slot], 0, total * sizeof(float), nullptr));
    HIPCHK(hipMemsetAsync(p->blobh[slot], 0, 2 * h_total * sizeof(uint16_t), nullptr));
    HIPCHK(hipMemsetAsync(p->xblob[slot], 0, xbytes, nullptr));
    hhr_launch_actor(p, slot, d, nullptr);
    return hhr_finish_load();
}

extern "C" int hh_policy_set_critic(hh_policy *p, int32_t slot, const hh_critic_weights *w) {
    if (!p || !w || slot < 0 || slot >= HH_POLICY_MAX_NETS || w->kind < 0 || w->kind > 3) { g_err = "bad argument"; return HH_E_ARG; }
    if (!p->blob[slot] || p->bank.net[slot].kind != w->kind) { g_err = "hh_policy_set_critic: load the actor of the same kind into this slot first (hh_policy_set_net)"; return HH_E_ARG; }
    const bool att = w->kind <= HH_NET_FIGHT2;
    if (!hhr_critic_complete(w, att)) { g_err = "hh_policy_set_critic: missing weight pointer"; return HH_E_ARG; }
    HH_GUARD(p);
    hh_critic_weights d = *w;
    if (!att) d.v_w[1] = d.v_w[2] = d.v_b[1] = d.v_b[2] = d.att_in_proj_w = d.att_in_proj_b = d.att_out_w = d.att_out_b = nullptr;
    HhrSrc src[14];
    int n = 0, in0[3], nin[3], wd[3], out0[3];
    const int nb = hhr_critic_blocks(w->kind, in0, nin, wd, out0);
    for (int b = 0; b < nb; b++) { src[n++] = {&d.v_w[b], (size_t)wd[b] * nin[b]}; src[n++] = {&d.v_b[b], (size_t)wd[b]}; }
    if (att) { src[n++] = {&d.att_in_proj_w, 450 * 150}; src[n++] = {&d.att_in_proj_b, 450}; src[n++] = {&d.att_out_w, 150 * 150}; src[n++] = {&d.att_out_b, 150}; }
    src[n++] = {&d.shared_w, 500 * 500}; src[n++] = {&d.shared_b, 500}; src[n++] = {&d.val_w, 500}; src[n++] = {&d.val_b, 1};
    HhrStage stage;
    HIPCHK(stage.upload(src, n));
    const int d1 = HHC_DIMS[w->kind][0], a1 = HHC_DIMS[w->kind][1], d2 = HHC_DIMS[w->kind][2], a2 = HHC_DIMS[w->kind][3];
    /* fragment planes (halves): w1 [80 x 512] | wov [160 x 256] | ws [512 x 512] | wa [512 x 32]; then the float biases b1 | bs | bov | ba */
    const size_t h_w1 = 0, h_wov = h_w1 + (size_t)(HHC_XK / 16) * 2 * HHP_H * 8, h_ws = h_wov + (size_t)(HHC_ATT_W / 16) * 2 * HHC_ATT_J * 8,
                 h_wa = h_ws + (size_t)32 * 2 * HHP_H * 8, h_total = h_wa + (size_t)32 * 2 * HHP_OUT * 8;
    const size_t o_b1 = 0, o_bs = 512, o_bov = 1024, o_ba = 1024 + HHC_ATT_W, n_bias = o_ba + HHP_OUT;
    const size_t plane_bytes = h_total * sizeof(uint16_t), bytes = 2 * plane_bytes + n_bias * sizeof(float);
    /* the same value branch as ONE linear stream of 1 KB fragments for hh_k_policy_w16_ppo (chunk order of hhx_critic_tile) + its biases */
    const size_t xbytes = (size_t)HHXC_STREAM_PIECES * HHW_PIECE, xbias = (size_t)(512 + 512 + 160 + 32) * sizeof(float);
    if (!p->cxblob[slot]) HIPCHK(hipMalloc(&p->cxblob[slot], xbytes + xbias));
    if (!p->cblob[slot]) HIPCHK(hipMalloc(&p->cblob[slot], bytes));
    HhpCritX &Cx = p->cbankx.c[slot];
    const float *xb = reinterpret_cast<const float *>(p->cxblob[slot] + xbytes);
    Cx.stream = reinterpret_cast<const unsigned char *>(p->cxblob[slot]);
    Cx.b1 = xb; Cx.bs = xb + 512; Cx.bov = xb + 1024; Cx.ba = xb + 1184;
    Cx.d1 = d1; Cx.a1 = a1; Cx.d2 = d2; Cx.a2 = a2; Cx.has_att = att ? 1 : 0; Cx.loaded = 1;
    char *c = p->cblob[slot];
    HhpCrit &Cn = p->cbank.c[slot];
    const uint16_t *bh = reinterpret_cast<const uint16_t *>(c), *bl = reinterpret_cast<const uint16_t *>(c + plane_bytes);
    const float *bf = reinterpret_cast<const float *>(c + 2 * plane_bytes);
    Cn.w1h = reinterpret_cast<const float4 *>(bh + h_w1); Cn.w1l = reinterpret_cast<const float4 *>(bl + h_w1);
    Cn.wovh = reinterpret_cast<const float4 *>(bh + h_wov); Cn.wovl = reinterpret_cast<const float4 *>(bl + h_wov);
    Cn.wsh = reinterpret_cast<const float4 *>(bh + h_ws); Cn.wsl = reinterpret_cast<const float4 *>(bl + h_ws);
    Cn.wah = reinterpret_cast<const float4 *>(bh + h_wa); Cn.wal = reinterpret_cast<const float4 *>(bl + h_wa);
    Cn.b1 = bf + o_b1; Cn.bs = bf + o_bs; Cn.bov = bf + o_bov; Cn.ba = bf + o_ba;
    Cn.d1 = d1; Cn.a1 = a1; Cn.d2 = d2; Cn.a2 = a2; Cn.has_att = att ? 1 : 0; Cn.loaded = 1;
    HIPCHK(hipMemsetAsync(p->cblob[slot], 0, bytes, nullptr));
    HIPCHK(hipMemsetAsync(p->cxblob[slot], 0, xbytes + xbias, nullptr));
    hhr_launch_critic(p, slot, d, nullptr);
    return hhr_finish_load();
}

extern "C" int hh_policy_refresh(hh_policy *p, int32_t slot, const hh_net_weights *w, const hh_critic_weights *cw, void *stream) {
    if (!p || !w || slot < 0 || slot >= HH_POLICY_MAX_NETS) { g_err = "hh_policy_refresh: bad argument"; return HH_E_ARG; }
    if (!p->blob[slot] || !p->xblob[slot]) { g_err = "hh_policy_refresh: the slot is empty (load it once with hh_policy_set_net)"; return HH_E_ARG; }
    const HhpNet &N = p->bank.net[slot];
    if (w->kind != N.kind) { g_err = "hh_policy_refresh: actor->kind differs from the network loaded in the slot"; return HH_E_ARG; }
    const bool att = N.has_att != 0;
    if (!hhr_actor_complete(w, att)) { g_err = "hh_policy_refresh: missing actor weight pointer"; return HH_E_ARG; }
    const bool crit = p->cbank.c[slot].loaded && p->cbankx.c[slot].loaded;
    if (crit && !cw) { g_err = "hh_policy_refresh: the slot's value branch is loaded: refresh it together with the actor (critic != NULL)"; return HH_E_ARG; }
    if (!crit && cw) { g_err = "hh_policy_refresh: the slot has no value branch loaded (hh_policy_set_critic): critic must be NULL"; return HH_E_ARG; }
    if (cw && cw->kind != N.kind) { g_err = "hh_policy_refresh: critic->kind differs from the network loaded in the slot"; return HH_E_ARG; }
    if (cw && !hhr_critic_complete(cw, att)) { g_err = "hh_policy_refresh: missing critic weight pointer"; return HH_E_ARG; }
    HH_GUARD(p);
    hhr_launch_actor(p, slot, *w, (hipStream_t)stream);
    if (cw) hhr_launch_critic(p, slot, *cw, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

/* one packed part of a slot (HH_POLICY_PART_*) where the forward kernels read it: its start and its size in bytes */
static int hhr_policy_part(const hh_policy *p, int32_t slot, int32_t part, const char **src, int64_t *bytes) {
    if (slot < 0 || slot >= HH_POLICY_MAX_NETS || !p->blob[slot]) { g_err = "hh_policy_copy_packed: the slot is empty"; return HH_E_ARG; }
    const HhpNet &N = p->bank.net[slot];
    const HhpNetH &H = p->bankh.net[slot];
    switch (part) {
    case HH_POLICY_PART_BLOB: *src = reinterpret_cast<const char *>(p->blob[slot]); *bytes = (int64_t)((N.ba + HHP_OUT) - p->blob[slot]) * 4; return HH_OK;
    case HH_POLICY_PART_PLANES: /* the hi plane, then the lo plane; w1 is the first section of both */
        *src = reinterpret_cast<const char *>(p->blobh[slot]);
        *bytes = 2 * (int64_t)(reinterpret_cast<const char *>(H.w1l) - reinterpret_cast<const char *>(H.w1h));
        return HH_OK;
    case HH_POLICY_PART_STREAM: *src = reinterpret_cast<const char *>(p->xblob[slot]); *bytes = (int64_t)HHX_STREAM_PIECES * HHW_PIECE; return HH_OK;
    case HH_POLICY_PART_CRITIC:
        if (!p->cblob[slot]) break;
        *src = p->cblob[slot];
        *bytes = (int64_t)(reinterpret_cast<const char *>(p->cbank.c[slot].ba + HHP_OUT) - p->cblob[slot]);
        return HH_OK;
    case HH_POLICY_PART_CRITIC_STREAM:
        if (!p->cxblob[slot]) break;
        *src = p->cxblob[slot];
        *bytes = (int64_t)(reinterpret_cast<const char *>(p->cbankx.c[slot].ba + 32) - p->cxblob[slot]);
        return HH_OK;
    default: g_err = "hh_policy_copy_packed: unknown part"; return HH_E_ARG;
    }
    g_err = "hh_policy_copy_packed: the slot has no value branch (hh_policy_set_critic)";
    return HH_E_ARG;
}
extern "C" int hh_policy_copy_packed(hh_policy *p, int32_t slot, int32_t part, void *dst, int64_t cap, int64_t *bytes, void *stream) {
    if (!p || !bytes) { g_err = "hh_policy_copy_packed: bad argument"; return HH_E_ARG; }
    const char *src = nullptr;
    int64_t n = 0;
    const int rc = hhr_policy_part(p, slot, part, &src, &n);
    if (rc != HH_OK) return rc;
    *bytes = n;
    if (!dst) return HH_OK;
    if (cap < n) { g_err = "hh_policy_copy_packed: the destination is smaller than the part"; return HH_E_ARG; }
    HH_GUARD(p);
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return HH_OK;
}

static bool hhr_commander_complete(const hh_commander_weights *w, const char *who) {
    const float *need[] = {w->act_w_ih, w->act_w_hh, w->act_b_ih, w->act_b_hh, w->shared_w, w->shared_b, w->act_out_w, w->act_out_b,
                           w->val_w_ih, w->val_w_hh, w->val_b_ih, w->val_b_hh, w->val_out_w, w->val_out_b};
    for (const float *q : need) if (!q) { g_err = std::string(who) + ": missing weight pointer"; return false; }
    for (int k = 0; k < 4; k++) if (!w->inp_w[k] || !w->inp_b[k] || !w->v_w[k] || !w->v_b[k]) { g_err = std::string(who) + ": missing input layer"; return false; }
    return true;
}
/* a laid-out commander from [dev] sources: one launch on st */
static void hhr_launch_commander(hh_commander *c, const hh_commander_weights &w, hipStream_t st) {
    HhrCommanderArgs a;
    memset(&a, 0, sizeof(a));
    a.w = w;
    const HhcNet &N = c->net;
    for (int b = 0; b < 2; b++) {
        const HhcBranch &Br = N.br[b];
        a.h_w1[b] = hhr_h16(Br.w1h); a.l_w1[b] = hhr_h16(Br.w1l); a.h_wg[b] = hhr_h16(Br.wgh); a.l_wg[b] = hhr_h16(Br.wgl);
        a.b1[b] = const_cast<float *>(Br.b1); a.bg[b] = const_cast<float *>(Br.bg); a.wo[b] = const_cast<float *>(Br.wo); a.bo[b] = const_cast<float *>(Br.bo);
    }
    a.h_ws = hhr_h16(N.wsh); a.l_ws = hhr_h16(N.wsl); a.bs = const_cast<float *>(N.bs);
    int e = 0;
    for (int q = 0; q < 8; q++) {
        const int k = q & 3;
        a.c0[q] = q < 4 ? HHC_L1A_C0[k] : HHC_L1V_C0[k];
        a.nc[q] = q < 4 ? HHC_L1A_C1[k] - HHC_L1A_C0[k] : HHC_L1V_IN[k];
        a.out0[q] = q < 4 ? HHC_L1A_OUT0[k] : HHC_L1V_OUT0[k];
        a.end[q] = e += (q < 4 ? HHC_L1A_WD[k] : HHC_L1V_WD[k]) * (a.nc[q] + 1);
    }
    a.end[8] = e += HH_CMD_HIDDEN * (HH_CMD_HIDDEN + 1);
    a.end[9] = e += HH_CMD_HIDDEN * (HH_CMD_HIDDEN + 1);
    a.end[10] = e += 500 * 501;
    hipLaunchKernelGGL(hh_k_refresh_commander, dim3((e + HHR_THREADS - 1) / HHR_THREADS), dim3(HHR_THREADS), 0, st, a);
}

extern "C" int hh_commander_set_weights(hh_commander *c, const hh_commander_weights *w) {
    if (!c || !w) { g_err = "hh_commander_set_weights: bad argument"; return HH_E_ARG; }
    if (!hhr_commander_complete(w, "hh_commander_set_weights")) return HH_E_ARG;
    HH_GUARD(c);
    hh_commander_weights d = *w;
    HhrSrc src[30];
    int n = 0;
    for (int k = 0; k < 4; k++) {
        src[n++] = {&d.inp_w[k], (size_t)HHC_L1A_WD[k] * (HHC_L1A_C1[k] - HHC_L1A_C0[k])}; src[n++] = {&d.inp_b[k], (size_t)HHC_L1A_WD[k]};
        src[n++] = {&d.v_w[k], (size_t)HHC_L1V_WD[k] * HHC_L1V_IN[k]}; src[n++] = {&d.v_b[k], (size_t)HHC_L1V_WD[k]};
    }
    const size_t gw = (size_t)3 * HH_CMD_HIDDEN * HH_CMD_HIDDEN, gb = 3 * HH_CMD_HIDDEN; /* gate rows r | z | n */
    src[n++] = {&d.act_w_ih, gw}; src[n++] = {&d.act_w_hh, gw}; src[n++] = {&d.act_b_ih, gb}; src[n++] = {&d.act_b_hh, gb};
    src[n++] = {&d.val_w_ih, gw}; src[n++] = {&d.val_w_hh, gw}; src[n++] = {&d.val_b_ih, gb}; src[n++] = {&d.val_b_hh, gb};
    src[n++] = {&d.shared_w, 500 * 500}; src[n++] = {&d.shared_b, 500};
    src[n++] = {&d.act_out_w, HH_CMD_ACTIONS * 500}; src[n++] = {&d.act_out_b, HH_CMD_ACTIONS}; src[n++] = {&d.val_out_w, 500}; src[n++] = {&d.val_out_b, 1};
    HhrStage stage;
    HIPCHK(stage.upload(src, n));
    const int K1[2] = {48, 112};
    /* halves: w1 actor | w1 critic | wg actor | wg critic | ws */
    const size_t n_w1a = (size_t)48 * 512, n_w1c = (size_t)112 * 512, n_wg = (size_t)HHC_KG * HHC_JG;
    const size_t h_w1[2] = {0, n_w1a}, h_wg[2] = {n_w1a + n_w1c, n_w1a + n_w1c + n_wg}, h_ws = n_w1a + n_w1c + 2 * n_wg, h_total = h_ws + (size_t)HHC_KS * HHC_KS;
    /* floats: b1 a | b1 c | bg a | bg c | bs | wo a [3][512] | wo c [512] | bo a [4] | bo c [4] */
    const size_t f_b1[2] = {0, 512}, f_bg[2] = {1024, 1920}, f_bs = 2816, f_wo[2] = {3328, 4864}, f_bo[2] = {5376, 5380}, f_total = 5384;
    const size_t plane_bytes = h_total * sizeof(uint16_t), bytes = 2 * plane_bytes + f_total * sizeof(float);
    if (!c->blob) HIPCHK(hipMalloc(&c->blob, bytes));
    const uint16_t *bh = reinterpret_cast<const uint16_t *>(c->blob), *bl = reinterpret_cast<const uint16_t *>(c->blob + plane_bytes);
    const float *bf = reinterpret_cast<const float *>(c->blob + 2 * plane_bytes);
    HhcNet &N = c->net;
    for (int b = 0; b < 2; b++) {
        HhcBranch &Br = N.br[b];
        Br.w1h = reinterpret_cast<const float4 *>(bh + h_w1[b]); Br.w1l = reinterpret_cast<const float4 *>(bl + h_w1[b]);
        Br.wgh = reinterpret_cast<const float4 *>(bh + h_wg[b]); Br.wgl = reinterpret_cast<const float4 *>(bl + h_wg[b]);
        Br.b1 = bf + f_b1[b]; Br.bg = bf + f_bg[b]; Br.wo = bf + f_wo[b]; Br.bo = bf + f_bo[b];
        Br.k1 = K1[b];
    }
    N.wsh = reinterpret_cast<const float4 *>(bh + h_ws); N.wsl = reinterpret_cast<const float4 *>(bl + h_ws);
    N.bs = bf + f_bs;
    c->loaded = 1;
    HIPCHK(hipMemsetAsync(c->blob, 0, bytes, nullptr)); /* the kernel writes no padding */
    hhr_launch_commander(c, d, nullptr);
    return hhr_finish_load();
}

extern "C" int hh_commander_refresh_weights(hh_commander *c, const hh_commander_weights *w, void *stream) {
    if (!c || !w) { g_err = "hh_commander_refresh_weights: bad argument"; return HH_E_ARG; }
    if (!c->loaded || !c->blob) { g_err = "hh_commander_refresh_weights: no weights loaded (hh_commander_set_weights allocates the buffers once)"; return HH_E_ARG; }
    if (!hhr_commander_complete(w, "hh_commander_refresh_weights")) return HH_E_ARG;
    HH_GUARD(c);
    hhr_launch_commander(c, *w, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_commander_copy_packed(hh_commander *c, int32_t part, void *dst, int64_t cap, int64_t *bytes, void *stream) {
    if (!c || !bytes) { g_err = "hh_commander_copy_packed: bad argument"; return HH_E_ARG; }
    if (!c->loaded || !c->blob) { g_err = "hh_commander_copy_packed: no weights loaded"; return HH_E_ARG; }
    const HhcNet &N = c->net;
    const char *planes = c->blob, *f32 = reinterpret_cast<const char *>(N.br[0].b1); /* the fp32 section starts with the actor's b1 */
    const char *src;
    int64_t n;
    if (part == HH_COMMANDER_PART_PLANES) { src = planes; n = (int64_t)(f32 - planes); }
    else if (part == HH_COMMANDER_PART_F32) { src = f32; n = (int64_t)(reinterpret_cast<const char *>(N.br[1].bo + 4) - f32); }
    else { g_err = "hh_commander_copy_packed: unknown part"; return HH_E_ARG; }
    *bytes = n;
    if (!dst) return HH_OK;
    if (cap < n) { g_err = "hh_commander_copy_packed: the destination is smaller than the part"; return HH_E_ARG; }
    HH_GUARD(c);
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return HH_OK;
}

#endif /* HH_WEIGHT_REFRESH_H */
