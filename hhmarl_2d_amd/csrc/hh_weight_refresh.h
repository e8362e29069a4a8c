/*
 * hh_weight_refresh.h — the learner's new weights into the samplers on the device (C ABI: hh_policy_refresh / hh_policy_copy_packed in
 * include/hh_policy.h, hh_commander_refresh_weights / hh_commander_copy_packed in include/hh_commander.h).
 *
 * hh_policy_set_net / hh_policy_set_critic / hh_commander_set_weights repack fp32 HOST arrays on the CPU and upload them with synchronous
 * copies.  The kernels here read the learner's fp32 DEVICE tensors (the reference's state_dict layout) and write, in place and ordered on
 * the caller's stream, the same bytes into the same buffers: the fp32 blob, the (hi, lo) fp16 fragment planes, the 1 KB fragment streams
 * and, for Fight1 / Fight2, the folded attention (Wov = Wo Wv, bov = Wo bv + bo in fp64, m = 0, 1, ... in order, multiply and add
 * rounded separately like the host's loop).  One thread per SOURCE element (and one per bias row): it computes the destination of every
 * packed form the element feeds through the index maps the host loops use (hhp_pidx, hhp_hidx, hhp_hidx_t, hhx_at / hhw16_korder) and
 * splits with the host's own hhp_f2h / hhp_h2f.  The sections' addresses are the bank's own (HhpNet, HhpNetH, HhpBankX, HhpCrit,
 * HhpCritX, HhcNet), i.e. exactly where the forward kernels read.  Padding is never written: the host load zeroed it and a refresh keeps
 * the kind, hence the layout.  No allocation, no host synchronisation, no scratch: a refresh can be captured into a HIP graph.
 */
#ifndef HH_WEIGHT_REFRESH_H
#define HH_WEIGHT_REFRESH_H

#define HHR_THREADS 256

__device__ __forceinline__ void hhr_split(uint16_t *hi, uint16_t *lo, size_t at, float v) {
    const uint16_t h = hhp_f2h(v);
    hi[at] = h;
    lo[at] = hhp_f2h(v - hhp_h2f(h));
}
/* hhx_put on the device: element (k, col) into fragment piece `piece_hi` of a stream (its lo half is the next piece) */
__device__ __forceinline__ void hhr_xput(uint16_t *S, size_t piece_hi, int k, int col, bool nat, float v) {
    hhr_split(S + piece_hi * (HHW_PIECE / 2), S + (piece_hi + 1) * (HHW_PIECE / 2), hhx_at(k, col, nat), v);
}
/* the host's attention fold: s = 0; s += Wo[j][m] Wv[m][k] for m = 0 .. n - 1 in fp64 (the bias: s = bo[j]; s += Wo[j][m] bv[m]) */
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

/* ---- actor: hhp_set_net's four forms.  Sections (flat thread index, cumulative ends): inp1..inp3 as [wd][nc + 1] (column nc = the
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

/* ---- value branch: hhp_set_critic's planes + biases and its hh_k_policy_w16_ppo stream (with the branch's own copy of the shared layer).
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

/* ---- commander: hhc_set_weights' planes and fp32 section.  Sections: the eight first-layer blocks (actor inp1..inp4, critic v1..v4) as
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
    hipStream_t st = (hipStream_t)stream;
    {
        HhrActorArgs a;
        memset(&a, 0, sizeof(a));
        a.w = *w;
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
        a.end[5] = e += att ? 100 * 101 : 0;
        hipLaunchKernelGGL(hh_k_refresh_actor, dim3((e + HHR_THREADS - 1) / HHR_THREADS), dim3(HHR_THREADS), 0, st, a);
    }
    if (cw) {
        const HhpCrit &Cn = p->cbank.c[slot];
        const HhpCritX &Cx = p->cbankx.c[slot];
        HhrCriticArgs a;
        memset(&a, 0, sizeof(a));
        a.w = *cw;
        a.h_w1 = hhr_h16(Cn.w1h); a.l_w1 = hhr_h16(Cn.w1l); a.h_wov = hhr_h16(Cn.wovh); a.l_wov = hhr_h16(Cn.wovl);
        a.h_ws = hhr_h16(Cn.wsh); a.l_ws = hhr_h16(Cn.wsl); a.h_wa = hhr_h16(Cn.wah); a.l_wa = hhr_h16(Cn.wal);
        a.b1 = const_cast<float *>(Cn.b1); a.bs = const_cast<float *>(Cn.bs); a.bov = const_cast<float *>(Cn.bov); a.ba = const_cast<float *>(Cn.ba);
        a.xb1 = const_cast<float *>(Cx.b1); a.xbs = const_cast<float *>(Cx.bs); a.xbov = const_cast<float *>(Cx.bov); a.xba = const_cast<float *>(Cx.ba);
        a.X = reinterpret_cast<uint16_t *>(p->cxblob[slot]);
        a.att = att ? 1 : 0;
        const int d1 = HHC_DIMS[N.kind][0], a1 = HHC_DIMS[N.kind][1], n_in = d1 + a1 + HHC_DIMS[N.kind][2] + HHC_DIMS[N.kind][3];
        int e = 0;
        if (att) { /* v1 [own obs | own act], v2 [other obs | other act], v3 [all]: columns 0, 175, 350 of cat(v1, v2, y3) */
            const int in0[3] = {0, d1 + a1, 0}, in1[3] = {d1 + a1, n_in, n_in}, wd[3] = {175, 175, 150}, out0[3] = {0, 175, 350};
            for (int b = 0; b < 3; b++) {
                a.in0[b] = in0[b]; a.nin[b] = in1[b] - in0[b]; a.out0[b] = out0[b];
                a.end[b] = e += wd[b] * (a.nin[b] + 1);
            }
        } else { /* inp1_val [all] -> 500 */
            a.nin[0] = n_in;
            a.end[0] = e += 500 * (n_in + 1);
            a.end[1] = a.end[2] = e;
        }
        a.end[3] = e += 500 * 501;
        a.end[4] = e += 501;
        a.end[5] = e += att ? 150 * 151 : 0;
        hipLaunchKernelGGL(hh_k_refresh_critic, dim3((e + HHR_THREADS - 1) / HHR_THREADS), dim3(HHR_THREADS), 0, st, a);
    }
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

extern "C" int hh_commander_refresh_weights(hh_commander *c, const hh_commander_weights *w, void *stream) {
    if (!c || !w) { g_err = "hh_commander_refresh_weights: bad argument"; return HH_E_ARG; }
    if (!c->loaded || !c->blob) { g_err = "hh_commander_refresh_weights: no weights loaded (hh_commander_set_weights allocates the buffers once)"; return HH_E_ARG; }
    const float *need[] = {w->act_w_ih, w->act_w_hh, w->act_b_ih, w->act_b_hh, w->shared_w, w->shared_b, w->act_out_w, w->act_out_b,
                           w->val_w_ih, w->val_w_hh, w->val_b_ih, w->val_b_hh, w->val_out_w, w->val_out_b};
    for (const float *q : need) if (!q) { g_err = "hh_commander_refresh_weights: missing weight pointer"; return HH_E_ARG; }
    for (int k = 0; k < 4; k++) if (!w->inp_w[k] || !w->inp_b[k] || !w->v_w[k] || !w->v_b[k]) { g_err = "hh_commander_refresh_weights: missing input layer"; return HH_E_ARG; }
    HhrCommanderArgs a;
    memset(&a, 0, sizeof(a));
    a.w = *w;
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
    HH_GUARD(c);
    hipLaunchKernelGGL(hh_k_refresh_commander, dim3((e + HHR_THREADS - 1) / HHR_THREADS), dim3(HHR_THREADS), 0, (hipStream_t)stream, a);
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
