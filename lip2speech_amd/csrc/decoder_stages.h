// The launch descriptors of the two decoder stages around the decode loop: the prologue (decoder.py:382-410) and the post-net (decoder.py:143-156).
// Host code only, no kernels.  Inference (l2s_api.hip prologue_run, postnet_layer) and the training forward (train_decoder.hip prologue_train_fwd,
// postnet_train_fwd) build every GEMM of these stages here and overlay only what is their own: inference the launcher (split-K, tap-split, plain), the
// masked and persistent branches and the post-net's time window; training the Zout tape stores, the dropout masks and the batch-statistics path.
#pragma once
#include "l2s_common.h"
#include "l2s_model.h"
#include "post_wino.h"

namespace l2s {

// ---------------------------------------------------------------- Conv1d / linear descriptors
// Conv1d over channel-last sequences (B, Tin, Cin at row stride lda) with the layer's folded scale / shift; planes: carry the weight's bf16 planes
inline GemmP conv_gemm(const float* X, int lda, int B, int Tin, int Cin, const ConvW& c, int Cout, int taps, int stride, int pad, float* out, int ldc,
                       int act, bool planes = true) {
    const int Tout = (Tin + 2 * pad - taps) / stride + 1;
    GemmP p = gemm_plain(X, lda, c.W, out, ldc, B * Tout, Cout, taps * Cin);
    p.Tout = Tout; p.Tin = Tin; p.taps = taps; p.stride = stride; p.pad = pad; p.Cin = Cin;
    p.scale = c.scale; p.shift = c.shift; p.actw = c.actw; p.act = act;
    if (planes) p.W3 = c.W3;
    return p;
}
// Linear with bias (shift) and activation
inline GemmP lin_gemm(const float* A, int lda, const ConvW& c, float* out, int ldc, int M, int N, int K, int act) {
    GemmP p = gemm_plain(A, lda, c.W, out, ldc, M, N, K);
    p.shift = c.shift; p.actw = c.actw; p.act = act;
    return p;
}
// pointwise conv of the trunk: columns [a_off, a_off + K) of A into columns c_off + n * cstride of C (the channel shuffle)
inline GemmP pw_gemm(const float* A, int lda, int a_off, const ConvW& c, float* C, int ldc, int c_off, int cstride, int64_t M, int N, int K, int act,
                     bool planes = true) {
    GemmP p = gemm_plain(A + a_off, lda, c.W, C + c_off, ldc, (int)M, N, K);
    p.scale = c.scale; p.shift = c.shift; p.actw = c.actw; p.act = act; p.c_cstride = cstride;
    if (planes) p.W3 = c.W3;
    return p;
}
inline GemmBatch gemm_pair(const GemmP& a, const GemmP& b) {
    GemmBatch gb{};
    gb.p[0] = a; gb.p[1] = b; gb.count = 2;
    return gb;
}

// ---------------------------------------------------------------- the prologue's activations
// resid (BT, 512); s_e, s_a (B, 512); gin (BT, 4096) BiLSTM input gates; rnn (BT, 1024); cellcat (B, 1024); cat (BT, PRO_CAT) [x | K branches | V branches];
// cmap[j] (B * L[j], 512); pooled (R, 2560), R = B * m; wv, tA, tB, tC (R, 256); logits (R, VOC); zsoft (R, VOCP); frag16: hf[d] ping-pong, cf[d]
constexpr int PRO_CAT = 4608;      // columns of cat: x, four K branches, four V branches, 512 each
struct ProBufs {
    float *resid, *s_e, *s_a, *gin, *rnn, *cellcat, *cat, *cmap[4], *pooled, *wv, *tA, *tB, *tC, *logits, *zsoft;
    float *hf[2][2], *cf[2];
    int L[4], m;
};
inline void pro_carve_lstm(Bump& bp, int B, ProBufs& b) {
    const int64_t Bp = pad16(B);
    for (int d = 0; d < 2; ++d) { b.hf[d][0] = bp.f(Bp * 512); b.hf[d][1] = bp.f(Bp * 512); b.cf[d] = bp.f(Bp * 512); }
}

// One prologue call: a builder per launch.  planes: the descriptors carry their weights' bf16 planes (inference under "gemm_x3_dma"; training never)
struct Prologue {
    const Weights& w; const ProBufs& b; float* state; StateLayout sl; int B, T; bool planes;
    int BT() const { return B * T; }
    int R() const { return B * b.m; }

    GemmP resid(const float* vis) const { return lin_gemm(vis, 1024, w.resid, b.resid, 512, BT(), 512, 1024, ACT_NONE); }
    GemmBatch sites(const float* emb) const {
        return gemm_pair(lin_gemm(emb, 256, w.enc_site, b.s_e, 512, B, 512, 256, ACT_PSINE), lin_gemm(emb, 256, w.attn_site, b.s_a, 512, B, 512, 256, ACT_PSINE));
    }
    GemmP bilstm_in(const float* vis) const {      // input gates of both directions: (BT, 1024) x (1024, 4096)
        GemmP p = gemm_plain(vis, 1024, w.wih_cat, b.gin, 4096, BT(), 4096, 1024);
        p.shift = w.bih_cat;
        if (planes) p.W3 = w.wih_cat3;
        return p;
    }
    GemmP e_c() const { return lin_gemm(b.cellcat, 1024, w.e_c, state + sl.ecell, 512, B, 512, 1024, ACT_NONE); }
    GemmP enc_proj() const {      // encoder_proj(rnn) + residual + s_a (broadcast over the T frames of a clip) -> cat[:, 0:512]
        GemmP p = lin_gemm(b.rnn, 1024, w.enc_proj, b.cat, PRO_CAT, BT(), 512, 1024, ACT_NONE);
        p.R1 = b.resid; p.ldr1 = 512;
        p.R2 = b.s_a; p.ldr2 = 512; p.r2_div = T;
        return p;
    }
    GemmP mh_branch(int kv, int j) const {      // MultiHop branch j of K (kv = 0) or V: cat[:, 0:512] -> its 512 columns of cat
        return conv_gemm(b.cat, PRO_CAT, B, T, 512, w.mh_branch[kv][j], 512, MH_KS[j], 1, MH_KS[j] / 2, b.cat + 512 + (kv * 4 + j) * 512, PRO_CAT, ACT_SILU, planes);
    }
    GemmBatch mh_bott() const {      // the K and V bottlenecks (+PSine +pos[t]); V reads [x | V branches]
        GemmBatch bb{};
        for (int kv = 0; kv < 2; ++kv) {
            GemmP& p = bb.p[kv];
            p = lin_gemm(b.cat, PRO_CAT, w.mh_bott[kv], state + (kv == 0 ? sl.k : sl.v), 512, BT(), 512, 2560, ACT_PSINE);
            if (kv == 1) { p.a_split = 512; p.a_gap = 2048; }
            p.R1 = w.pos; p.ldr1 = 512; p.r1_mod = T;
        }
        bb.count = 2;
        return bb;
    }
    GemmP vproj() const { return lin_gemm(state + sl.v, 512, w.vproj, state + sl.vp, 256, BT(), 256, 512, ACT_NONE); }      // V' = V W_ap^T + b_ap
    GemmBatch ct_branches() const {      // Content.agg: K = 512 * ks, stride ks; the rows shrink with ks
        GemmBatch gb{};
        for (int j = 0; j < 4; ++j) gb.p[j] = conv_gemm(b.cat, PRO_CAT, B, T, 512, w.ct_branch[j], 512, CT_KS[j], CT_KS[j], 0, b.cmap[j], 512, ACT_SILU, planes);
        gb.count = 4;
        return gb;
    }
    PoolCatP pool_cat() const {      // x and the four maps, each pooled to m slots, side by side
        PoolCatP pc{};
        pc.x[0] = b.cat; pc.L[0] = T; pc.ld[0] = PRO_CAT;
        for (int j = 0; j < 4; ++j) { pc.x[j + 1] = b.cmap[j]; pc.L[j + 1] = b.L[j]; pc.ld[j + 1] = 512; }
        pc.nmaps = 5; pc.B = B; pc.m = b.m; pc.C = 512; pc.out = b.pooled;
        return pc;
    }
    PoolDiv pool_div() const {      // frames per slot of each map (the masked pool)
        PoolDiv pd{};
        pd.div[0] = 1;
        for (int j = 0; j < 4; ++j) pd.div[j + 1] = CT_KS[j];
        return pd;
    }
    GemmP ct_bott() const { return lin_gemm(b.pooled, 2560, w.ct_bott, b.wv, 256, R(), 256, 2560, ACT_NONE); }
    GemmP ct_lin(const float* in, const ConvW& c, float* out) const { return lin_gemm(in, 256, c, out, 256, R(), 256, 256, ACT_SILU); }
    GemmBatch ct_pair0() const { return gemm_pair(ct_lin(b.wv, w.ct_k0, b.tA), ct_lin(b.wv, w.ct_fc0, b.tB)); }                       // k0 | fc0
    GemmBatch ct_pair2() const { return gemm_pair(ct_lin(b.tA, w.ct_k2, state + sl.ckey), ct_lin(b.tB, w.ct_fc2, b.tC)); }            // k2 | fc2
    GemmP ct_fc4() const { return lin_gemm(b.tC, 256, w.ct_fc4, b.logits, VOC, R(), VOC, 256, ACT_SILU); }
    GemmP ct_emb() const { return gemm_plain(b.zsoft, VOCP, w.ct_emb.W, state + sl.cval, 256, R(), 256, VOCP); }
    // P = value W_ih[:, content]^T (decoder.py:262-271 feeds alpha @ value straight into the LSTM: no bias, no nonlinearity in between), stored as
    // P[b][packed gate row][j], j fastest at pitch cp_pitch = ceil4(m): a clip's m value rows are read as a one-tap sequence of cp_pitch output rows (the rows
    // past m read as padding: zeros, like the rows of a masked clip's unused slots, whose values are zero) and stored channel-first per clip.  K = 256: always
    // the f32 tile kernel, whose rows do not depend on each other - a clip's table is the same bits alone, padded or in a group
    GemmP cproj() const {
        GemmP p = lin_gemm(state + sl.cval, 256, w.cproj, state + sl.cp, 2048, B * sl.cp_pitch, 2048, 256, ACT_NONE);
        p.Tout = sl.cp_pitch; p.Tin = b.m; p.c_tr_T = sl.cp_pitch;
        return p;
    }
};

// the BiLSTM starts from h0 = c0 = s_e in both directions (decoder.py:386-389); the other half of the h ping-pong starts at zero
inline int bilstm_start(const ProBufs& b, int B, hipStream_t s) {
    for (int d = 0; d < 2; ++d) {
        if (launch_to_frag(b.s_e, 512, B, 512, b.hf[d][0], 512, 0, 0, s)) return 1;
        if (launch_to_frag(b.s_e, 512, B, 512, b.cf[d], 512, 0, 0, s)) return 1;
        if (launch_fill(b.hf[d][1], (int64_t)pad16(B) * 512, 0.f, s)) return 1;
    }
    return 0;
}
// the decoder's initial hidden state = the BiLSTM finals (fwd -> layer 0, bwd -> layer 1), kept in the state as frag16; cellcat = cat(c_fwd, c_bwd).
// fwd = false: the forward direction's parts are skipped (a masked call has captured them row by row)
inline int bilstm_finals(const ProBufs& b, float* state, const StateLayout& sl, int B, int T, bool fwd, hipStream_t s) {
    const int fin = T & 1;      // the buffer holding the final hidden states
    const int64_t n = (int64_t)pad16(B) * 512;
    if (fwd) L2S_CHECK_HIP(hipMemcpyAsync(state + sl.h, b.hf[0][fin], sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    L2S_CHECK_HIP(hipMemcpyAsync(state + sl.h + n, b.hf[1][fin], sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    if (fwd && launch_from_frag(b.cf[0], 512, B, 512, b.cellcat, 1024, 0, s)) return 1;
    return launch_from_frag(b.cf[1], 512, B, 512, b.cellcat, 1024, 512, s);
}

// ---------------------------------------------------------------- the post-net
// layer 0..4 over the whole of every sequence: 5 taps, pad 2; layers 1-3 add their input, layer 4 adds mel and stores channel-first (B, 80, S)
inline GemmP post_layer(const Weights& w, int layer, const float* in, float* out, const float* mel, int B, int S, bool planes = false) {
    const int cin = layer == 0 ? NM : 512, cout = layer == 4 ? NM : 512;
    GemmP p = conv_gemm(in, cin, B, S, cin, w.post[layer], cout, 5, 1, 2, out, cout, layer == 4 ? ACT_NONE : ACT_PSINE, planes);
    if (layer >= 1 && layer <= 3) { p.R1 = in; p.ldr1 = 512; }
    if (layer == 4) { p.R1 = mel; p.ldr1 = NM; p.c_tr_T = S; }
    return p;
}
// layers 1-3 in their Winograd F(4,5) form (post_wino.h): the eight point-wise products M_p = V_p U_p^T, rows = tile rows (clips x ceil(S / 4)), N = K = 512,
// plain store.  Always the split-bf16 family (x3 bit 8); planes: the U_p's bf16 planes travel too
inline GemmBatch post_wino_products(const Weights& w, int layer, const float* V, float* M, int rows, bool planes) {
    GemmBatch gb{};
    for (int p = 0; p < WINO_P; ++p) {
        GemmP& g = gb.p[p];
        g = gemm_plain(V + (int64_t)p * rows * 512, 512, wino_u(w.post_wino[layer], 512, p), M + (int64_t)p * rows * 512, 512, rows, 512, 512);
        g.x3 |= 8;
        if (planes) g.W3 = wino_u3(w.post_wino[layer], 512, p);
    }
    gb.count = WINO_P;
    return gb;
}

}  // namespace l2s
