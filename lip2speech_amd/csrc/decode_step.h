// The launch descriptors of the three recurrences that go through launch_skinny: the decoder step (phases A - F, decoder.py:353-375), one
// direction of the prologue's BiLSTM step and the voice tower's LSTM step.  Host code only, no kernels.  Every caller - the inference loop
// (l2s_api.hip decode_launches: free-running, teacher-forced, masked, captured), the training forward (train_decoder.hip decode_train_fwd), the
// two chain microbenches and the site hook of include/l2s_diag.h - builds its launches here and overlays only what is its own: inference the
// early-stop control fields, training the tape stores, the dropout masks and the dropped h0 operand of layer 1.  tests/golden/skinny_forms.json
// "sites" holds these groups as integers; tests/test_step_sites_gpu.py compares the two.
#pragma once
#include "l2s_common.h"
#include "l2s_model.h"

namespace l2s {

// ---------------------------------------------------------------- the step's buffers
// frag16 (rows padded to 16): h0/h1 ping-pong, c0, c1, av (a @ v, or o = a @ V'), p1, cc (content), uu (u of the literal step), p2f, yf (the frame
// fed back, K = 96); plain [B][.]: q, qc, p2 (prenet of the literal step), al (content soft-max weights, CONTENT_HOIST_MAX_M per row: the K = 768 form only)
struct StepBufs {
    float *h0[2], *h1[2], *c0, *c1, *av, *p1, *cc, *uu, *p2f, *yf, *q, *qc, *p2, *al;
};
constexpr int64_t step_alpha_floats(int B) { return (int64_t)B * CONTENT_HOIST_MAX_M; }
inline StepBufs step_carve(Bump& bp, int B, bool alpha = false) {      // h0[0] first: training zero-fills the whole run from there; alpha: inference carves al, last
    const int64_t Bp = pad16(B);
    StepBufs d;
    for (int i = 0; i < 2; ++i) d.h0[i] = bp.f(Bp * 512);
    for (int i = 0; i < 2; ++i) d.h1[i] = bp.f(Bp * 512);
    d.c0 = bp.f(Bp * 512); d.c1 = bp.f(Bp * 512); d.av = bp.f(Bp * 512);
    d.p1 = bp.f(Bp * 256); d.cc = bp.f(Bp * 256); d.uu = bp.f(Bp * 256); d.p2f = bp.f(Bp * 256);
    d.yf = bp.f(Bp * 96);
    d.q = bp.f((int64_t)B * 512); d.qc = bp.f((int64_t)B * 256); d.p2 = bp.f((int64_t)B * 256);
    d.al = alpha ? bp.f(step_alpha_floats(B)) : nullptr;
    return d;
}

// ---------------------------------------------------------------- the step's form
enum Lstm0Operand {
    L0_LITERAL,      // w.lstm0 on [content | u | h0], K = 1024: the literal 6-phase step
    L0_K1536,        // w.lstm0f on [content | prenet | a @ v | h0]: attention_proj pre-multiplied into W_ih
    L0_K1280,        // w.lstm0v on [content | prenet | o | h0], o = a @ V' (V' from the prologue)
    L0_K1024_SUM,    // w.lstm0 on [content | prenet + o | h0]: the sum formed by the operand loader (SkinnyP::a_sum)
    L0_K768,         // w.lstm0c on [prenet + o | h0]: the content columns hoisted too - the attention launch stores alpha instead of content = alpha @ value,
                     //   the cell threads add sum_j alpha_j P_j with P = value W_ih[:, content]^T from the prologue (the state's cp table)
};
struct StepForm {
    bool fold;               // phase-merged 4-launch step (option "fold_step_weights") or the literal 6 phases
    Lstm0Operand lstm0;
    bool planes;             // the groups carry their weights' bf16 planes (SkW::W3): inference does, training stays on the f32 forms
    bool vproj() const { return lstm0 == L0_K1280 || lstm0 == L0_K1024_SUM || lstm0 == L0_K768; }      // the attention launch writes o = a @ V' (K = 256) into av
    bool choist() const { return lstm0 == L0_K768; }
};
// inference and the chain microbenches: option "hoist_vproj" picks LSTM0's operand layout of the folded step; m = content slots of the call's clips (T / 7)
inline StepForm step_form(const Weights& w, const Options& o, bool fold, int m) {
    const bool vhoist = fold && o.hoist_vproj && w.lstm0v.W && w.vproj.W;
    const bool vsum = vhoist && o.hoist_vproj >= 2 && skinny_sum_supported(o);
    // 3: the step is folded, the summed-segment form exists, the K = 768 planes exist, and the clip's table is worth reading (CONTENT_HOIST_MAX_M, l2s_common.h)
    const bool chst = vsum && o.hoist_vproj >= 3 && w.lstm0c.W && w.lstm0c.W3 && w.cproj.W && m >= 1 && m <= CONTENT_HOIST_MAX_M;
    return {fold, !fold ? L0_LITERAL : chst ? L0_K768 : vsum ? L0_K1024_SUM : vhoist ? L0_K1280 : L0_K1536, true};
}
// training: folded onto lstm0f (its backward pass knows that layout), or literal; no planes
inline StepForm step_form_train(bool fold) { return {fold, fold ? L0_K1536 : L0_LITERAL, false}; }

// ---------------------------------------------------------------- groups
inline SkinnyP sk_base(const SkW& sw, int B, bool planes = true) {
    SkinnyP p{};
    p.W = sw.W; p.W3 = planes ? sw.W3 : nullptr; p.bias = sw.bias; p.actw = sw.actw;
    p.B = B; p.N = sw.N; p.K = sw.K;
    p.act = ACT_NONE; p.epi = SK_PLAIN;
    return p;
}
inline SkinnyBatch sk_batch1(const SkinnyP& p, int ntiles) {
    SkinnyBatch sb{};
    sb.p[0] = p; sb.ntiles[0] = ntiles; sb.count = 1;
    return sb;
}
inline void sk_lstm_epi(SkinnyP& p, int H, float* c, float* h_out) {
    p.epi = SK_LSTM; p.H = H; p.c_in = c; p.c_out = c; p.h_out = h_out; p.h_out_K = H; p.h_out_off = 0;
}

// where a step's mel frame and stop logit go: mel (B, S, 80), stop (B, S), the per-clip constant of the stop logit
struct StepOut { float* mel; float* stop; const float* stop_const; int S; };

// the prenet reads an explicit frame (BOS, a teacher frame, the y of the literal step) - else, folded, h1 through prenet1 o fc_out
inline bool step_from_frame(const StepForm& f, int i, bool forced) { return !f.fold || i == 0 || forced; }
// the folded step finishes in the next step's first launch; only the literal step, and the last folded one, launch phase F
inline bool step_has_phase_f(const StepForm& f, int i, int S) { return !f.fold || i == S - 1; }

// fc_out + stop of step `step` on h1buf (SK_MEL); yfrag: where the frame is fed back from (literal step), or null
inline SkinnyP step_fc(const StepForm& f, const Weights& w, int B, const float* h1buf, float* yfrag, const StepOut& o, int step) {
    SkinnyP a = sk_base(w.fc, B, f.planes);
    a.seg[0] = {h1buf, 32}; a.nseg = 1; a.epi = SK_MEL;
    a.mel = o.mel + (int64_t)step * NM_; a.ld_mel_b = (int64_t)o.S * NM_;
    a.stop = o.stop + step; a.ld_stop_b = o.S; a.stop_const = o.stop_const; a.yfrag = yfrag;
    return a;
}

// phase A of step i: [0] prenet layer 1, [1] Q (+PSine +pos[i]), [2] content Q (+SiLU); folded and i > 0: [3] mel frame + stop logit of step i - 1
inline SkinnyBatch step_phase_a(const StepForm& f, const Weights& w, const StepBufs& d, int B, int i, bool from_frame, const StepOut& o) {
    const int cur = i & 1;
    SkinnyBatch sb{};
    SkinnyP& a = sb.p[0];
    a = sk_base(from_frame ? w.pre1 : w.pre1f, B, f.planes);
    if (from_frame) a.seg[0] = {d.yf, 5}; else a.seg[0] = {d.h1[cur], 32};
    a.nseg = 1; a.act = ACT_PSINE; a.epi = SK_FRAG; a.out = d.p1; a.ldo = 256;
    sb.ntiles[0] = 16;
    SkinnyP& b = sb.p[1];
    b = sk_base(w.q, B, f.planes);
    b.seg[0] = {d.h0[cur], 32}; b.seg[1] = {d.h1[cur], 32}; b.nseg = 2; b.act = ACT_PSINE; b.epi = SK_PLAIN; b.out = d.q; b.ldo = 512;
    b.addrow = w.pos + (int64_t)i * 512;
    sb.ntiles[1] = w.q.tiles;
    SkinnyP& c = sb.p[2];
    c = sk_base(w.cq, B, f.planes);
    c.seg[0] = {d.c0, 32}; c.seg[1] = {d.c1, 32}; c.nseg = 2; c.act = ACT_SILU; c.epi = SK_PLAIN; c.out = d.qc; c.ldo = 256;
    sb.ntiles[2] = w.cq.tiles;
    sb.count = 3;
    if (f.fold && i > 0) { sb.p[3] = step_fc(f, w, B, d.h1[cur], nullptr, o, i - 1); sb.ntiles[3] = w.fc.tiles; sb.count = 4; }
    return sb;
}

// phase B of step i: attention + content attention per batch row, and prenet layer 2 in the same grid.  attn: (B, S, T) or null
struct StepAttn { AttnP at; SkinnyP pre2; int pre2_tiles; };
inline StepAttn step_phase_b(const StepForm& f, const Weights& w, const StepBufs& d, float* state, const StateLayout& sl, int B, int T, int i, int S,
                             float* attn, int attn_logits) {
    StepAttn r{};
    AttnP& at = r.at;
    at.q = d.q; at.ldq = 512; at.k = state + sl.k; at.v = state + sl.v; at.tau = w.tau; at.av_frag = d.av;
    if (f.vproj()) at.vp = state + sl.vp;      // d.av then holds o = a @ V' (frag16, K = 256)
    at.attn_out = attn ? attn + (int64_t)i * T : nullptr; at.ld_attn_b = (int64_t)S * T; at.attn_logits = attn_logits;
    at.qc = d.qc; at.ldqc = 256; at.ckey = state + sl.ckey; at.cval = state + sl.cval; at.tau_c = w.tau_c; at.cc_frag = d.cc;
    if (f.choist()) at.alpha_out = d.al;       // the content blocks store alpha; d.cc is not written (nor read)
    at.B = B; at.T = T; at.m = sl.m;
    SkinnyP& pr = r.pre2;
    pr = sk_base(w.pre2, B, f.planes);
    pr.seg[0] = {d.p1, 16}; pr.nseg = 1; pr.act = ACT_PSINE; pr.ldo = 256;
    if (f.fold) { pr.epi = SK_FRAG; pr.out = d.p2f; }
    else { pr.epi = SK_PLAIN; pr.out = d.p2; }
    r.pre2_tiles = w.pre2.tiles;
    return r;
}

// phase C (literal step only): u = prenet + attention_proj(a @ v)
inline SkinnyBatch step_phase_c(const StepForm& f, const Weights& w, const StepBufs& d, int B) {
    SkinnyP a = sk_base(w.aproj, B, f.planes);
    a.seg[0] = {d.av, 32}; a.nseg = 1; a.epi = SK_FRAG; a.out = d.uu; a.ldo = 256; a.add = d.p2; a.ld_add = 256;
    return sk_batch1(a, w.aproj.tiles);
}

// phase D of step i: LSTM layer 0, h0[cur] -> h0[nxt], on the operand layout of the form.  cp / cp_pitch: the call's P table (StateLayout::cp; L0_K768 only)
inline SkinnyBatch step_phase_d(const StepForm& f, const Weights& w, const StepBufs& d, int B, int i, const float* cp = nullptr, int cp_pitch = 0) {
    const int cur = i & 1, nxt = cur ^ 1;
    SkinnyP a = sk_base(f.lstm0 == L0_K1536 ? w.lstm0f : f.lstm0 == L0_K1280 ? w.lstm0v : f.lstm0 == L0_K768 ? w.lstm0c : w.lstm0, B, f.planes);
    a.seg[0] = {d.cc, 16};
    switch (f.lstm0) {
    case L0_K768:      // segment 0 stays, empty: the summed segment is segment 1 in every layout that has one
        a.seg[0] = {d.p2f, 0}; a.seg[1] = {d.p2f, 16}; a.a_sum = d.av; a.seg[2] = {d.h0[cur], 32}; a.nseg = 3;
        a.hoist_p = cp; a.hoist_alpha = d.al; a.hoist_pitch = cp_pitch;
        break;
    case L0_LITERAL:   a.seg[1] = {d.uu, 16}; a.seg[2] = {d.h0[cur], 32}; a.nseg = 3; break;
    case L0_K1024_SUM: a.seg[1] = {d.p2f, 16}; a.a_sum = d.av; a.seg[2] = {d.h0[cur], 32}; a.nseg = 3; break;
    case L0_K1280:     a.seg[1] = {d.p2f, 16}; a.seg[2] = {d.av, 16}; a.seg[3] = {d.h0[cur], 32}; a.nseg = 4; break;
    case L0_K1536:     a.seg[1] = {d.p2f, 16}; a.seg[2] = {d.av, 32}; a.seg[3] = {d.h0[cur], 32}; a.nseg = 4; break;
    }
    sk_lstm_epi(a, 512, d.c0, d.h0[nxt]);
    return sk_batch1(a, 128);
}

// phase E of step i: LSTM layer 1 on the new h0, h1[cur] -> h1[nxt]
inline SkinnyBatch step_phase_e(const StepForm& f, const Weights& w, const StepBufs& d, int B, int i) {
    const int cur = i & 1, nxt = cur ^ 1;
    SkinnyP a = sk_base(w.lstm1, B, f.planes);
    a.seg[0] = {d.h0[nxt], 32}; a.seg[1] = {d.h1[cur], 32}; a.nseg = 2;
    sk_lstm_epi(a, 512, d.c1, d.h1[nxt]);
    return sk_batch1(a, w.lstm1.tiles);
}

// phase F of step i: its mel frame + stop logit on the new h1; the literal step feeds the frame back through yf
inline SkinnyBatch step_phase_f(const StepForm& f, const Weights& w, const StepBufs& d, int B, int i, const StepOut& o) {
    return sk_batch1(step_fc(f, w, B, d.h1[(i & 1) ^ 1], f.fold ? nullptr : d.yf, o, i), w.fc.tiles);
}

// ---------------------------------------------------------------- the two other recurrences
// direction d of the prologue's BiLSTM at frame t of T, as group d of sb: input gates from gin (B*T, 4096), hidden state also to rnn (B*T, 1024)
inline void bilstm_step_group(SkinnyBatch& sb, int d, const Weights& w, bool planes, int B, int T, int t, const float* h_cur, float* h_nxt, float* c,
                              const float* gin, float* rnn) {
    SkinnyP& p = sb.p[d];
    p = sk_base(w.whh[d], B, planes);
    p.seg[0] = {h_cur, 32}; p.nseg = 1;
    sk_lstm_epi(p, 512, c, h_nxt);
    p.pre = gin + (int64_t)t * 4096 + d * 2048; p.ld_pre = (int64_t)T * 4096;
    p.h_seq = rnn + (int64_t)t * 1024 + d * 512; p.ld_hseq = (int64_t)T * 1024;
    sb.ntiles[d] = w.whh[d].tiles;
}

// layer l of the voice tower on `rows` rows: input gates pre (row stride ld_pre), hidden state also to h_seq (row stride ld_hseq)
inline SkinnyBatch spk_lstm_step(const Weights& w, int l, int rows, const float* h_cur, float* h_nxt, float* c, const float* pre, int64_t ld_pre,
                                 float* h_seq, int64_t ld_hseq) {
    SkinnyP p = sk_base(w.spk_hh[l], rows);
    p.seg[0] = {h_cur, 16}; p.nseg = 1;
    sk_lstm_epi(p, 256, c, h_nxt);
    p.pre = pre; p.ld_pre = ld_pre;
    p.h_seq = h_seq; p.ld_hseq = ld_hseq;
    return sk_batch1(p, w.spk_hh[l].tiles);
}

}  // namespace l2s
