// C-ABI of libl2s_hip.so (include/l2s.h): workspace planning and the launch sequences of the visual encoder,
// decoder prologue, decode loop and post-net (the weight blob is built and refreshed in l2s_pack.hip).  Host code
// only orchestrates; all arithmetic is in the kernels of gemm_nt.hip / encoder_kernels.hip / skinny.hip / decoder_kernels.hip.
#include "../../include/l2s.h"
#ifdef L2S_DIAG
#include "../../include/l2s_diag.h"
#endif
#include "host_table.h"
#include "l2s_model.h"
#include "pdecode.h"
#include "decode_step.h"
#include "decoder_stages.h"
#include "post_wino.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#ifdef L2S_DIAG
#include <cxxabi.h>
#include <dlfcn.h>      // l2s_op_skinny_form names a kernel by its symbol
#endif
#include <functional>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

namespace l2s {

// ------------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

// ------------------------------------------------------------------------------------------------ options
static Options g_default_opt;          // process defaults: what l2s_model_create copies into a new model (l2s_set_option)
int set_option_field(Options& o, const char* name, int value) {
    struct Row { const char* name; int Options::*field; };
    // what the product library (include/l2s.h) offers: precision legs, semantics, documented modes
    static const Row product[] = {
        {"persist_decode", &Options::persist}, {"use_graph", &Options::graph}, {"fold_step_weights", &Options::fold}, {"refresh_map", &Options::refresh_map},
        {"infer_bf16", &Options::infer_bf16}, {"train_bf16", &Options::train_bf16}, {"gemm_x3", &Options::gemm_x3}, {"frontend_x3", &Options::frontend_x3},
        {"trunk_x3", &Options::trunk_x3}, {"lstm_x3", &Options::lstm_x3}, {"early_stop", &Options::early_stop},
        {"persist_frames", &Options::persist_frames}, {"persist_masked", &Options::persist_masked}};
    for (auto& t : product)
        if (!std::strcmp(name, t.name)) { o.*(t.field) = value; return 0; }
#ifdef L2S_DIAG
    // block-form A/B switches of the same arithmetic (include/l2s_diag.h): libl2s_diag.so only
    static const Row diag[] = {
        {"overlap_postnet", &Options::overlap_postnet}, {"fuse_trunk", &Options::fuse_trunk}, {"fuse_s2", &Options::fuse_s2},
        {"skinny_static", &Options::skinny_static}, {"skinny_sized", &Options::skinny_sized}, {"skinny_split", &Options::skinny_split},
        {"skinny_split8", &Options::skinny_split8}, {"skinny_rc", &Options::rc_shape}, {"skinny_rc_jb", &Options::rc_jb}, {"skinny_rc_multi", &Options::rc_shape_multi},
        {"skinny_flat", &Options::skinny_flat}, {"hoist_vproj", &Options::hoist_vproj}, {"attn_lds", &Options::attn_lds}, {"flat_half", &Options::flat_half},
        {"half_min_mts", &Options::half_min_mts}, {"gemm_x3_dma", &Options::gemm_x3_dma}, {"trunk_chain", &Options::trunk_chain}, {"frontend_solo", &Options::frontend_solo}, {"flat_xcd", &Options::flat_xcd}, {"attn_skip0", &Options::attn_skip0},
        {"post_wino", &Options::post_wino}};
    for (auto& t : diag)
        if (!std::strcmp(name, t.name)) { o.*(t.field) = value; return 0; }
#endif
    return 1;
}

// ------------------------------------------------------------------------------------------------ profiling
struct ProfEntry { std::string name; int64_t launches = 0; double total_ms = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> pending; };
bool g_prof_on = false;
static std::vector<ProfEntry> g_prof;
static std::map<std::string, int> g_prof_idx;
static thread_local int g_prof_cur = -1;          // a begin/end pair runs on one host thread; several threads may drive launches (InflightPool)
static thread_local hipEvent_t g_prof_start;
static std::mutex g_prof_mu;                      // guards g_prof / g_prof_idx

void prof_begin(const char* name, hipStream_t s) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto it = g_prof_idx.find(name);
    int idx;
    if (it == g_prof_idx.end()) {
        idx = (int)g_prof.size();
        g_prof.push_back(ProfEntry{name});
        g_prof_idx[name] = idx;
    } else {
        idx = it->second;
    }
    g_prof_cur = idx;
    (void)hipEventCreate(&g_prof_start);
    (void)hipEventRecord(g_prof_start, s);
}
void prof_end(hipStream_t s) {
    if (!g_prof_on || g_prof_cur < 0) return;
    hipEvent_t stop;
    (void)hipEventCreate(&stop);
    (void)hipEventRecord(stop, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof[g_prof_cur].pending.emplace_back(g_prof_start, stop);
    g_prof[g_prof_cur].launches++;
    g_prof_cur = -1;
}
void prof_count(const char* name, int64_t n) {      // a counter among the entries (e.g. the pair blocks of the ragged front-end's grid): no events, no time
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto it = g_prof_idx.find(name);
    if (it == g_prof_idx.end()) {
        g_prof_idx[name] = (int)g_prof.size();
        g_prof.push_back(ProfEntry{name});
        it = g_prof_idx.find(name);
    }
    g_prof[it->second].launches += n;
}
static void prof_drain() {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& e : g_prof) {
        for (auto& pr : e.pending) {
            (void)hipEventSynchronize(pr.second);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) e.total_ms += ms;
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
        e.pending.clear();
    }
}

}  // namespace l2s

namespace l2s {

// ------------------------------------------------------------------------------------------------ workspace
struct EncPlan {
    int NF, Hp;
    int64_t act_a, act_b, t1, t2, last;
};
static EncPlan enc_plan(int NF, int H) {      // NF frames: B * T of a padded call, sum len of a ragged one
    EncPlan p{};
    p.NF = NF;
    p.Hp = H / 4;
    int64_t hw = (int64_t)p.Hp * p.Hp;
    int64_t amax = (int64_t)p.NF * hw * STAGE_CH[0], t1 = 0, t2 = 0;
    int cin = STAGE_CH[0];
    int h = p.Hp;
    for (int st = 0; st < 3; ++st) {
        int cout = STAGE_CH[st + 1], half = cout / 2;
        int ho = (h + 1) / 2;
        int64_t in_px = (int64_t)p.NF * h * h, out_px = (int64_t)p.NF * ho * ho;
        t1 = std::max(t1, std::max(in_px * half, out_px * half));     // pw1 output (stride-2: input resolution)
        t2 = std::max(t2, std::max(out_px * cin, out_px * half));     // dw outputs
        amax = std::max(amax, out_px * cout);
        cin = cout;
        h = ho;
    }
    p.act_a = amax; p.act_b = amax; p.t1 = t1; p.t2 = t2;
    p.last = (int64_t)p.NF * h * h * LAST_CH;
    return p;
}
static int64_t enc_ws_floats(int NF, int H) {
    EncPlan p = enc_plan(NF, H);
    return p.act_a + p.act_b + p.t1 + p.t2 + p.last + 64 * 8;
}

static int64_t prologue_ws_floats(int B, int T) {
    int L[4];
    int m = content_lens(T, L);
    int64_t BT = (int64_t)B * T, n = 0;
    n += BT * 4096;            // BiLSTM input gates
    n += BT * 1024;            // rnn_out
    n += BT * 512;             // residual
    n += (int64_t)B * 512 * 2; // s_e, s_a
    n += (int64_t)pad16(B) * 512 * 6;   // h,c frags for both directions (ping-pong h)
    n += (int64_t)B * 1024;    // cell cat
    n += BT * 4608;            // cat buffer [x | K branches | V branches]
    for (int j = 0; j < 4; ++j) n += (int64_t)B * L[j] * 512;
    n += (int64_t)B * m * 2560;
    n += (int64_t)B * m * 256 * 4;
    n += (int64_t)B * m * (VOC + VOCP);
    n += 8 * std::max((int64_t)B * m * 256, (int64_t)B * 512);   // split-K partial products
    for (int j = 1; j < 4; ++j) n += (int64_t)CT_KS[j] * B * L[j] * 512;   // per-tap partial products of Content.agg
    n += 8 * BT * 512;                                                      // split-K partial products of the two MultiHop bottlenecks
    if (B <= 2) n += pbilstm_ws_bytes() / 4 + 64;                           // exchange granules of the persistent BiLSTM
    return n + 64 * 44;
}
static int64_t decode_ws_floats(int B) {
    int64_t Bp = pad16(B);
    return Bp * (512 * 4 + 512 * 2 + 512 + 256 * 4 + 96) + (int64_t)B * (512 + 256 + 256) + step_alpha_floats(B) + 64 * 25 + (B + 2 + 64) /* EsCtl */ + (B <= 8 ? pdecode_ws_bytes(B) / 4 + 64 : 0);
}
constexpr int POST_TAPSPLIT_ROWS = 640;      // a batch with at most this many post-net rows (one or two clips of 300 frames) runs its Conv1d layers one K slice per tap
constexpr int POST_WINO_ROWS = 4096;         // a batch with at least this many post-net rows runs layers 1-3 in their Winograd F(4,5) form (option "post_wino")
// the Winograd route's V and M: eight point planes of B * ceil(S / 4) tile rows each - 2x a layer buffer apiece, rounded up to whole tiles
static int64_t post_wino_floats(int B, int S) { return (int64_t)WINO_P * B * wino_tiles(S) * 512; }
// does postnet_run take the Winograd route for these rows?  Decided on the rows of ONE batch, as the tap split is, so that a batch meets the same arithmetic alone
// and in a group (a model with "overlap_postnet" keeps the direct layer: postnet_run is where its windowed route lands under profiling, graphs or a teacher)
static bool post_wino_route(const l2s_model* m, int B, int S) {
    return !m->opt.infer_bf16 && m->opt.gemm_x3 && !m->opt.overlap_postnet && m->w.post_wino[1] &&
           (m->opt.post_wino >= 2 || (m->opt.post_wino == 1 && (int64_t)B * S / gemm_x3_group() >= POST_WINO_ROWS));
}
// Option "early_stop": how far past a clip's stop crossing the loop must decode so that the kept frames of the post-net have the bits of the full call.  A
// direct layer's frame j reads j - 2 .. j + 2 (ES_MARGIN = 5 x 2); a Winograd layer's tile mixes its eight input frames in every point plane, so in bits
// frame j depends on up to five frames either side: 2 + 3 x 5 + 2 when the call's post-net takes that route.  Thread-local, set by l2s_inference's body
constexpr int ES_MARGIN_WINO = 2 * (ES_POST_TAPS / 2) + 3 * (WINO_P - WINO_M + 1);
static int& es_margin() { static thread_local int margin = ES_MARGIN; return margin; }
struct EsMarginScope { int prev; explicit EsMarginScope(int v) : prev(es_margin()) { es_margin() = v; } ~EsMarginScope() { es_margin() = prev; } };
static int64_t postnet_ws_floats(int B, int S) {
    return (int64_t)B * S * 512 * ((int64_t)B * S <= POST_TAPSPLIT_ROWS * MAX_GROUP ? 9 : 4) + 2 * post_wino_floats(B, S) + 64 * 9;
}

// ------------------------------------------------------------------------------------------------ encoder

static FrameSrc frame_src(const float* video, int B) { FrameSrc f{}; f.p[0] = video; f.per = B; return f; }

// rg (a ragged group, l2s_inference_ragged): the front-end and the trunk run on the rg->NF real frames of the group's clips, compact; vis comes out as
// (rg->N, rg->Tmax, 1024) with zero rows past each clip's length.  B, T are then rg->N, rg->Tmax.
// whether a run of `run` stride-1 units starting with U at map size h goes out as ONE stage-chain launch (a fused trunk: "fuse_trunk").  One statement of
// the rule for encoder_run's loop and for the tap check that runs before the first launch; a macro, so that the loop compiles to the code it was
#define S1_RUN_CHAINED(m, U, run, h) \
    ((m)->opt.trunk_chain && ((h) >= 6 || (m)->opt.trunk_chain >= 2) && (m)->opt.trunk_x3 && (U).pw1_p3 && (U).pw2_p3 && (run) >= 2 && (run) <= S1_CHAIN_MAX)
#ifdef L2S_DIAG      // stage taps (l2s_op_encoder_taps): a host-side copy of the buffer a launch has just written, device to device on the call's stream
static int enc_tap(float* const* taps, int i, const float* src, int64_t n, hipStream_t s) {
    if (taps && taps[i]) L2S_CHECK_HIP(hipMemcpyAsync(taps[i], src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
static int enc_tap_interior(int u) {
    set_error("l2s: encoder tap of unit " + std::to_string(u) + " asked for, but the unit is interior to a stage-chain launch and its output never reaches memory (option \"trunk_chain\")");
    return 1;
}
// before the first launch: walks the units as encoder_run's loop does and refuses a tap of a unit that a stage-chain launch keeps on chip
static int enc_taps_check(const l2s_model* m, float* const* taps, int h) {
    if (!taps || !m->opt.fuse_trunk) return 0;
    for (int u = 0; u < N_UNITS; ++u) {
        const UnitW& U = m->w.unit[u];
        if (U.stride2) { h = (h + 1) / 2; continue; }
        int run = 1;
        while (u + run < N_UNITS && !m->w.unit[u + run].stride2 && m->w.unit[u + run].half == U.half) ++run;
        if (!S1_RUN_CHAINED(m, U, run, h)) continue;
        for (int i = 0; i < run - 1; ++i)
            if (taps[1 + u + i]) return enc_tap_interior(u + i);
        u += run - 1;
    }
    return 0;
}
#define L2S_ENC_TAP(i, src, n) do { if (enc_tap(taps, i, src, n, s)) return 1; } while (0)
#define L2S_ENC_TAPS_ARG , float* const* taps = nullptr
#else
#define L2S_ENC_TAP(i, src, n) do {} while (0)
#define L2S_ENC_TAPS_ARG
#endif
static int encoder_run(l2s_model* m, const FrameSrc& video, int B, int T, int H, int W, const float* emb, float* vis,
                       float* feat, void* ws, int64_t ws_bytes, hipStream_t s, const RaggedTab* rg = nullptr L2S_ENC_TAPS_ARG) {
    X3Scope x3scope(m->opt.infer_bf16 ? 0 : m->opt.gemm_x3);
    Bf16Scope bf16scope(m->opt.infer_bf16);      // the bf16 leg: bf16-operand GEMM / Conv1d kernels instead of the f32 / split-bf16 ones
    const Weights& w = m->w;
    EncPlan pl = enc_plan(rg ? rg->NF : B * T, H);
    Bump bp(ws, ws_bytes);
    float* a = bp.f(pl.act_a); float* b = bp.f(pl.act_b); float* t1 = bp.f(pl.t1); float* t2 = bp.f(pl.t2); float* last = bp.f(pl.last);
    L2S_REQUIRE(!bp.overflow, "encoder workspace too small");
#ifdef L2S_DIAG
    if (enc_taps_check(m, taps, pl.Hp)) return 1;
#endif
    FrontendW fe = w.fe;
    if (!m->opt.frontend_x3) fe.w3 = nullptr;
    fe.pair = m->opt.frontend_x3 >= 2; fe.pipe = m->opt.frontend_x3 == 3;
    fe.solo = m->opt.frontend_solo && (m->opt.frontend_solo >= 2 || chains_hint() >= 2);
    if (!m->opt.infer_bf16) fe.w1 = nullptr;
    if (rg ? launch_frontend_ragged(fe, video, *rg, H, W, a, s) : launch_frontend(fe, video, B, T, H, W, a, s)) return 1;
    L2S_ENC_TAP(0, a, (int64_t)pl.NF * pl.Hp * pl.Hp * STAGE_CH[0]);
    float* x = a; float* y = b;
    int h = pl.Hp;
    const int NF = pl.NF;
    for (int u = 0; u < N_UNITS; ++u) {
        const UnitW& U = w.unit[u];
        const int half = U.half, cout = 2 * half;
        if (U.stride2 && m->opt.fuse_trunk && m->opt.fuse_s2) {
            ShuffleS2P sp{};
            sp.x = x; sp.out = y;
            sp.wd1 = U.b1_dw.w9; sp.sd1 = U.b1_dw.scale; sp.bd1 = U.b1_dw.shift;
            sp.wb1f = U.b1_frag; sp.sb1 = U.b1_pw.scale; sp.bb1 = U.b1_pw.shift;
            sp.w1f = U.pw1_frag; sp.s1 = U.pw1.scale; sp.b1 = U.pw1.shift;
            sp.wd = U.dw.w9; sp.sd = U.dw.scale; sp.bd = U.dw.shift;
            sp.w2f = U.pw2_frag; sp.s2 = U.pw2.scale; sp.b2 = U.pw2.shift;
            sp.NF = NF; sp.h = h; sp.ho = (h + 1) / 2; sp.cin = U.cin; sp.half = half; sp.Kin = U.kin; sp.Kh = U.kpad;
            sp.Ro = U.cin == 232 ? 3 : 2;                      // informational: fixed by the kernel instance
            if (m->opt.trunk_x3) { sp.wb1p = U.b1_p3; sp.w1p = U.pw1_p3; sp.w2p = U.pw2_p3; }
            if (launch_shuffle_s2(sp, s)) return 1;
            h = sp.ho;
        } else if (U.stride2) {
            const int cin = U.cin, ho = (h + 1) / 2;
            const int64_t in_px = (int64_t)NF * h * h, out_px = (int64_t)NF * ho * ho;
            // banch1: dw s2 (+BN) -> pw (+BN+ReLU) -> even output channels
            if (launch_dwconv(x, NF, h, h, cin, 0, cin, 2, U.b1_dw.w9, U.b1_dw.scale, U.b1_dw.shift, t2, cin, 0, s)) return 1;
            if (launch_gemm1(pw_gemm(t2, cin, 0, U.b1_pw, y, cout, 0, 2, out_px, half, cin, ACT_RELU), s, "shuffle_pw_gemm")) return 1;
            // banch2: pw -> dw s2 -> pw -> odd output channels
            if (launch_gemm1(pw_gemm(x, cin, 0, U.pw1, t1, half, 0, 1, in_px, half, cin, ACT_RELU), s, "shuffle_pw_gemm")) return 1;
            if (launch_dwconv(t1, NF, h, h, half, 0, half, 2, U.dw.w9, U.dw.scale, U.dw.shift, t2, half, 0, s)) return 1;
            if (launch_gemm1(pw_gemm(t2, half, 0, U.pw2, y, cout, 1, 2, out_px, half, half, ACT_RELU), s, "shuffle_pw_gemm")) return 1;
            h = ho;
        } else if (m->opt.fuse_trunk) {
            auto s1_params = [&](const UnitW& V, const float* in, float* outp) {
                ShuffleS1P sp{};
                sp.x = in; sp.out = outp;
                sp.w1f = V.pw1_frag; sp.s1 = V.pw1.scale; sp.b1 = V.pw1.shift;
                sp.wd = V.dw.w9; sp.sd = V.dw.scale; sp.bd = V.dw.shift;
                sp.w2f = V.pw2_frag; sp.s2 = V.pw2.scale; sp.b2 = V.pw2.shift;
                sp.NF = NF; sp.h = h; sp.half = V.half; sp.Kpad = V.kpad;
                sp.F = h >= 11 ? 1 : 2;                        // informational: fixed by the kernel instance
                if (m->opt.trunk_x3) { sp.w1p = V.pw1_p3; sp.w2p = V.pw2_p3; }      // pointwise convs on the bf16 matrix cores (exact split)
                return sp;
            };
            // the run of stride-1 units that starts here (the rest of the stage) as ONE launch: the map stays on chip between the units
            int run = 1;
            while (u + run < N_UNITS && !w.unit[u + run].stride2 && w.unit[u + run].half == half) ++run;
            if (S1_RUN_CHAINED(m, U, run, h)) {
                ShuffleS1P chain[S1_CHAIN_MAX];
                for (int i = 0; i < run; ++i) chain[i] = s1_params(w.unit[u + i], x, y);
                if (launch_shuffle_s1_chain(chain, run, s)) return 1;
                u += run - 1;
            } else {
                const ShuffleS1P sp = s1_params(U, x, y);
                if (launch_shuffle_s1(sp, s)) return 1;
            }
        } else {
            const int64_t px = (int64_t)NF * h * h;
            if (launch_copy_cols(x, cout, 0, y, cout, 0, 2, px, half, s)) return 1;
            if (launch_gemm1(pw_gemm(x, cout, half, U.pw1, t1, half, 0, 1, px, half, half, ACT_RELU), s, "shuffle_pw_gemm")) return 1;
            if (launch_dwconv(t1, NF, h, h, half, 0, half, 1, U.dw.w9, U.dw.scale, U.dw.shift, t2, half, 0, s)) return 1;
            if (launch_gemm1(pw_gemm(t2, half, 0, U.pw2, y, cout, 1, 2, px, half, half, ACT_RELU), s, "shuffle_pw_gemm")) return 1;
        }
        L2S_ENC_TAP(1 + u, y, (int64_t)NF * h * h * cout);      // u: the unit whose output y now holds (the last one of a chain)
        std::swap(x, y);
    }
    const int64_t px = (int64_t)NF * h * h;
    {
        GemmP pc = pw_gemm(x, STAGE_CH[3], 0, w.conv_last, last, LAST_CH, 0, 1, px, LAST_CH, STAGE_CH[3], ACT_RELU);
        if (!m->opt.gemm_x3_dma) pc.W3 = nullptr;
        if (launch_gemm1(pc, s, "conv_last_gemm")) return 1;
    }
    L2S_ENC_TAP(N_UNITS + 1, last, px * LAST_CH);
    if (rg) return launch_pool_norm_cat_ragged(last, *rg, h * h, LAST_CH, emb, L2S_D_EMB, vis, L2S_D_VIS, s);
    if (launch_pool_norm_cat(last, NF, h * h, LAST_CH, emb, L2S_D_EMB, T, vis, L2S_D_VIS, feat, s)) return 1;
    return 0;
}

// ------------------------------------------------------------------------------------------------ decoder prologue
// ---- per-clip video lengths (the *_masked entry points, include/l2s.h)
int check_lengths(const int32_t* video_lengths, int B, int T) {      // (shared with the l2s_train_*_masked_fwd / _masked_bwd entry points: l2s_common.h)
    L2S_REQUIRE(video_lengths, "video_lengths is null");
    for (int b = 0; b < B; ++b)
        if (video_lengths[b] < 7 || video_lengths[b] > T) {
            set_error("l2s: video_lengths[" + std::to_string(b) + "] = " + std::to_string(video_lengths[b]) + " is outside [7, T = " + std::to_string(T) + "]");
            return 1;
        }
    return 0;
}
// Where the uniform BiLSTM recurrence needs its two row kernels (step = launch index 0 .. T-1; the forward direction reads frame `step`, the backward
// direction frame T-1-step): capture AFTER the steps at which some clip's last frame was read forward (step = len_b - 1), reset BEFORE the steps at which
// a shorter clip's last frame is read backward (step = T - len_b, len_b < T).  Both ascending, without repeats.
static void masked_bilstm_plan(const int32_t* video_lengths, int B, int T, std::vector<int>& capture, std::vector<int>& reset) {
    capture.clear(); reset.clear();
    for (int b = 0; b < B; ++b) {
        capture.push_back(video_lengths[b] - 1);
        if (video_lengths[b] < T) reset.push_back(T - video_lengths[b]);
    }
    for (std::vector<int>* v : {&capture, &reset}) { std::sort(v->begin(), v->end()); v->erase(std::unique(v->begin(), v->end()), v->end()); }
}
static int64_t len_table_bytes(int B) { return align_up(len_table_words(B) * 4, 256); }

// The envelope of the persistent latency forms (pdecode.hip), the part that the prologue and the decode loop share: the options allow them for this
// call, it is no grouped call, and its clips fit the decode loop's forms.  Each stage adds its own terms and then asks pdecode_gate(T), once.
static bool persist_envelope(const l2s_model* m, bool masked, int B, int T, int mT) {
    return (!masked || m->opt.persist_masked > 0) && m->opt.persist > 0 && B <= m->opt.persist && !grouped_entry() && pdecode_supported(B, T, mT, m->opt.persist_frames);
}

// lens (a masked call): row b computes what clip b alone at T = len_b computes (the launch-per-step recurrence, or pbilstm_kernel's masked form: "persist_masked")
static int prologue_run(l2s_model* m, const float* vis, const float* emb, const float* gumbel, int B, int T,
                        float* state, float* content_dis, void* ws, int64_t ws_bytes, hipStream_t s, ClipLens lens = {},
                        bool free_running = true) {      // free_running = false: the prologue of a teacher-forced masked call (launch route, whatever "persist_masked" says)
    X3Scope x3scope(m->opt.infer_bf16 ? 0 : m->opt.gemm_x3);
    Bf16Scope bf16scope(m->opt.infer_bf16);      // the bf16 leg: bf16-operand GEMM / Conv1d kernels instead of the f32 / split-bf16 ones
    const Weights& w = m->w;
    StateLayout sl = state_layout(B, T);
    ProBufs pb{};
    int* const L = pb.L;
    const int mT = pb.m = content_lens(T, L);
    L2S_REQUIRE(T >= 7 && T <= L2S_MAX_STEPS, "T must be in [7, 300] (Content.agg stride-7 branch; positional table)");
    const int BT = B * T, Bp = pad16(B);
    Bump bp(ws, ws_bytes);
    pb.gin = bp.f((int64_t)BT * 4096);
    pb.rnn = bp.f((int64_t)BT * 1024);
    pb.resid = bp.f((int64_t)BT * 512);
    pb.s_e = bp.f((int64_t)B * 512);
    pb.s_a = bp.f((int64_t)B * 512);
    pro_carve_lstm(bp, B, pb);
    pb.cellcat = bp.f((int64_t)B * 1024);
    pb.cat = bp.f((int64_t)BT * 4608);
    for (int j = 0; j < 4; ++j) pb.cmap[j] = bp.f((int64_t)B * L[j] * 512);
    pb.pooled = bp.f((int64_t)B * mT * 2560);
    for (float** t : {&pb.wv, &pb.tA, &pb.tB, &pb.tC}) *t = bp.f((int64_t)B * mT * 256);
    pb.logits = bp.f((int64_t)B * mT * VOC);
    pb.zsoft = bp.f((int64_t)B * mT * VOCP);
    float* part = bp.f(8 * std::max((int64_t)B * mT * 256, (int64_t)B * 512));
    int64_t tap_floats = 0;
    for (int j = 1; j < 4; ++j) tap_floats += (int64_t)CT_KS[j] * B * L[j] * 512;
    float* tap_part = bp.f(tap_floats);
    float* bott_part = bp.f((int64_t)8 * BT * 512);
    // one or two clips of a single-batch call: the BiLSTM recurrence as ONE persistent launch (pdecode.hip pbilstm_kernel; option "persist_decode")
    // (the envelope of the latency path; a persistent launch that timed out since the last call fails THIS call once: pdecode_gate)
    const int pgate = (persist_envelope(m, (bool)lens, B, T, mT) && pbilstm_supported(B, T) && (!lens || free_running)) ? pdecode_gate(T) : 0;
    if (pgate < 0) return 1;
    const bool pbi = pgate > 0;
    float* pbx = pbi ? bp.f(pbilstm_ws_bytes() / 4 + 64) : nullptr;
    L2S_REQUIRE(!bp.overflow, "prologue workspace too small");

    // every descriptor of this stage is built in decoder_stages.h; what follows picks the launcher of each and runs the masked and persistent branches
    const Prologue pro{w, pb, state, sl, B, T, m->opt.gemm_x3_dma != 0};
    // residual_bottleneck (120 tiles: four K slices), site embeddings, BiLSTM input gates
    if (launch_gemm_splitk(pro.resid(vis), 4, bott_part, s, "prologue_gemm")) return 1;
    if (launch_gemm(pro.sites(emb), s, "prologue_gemm")) return 1;
    if (launch_gemm1(pro.bilstm_in(vis), s, "bilstm_input_gemm")) return 1;
    if (pbi) {
        PBiP q{};
        q.Whh0 = w.whh[0].W; q.Whh1 = w.whh[1].W; q.gin = pb.gin; q.s_e = pb.s_e; q.rnn = pb.rnn; q.h_state = state + sl.h; q.cellcat = pb.cellcat; q.B = B; q.T = T;
        q.lens = lens.dev;      // masked: pair (direction, clip) runs its clip's own length; the masked steps below are those of the launch route
        if (launch_pbilstm(q, pbx, pbilstm_ws_bytes(), s)) return 1;
    } else {
    if (bilstm_start(pb, B, s)) return 1;
    std::vector<int> cap_steps, rst_steps;
    size_t cap_i = 0, rst_i = 0;
    if (lens) {
        masked_bilstm_plan(lens.host, B, T, cap_steps, rst_steps);
        if (launch_fill(state + sl.h, (int64_t)Bp * 512, 0.f, s)) return 1;      // forward finals arrive row by row; the padded rows stay zero
    }
    for (int step = 0; step < T; ++step) {
        SkinnyBatch sb{};
        const int cur = step & 1, nxt = cur ^ 1;
        if (rst_i < rst_steps.size() && rst_steps[rst_i] == step) {      // backward rows whose clip ends at frame T-1-step start here, from s_e
            ++rst_i;
            if (launch_bilstm_reset(pb.hf[1][cur], pb.cf[1], lens.dev, B, T - 1 - step, pb.s_e, s)) return 1;
        }
        for (int d = 0; d < 2; ++d) bilstm_step_group(sb, d, w, true, B, T, d == 0 ? step : T - 1 - step, pb.hf[d][cur], pb.hf[d][nxt], pb.cf[d], pb.gin, pb.rnn);
        sb.count = 2;
        if (launch_skinny(sb, s, "bilstm_step", m->opt)) return 1;
        if (cap_i < cap_steps.size() && cap_steps[cap_i] == step) {      // forward rows whose clip ended at frame `step`: their finals, now
            ++cap_i;
            if (launch_bilstm_capture(pb.hf[0][nxt], pb.cf[0], lens.dev, B, step, state + sl.h, pb.cellcat, 1024, s)) return 1;
        }
    }
    if (bilstm_finals(pb, state, sl, B, T, !lens, s)) return 1;      // a masked call has captured the forward finals row by row
    }
    // encoder_cell = E_C(cat(c_fwd, c_bwd)): B rows x 512 columns = 8 tiles: split K = 1024 eight ways
    if (launch_gemm_splitk(pro.e_c(), 8, part, s, "prologue_gemm")) return 1;
    if (launch_stop_const(state + sl.ecell, w.stop_tail, w.stop_bias, B, state + sl.stopc, s)) return 1;
    // enc = encoder_proj(rnn_out) + s_a (broadcast over T) + residual  -> cat[:, 0:512] and the state
    if (launch_gemm_splitk(pro.enc_proj(), 4, bott_part, s, "prologue_gemm")) return 1;
    // with lengths: rows t >= len_b become zeros on the way (the K / V convolutions below then read past a clip's end what a solo call reads as padding)
    if (lens ? launch_mask_copy_rows(pb.cat, PRO_CAT, state + sl.enc, 512, lens.dev, B, T, 512, s)
             : launch_copy_cols(pb.cat, PRO_CAT, 0, state + sl.enc, 512, 0, 1, BT, 512, s)) return 1;
    // MultiHopConv branches of K and V (8 convs, one grouped launch), then the two bottlenecks (+PSine +pos)
    {
        // longest K first: the groups are dispatched in order, and the 11-tap convs (K = 5632) would otherwise start last and run alone
        GemmBatch gb{};
        for (int j = 3; j >= 0; --j)
            for (int kv = 0; kv < 2; ++kv) gb.p[gb.count++] = pro.mh_branch(kv, j);
        if (launch_gemm(gb, s, "multihop_conv_gemm")) return 1;
        // 2 x 120 tiles with K = 2560 is one block per CU and 80 dependent K iterations: four K slices each
        if (launch_gemm_splitk_group(pro.mh_bott(), 4, bott_part, s, "multihop_bottleneck_gemm")) return 1;
        // V' = V W_ap^T + b_ap: attention_proj (decoder.py:420) applied to the values once per clip instead of to a @ v at every step
        if (w.vproj.W && launch_gemm1(pro.vproj(), s, "prologue_gemm")) return 1;
    }
    // Content.encode (decoder.py:239-260)
    {
        // (4..29) x B rows by 512 columns: 16-120 tiles per branch with K up to 3584 - one slice per tap instead (16 slices, 472 tiles of K = 512)
        if (launch_gemm_tapsplit(pro.ct_branches(), tap_part, s, "content_agg_gemm")) return 1;
        if (lens ? launch_pool_cat_masked(pro.pool_cat(), pro.pool_div(), lens.dev, s) : launch_pool_cat(pro.pool_cat(), s)) return 1;
        if (launch_gemm_splitk(pro.ct_bott(), 8, part, s, "content_gemm")) return 1;       // 4B rows x 256 columns = 8 tiles with K = 2560
        if (launch_gemm(pro.ct_pair0(), s, "content_gemm")) return 1;
        if (launch_gemm(pro.ct_pair2(), s, "content_gemm")) return 1;
        if (launch_gemm1(pro.ct_fc4(), s, "content_gemm")) return 1;
        if (launch_gumbel_softmax(pb.logits, gumbel, pro.R(), VOC, 0.1f, pb.zsoft, VOCP, content_dis, s)) return 1;
        if (lens && launch_zero_slot_rows(pb.zsoft, VOCP, content_dis, VOC, B, mT, lens.dev, s)) return 1;      // slots i >= m_b: zero z (so zero values) and zero content_dis
        if (launch_gemm1(pro.ct_emb(), s, "content_gemm")) return 1;
        // the content columns of LSTM layer 0 applied to the values once per call (option "hoist_vproj" = 3): clips short enough to have a table (StateLayout::cp)
        if (w.cproj.W && sl.cp_pitch && launch_gemm1(pro.cproj(), s, "content_hoist_gemm")) return 1;
    }
    // decoder cell state starts at zero (decoder.py:406)
    if (launch_fill(state + sl.c, (int64_t)Bp * 512 * 2, 0.f, s)) return 1;
    return 0;
}

// ------------------------------------------------------------------------------------------------ decode loop
// options (l2s_common.h Options, per model): "fold_step_weights" - phase-merged step (4 launches) vs the literal 6-phase step; "overlap_postnet" -
// l2s_inference runs the post-net in time windows on a second stream under the decode loop (bit-identical; measured SLOWER on MI355X, 13.1 vs
// 12.0 ms: the GEMM blocks delay the latency-critical step launches); "use_graph" - replay the loop from a captured hipGraph (measured slower
// than stream launches on MI355X: 15.0 vs 13.7 ms)

// The launches of one step - groups, K segments, epilogues, tile counts - are built in decode_step.h; this loop overlays the early-stop control fields.
// on_frames(n): called (if set) right after the launch that completes mel frames [0, n) has been enqueued on `s`
static int decode_launches(l2s_model* m, float* state, int B, int T, int S, const float* teacher, const uint8_t* teacher_mask,
                           float* mel, float* stop, float* attn, int attn_logits, void* ws, int64_t ws_bytes, hipStream_t s, bool fold,
                           const std::function<int(int)>* on_frames = nullptr, bool early = false, ClipLens lens = {}) {
    const Weights& w = m->w;
    StateLayout sl = state_layout(B, T);
    const int Bp = pad16(B);
    const StepForm form = step_form(w, m->opt, fold, sl.m);
    Bump bp(ws, ws_bytes);
    const StepBufs d = step_carve(bp, B, true);
    // option "early_stop" (free-running loops only): this call's control block, armed on the stream - chains in flight on other streams have their own
    EsCtl* const es = early ? reinterpret_cast<EsCtl*>(bp.f(B + 2)) : nullptr;
    L2S_REQUIRE(!bp.overflow, "decode workspace too small");
    L2S_REQUIRE(!early || !teacher, "early stop is for free-running loops");
    if (es) L2S_CHECK_HIP(hipMemsetAsync(es, 0, sizeof(int) * (B + 2), s));
    const int* const es_end = es ? &es->end_rel : nullptr;

    // initial state: h from the prologue, c = 0, y = BOS; padded rows of every frag buffer zero
    L2S_CHECK_HIP(hipMemcpyAsync(d.h0[0], state + sl.h, sizeof(float) * Bp * 512, hipMemcpyDeviceToDevice, s));
    L2S_CHECK_HIP(hipMemcpyAsync(d.h1[0], state + sl.h + (int64_t)Bp * 512, sizeof(float) * Bp * 512, hipMemcpyDeviceToDevice, s));
    // one fill over the contiguous run h0[1] .. p2f is not possible (h0[0]/h1[0] sit in between); fill individually
    float* zero512[] = {d.h0[1], d.h1[1], d.c0, d.c1, d.av};
    for (float* z : zero512) if (launch_fill(z, (int64_t)Bp * 512, 0.f, s)) return 1;
    float* zero256[] = {d.p1, d.cc, d.uu, d.p2f};
    for (float* z : zero256) if (launch_fill(z, (int64_t)Bp * 256, 0.f, s)) return 1;
    if (launch_to_frag(w.bos, 0, B, 80, d.yf, 80, 0, 1, s)) return 1;

    const StepOut out{mel, stop, state + sl.stopc, S};
    // early stop: every launch carries the step it belongs to; the fc / stop group that finishes step `step` keeps the stop bookkeeping
    auto es_launch = [&](SkinnyBatch& sb, int step) { sb.es_end = es_end; sb.es_step = step - S; };
    auto es_fc = [&](SkinnyP& a, int step) {
        if (es) { a.es_ctl = reinterpret_cast<int*>(es); a.es_end = std::min(S, step + 1 + es_margin()) - S; }
    };

    for (int i = 0; i < S; ++i) {
        const bool forced = teacher && teacher_mask && teacher_mask[i];
        if (forced)
            if (launch_to_frag(teacher + (int64_t)i * NM, S * NM, B, 80, d.yf, 80, 0, 0, s)) return 1;
        {   // phase A: prenet layer 1, Q (+PSine +pos[i]), content Q (+SiLU) [, mel frame + stop logit of step i-1]
            SkinnyBatch sb = step_phase_a(form, w, d, B, i, step_from_frame(form, i, forced), out);
            const bool rides = sb.count == 4;
            if (rides) es_fc(sb.p[3], i - 1);
            // the folded launch also finishes step i - 1 (its mel frame and stop logit): it is skipped as part of THAT step, i.e. one step later
            es_launch(sb, rides ? i - 1 : i);
            if (launch_skinny(sb, s, fold ? "step_prenet1_q_cq_fc" : "step_prenet1_q_cq", m->opt)) return 1;
            if (rides && on_frames && (*on_frames)(i)) return 1;
        }
        {   // phase B: attention + content attention per batch row; prenet layer 2
            StepAttn b = step_phase_b(form, w, d, state, sl, B, T, i, S, attn, attn_logits);
            b.at.es_end = es_end; b.at.es_step = i - S;
            if (lens ? launch_step_attn_masked(b.at, b.pre2, b.pre2_tiles, lens.dev, s, m->opt.attn_lds, m->opt.attn_skip0)
                     : launch_step_attn(b.at, b.pre2, b.pre2_tiles, s, m->opt.attn_lds, m->opt.attn_skip0)) return 1;
        }
        if (!fold) {   // phase C: u = prenet + attention_proj(a @ v)
            SkinnyBatch sb = step_phase_c(form, w, d, B);
            es_launch(sb, i);
            if (launch_skinny(sb, s, "step_attention_proj", m->opt)) return 1;
        }
        {   // phase D: LSTM layer 0 on cat(content, u), h0  (folded: cat(content, prenet, a@v) against [W_ih | W_ih_u W_ap | W_hh])
            SkinnyBatch sb = step_phase_d(form, w, d, B, i, state + sl.cp, sl.cp_pitch);
            es_launch(sb, i);
            if (launch_skinny(sb, s, "step_lstm_cell", m->opt)) return 1;
        }
        {   // phase E: LSTM layer 1 on the new h0
            SkinnyBatch sb = step_phase_e(form, w, d, B, i);
            es_launch(sb, i);
            if (launch_skinny(sb, s, "step_lstm_cell", m->opt)) return 1;
        }
        if (step_has_phase_f(form, i, S)) {   // phase F: mel frame + stop logit (folded mode: only the last step needs its own launch)
            SkinnyBatch sb = step_phase_f(form, w, d, B, i, out);
            es_fc(sb.p[0], i);
            es_launch(sb, i);
            if (launch_skinny(sb, s, "step_fc_out_stop", m->opt)) return 1;
            if (on_frames && (*on_frames)(i + 1)) return 1;
        }
    }
    return 0;
}

static int side_stream_ready(l2s_model* m) {      // the model's side stream and its two events, made on first use (m->side_mu held)
    if (m->side) return 0;
    L2S_CHECK_HIP(hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking));
    L2S_CHECK_HIP(hipEventCreateWithFlags(&m->ev_in, hipEventDisableTiming));
    L2S_CHECK_HIP(hipEventCreateWithFlags(&m->ev_out, hipEventDisableTiming));
    return 0;
}

static int decode_run(l2s_model* m, float* state, int B, int T, int S, const float* teacher, const uint8_t* teacher_mask,
                      float* mel, float* stop, float* attn, int attn_logits, void* ws, int64_t ws_bytes, hipStream_t s, bool may_stop_early, ClipLens lens = {}) {
    L2S_REQUIRE(S >= 1 && S <= L2S_MAX_STEPS, "S must be in [1, 300] (positional table)");
    const bool fold = m->opt.fold != 0 && m->folded_valid;
    // option "early_stop": free-running loops only (a teacher-forced loop's S comes from the target).  The steps the loop never reaches are exact zeros
    // in the staged outputs: zero-filled on the stream first
    const bool early = may_stop_early && m->opt.early_stop != 0 && !teacher;
    if (early) {
        L2S_CHECK_HIP(hipMemsetAsync(mel, 0, sizeof(float) * B * S * NM, s));
        L2S_CHECK_HIP(hipMemsetAsync(stop, 0, sizeof(float) * B * S, s));
        if (attn) L2S_CHECK_HIP(hipMemsetAsync(attn, 0, sizeof(float) * B * S * T, s));
    }
    // the latency form: one launch for the whole loop (with lengths: option "persist_masked") - free-running, on the folded weights
    const Weights& w = m->w;
    StateLayout sl = state_layout(B, T);
    const int pgate = (persist_envelope(m, (bool)lens, B, T, sl.m) && !teacher && fold && w.vproj.W && w.pre1f.W && w.lstm0.W && w.lstm1.W) ? pdecode_gate(T) : 0;
    if (pgate < 0) return 1;      // an earlier persistent launch on this device gave up (its outputs are NaN): reported here, once
    if (pgate > 0) {
        PDecP p{};
        p.Wq = w.q.W; p.bq = w.q.bias; p.aq = w.q.actw;
        p.Wcq = w.cq.W; p.bcq = w.cq.bias;
        p.Wp1f = w.pre1f.W; p.bp1f = w.pre1f.bias; p.ap1 = w.pre1f.actw;
        p.Wp1 = w.pre1.W; p.bp1 = w.pre1.bias;
        p.Wp2 = w.pre2.W; p.bp2 = w.pre2.bias; p.ap2 = w.pre2.actw;
        p.Wl0 = w.lstm0.W; p.bl0 = w.lstm0.bias; p.Wl1 = w.lstm1.W; p.bl1 = w.lstm1.bias;
        p.Wfc = w.fc.W; p.bfc = w.fc.bias;
        p.pos = w.pos; p.tau = w.tau; p.tau_c = w.tau_c; p.bos = w.bos;
        p.k = state + sl.k; p.vp = state + sl.vp; p.ckey = state + sl.ckey; p.cval = state + sl.cval;
        p.h_init = state + sl.h; p.stop_const = state + sl.stopc;
        p.mel = mel; p.stop = stop; p.attn = attn; p.attn_logits = attn_logits;
        p.B = B; p.T = T; p.m = sl.m; p.S = S;
        p.early = early ? es_margin() : 0;
        return launch_pdecode(p, ws, ws_bytes, s, lens);
    }
    const bool use_graph = m->opt.graph && !teacher && !g_prof_on && !early && !lens;      // "early_stop" and per-clip lengths take the plain route: a replayed graph knows no control block / length table of this call
    if (!use_graph) return decode_launches(m, state, B, T, S, teacher, teacher_mask, mel, stop, attn, attn_logits, ws, ws_bytes, s, fold, nullptr, early, lens);

    std::lock_guard<std::mutex> side_lock(m->side_mu);      // graph cache, side stream and events are per model; chains of other threads wait here
    if (side_stream_ready(m)) return 1;
    l2s_model::GraphEntry* hit = nullptr;
    for (auto& g : m->graphs)
        if (g.B == B && g.T == T && g.S == S && g.attn_logits == attn_logits && g.fold == (int)fold && g.state == state && g.mel == mel &&
            g.stop == stop && g.attn == attn && g.ws == ws) { hit = &g; break; }
    if (!hit) {
        hipGraph_t graph = nullptr;
        L2S_CHECK_HIP(hipStreamBeginCapture(m->side, hipStreamCaptureModeThreadLocal));
        int rc = decode_launches(m, state, B, T, S, nullptr, nullptr, mel, stop, attn, attn_logits, ws, ws_bytes, m->side, fold);
        hipError_t ce = hipStreamEndCapture(m->side, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return 1; }
        L2S_CHECK_HIP(ce);
        hipGraphExec_t exec = nullptr;
        L2S_CHECK_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        if (m->graphs.size() >= 8) {           // small FIFO: shapes/buffers rarely change in a serving loop
            (void)hipGraphExecDestroy(m->graphs.front().exec);
            (void)hipGraphDestroy(m->graphs.front().graph);
            m->graphs.erase(m->graphs.begin());
        }
        m->graphs.push_back({B, T, S, attn_logits, (int)fold, state, mel, stop, attn, ws, graph, exec});
        hit = &m->graphs.back();
    }
    L2S_CHECK_HIP(hipEventRecord(m->ev_in, s));
    L2S_CHECK_HIP(hipStreamWaitEvent(m->side, m->ev_in, 0));
    L2S_CHECK_HIP(hipGraphLaunch(hit->exec, m->side));
    L2S_CHECK_HIP(hipEventRecord(m->ev_out, m->side));
    L2S_CHECK_HIP(hipStreamWaitEvent(s, m->ev_out, 0));
    return 0;
}

// ------------------------------------------------------------------------------------------------ postnet
struct PostBufs { float* x[4]; float* part = nullptr; float* wv = nullptr; float* wm = nullptr; };      // wv, wm: the Winograd route's V and M

static int postnet_alloc(Bump& bp, int B, int S, PostBufs& pb) {
    for (int i = 0; i < 4; ++i) pb.x[i] = bp.f((int64_t)B * S * 512);
    // few rows (one or two clips alone: 5-10 row tiles x 8 column tiles on 256 CUs, K = 2560 deep: 67 us per layer): one K slice per tap in one grouped
    // launch + a finish kernel that adds the taps in order (launch_gemm_tapsplit; 40 -> 200 tiles).  Decided on the rows of ONE batch, so that a batch
    // meets the same arithmetic alone and in a group.
    pb.part = ((int64_t)B * S / gemm_x3_group() <= POST_TAPSPLIT_ROWS) ? bp.f((int64_t)B * S * 512 * 5) : nullptr;
    pb.wv = bp.f(post_wino_floats(B, S)); pb.wm = bp.f(post_wino_floats(B, S));
    return bp.overflow ? 1 : 0;
}

// One post-net layer (decoder.py:143-156) over the frames [t0, t1) of every sequence; layer 0..4.
// Layer i reads buffer i (mel for i = 0) and writes buffer i+1 (mel_post, channel-first, for i = 4).
// wino: layers 1-3 of a full-range call in their Winograd F(4,5) form (post_wino_route): input transform, the eight products as ONE grouped launch of the
// split-bf16 family (whatever the rows: wide and narrow tile give the same bits), output transform with the layer's epilogue.
static int postnet_layer(const Weights& w, int layer, const float* mel, const PostBufs& pb, float* mel_post, int B, int S, int t0, int t1, hipStream_t s, bool dma_weights,
                         bool wino = false) {
    if (t1 <= t0) return 0;
    if (wino && layer >= 1 && layer <= 3 && t0 == 0 && t1 == S) {
        L2S_REQUIRE(w.post_wino[layer] && pb.wv && pb.wm, "post-net: no Winograd weights / workspace");
        if (launch_post_wino_in(pb.x[layer - 1], B, S, 512, pb.wv, s)) return 1;
        if (launch_gemm(post_wino_products(w, layer, pb.wv, pb.wm, B * wino_tiles(S), dma_weights), s, "postnet_conv_gemm")) return 1;
        return launch_post_wino_out(pb.wm, B, S, 512, w.post[layer].scale, w.post[layer].shift, w.post[layer].actw, pb.x[layer - 1], pb.x[layer], s);
    }
    const bool tapsplit = pb.part && t0 == 0 && t1 == S;
    // the full-range descriptor is decoder_stages.h's; the weight planes go with the plain route only, and so does the time window
    GemmP p = post_layer(w, layer, layer == 0 ? mel : pb.x[layer - 1], layer == 4 ? mel_post : pb.x[layer], mel, B, S, dma_weights && !tapsplit);
    if (tapsplit) {
        GemmBatch gb{};
        gb.p[0] = p; gb.count = 1;
        return launch_gemm_tapsplit(gb, pb.part, s, "postnet_conv_gemm");
    }
    p.M = B * (t1 - t0); p.Tout = t1 - t0; p.win_T = S; p.win_off = t0;
    return launch_gemm1(p, s, "postnet_conv_gemm");
}

// ev (l2s_forward_eval_ragged; null for every other caller): row b decodes a batch of ev->clips[b].S <= S steps.  The caller has zeroed the rows j >= S_b
// of mel; here the same rows of the outputs of layers 0..3 are zeroed, so that the next layer's taps read past a row's end the zeros its batch's own call
// reads as padding (the same operands in the same K order: the same bits at j < S_b).  Rows j >= S_b of mel_post are the caller's to drop.
static int postnet_run(l2s_model* m, const float* mel, int B, int S, float* mel_post, float* mel_cf, void* ws, int64_t ws_bytes, hipStream_t s,
                       const EvalTab* ev = nullptr) {
    X3Scope x3scope(m->opt.infer_bf16 ? 0 : m->opt.gemm_x3);
    Bf16Scope bf16scope(m->opt.infer_bf16);      // the bf16 leg: bf16-operand GEMM / Conv1d kernels instead of the f32 / split-bf16 ones
    const Weights& w = m->w;
    Bump bp(ws, ws_bytes);
    PostBufs pb;
    L2S_REQUIRE(postnet_alloc(bp, B, S, pb) == 0, "postnet workspace too small");
    L2S_REQUIRE(!ev || (ev->N == B && ev->Smax == S), "postnet: the step table does not match the rows");
    const bool wino = post_wino_route(m, B, S);
    for (int layer = 0; layer < 5; ++layer) {
        if (postnet_layer(w, layer, mel, pb, mel_post, B, S, 0, S, s, m->opt.gemm_x3_dma != 0, wino)) return 1;
        if (ev && layer < 4 && launch_zero_rows_past_s(pb.x[layer], 512, *ev, s)) return 1;
    }
    if (mel_cf && launch_transpose_bsc(mel, B, S, NM, mel_cf, s)) return 1;
    return 0;
}

// ------------------------------------------------------------------------------------------------ speaker encoder
static int64_t spk_ws_floats(int B, int N) {
    const int64_t L = N / 160 + 1, R = (int64_t)B * L;
    return R * (400 + 402 + 204 + 40 + 1024 + 256 * 2) + (int64_t)pad16(B) * 256 * 3 + (int64_t)B * 256 + 64 * 16;
}
static int64_t spk_ws_bytes(int B, int N) { return spk_ws_floats(B, N) * (int64_t)sizeof(float) + (1 << 12); }

// SpeakerEncoder.inference (audio.py:131-150): mel40 -> 3 x LSTM(256), zero initial state -> Linear(h_last) -> ReLU -> L2 norm
#ifdef L2S_DIAG      // stage taps (l2s_op_speaker_taps): a host-side copy after the stage, device to device on the call's stream - layer 0's sequence shares its buffer with layer 2's
static int spk_tap(float* const* taps, int i, const float* src, int64_t n, hipStream_t s) {
    if (taps && taps[i]) L2S_CHECK_HIP(hipMemcpyAsync(taps[i], src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
#define L2S_SPK_TAP(i, src, n) do { if (spk_tap(taps, i, src, n, s)) return 1; } while (0)
#define L2S_SPK_TAPS_ARG , float* const* taps = nullptr
#else
#define L2S_SPK_TAP(i, src, n) do {} while (0)
#define L2S_SPK_TAPS_ARG
#endif
static int speaker_run(l2s_model* m, const float* audio, int B, int N, float* emb, void* ws, int64_t ws_bytes, hipStream_t s L2S_SPK_TAPS_ARG) {
    X3Scope x3scope(m->opt.infer_bf16 ? 0 : m->opt.gemm_x3);
    Bf16Scope bf16scope(m->opt.infer_bf16);      // the bf16 leg: bf16-operand GEMM / Conv1d kernels instead of the f32 / split-bf16 ones
    const Weights& w = m->w;
    L2S_REQUIRE(N > 200, "audio shorter than the reflect padding (200 samples)");
    const int L = N / 160 + 1, Bp = pad16(B);
    const int64_t R = (int64_t)B * L;
    Bump bp(ws, ws_bytes);
    float* frames = bp.f(R * 400); float* spec = bp.f(R * 402); float* power = bp.f(R * 204); float* mel = bp.f(R * 40);
    float* pre = bp.f(R * 1024); float* hseq[2] = {bp.f(R * 256), bp.f(R * 256)};
    float* hf[2] = {bp.f((int64_t)Bp * 256), bp.f((int64_t)Bp * 256)}; float* cf = bp.f((int64_t)Bp * 256);
    float* lin = bp.f((int64_t)B * 256);
    // the published size, not what the carve above happens to need: its alignment slack would let a short workspace through
    L2S_REQUIRE(!bp.overflow && ws_bytes >= spk_ws_bytes(B, N), "speaker-encoder workspace too small");
    if (launch_frame_window(audio, B, N, L, 400, 160, w.spk_window, frames, s)) return 1;
    if (launch_gemm1(gemm_plain(frames, 400, w.spk_dft, spec, 402, (int)R, 402, 400), s, "spk_dft_gemm")) return 1;
    L2S_SPK_TAP(0, spec, R * 402);
    if (launch_power(spec, 402, R, 201, power, 204, s)) return 1;
    L2S_SPK_TAP(1, power, R * 204);
    if (launch_gemm1(gemm_plain(power, 204, w.spk_fbT, mel, 40, (int)R, 40, 204), s, "spk_mel_gemm")) return 1;
    L2S_SPK_TAP(2, mel, R * 40);
    const float* x = mel;
    int xin = 40;
    for (int l = 0; l < 3; ++l) {
        GemmP g = gemm_plain(x, xin, w.spk_ih[l].W, pre, 1024, (int)R, 1024, xin);
        g.shift = w.spk_ih[l].shift;
        if (launch_gemm1(g, s, "spk_lstm_input_gemm")) return 1;
        if (launch_fill(hf[0], (int64_t)Bp * 256, 0.f, s)) return 1;
        if (launch_fill(hf[1], (int64_t)Bp * 256, 0.f, s)) return 1;
        if (launch_fill(cf, (int64_t)Bp * 256, 0.f, s)) return 1;
        float* out = hseq[l & 1];
        for (int t = 0; t < L; ++t) {
            const SkinnyBatch sb = spk_lstm_step(w, l, B, hf[t & 1], hf[(t & 1) ^ 1], cf, pre + (int64_t)t * 1024, (int64_t)L * 1024, out + (int64_t)t * 256, (int64_t)L * 256);
            if (launch_skinny(sb, s, "spk_lstm_step", m->opt)) return 1;
        }
        L2S_SPK_TAP(3 + l, out, R * 256);
        x = out;
        xin = 256;
    }
    // embeds = normalize(relu(linear(h_last))), h_last = top layer's output at the last frame
    GemmP g = gemm_plain(x + (int64_t)(L - 1) * 256, L * 256, w.spk_linear.W, lin, 256, B, 256, 256);
    g.shift = w.spk_linear.shift; g.act = ACT_RELU;
    if (launch_gemm1(g, s, "spk_linear_gemm")) return 1;
    L2S_SPK_TAP(6, lin, (int64_t)B * 256);
    return launch_pool_norm_cat(lin, B, 1, 256, nullptr, 0, 1, nullptr, 0, emb, s);
}

// ---- the tower over B clips of unequal length (l2s_speaker_encoder_packed): every clip as speaker_run computes it alone at B = 1, N = n_b.
// Rows in the time-major compact layout (torch's PackedSequence): clips by frame count L_b = n_b / 160 + 1 descending, ties in call order; frame l of
// the clip of rank r is row step_row0[l] + r of R = sum L_b, step_row0 the prefix sum of step_rows[t] = #{b : L_b > t}.  Step t of the recurrence is
// then the contiguous block of step_rows[t] rows at step_row0[t], and the rows that have ended are the LAST ones of the state buffers: the count only
// falls, so they are never read again and the cell kernel needs no mask.
struct SpkPlan { std::vector<int32_t> order, step_rows, step_row0; int L_max = 0; int64_t R = 0; };
static int spk_packed_plan(const int64_t* n_samples, int B, SpkPlan& pl) {
    L2S_REQUIRE(n_samples, "l2s speaker packed: n_samples is null");
    if (B < 1 || B > L2S_SPK_MAX_CLIPS) {
        set_error("l2s speaker packed: B = " + std::to_string(B) + " is outside [1, L2S_SPK_MAX_CLIPS = " + std::to_string(L2S_SPK_MAX_CLIPS) + "]");
        return 1;
    }
    pl = SpkPlan{};
    for (int b = 0; b < B; ++b) {
        if (n_samples[b] <= 200 || n_samples[b] > (1ll << 30)) {
            set_error("l2s speaker packed: n_samples[" + std::to_string(b) + "] = " + std::to_string(n_samples[b]) +
                      " is outside [201, 2^30] (the reflect padding of 200 needs more than 200 samples)");
            return 1;
        }
        const int L = (int)(n_samples[b] / 160) + 1;
        pl.R += L;
        pl.L_max = std::max(pl.L_max, L);
    }
    if (pl.R > L2S_SPK_MAX_ROWS) {
        set_error("l2s speaker packed: R = " + std::to_string(pl.R) + " frames exceed L2S_SPK_MAX_ROWS = " + std::to_string(L2S_SPK_MAX_ROWS));
        return 1;
    }
    pl.order.resize(B);
    for (int b = 0; b < B; ++b) pl.order[b] = b;
    std::stable_sort(pl.order.begin(), pl.order.end(), [&](int a, int b) { return n_samples[a] / 160 > n_samples[b] / 160; });
    pl.step_rows.assign(pl.L_max, 0);
    pl.step_row0.assign(pl.L_max + 1, 0);
    for (int b = 0; b < B; ++b) pl.step_rows[n_samples[b] / 160] += 1;      // clips ENDING at step t ...
    for (int t = pl.L_max - 2; t >= 0; --t) pl.step_rows[t] += pl.step_rows[t + 1];      // ... summed from the back: clips with L_b > t
    for (int t = 0; t < pl.L_max; ++t) pl.step_row0[t + 1] = pl.step_row0[t] + pl.step_rows[t];
    return 0;
}
// the device table: B x SpkRank in rank order (written by the caller through the returned host pointer), then step_row0
struct SpkTable { int64_t ranks, row0; };
static SpkTable spk_table(HostTable& t, int B, int L_max, const int32_t* step_row0) { return SpkTable{t.rec<SpkRank>(nullptr, B), t.i32(step_row0, L_max + 1)}; }
static int64_t spk_table_words(int B, int L_max) { HostTable t(false); spk_table(t, B, L_max, nullptr); return t.words(); }
static int64_t spk_ws_bytes_packed(const SpkPlan& pl, int B) {
    const int64_t f = pl.R * (400 + 402 + 204 + 40 + 1024 + 256 * 2) + (int64_t)pad16(B) * 256 * 3 + (int64_t)B * 256 * 2 + 64 * 16;
    return f * (int64_t)sizeof(float) + align_up(spk_table_words(B, pl.L_max) * 4, 256) + (1 << 12);
}

static int speaker_packed_run(l2s_model* m, const float* audio, const int64_t* offsets, const int64_t* n_samples, const SpkPlan& pl, int B, float* emb, void* ws,
                              int64_t ws_bytes, hipStream_t s L2S_SPK_TAPS_ARG) {
    X3Scope x3scope(m->opt.infer_bf16 ? 0 : m->opt.gemm_x3);
    Bf16Scope bf16scope(m->opt.infer_bf16);      // the bf16 leg: bf16-operand GEMM / Conv1d kernels instead of the f32 / split-bf16 ones
    const Weights& w = m->w;
    const int Bp = pad16(B), L = pl.L_max;
    const int64_t R = pl.R;
    Bump bp(ws, ws_bytes);
    float* frames = bp.f(R * 400); float* spec = bp.f(R * 402); float* power = bp.f(R * 204); float* mel = bp.f(R * 40);
    float* pre = bp.f(R * 1024); float* hseq[2] = {bp.f(R * 256), bp.f(R * 256)};
    float* hf[2] = {bp.f((int64_t)Bp * 256), bp.f((int64_t)Bp * 256)}; float* cf = bp.f((int64_t)Bp * 256);
    float* hlast = bp.f((int64_t)B * 256); float* lin = bp.f((int64_t)B * 256);
    int32_t* table = reinterpret_cast<int32_t*>(bp.f(spk_table_words(B, L)));
    L2S_REQUIRE(!bp.overflow && ws_bytes >= spk_ws_bytes_packed(pl, B), "speaker-encoder workspace too small (l2s_speaker_workspace_bytes_packed)");
    HostTable t;
    const SpkTable st = spk_table(t, B, L, pl.step_row0.data());
    SpkRank* hr = t.host<SpkRank>(st.ranks);
    for (int r = 0; r < B; ++r) { const int b = pl.order[r]; hr[r] = SpkRank{offsets[b], (int32_t)n_samples[b], b}; }
    if (t.upload(table, s)) return 1;
    const SpkRank* ranks = table_seg<SpkRank>(table, st.ranks);
    const int* row0 = table + st.row0;
    if (launch_frame_window_packed(audio, ranks, row0, B, L, 400, 160, w.spk_window, frames, s)) return 1;
    if (launch_gemm1(gemm_plain(frames, 400, w.spk_dft, spec, 402, (int)R, 402, 400), s, "spk_dft_gemm")) return 1;
    L2S_SPK_TAP(0, spec, R * 402);
    if (launch_power(spec, 402, R, 201, power, 204, s)) return 1;
    L2S_SPK_TAP(1, power, R * 204);
    if (launch_gemm1(gemm_plain(power, 204, w.spk_fbT, mel, 40, (int)R, 40, 204), s, "spk_mel_gemm")) return 1;
    L2S_SPK_TAP(2, mel, R * 40);
    const float* x = mel;
    int xin = 40;
    for (int l = 0; l < 3; ++l) {
        GemmP g = gemm_plain(x, xin, w.spk_ih[l].W, pre, 1024, (int)R, 1024, xin);
        g.shift = w.spk_ih[l].shift;
        if (launch_gemm1(g, s, "spk_lstm_input_gemm")) return 1;
        if (launch_fill(hf[0], (int64_t)Bp * 256, 0.f, s)) return 1;
        if (launch_fill(hf[1], (int64_t)Bp * 256, 0.f, s)) return 1;
        if (launch_fill(cf, (int64_t)Bp * 256, 0.f, s)) return 1;
        float* out = hseq[l & 1];
        for (int t = 0; t < L; ++t) {      // the unmasked cell launch on the step's own rows: state rows 0 .. step_rows[t] - 1 are the clips of those ranks
            const SkinnyBatch sb = spk_lstm_step(w, l, pl.step_rows[t], hf[t & 1], hf[(t & 1) ^ 1], cf, pre + (int64_t)pl.step_row0[t] * 1024, 1024,
                                                 out + (int64_t)pl.step_row0[t] * 256, 256);
            if (launch_skinny(sb, s, "spk_lstm_step", m->opt)) return 1;
        }
        L2S_SPK_TAP(3 + l, out, R * 256);
        x = out;
        xin = 256;
    }
    // embeds = normalize(relu(linear(h_last))), h_last = top layer's output at each clip's own last frame, gathered into call order
    if (launch_spk_last_hidden(x, ranks, row0, B, hlast, s)) return 1;
    GemmP g = gemm_plain(hlast, 256, w.spk_linear.W, lin, 256, B, 256, 256);
    g.shift = w.spk_linear.shift; g.act = ACT_RELU;
    if (launch_gemm1(g, s, "spk_linear_gemm")) return 1;
    L2S_SPK_TAP(6, lin, (int64_t)B * 256);
    return launch_pool_norm_cat(lin, B, 1, 256, nullptr, 0, 1, nullptr, 0, emb, s);
}

// everything that can be refused is refused here, before the first launch: the outputs of a failed call are untouched
static int speaker_packed_entry(l2s_model* m, const float* audio, const int64_t* offsets, const int64_t* n_samples, int B, float* emb, void* ws, int64_t ws_bytes,
                                hipStream_t s L2S_SPK_TAPS_ARG) {
    L2S_REQUIRE(audio && offsets && n_samples && emb && ws, "l2s speaker packed: null argument");
    SpkPlan pl;
    if (spk_packed_plan(n_samples, B, pl)) return 1;
    for (int b = 0; b < B; ++b)
        if (offsets[b] < 0) { set_error("l2s speaker packed: offsets[" + std::to_string(b) + "] = " + std::to_string(offsets[b]) + " is negative"); return 1; }
    L2S_REQUIRE(m && m->finalized, "model not finalized (call l2s_model_finalize)");
    L2S_REQUIRE(m->has_spk, "model holds no speaker_encoder.* weights");
#ifdef L2S_DIAG
    return speaker_packed_run(m, audio, offsets, n_samples, pl, B, emb, ws, ws_bytes, s, taps);
#else
    return speaker_packed_run(m, audio, offsets, n_samples, pl, B, emb, ws, ws_bytes, s);
#endif
}

}  // namespace l2s

// ================================================================================================ C ABI
using namespace l2s;

extern "C" {

int l2s_abi_version(void) { return 2; }
const char* l2s_last_error(void) { return g_err.c_str(); }

int l2s_model_create(l2s_model** out) {
    L2S_REQUIRE(out != nullptr, "null out pointer");
    *out = new l2s_model();
    (*out)->opt = g_default_opt;
    return 0;
}
int l2s_model_set_tensor(l2s_model* m, const char* key, const float* host_data, int64_t numel) {
    L2S_REQUIRE(m && key && host_data && numel >= 0, "bad arguments");
    m->host[key].assign(host_data, host_data + numel);
    m->finalized = false;
    return 0;
}
int l2s_model_finalize(l2s_model* m, void* stream) {
    L2S_REQUIRE(m != nullptr, "null model");
    int rc = pack_model(m, (hipStream_t)stream);
    if (rc == 0) m->host.clear();
    return rc;
}
int l2s_model_destroy(l2s_model* m) {
    if (!m) return 0;
    drop_graphs(m);
    if (m->side) { (void)hipStreamDestroy(m->side); (void)hipEventDestroy(m->ev_in); (void)hipEventDestroy(m->ev_out); }
    for (auto e : m->ev_pool) (void)hipEventDestroy(e);
    free_model_device(m);
    delete m;
    return 0;
}

int l2s_min_T(int T) { int L[4]; return content_lens(T, L); }

// one pass over B rows padded to T whose encoder works on enc_frames frames (B * T, or the frames of a ragged group)
static int64_t path_ws_bytes(int enc_frames, int B, int T, int H, int S) {
    int64_t enc = enc_ws_floats(enc_frames, H), pro = prologue_ws_floats(B, T), dec = decode_ws_floats(B), post = postnet_ws_floats(B, S);
    int64_t io = (int64_t)B * T * 1024 + l2s_state_floats(B, T) + (int64_t)B * S * (NM + 1) + 64 * 8;   // l2s_inference intermediates
    int64_t mx = std::max(std::max(enc, pro), dec + post + 64);      // decode and post-net buffers are live together (overlap)
    return (mx + io) * (int64_t)sizeof(float) + (1 << 16);
}
int64_t l2s_workspace_bytes(int B, int T, int H, int W, int S) {
    (void)W;
    return path_ws_bytes(B * T, B, T, H, S);
}
int64_t l2s_state_floats(int B, int T) { return state_layout(B, T).total; }
int64_t l2s_state_offset(int B, int T, int field) {
    StateLayout s = state_layout(B, T);
    switch (field) {
        case L2S_ST_K: return s.k;
        case L2S_ST_V: return s.v;
        case L2S_ST_CKEY: return s.ckey;
        case L2S_ST_CVAL: return s.cval;
        case L2S_ST_ECELL: return s.ecell;
        case L2S_ST_H: return s.h;
        case L2S_ST_C: return s.c;
        case L2S_ST_ENC: return s.enc;
        case L2S_ST_STOPC: return s.stopc;
        case L2S_ST_VP: return s.vp;
        case L2S_ST_CP: return s.cp;
    }
    return -1;
}

#define L2S_MODEL_READY(m) L2S_REQUIRE((m) && (m)->finalized, "model not finalized (call l2s_model_finalize)")
#define L2S_ENC_READY(m) L2S_MODEL_READY(m); L2S_REQUIRE((m)->has_enc, "model holds no encoder.* weights")
#define L2S_DEC_READY(m) L2S_MODEL_READY(m); L2S_REQUIRE((m)->has_dec, "model holds no decoder.* weights")

int l2s_encoder_fwd(l2s_model* m, const float* video, int B, int T, int H, int W, float* feat, void* ws, int64_t ws_bytes, void* stream) {
    L2S_ENC_READY(m);
    L2S_REQUIRE(video && feat && ws && B > 0 && T > 0, "bad arguments");
    return encoder_run(m, frame_src(video, B), B, T, H, W, nullptr, nullptr, feat, ws, ws_bytes, (hipStream_t)stream);
}

int l2s_normalise_pad_frames(const uint8_t* packed_u8, const int64_t* offsets, const int32_t* frames, int B, int T, int H, int W, float* video,
                             void* stream) {
    L2S_REQUIRE(packed_u8 && offsets && frames && video && B > 0 && T > 0, "bad arguments");
    return launch_normalise_pad(packed_u8, offsets, frames, B, T, H, W, video, (hipStream_t)stream);
}

int l2s_resize_check(const l2s_resize_job* jobs, int n, int64_t packed_bytes, int mode, int B, int T, int oh, int ow) {
    return resize_check(jobs, n, packed_bytes, mode, B, T, oh, ow);
}

int l2s_resize_normalise(const uint8_t* packed_u8, int64_t packed_bytes, const l2s_resize_job* jobs, int n, int mode, int B, int T, int oh, int ow, float* out,
                         void* stream) {
    return launch_resize_normalise(packed_u8, packed_bytes, jobs, n, mode, B, T, oh, ow, out, (hipStream_t)stream);
}

int l2s_align_check(const l2s_align_job* jobs, int n, int64_t packed_bytes) { return align_check(jobs, n, packed_bytes); }

int l2s_align_faces(const uint8_t* packed_in, int64_t packed_bytes, const l2s_align_job* jobs, int n, uint8_t* packed_out, void* stream) {
    return launch_align_faces(packed_in, packed_bytes, jobs, n, packed_out, (hipStream_t)stream);
}

int l2s_build_visual(const float* feat, const float* emb, int B, int T, float* vis, void* stream) {
    L2S_REQUIRE(feat && emb && vis && B > 0 && T > 0, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (launch_copy_cols(feat, L2S_D_FEAT, 0, vis, L2S_D_VIS, 0, 1, (int64_t)B * T, L2S_D_FEAT, s)) return 1;
    return launch_tile_rows(emb, L2S_D_EMB, vis + L2S_D_FEAT, L2S_D_VIS, B, T, L2S_D_EMB, s);
}

// The staged pair.  Each entry point and its *_masked twin (further down) share one body; masked = the *_masked name: its video_lengths are checked, and
// the call writes its own length table at the front of its workspace (l2s_workspace_bytes_masked)
static int staged_lens(const int32_t* video_lengths, int B, int T, void*& ws, int64_t& ws_bytes, hipStream_t s, ClipLens& lens) {
    if (check_lengths(video_lengths, B, T)) return 1;
    L2S_REQUIRE(ws_bytes > len_table_bytes(B), "workspace too small (l2s_workspace_bytes_masked)");
    lens = {reinterpret_cast<int*>(ws), video_lengths};
    if (launch_len_table(video_lengths, B, lens.dev, s)) return 1;
    ws = (char*)ws + len_table_bytes(B); ws_bytes -= len_table_bytes(B);
    return 0;
}
static int prologue_entry(l2s_model* m, const float* vis, const float* emb, const float* gumbel, int B, int T, float* state, float* content_dis,
                          void* ws, int64_t ws_bytes, void* stream, bool masked, const int32_t* video_lengths) {
    L2S_DEC_READY(m);
    L2S_REQUIRE(vis && emb && gumbel && state && ws && B > 0, "bad arguments");
    ClipLens lens;
    if (masked && staged_lens(video_lengths, B, T, ws, ws_bytes, (hipStream_t)stream, lens)) return 1;
    return prologue_run(m, vis, emb, gumbel, B, T, state, content_dis, ws, ws_bytes, (hipStream_t)stream, lens);
}
int l2s_decoder_prologue(l2s_model* m, const float* vis, const float* emb, const float* gumbel, int B, int T, float* state,
                         float* content_dis, void* ws, int64_t ws_bytes, void* stream) {
    return prologue_entry(m, vis, emb, gumbel, B, T, state, content_dis, ws, ws_bytes, stream, false, nullptr);
}
static int decode_steps_entry(l2s_model* m, float* state, int B, int T, int S, const float* teacher, const uint8_t* teacher_mask, float* mel, float* stop,
                              float* attn, int attn_logits, void* ws, int64_t ws_bytes, void* stream, bool masked, const int32_t* video_lengths) {
    L2S_DEC_READY(m);
    L2S_REQUIRE(state && mel && stop && ws && B > 0, "bad arguments");
    ClipLens lens;
    if (masked && staged_lens(video_lengths, B, T, ws, ws_bytes, (hipStream_t)stream, lens)) return 1;
    return decode_run(m, state, B, T, S, teacher, teacher_mask, mel, stop, attn, attn_logits, ws, ws_bytes, (hipStream_t)stream, true, lens);
}
int l2s_decode_steps(l2s_model* m, float* state, int B, int T, int S, const float* teacher, const uint8_t* teacher_mask, float* mel,
                     float* stop, float* attn, int attn_logits, void* ws, int64_t ws_bytes, void* stream) {
    return decode_steps_entry(m, state, B, T, S, teacher, teacher_mask, mel, stop, attn, attn_logits, ws, ws_bytes, stream, false, nullptr);
}

int l2s_postnet(l2s_model* m, const float* mel, int B, int S, float* mel_post, float* mel_cf, void* ws, int64_t ws_bytes, void* stream) {
    L2S_DEC_READY(m);
    L2S_REQUIRE(mel && mel_post && ws && B > 0 && S > 0, "bad arguments");
    return postnet_run(m, mel, B, S, mel_post, mel_cf, ws, ws_bytes, (hipStream_t)stream);
}

int64_t l2s_speaker_workspace_bytes(int B, int n_samples) { return spk_ws_bytes(B, n_samples); }

int l2s_speaker_encoder_fwd(l2s_model* m, const float* audio, int B, int n_samples, float* emb, void* ws, int64_t ws_bytes, void* stream) {
    L2S_MODEL_READY(m);
    L2S_REQUIRE(m->has_spk, "model holds no speaker_encoder.* weights");
    L2S_REQUIRE(audio && emb && ws && B > 0, "bad arguments");
    return speaker_run(m, audio, B, n_samples, emb, ws, ws_bytes, (hipStream_t)stream);
}

int l2s_speaker_packed_plan(const int64_t* n_samples, int B, int32_t* order, int32_t* step_rows, int32_t* step_row0, int* L_max, int64_t* R) {
    L2S_REQUIRE(order && step_rows && step_row0 && L_max && R, "bad arguments");
    SpkPlan pl;
    if (spk_packed_plan(n_samples, B, pl)) return 1;
    std::copy(pl.order.begin(), pl.order.end(), order);
    std::copy(pl.step_rows.begin(), pl.step_rows.end(), step_rows);
    std::copy(pl.step_row0.begin(), pl.step_row0.end(), step_row0);
    *L_max = pl.L_max; *R = pl.R;
    return 0;
}

int64_t l2s_speaker_workspace_bytes_packed(const int64_t* n_samples, int B) {
    SpkPlan pl;
    if (spk_packed_plan(n_samples, B, pl)) return -1;
    return spk_ws_bytes_packed(pl, B);
}

int l2s_speaker_encoder_packed(l2s_model* m, const float* audio_packed, const int64_t* offsets, const int64_t* n_samples, int B, float* emb, void* ws,
                               int64_t ws_bytes, void* stream) {
    return speaker_packed_entry(m, audio_packed, offsets, n_samples, B, emb, ws, ws_bytes, (hipStream_t)stream);
}

int64_t l2s_face_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H != 160 || W != 160) { set_error("l2s_face_workspace_bytes: faces are 160 x 160 (B > 0)"); return -1; }
    const int64_t f = face_ws_floats(B);
    return f < 0 ? -1 : f * (int64_t)sizeof(float) + (1 << 12);
}

int l2s_face_encoder_fwd(l2s_model* m, const float* faces, int64_t batch_stride, int B, int H, int W, float* proj, float* emb, void* ws, int64_t ws_bytes,
                         void* stream) {
    L2S_MODEL_READY(m);
    L2S_REQUIRE(m->has_face, "model holds no vgg_face.* weights");
    L2S_REQUIRE(H == 160 && W == 160, "the face tower takes 160 x 160 faces");
    L2S_REQUIRE(faces && emb && ws && B > 0 && batch_stride >= (int64_t)3 * H * W, "bad arguments");
    return face_run(m, faces, batch_stride, B, proj, emb, ws, ws_bytes, (hipStream_t)stream, nullptr);
}

int l2s_output_lengths(const float* stop, int B, int S, int64_t* lengths, void* stream) {
    L2S_REQUIRE(stop && lengths && B > 0 && S > 0, "bad arguments");
    return launch_output_lengths(stop, B, S, lengths, (hipStream_t)stream);
}

// What one pass over a batch hands back.  inference(): mel_post + lengths (+ post-softmax attention); forward(tf_ratio) in eval mode
// (decoder.py:320-379): mel_cf, mel_post, stop, attention LOGITS, content_dis.
struct PathOut {
    float* mel_post = nullptr; float* mel_cf = nullptr; float* stop = nullptr; int64_t* lengths = nullptr;
    float* attn = nullptr; int attn_logits = 0; float* content_dis = nullptr;
    // l2s_forward_eval_ragged: the caller's buffer for the decoded row-major mel (B,S,80) - it moves the frames into its own blocks afterwards - and the
    // per-row step counts of the post-net (postnet_run); null when every row has the call's S
    float* mel = nullptr; const EvalTab* ev = nullptr;
};

static int path_run(l2s_model* m, const FrameSrc& video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S,
                    const float* teacher, const uint8_t* teacher_mask, const PathOut& o, void* ws, int64_t ws_bytes, hipStream_t s,
                    const int32_t* video_lengths = nullptr, const RaggedTab* rg = nullptr) {      // rg: the encoder stage of a ragged group (encoder_run)
    X3Scope x3scope(m->opt.infer_bf16 ? 0 : m->opt.gemm_x3);
    Bf16Scope bf16scope(m->opt.infer_bf16);      // the bf16 leg: bf16-operand GEMM / Conv1d kernels instead of the f32 / split-bf16 ones
    Bump bp(ws, ws_bytes);
    const ClipLens lens{video_lengths ? reinterpret_cast<int*>(bp.f(len_table_bytes(B) / 4)) : nullptr, video_lengths};      // the *_masked entry points (l2s_workspace_bytes_masked)
    float* vis = bp.f((int64_t)B * T * 1024);
    float* state = bp.f(l2s_state_floats(B, T));
    float* mel = o.mel ? o.mel : bp.f((int64_t)B * S * NM);
    float* stop = o.stop ? o.stop : bp.f((int64_t)B * S);
    L2S_REQUIRE(!bp.overflow, "workspace too small (l2s_workspace_bytes)");
    void* rest = (char*)ws + bp.off;
    const int64_t rest_bytes = ws_bytes - bp.off;
    if (lens && launch_len_table(video_lengths, B, lens.dev, s)) return 1;
    if (encoder_run(m, video, B, T, H, W, emb, vis, nullptr, rest, rest_bytes, s, rg)) return 1;
    if (prologue_run(m, vis, emb, gumbel, B, T, state, o.content_dis, rest, rest_bytes, s, lens, !teacher)) return 1;
    const bool early = m->opt.early_stop != 0 && !teacher && o.lengths;      // l2s_inference(_multi); l2s_forward_eval's S comes from the target
    const bool plain = !m->opt.overlap_postnet || g_prof_on || m->opt.graph || teacher || o.mel_cf || early || lens;      // "early_stop" and lengths take the plain route
    if (plain) {
        EsMarginScope margin(post_wino_route(m, B, S) ? ES_MARGIN_WINO : ES_MARGIN);      // an early stop leaves the post-net the frames its route reads
        if (decode_run(m, state, B, T, S, teacher, teacher_mask, mel, stop, o.attn, o.attn_logits, rest, rest_bytes, s, early, lens)) return 1;
        if (o.ev && launch_zero_rows_past_s(mel, NM, *o.ev, s)) return 1;      // the frames a shorter batch's rows decoded past their own S: zeros for the post-net's taps
        if (postnet_run(m, mel, B, S, o.mel_post, o.mel_cf, rest, rest_bytes, s, o.ev)) return 1;
    } else {
        // The decode loop is a chain of small latency-bound launches that leaves most CUs idle, and the post-net of frame t
        // only needs mel frames t-10..t+10: run the post-net in time windows on a second stream while later steps decode.
        std::lock_guard<std::mutex> side_lock(m->side_mu);      // the side stream and its events are per model: one chain at a time enqueues on them
        if (side_stream_ready(m)) return 1;
        Bump pbump((char*)rest + align_up(decode_ws_floats(B) * (int64_t)sizeof(float), 256), rest_bytes - align_up(decode_ws_floats(B) * (int64_t)sizeof(float), 256));
        PostBufs pb;
        L2S_REQUIRE(postnet_alloc(pbump, B, S, pb) == 0, "workspace too small (l2s_workspace_bytes)");
        int done[5] = {0, 0, 0, 0, 0};      // frames finished per post-net layer
        size_t ev_used = 0;
        const int chunk = 64, tail = 12;
        std::function<int(int)> on_frames = [&](int n) -> int {
            const bool boundary = (n == S) || (n % chunk == 0 && n < S - tail) || (n == S - tail && S > tail);
            if (!boundary) return 0;
            if (ev_used >= m->ev_pool.size()) {
                hipEvent_t e;
                L2S_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                m->ev_pool.push_back(e);
            }
            hipEvent_t ev = m->ev_pool[ev_used++];
            L2S_CHECK_HIP(hipEventRecord(ev, s));
            L2S_CHECK_HIP(hipStreamWaitEvent(m->side, ev, 0));
            for (int layer = 0; layer < 5; ++layer) {
                const int end = n == S ? S : std::max(done[layer], n - 2 * (layer + 1));
                if (postnet_layer(m->w, layer, mel, pb, o.mel_post, B, S, done[layer], end, m->side, m->opt.gemm_x3_dma != 0)) return 1;
                done[layer] = end;
            }
            return 0;
        };
        // the side stream must not start before earlier work on `s` (previous users of these buffers) is done
        L2S_CHECK_HIP(hipEventRecord(m->ev_in, s));
        L2S_CHECK_HIP(hipStreamWaitEvent(m->side, m->ev_in, 0));
        if (decode_launches(m, state, B, T, S, nullptr, nullptr, mel, stop, o.attn, o.attn_logits, rest, rest_bytes, s, m->opt.fold != 0 && m->folded_valid, &on_frames)) return 1;
        L2S_CHECK_HIP(hipEventRecord(m->ev_out, m->side));
        L2S_CHECK_HIP(hipStreamWaitEvent(s, m->ev_out, 0));
    }
    if (o.lengths && launch_output_lengths(stop, B, S, o.lengths, s)) return 1;
    // option "early_stop": the frames every caller drops (j >= lengths[b]) come back as exact zeros - the reference's output masked by its own lengths
    if (early && launch_mask_by_lengths(o.lengths, B, S, T, o.mel_post, o.attn, s)) return 1;
    return 0;
}

static int inference_entry(l2s_model* m, const float* video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S, float* mel_post,
                           int64_t* lengths, float* attn, void* ws, int64_t ws_bytes, void* stream, bool masked, const int32_t* video_lengths) {
    L2S_ENC_READY(m);
    L2S_DEC_READY(m);
    L2S_REQUIRE(video && emb && gumbel && mel_post && lengths && ws && B > 0, "bad arguments");
    if (masked && check_lengths(video_lengths, B, T)) return 1;
    PathOut o;
    o.mel_post = mel_post; o.lengths = lengths; o.attn = attn;
    return path_run(m, frame_src(video, B), emb, gumbel, B, T, H, W, S, nullptr, nullptr, o, ws, ws_bytes, (hipStream_t)stream, video_lengths);
}
int l2s_inference(l2s_model* m, const float* video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S,
                  float* mel_post, int64_t* lengths, float* attn, void* ws, int64_t ws_bytes, void* stream) {
    return inference_entry(m, video, emb, gumbel, B, T, H, W, S, mel_post, lengths, attn, ws, ws_bytes, stream, false, nullptr);
}
// Lip2Speech.forward(..., tf_ratio) in eval() mode / under no_grad (model.py:23-40 + decoder.py:320-379; what evaluate.py:38 runs at
// tf_ratio = 1): S = mels.shape[2] steps, attention LOGITS out, optional teacher frames for the steps the caller's scheduled-sampling
// draws selected.  One launch chain, like l2s_inference.
static int forward_eval_entry(l2s_model* m, const float* video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S, const float* teacher,
                              const uint8_t* teacher_mask, float* mel_cf, float* mel_post, float* stop, float* attn_logits, float* content_dis, void* ws,
                              int64_t ws_bytes, void* stream, bool masked, const int32_t* video_lengths) {
    L2S_ENC_READY(m);
    L2S_DEC_READY(m);
    L2S_REQUIRE(video && emb && gumbel && mel_post && stop && ws && B > 0, "bad arguments");
    L2S_REQUIRE((teacher != nullptr) == (teacher_mask != nullptr), "teacher frames and teacher_mask come together");
    if (masked && check_lengths(video_lengths, B, T)) return 1;
    PathOut o;
    o.mel_post = mel_post; o.mel_cf = mel_cf; o.stop = stop; o.attn = attn_logits; o.attn_logits = 1; o.content_dis = content_dis;
    return path_run(m, frame_src(video, B), emb, gumbel, B, T, H, W, S, teacher, teacher_mask, o, ws, ws_bytes, (hipStream_t)stream, video_lengths);
}
int l2s_forward_eval(l2s_model* m, const float* video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S,
                     const float* teacher, const uint8_t* teacher_mask, float* mel_cf, float* mel_post, float* stop, float* attn_logits,
                     float* content_dis, void* ws, int64_t ws_bytes, void* stream) {
    return forward_eval_entry(m, video, emb, gumbel, B, T, H, W, S, teacher, teacher_mask, mel_cf, mel_post, stop, attn_logits, content_dis, ws, ws_bytes, stream, false, nullptr);
}

// ---- per-clip video lengths: row b of a zero-padded batch computes what clip b computes alone at T = len_b (include/l2s.h).  New entry points only: the
// launch-per-phase route whatever "use_graph" says, or (options "persist_decode" and "persist_masked", free-running, persist_envelope) the persistent forms.
int64_t l2s_workspace_bytes_masked(int B, int T, int H, int W, int S) { return l2s_workspace_bytes(B, T, H, W, S) + len_table_bytes(B) + 256; }

int l2s_masked_bilstm_plan(const int32_t* video_lengths, int B, int T, int32_t* capture_steps, int32_t* reset_steps, int* n_capture, int* n_reset) {
    L2S_REQUIRE(B > 0 && capture_steps && reset_steps && n_capture && n_reset, "bad arguments");
    if (check_lengths(video_lengths, B, T)) return 1;
    std::vector<int> cap, rst;
    masked_bilstm_plan(video_lengths, B, T, cap, rst);
    std::copy(cap.begin(), cap.end(), capture_steps);
    std::copy(rst.begin(), rst.end(), reset_steps);
    *n_capture = (int)cap.size(); *n_reset = (int)rst.size();
    return 0;
}

int l2s_inference_masked(l2s_model* m, const float* video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S,
                         float* mel_post, int64_t* lengths, float* attn, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths) {
    return inference_entry(m, video, emb, gumbel, B, T, H, W, S, mel_post, lengths, attn, ws, ws_bytes, stream, true, video_lengths);
}
int l2s_forward_eval_masked(l2s_model* m, const float* video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S,
                            const float* teacher, const uint8_t* teacher_mask, float* mel_cf, float* mel_post, float* stop, float* attn_logits,
                            float* content_dis, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths) {
    return forward_eval_entry(m, video, emb, gumbel, B, T, H, W, S, teacher, teacher_mask, mel_cf, mel_post, stop, attn_logits, content_dis, ws, ws_bytes, stream, true, video_lengths);
}
int l2s_decoder_prologue_masked(l2s_model* m, const float* vis, const float* emb, const float* gumbel, int B, int T, float* state,
                                float* content_dis, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths) {
    return prologue_entry(m, vis, emb, gumbel, B, T, state, content_dis, ws, ws_bytes, stream, true, video_lengths);
}
int l2s_decode_steps_masked(l2s_model* m, float* state, int B, int T, int S, const float* teacher, const uint8_t* teacher_mask, float* mel,
                            float* stop, float* attn, int attn_logits, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths) {
    return decode_steps_entry(m, state, B, T, S, teacher, teacher_mask, mel, stop, attn, attn_logits, ws, ws_bytes, stream, true, video_lengths);
}

// Grouped inference: the G batches are rows g*B .. g*B+B-1 of ONE launch chain on ONE weight blob.  Every kernel of the path is row-independent
// (a row's arithmetic does not depend on how many rows share the launch), so each batch's results are bit-identical to l2s_inference on it.
int64_t l2s_workspace_bytes_multi(int G, int B, int T, int H, int W, int S) {
    int L[4];
    const int64_t rows = (int64_t)G * B;
    return l2s_workspace_bytes((int)rows, T, H, W, S) + align_up(rows * L2S_D_EMB * 4, 256) + align_up(rows * content_lens(T, L) * VOC * 4, 256) +
           align_up(rows * S * NM * 4, 256);      // + the gathered teacher frames of l2s_forward_eval_multi
}
int l2s_inference_multi(l2s_model* m, int G, const float* const* video, const float* const* emb, const float* const* gumbel, int B, int T, int H,
                        int W, int S, float* mel_post, int64_t* lengths, float* attn, void* ws, int64_t ws_bytes, void* stream) {
    L2S_ENC_READY(m);
    L2S_DEC_READY(m);
    L2S_REQUIRE(G >= 1 && G <= L2S_MAX_GROUP && video && emb && gumbel && mel_post && lengths && ws && B > 0, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    int L[4];
    const int mT = content_lens(T, L);
    Bump bp(ws, ws_bytes);
    float* emb_all = bp.f((int64_t)G * B * L2S_D_EMB);
    float* gum_all = bp.f((int64_t)G * B * mT * VOC);
    L2S_REQUIRE(!bp.overflow, "workspace too small (l2s_workspace_bytes_multi)");
    FrameSrc src{};
    src.per = B;
    for (int g = 0; g < G; ++g) {
        L2S_REQUIRE(video[g] && emb[g] && gumbel[g], "null batch pointer");
        src.p[g] = video[g];
        // the small per-batch operands are gathered (G x 32 KB + G x 256 KB at B = 32); the frames (102.6 MB per batch) are read in place
        L2S_CHECK_HIP(hipMemcpyAsync(emb_all + (int64_t)g * B * L2S_D_EMB, emb[g], sizeof(float) * B * L2S_D_EMB, hipMemcpyDeviceToDevice, s));
        L2S_CHECK_HIP(hipMemcpyAsync(gum_all + (int64_t)g * B * mT * VOC, gumbel[g], sizeof(float) * B * mT * VOC, hipMemcpyDeviceToDevice, s));
    }
    X3Group x3group(G);
    PathOut o;
    o.mel_post = mel_post; o.lengths = lengths; o.attn = attn;
    return path_run(m, src, emb_all, gum_all, G * B, T, H, W, S, nullptr, nullptr, o, (char*)ws + bp.off, ws_bytes - bp.off, s);
}

// The grouped form: G batches of the evaluate loop as rows of ONE launch chain (see l2s_inference_multi).  The batches of a group share S
// and the scheduled-sampling mask (at tf_ratio = 1 - evaluate.py - no step is ever teacher-forced, so any G batches group).
int l2s_forward_eval_multi(l2s_model* m, int G, const float* const* video, const float* const* emb, const float* const* gumbel,
                           const float* const* teacher, const uint8_t* teacher_mask, int B, int T, int H, int W, int S, float* mel_cf,
                           float* mel_post, float* stop, float* attn_logits, float* content_dis, void* ws, int64_t ws_bytes, void* stream) {
    L2S_ENC_READY(m);
    L2S_DEC_READY(m);
    L2S_REQUIRE(G >= 1 && G <= L2S_MAX_GROUP && video && emb && gumbel && mel_post && stop && ws && B > 0, "bad arguments");
    L2S_REQUIRE((teacher != nullptr) == (teacher_mask != nullptr), "teacher frames and teacher_mask come together");
    L2S_REQUIRE(S >= 1 && S <= L2S_MAX_STEPS, "S must be in [1, 300] (positional table)");
    hipStream_t s = (hipStream_t)stream;
    int L[4];
    const int mT = content_lens(T, L);
    Bump bp(ws, ws_bytes);
    float* emb_all = bp.f((int64_t)G * B * L2S_D_EMB);
    float* gum_all = bp.f((int64_t)G * B * mT * VOC);
    float* teach_all = teacher ? bp.f((int64_t)G * B * S * NM) : nullptr;
    L2S_REQUIRE(!bp.overflow, "workspace too small (l2s_workspace_bytes_multi)");
    FrameSrc src{};
    src.per = B;
    for (int g = 0; g < G; ++g) {
        L2S_REQUIRE(video[g] && emb[g] && gumbel[g] && (!teacher || teacher[g]), "null batch pointer");
        src.p[g] = video[g];
        L2S_CHECK_HIP(hipMemcpyAsync(emb_all + (int64_t)g * B * L2S_D_EMB, emb[g], sizeof(float) * B * L2S_D_EMB, hipMemcpyDeviceToDevice, s));
        L2S_CHECK_HIP(hipMemcpyAsync(gum_all + (int64_t)g * B * mT * VOC, gumbel[g], sizeof(float) * B * mT * VOC, hipMemcpyDeviceToDevice, s));
        if (teacher)
            L2S_CHECK_HIP(hipMemcpyAsync(teach_all + (int64_t)g * B * S * NM, teacher[g], sizeof(float) * B * S * NM, hipMemcpyDeviceToDevice, s));
    }
    X3Group x3group(G);
    PathOut o;
    o.mel_post = mel_post; o.mel_cf = mel_cf; o.stop = stop; o.attn = attn_logits; o.attn_logits = 1; o.content_dis = content_dis;
    return path_run(m, src, emb_all, gum_all, G * B, T, H, W, S, teach_all, teacher_mask, o, (char*)ws + bp.off, ws_bytes - bp.off, s);
}

// ---- ragged groups: G padded batches, each with its own B_g and T_g, as rows of ONE launch chain; every clip decoded as it would be alone, the encoder
// on the real frames only (include/l2s.h).  The decoder stages are those of ONE masked call of N = sum B_g clips padded to Tmax = max T_g.
static int ragged_plan(int G, const int32_t* batch_B, const int32_t* batch_T, const int32_t* video_lengths, std::vector<RaggedClip>& clips, RaggedTab& rg) {
    L2S_REQUIRE(batch_B && batch_T, "l2s ragged: batch_B / batch_T is null");
    if (G < 1 || G > L2S_MAX_GROUP) { set_error("l2s ragged: G = " + std::to_string(G) + " is outside [1, L2S_MAX_GROUP = " + std::to_string(L2S_MAX_GROUP) + "]"); return 1; }
    int64_t N = 0;
    int Tmax = 0;
    for (int g = 0; g < G; ++g) {
        if (batch_B[g] < 1) { set_error("l2s ragged: batch " + std::to_string(g) + " has B = " + std::to_string(batch_B[g]) + " clips"); return 1; }
        if (batch_T[g] < 7 || batch_T[g] > L2S_MAX_STEPS) {
            set_error("l2s ragged: batch " + std::to_string(g) + " has T = " + std::to_string(batch_T[g]) + ", outside [7, " + std::to_string(L2S_MAX_STEPS) + "]");
            return 1;
        }
        N += batch_B[g];
        Tmax = std::max(Tmax, (int)batch_T[g]);
    }
    if (N > L2S_MAX_RAGGED_CLIPS) { set_error("l2s ragged: N = " + std::to_string(N) + " clips exceed L2S_MAX_RAGGED_CLIPS = " + std::to_string(L2S_MAX_RAGGED_CLIPS)); return 1; }
    clips.clear();
    rg = RaggedTab{};
    rg.N = (int)N; rg.Tmax = Tmax;
    if (!video_lengths) return 0;      // the workspace query: shapes only
    for (int g = 0; g < G; ++g)
        for (int r = 0; r < batch_B[g]; ++r) {
            const int c = (int)clips.size(), len = video_lengths[c];
            if (len < 7 || len > batch_T[g]) {
                set_error("l2s ragged: video_lengths[" + std::to_string(c) + "] = " + std::to_string(len) + " (batch " + std::to_string(g) + ", row " + std::to_string(r) +
                          ") is outside [7, T = " + std::to_string(batch_T[g]) + "]");
                return 1;
            }
            clips.push_back(RaggedClip{g, r, batch_T[g], len, rg.NF, rg.NP});
            rg.NF += len; rg.NP += (len + 1) / 2;
        }
    return 0;
}

int l2s_ragged_plan(int G, const int32_t* batch_B, const int32_t* batch_T, const int32_t* video_lengths, int32_t* frame0, int32_t* pair0, int* N, int* Tmax) {
    L2S_REQUIRE(video_lengths && frame0 && pair0 && N && Tmax, "bad arguments");
    std::vector<RaggedClip> clips;
    RaggedTab rg;
    if (ragged_plan(G, batch_B, batch_T, video_lengths, clips, rg)) return 1;
    for (int c = 0; c < rg.N; ++c) { frame0[c] = clips[c].frame0; pair0[c] = clips[c].pair0; }
    frame0[rg.N] = rg.NF; pair0[rg.N] = rg.NP;
    *N = rg.N; *Tmax = rg.Tmax;
    return 0;
}

int64_t l2s_workspace_bytes_ragged(int G, const int32_t* batch_B, const int32_t* batch_T, int H, int W, int S) {
    (void)W;
    std::vector<RaggedClip> clips;
    RaggedTab rg;
    if (ragged_plan(G, batch_B, batch_T, nullptr, clips, rg)) return -1;
    int64_t frames = 0, pairs = 0;      // the worst case: every frame real
    for (int g = 0; g < G; ++g) { frames += (int64_t)batch_B[g] * batch_T[g]; pairs += (int64_t)batch_B[g] * ((batch_T[g] + 1) / 2); }
    int L[4];
    return path_ws_bytes((int)frames, rg.N, rg.Tmax, H, S) + len_table_bytes(rg.N) + 256 + align_up((int64_t)rg.N * L2S_D_EMB * 4, 256) +
           align_up((int64_t)rg.N * content_lens(rg.Tmax, L) * VOC * 4, 256) + align_up(ragged_table_words(rg.N) * 4, 256) + align_up(pairs * 4, 256);
}

// What the two ragged entry points refuse beyond the plan, before the first launch (`fn` names the entry point in the message), and the frame sources
static int ragged_refuse(l2s_model* m, const char* fn, int G, const float* const* video, const float* const* emb, const float* const* gumbel, int H, int W,
                         FrameSrc& src) {
    const std::string f(fn);
    L2S_REQUIRE(!m->opt.infer_bf16, f + ": option \"infer_bf16\" is set - the ragged front-end exists in the default form only");
    L2S_REQUIRE(m->opt.frontend_x3 == 3, f + ": option \"frontend_x3\" is not 3 - the ragged front-end exists in the default form only");
    L2S_REQUIRE(!m->opt.frontend_solo, f + ": option \"frontend_solo\" is set - the ragged front-end exists in the default form only");
    L2S_REQUIRE(H == W && (H == 96 || H == 88), "frontend supports 96x96 and 88x88 mouth crops");
    src = FrameSrc{};
    for (int g = 0; g < G; ++g) {
        if (!video[g] || !emb[g] || !gumbel[g] || (reinterpret_cast<uintptr_t>(video[g]) & 15u)) {
            set_error(f + ": batch " + std::to_string(g) + ": null pointer, or video not 16-byte aligned");
            return 1;
        }
        src.p[g] = video[g];
    }
    return 0;
}

// The operands of a ragged group at the front of its workspace: the gathered embeddings and Gumbel rows, the clip table and the front-end's pair map
// (rg.clips / rg.pair_clip are set).  bp is left behind them.
static int ragged_gather(int G, const float* const* emb, const float* const* gumbel, const int32_t* batch_B, const int32_t* batch_T,
                         const std::vector<RaggedClip>& clips, RaggedTab& rg, Bump& bp, float*& emb_all, float*& gum_all, hipStream_t s) {
    int L[4];
    const int mT = content_lens(rg.Tmax, L), N = rg.N;
    emb_all = bp.f((int64_t)N * L2S_D_EMB);
    gum_all = bp.f((int64_t)N * mT * VOC);
    RaggedClip* clips_dev = reinterpret_cast<RaggedClip*>(bp.f(ragged_table_words(N)));
    int* pair_clip = reinterpret_cast<int*>(bp.f(rg.NP));
    L2S_REQUIRE(!bp.overflow, "workspace too small (l2s_workspace_bytes_ragged)");
    // the small per-batch operands are gathered, the frames are read in place.  Clip c owns mT Gumbel rows of the group's buffer and uses the first
    // min_T(len) of them (a masked call's rule); its batch supplied min_T(T_g) <= mT rows per clip: one strided copy per batch, the rest zeros
    L2S_CHECK_HIP(hipMemsetAsync(gum_all, 0, sizeof(float) * (size_t)N * mT * VOC, s));
    for (int g = 0, c0 = 0; g < G; c0 += batch_B[g], ++g) {
        const size_t rowb = sizeof(float) * (size_t)content_lens(batch_T[g], L) * VOC;
        L2S_CHECK_HIP(hipMemcpyAsync(emb_all + (int64_t)c0 * L2S_D_EMB, emb[g], sizeof(float) * batch_B[g] * L2S_D_EMB, hipMemcpyDeviceToDevice, s));
        L2S_CHECK_HIP(hipMemcpy2DAsync(gum_all + (int64_t)c0 * mT * VOC, sizeof(float) * (size_t)mT * VOC, gumbel[g], rowb, rowb, batch_B[g], hipMemcpyDeviceToDevice, s));
    }
    if (launch_ragged_table(clips.data(), N, clips_dev, pair_clip, s)) return 1;
    rg.clips = clips_dev; rg.pair_clip = pair_clip;
    return 0;
}

int l2s_inference_ragged(l2s_model* m, int G, const float* const* video, const float* const* emb, const float* const* gumbel, const int32_t* batch_B,
                         const int32_t* batch_T, const int32_t* video_lengths, int H, int W, int S, float* mel_post, int64_t* lengths, float* attn, void* ws,
                         int64_t ws_bytes, void* stream) {
    L2S_ENC_READY(m);
    L2S_DEC_READY(m);
    L2S_REQUIRE(video && emb && gumbel && video_lengths && mel_post && lengths && ws, "bad arguments");
    // everything that can be refused is refused here, before the first launch: the outputs of a failed call are untouched
    std::vector<RaggedClip> clips;
    RaggedTab rg;
    if (ragged_plan(G, batch_B, batch_T, video_lengths, clips, rg)) return 1;
    FrameSrc src;
    if (ragged_refuse(m, "l2s_inference_ragged", G, video, emb, gumbel, H, W, src)) return 1;
    L2S_REQUIRE(S >= 1 && S <= L2S_MAX_STEPS, "S must be in [1, 300] (positional table)");
    hipStream_t s = (hipStream_t)stream;
    Bump bp(ws, ws_bytes);
    float *emb_all, *gum_all;
    if (ragged_gather(G, emb, gumbel, batch_B, batch_T, clips, rg, bp, emb_all, gum_all, s)) return 1;
    // the row-count-dependent kernel choices are made on the whole call's rows, as for one masked call of N clips: "rows of one batch" has no meaning here
    X3Group x3group(1);
    PathOut o;
    o.mel_post = mel_post; o.lengths = lengths; o.attn = attn;
    return path_run(m, src, emb_all, gum_all, rg.N, rg.Tmax, H, W, S, nullptr, nullptr, o, (char*)ws + bp.off, ws_bytes - bp.off, s, video_lengths, &rg);
}

// ---- the evaluate-shaped ragged group: every batch also has its own step count S_g (forward() decodes melspecs.shape[2] steps; include/l2s.h).  Free-running
// only.  The chain decodes all N rows for Smax = max S_g steps into staging buffers at pitch Smax / Tmax (the steps j >= S_g of a shorter batch's rows are
// wasted work), the post-net sees zeros past every row's own S_g (postnet_run), and small kernels move the rows into the packed per-batch blocks.
struct EvalPlan { std::vector<int64_t> mel_off, stop_off, attn_off, dis_off; int Smax = 0; bool uneven = false; };
static int eval_ragged_plan(int G, const int32_t* batch_B, const int32_t* batch_T, const int32_t* batch_S, const int32_t* video_lengths,
                            std::vector<RaggedClip>& clips, RaggedTab& rg, EvalPlan& pl) {
    if (ragged_plan(G, batch_B, batch_T, video_lengths, clips, rg)) return 1;
    L2S_REQUIRE(batch_S, "l2s ragged: batch_S is null");
    pl = EvalPlan{};
    pl.mel_off.assign(1, 0); pl.stop_off.assign(1, 0); pl.attn_off.assign(1, 0); pl.dis_off.assign(1, 0);
    int L[4];
    for (int g = 0; g < G; ++g) {
        const int64_t B = batch_B[g], T = batch_T[g], S = batch_S[g];
        if (S < 1 || S > L2S_MAX_STEPS) {
            set_error("l2s ragged: batch " + std::to_string(g) + " has S = " + std::to_string(S) + ", outside [1, " + std::to_string(L2S_MAX_STEPS) + "]");
            return 1;
        }
        pl.Smax = std::max(pl.Smax, (int)S);
        pl.mel_off.push_back(pl.mel_off.back() + B * NM * S);
        pl.stop_off.push_back(pl.stop_off.back() + B * S);
        pl.attn_off.push_back(pl.attn_off.back() + B * S * T);
        pl.dis_off.push_back(pl.dis_off.back() + B * content_lens((int)T, L) * VOC);
    }
    for (int g = 0; g < G; ++g) pl.uneven = pl.uneven || batch_S[g] != pl.Smax;
    return 0;
}

int l2s_forward_eval_ragged_plan(int G, const int32_t* batch_B, const int32_t* batch_T, const int32_t* batch_S, int64_t* mel_off, int64_t* stop_off,
                                 int64_t* attn_off, int64_t* dis_off, int* N, int* Tmax, int* Smax) {
    L2S_REQUIRE(mel_off && stop_off && attn_off && dis_off && N && Tmax && Smax, "bad arguments");
    std::vector<RaggedClip> clips;
    RaggedTab rg;
    EvalPlan pl;
    if (eval_ragged_plan(G, batch_B, batch_T, batch_S, nullptr, clips, rg, pl)) return 1;
    std::copy(pl.mel_off.begin(), pl.mel_off.end(), mel_off);
    std::copy(pl.stop_off.begin(), pl.stop_off.end(), stop_off);
    std::copy(pl.attn_off.begin(), pl.attn_off.end(), attn_off);
    std::copy(pl.dis_off.begin(), pl.dis_off.end(), dis_off);
    *N = rg.N; *Tmax = rg.Tmax; *Smax = pl.Smax;
    return 0;
}

// the staging buffers of l2s_forward_eval_ragged behind the ragged group's own workspace: the row-major mel, the stop logits, the channel-first mel_post,
// the attention logits and the content distribution at the staging pitches, and the step table
static int64_t eval_ragged_staging_bytes(int N, int Tmax, int Smax) {
    int L[4];
    const int64_t rows = (int64_t)N * Smax;
    return 2 * align_up(rows * NM * 4, 256) + align_up(rows * 4, 256) + align_up(rows * Tmax * 4, 256) +
           align_up((int64_t)N * content_lens(Tmax, L) * VOC * 4, 256) + align_up(eval_table_words(N) * 4, 256);
}

int64_t l2s_workspace_bytes_eval_ragged(int G, const int32_t* batch_B, const int32_t* batch_T, const int32_t* batch_S, int H, int W) {
    std::vector<RaggedClip> clips;
    RaggedTab rg;
    EvalPlan pl;
    if (eval_ragged_plan(G, batch_B, batch_T, batch_S, nullptr, clips, rg, pl)) return -1;
    return l2s_workspace_bytes_ragged(G, batch_B, batch_T, H, W, pl.Smax) + eval_ragged_staging_bytes(rg.N, rg.Tmax, pl.Smax);
}

int l2s_forward_eval_ragged(l2s_model* m, int G, const float* const* video, const float* const* emb, const float* const* gumbel, const int32_t* batch_B,
                            const int32_t* batch_T, const int32_t* batch_S, const int32_t* video_lengths, int H, int W, float* mel_cf, float* mel_post,
                            float* stop, float* attn_logits, float* content_dis, void* ws, int64_t ws_bytes, void* stream) {
    L2S_ENC_READY(m);
    L2S_DEC_READY(m);
    L2S_REQUIRE(video && emb && gumbel && video_lengths && mel_post && stop && ws, "bad arguments");
    // everything that can be refused is refused here, before the first launch: the outputs of a failed call are untouched
    std::vector<RaggedClip> clips;
    RaggedTab rg;
    EvalPlan pl;
    if (eval_ragged_plan(G, batch_B, batch_T, batch_S, video_lengths, clips, rg, pl)) return 1;
    FrameSrc src;
    if (ragged_refuse(m, "l2s_forward_eval_ragged", G, video, emb, gumbel, H, W, src)) return 1;
    hipStream_t s = (hipStream_t)stream;
    int L[4];
    const int N = rg.N, Tmax = rg.Tmax, Smax = pl.Smax, mTmax = content_lens(Tmax, L);
    Bump bp(ws, ws_bytes);
    float* mel_rm = bp.f((int64_t)N * Smax * NM);
    float* post_st = bp.f((int64_t)N * NM * Smax);
    float* stop_st = bp.f((int64_t)N * Smax);
    float* attn_st = attn_logits ? bp.f((int64_t)N * Smax * Tmax) : nullptr;
    float* dis_st = content_dis ? bp.f((int64_t)N * mTmax * VOC) : nullptr;
    EvalClip* ev_dev = reinterpret_cast<EvalClip*>(bp.f(eval_table_words(N)));
    L2S_REQUIRE(!bp.overflow, "workspace too small (l2s_workspace_bytes_eval_ragged)");
    float *emb_all, *gum_all;
    if (ragged_gather(G, emb, gumbel, batch_B, batch_T, clips, rg, bp, emb_all, gum_all, s)) return 1;
    std::vector<EvalClip> evc;
    evc.reserve(N);
    for (const RaggedClip& k : clips)
        evc.push_back(EvalClip{(int)batch_S[k.g], k.T, k.row, content_lens(k.T, L), (int)pl.mel_off[k.g], (int)pl.stop_off[k.g], (int)pl.attn_off[k.g],
                               (int)pl.dis_off[k.g]});
    if (launch_eval_table(evc.data(), N, ev_dev, s)) return 1;
    const EvalTab ev{ev_dev, N, Smax, Tmax, mTmax};
    // the row-count-dependent kernel choices (the split-bf16 thresholds, POST_TAPSPLIT_ROWS) are made on the rows of the whole call - N * Tmax, N * Smax -
    // as for one masked call of N clips, like l2s_inference_ragged
    X3Group x3group(1);
    PathOut o;
    o.mel_post = post_st; o.stop = stop_st; o.attn = attn_st; o.attn_logits = 1; o.content_dis = dis_st; o.mel = mel_rm;
    o.ev = pl.uneven ? &ev : nullptr;      // every S_g = Smax (GRID: all clips are 3 s): nothing to zero
    if (path_run(m, src, emb_all, gum_all, N, Tmax, H, W, Smax, nullptr, nullptr, o, (char*)ws + bp.off, ws_bytes - bp.off, s, video_lengths, &rg)) return 1;
    if (launch_eval_scatter(EV_MEL_POST, post_st, ev, mel_post, s)) return 1;
    if (launch_eval_scatter(EV_STOP, stop_st, ev, stop, s)) return 1;
    if (mel_cf && launch_eval_mel_cf(mel_rm, ev, mel_cf, s)) return 1;
    if (attn_logits && launch_eval_scatter(EV_ATTN, attn_st, ev, attn_logits, s)) return 1;
    if (content_dis && launch_eval_scatter(EV_DIS, dis_st, ev, content_dis, s)) return 1;
    return 0;
}

// ---- operator-level entry points
#ifdef L2S_DIAG      // operator-level test hooks: libl2s_diag.so (include/l2s_diag.h)
int l2s_op_gemm(const float* A, const float* Wt, const float* scale, const float* shift, const float* actw, float* C, int M, int N,
                int K, int act, void* stream) {
    GemmP p = gemm_plain(A, K, Wt, C, N, M, N, K);
    p.scale = scale; p.shift = shift; p.actw = actw; p.act = act;
    return launch_gemm1(p, (hipStream_t)stream, "op_gemm");
}
int l2s_op_conv1d(const float* X, const float* Wp, const float* scale, const float* shift, const float* actw, float* out, int B,
                  int Tin, int Cin, int Cout, int taps, int stride, int pad, int act, void* stream) {
    ConvW c; c.W = Wp; c.scale = scale; c.shift = shift; c.actw = actw;
    GemmP p = conv_gemm(X, Cin, B, Tin, Cin, c, Cout, taps, stride, pad, out, Cout, act);
    return launch_gemm1(p, (hipStream_t)stream, "op_conv1d");
}
// flags bit 8 of the two operators below: the weight operand as pre-split bf16 planes fetched by LDS-DMA (GemmP::W3; needs N % 256 == 0 and
// K % 16 == 0, ignored otherwise) - derived per call into a scratch buffer the library owns (operator tests and tools; the model paths keep their own)
static void* g_op_planes = nullptr;
static int64_t g_op_planes_bytes = 0;
static std::mutex g_op_planes_mu;
static const void* op_planes(const float* W, int N, int K, hipStream_t s) {
    if (N % 256 || K % 16) return nullptr;
    std::lock_guard<std::mutex> lk(g_op_planes_mu);
    const int64_t need = gemm_planes_bytes(N, K);
    if (need > g_op_planes_bytes) {
        if (g_op_planes) { (void)hipDeviceSynchronize(); (void)hipFree(g_op_planes); g_op_planes = nullptr; g_op_planes_bytes = 0; }
        if (hipMalloc(&g_op_planes, need) != hipSuccess) { g_op_planes = nullptr; return nullptr; }
        g_op_planes_bytes = need;
    }
    return launch_gemm_planes(W, N, K, g_op_planes, s) ? nullptr : g_op_planes;
}
int l2s_op_gemm_ex(const float* A, const float* Wt, const float* scale, const float* shift, const float* actw, float* C, int M, int N,
                   int K, int act, int flags, void* stream) {
    X3Scope x3scope((flags & 1) ? (3 | (flags & 4)) : 0);      // forced; flags bit 4: the narrow tile
    Bf16Scope bf16scope((flags & 2) ? 1 : 0);
    GemmP p = gemm_plain(A, K, Wt, C, N, M, N, K);
    p.scale = scale; p.shift = shift; p.actw = actw; p.act = act;
    if (flags & 8) p.W3 = op_planes(Wt, N, K, (hipStream_t)stream);
    return launch_gemm1(p, (hipStream_t)stream, "op_gemm");
}
int l2s_op_conv1d_ex(const float* X, const float* Wp, const float* scale, const float* shift, const float* actw, float* out, int B,
                     int Tin, int Cin, int Cout, int taps, int stride, int pad, int act, int flags, void* stream) {
    X3Scope x3scope((flags & 1) ? (3 | (flags & 4)) : 0);      // forced; flags bit 4: the narrow tile
    Bf16Scope bf16scope((flags & 2) ? 1 : 0);
    ConvW c; c.W = Wp; c.scale = scale; c.shift = shift; c.actw = actw;
    if (flags & 8) c.W3 = op_planes(Wp, Cout, taps * Cin, (hipStream_t)stream);
    GemmP p = conv_gemm(X, Cin, B, Tin, Cin, c, Cout, taps, stride, pad, out, Cout, act);
    return launch_gemm1(p, (hipStream_t)stream, "op_conv1d");
}
int l2s_op_conv1d_bwd(const float* dZ, const float* X, const float* Wp, float* dX, float* dWp, int B, int Tin, int Cin, int Cout, int taps,
                      int stride, int pad, void* stream) {
    L2S_REQUIRE(dZ && X && Wp, "bad arguments");
    const int Tout = (Tin + 2 * pad - taps) / stride + 1;
    if (dX) {
        L2S_REQUIRE(stride == 1, "dX of a strided Conv1d is computed on the (B*Tout, taps*Cin) view by the caller");
        if (launch_gemm_bwd(bwd_dx(dZ, Cout, Wp, dX, Cin, B, Tout, Tin, Cout, Cin, taps, pad, false), (hipStream_t)stream, "op_conv1d_dx")) return 1;
    }
    if (dWp && launch_gemm_bwd(bwd_dw(dZ, Cout, X, Cin, dWp, B, Tout, Tin, Cout, Cin, taps, stride, pad, false), (hipStream_t)stream, "op_conv1d_dw")) return 1;
    return 0;
}
// one backward GEMM through the launch functions of gemm_bwd.hip: the descriptor's integers go into a BwdGemmP as they stand - the vec rule, the slice
// clipping and every refusal are the launch functions' own
static BwdGemmP bwd_from_desc(const l2s_gemm_bwd_desc& d, const float* A, const float* B, float* C) {
    BwdGemmP p{};
    p.mode = d.mode; p.A = A; p.lda = d.lda; p.B = B; p.ldb = d.ldb; p.C = C; p.ldc = d.ldc; p.M = d.M; p.N = d.N; p.K = d.K;
    p.Tx = d.Tx; p.Tz = d.Tz; p.taps = d.taps; p.stride = d.stride; p.pad = d.pad; p.padp = d.padp; p.Nout = d.Nout; p.Cin = d.Cin;
    p.c_T = d.c_T; p.c_seq_stride = d.c_seq_stride; p.alpha = d.alpha; p.accumulate = d.accumulate;
    return p;
}
int l2s_op_gemm_bwd(const l2s_gemm_bwd_desc* d, const float* A, const float* B, float* C, const l2s_gemm_bwd_desc* d2, const float* A2, const float* B2,
                    float* C2, int splits, float* partials, int bf16, l2s_gemm_bwd_record* ran, void* stream) {
    if (ran) std::memset(ran, 0, sizeof *ran);
    L2S_REQUIRE(d && A && B && C && (d->mode == BWD_DX || d->mode == BWD_DW) && (!d2 || (A2 && B2 && C2)) && splits >= 0, "bad arguments");
    L2S_REQUIRE(d->Tx > 0 && d->Tz > 0 && d->taps > 0 && d->Nout > 0 && d->Cin > 0 && (!d2 || (d2->Tx > 0 && d2->Tz > 0 && d2->taps > 0 && d2->Nout > 0 && d2->Cin > 0)),
                "bad descriptor");
    Bf16Scope bf16scope(bf16 ? 1 : 0);
    gemm_bwd_clear_last_record();
    const BwdGemmP p = bwd_from_desc(*d, A, B, C);
    // the partial matrices a split writes: [slices after clipping][M][N] floats
    const int nkt = (d->K + 31) / 32;
    L2S_REQUIRE(std::min(splits, nkt) <= 1 || partials, "split-K needs a partials buffer");
    int rc;
    if (d2) rc = launch_gemm_bwd_dw_dx(p, splits, partials, bwd_from_desc(*d2, A2, B2, C2), (hipStream_t)stream, "op_gemm_bwd_dw_dx");
    else if (splits >= 1) rc = launch_gemm_bwd_splitk(p, splits, partials, (hipStream_t)stream, "op_gemm_bwd_splitk");
    else rc = launch_gemm_bwd(p, (hipStream_t)stream, "op_gemm_bwd");
    if (ran) *ran = gemm_bwd_last_record();
    return rc;
}
int l2s_op_gemm_bwd_recorder(int cmd, l2s_gemm_bwd_record* out, int cap, int* count) { return gemm_bwd_recorder(cmd, out, cap, count); }
int l2s_op_upload_table(const int32_t* host_words, int64_t n, int32_t* dst, void* stream) {
    L2S_REQUIRE(host_words && dst && n >= 0, "bad arguments");
    return table_upload(dst, host_words, n, (hipStream_t)stream);
}
int l2s_op_table_layout(const int32_t* a, int64_t n_a, const int64_t* b, int64_t n_b, int fill, int32_t* dst, int64_t* off_a, int64_t* off_b, int64_t* words,
                        void* stream) {
    L2S_REQUIRE(n_a >= 0 && n_b >= 0 && off_a && off_b && words && (fill ? a && b : !dst), "bad arguments");
    HostTable t(fill != 0);
    *off_a = t.i32(a, n_a); *off_b = t.i64(b, n_b); *words = t.words();
    return dst ? t.upload(dst, (hipStream_t)stream) : 0;
}
int l2s_op_post_wino_matrices(double* AT, double* G, double* BT) {      // host only: the constants the three transform kernels are compiled with
    L2S_REQUIRE(AT && G && BT, "bad arguments");
    for (int i = 0; i < WINO_M; ++i) for (int p = 0; p < WINO_P; ++p) AT[i * WINO_P + p] = WINO_AT[i][p];
    for (int p = 0; p < WINO_P; ++p) for (int k = 0; k < WINO_R; ++k) G[p * WINO_R + k] = WINO_G[p][k];
    for (int p = 0; p < WINO_P; ++p) for (int i = 0; i < WINO_P; ++i) BT[p * WINO_P + i] = WINO_BT[p][i];
    return 0;
}
int l2s_op_frontend(l2s_model* m, const float* video, int B, int T, int H, int W, float* out, void* stream) {
    L2S_ENC_READY(m);
    FrontendW fe = m->w.fe;
    if (!m->opt.frontend_x3) fe.w3 = nullptr;
    fe.pair = m->opt.frontend_x3 >= 2; fe.pipe = m->opt.frontend_x3 == 3;
    if (!m->opt.infer_bf16) fe.w1 = nullptr;
    return launch_frontend(fe, frame_src(video, B), B, T, H, W, out, (hipStream_t)stream);
}
int l2s_op_face_conv2d(const float* x, int64_t x_bstride, int B, int H, int W, int Cin, const float* w, const float* scale, const float* shift,
                       const float* res, int relu, float* y, int Cout, int kh, int kw, int stride, int ph, int pw, void* stream) {
    L2S_REQUIRE(x && w && scale && shift && y && B > 0 && Cin > 0 && Cout > 0 && kh > 0 && kw > 0 && stride > 0, "bad arguments");
    FaceConvP p{};
    p.x = x; p.x_bstride = x_bstride; p.nchw = x_bstride > 0; p.H = H; p.W = W; p.Cin = Cin; p.ldx = Cin; p.xoff = 0;
    L2S_REQUIRE(!p.nchw || x_bstride >= (int64_t)Cin * H * W, "bad batch stride");
    p.w = w; p.scale = scale; p.shift = shift; p.res = res; p.ldr = Cout; p.relu = relu;
    p.y = y; p.ldy = Cout; p.yoff = 0;
    p.kh = kh; p.kw = kw; p.stride = stride; p.ph = ph; p.pw = pw;
    p.Ho = (H + 2 * ph - kh) / stride + 1; p.Wo = (W + 2 * pw - kw) / stride + 1;
    L2S_REQUIRE(p.Ho > 0 && p.Wo > 0, "empty output");
    p.M = B * p.Ho * p.Wo; p.N = Cout; p.K = kh * kw * Cin;
    int kc;
    const int ns = face_conv_splits(p.Ho * p.Wo, p.K, &kc);
    const int64_t part_floats = ns > 1 ? (int64_t)ns * p.M * p.N : 0;
    float* part = nullptr;
    if (part_floats) L2S_CHECK_HIP(hipMalloc(&part, part_floats * sizeof(float)));
    const int rc = launch_face_conv(p, part, part_floats, (hipStream_t)stream);
    if (part) { (void)hipStreamSynchronize((hipStream_t)stream); (void)hipFree(part); }
    return rc;
}
int l2s_op_face_taps(l2s_model* m, const float* faces, int64_t batch_stride, int B, float* const* taps, float* proj, float* emb, void* ws, int64_t ws_bytes,
                     void* stream) {
    L2S_MODEL_READY(m);
    L2S_REQUIRE(m->has_face, "model holds no vgg_face.* weights");
    L2S_REQUIRE(faces && taps && emb && ws && B > 0 && batch_stride >= (int64_t)3 * 160 * 160, "bad arguments");
    return face_run(m, faces, batch_stride, B, proj, emb, ws, ws_bytes, (hipStream_t)stream, taps);
}
int l2s_op_encoder_taps(l2s_model* m, const float* video, int B, int T, int H, int W, float* const* taps, float* feat, void* ws, int64_t ws_bytes, void* stream) {
    L2S_ENC_READY(m);
    L2S_REQUIRE(video && taps && feat && ws && B > 0 && T > 0, "bad arguments");
    // the published size of the call, not what the encoder's carve happens to need
    L2S_REQUIRE(ws_bytes >= l2s_workspace_bytes(B, T, H, W, 1), "encoder workspace too small");
    return encoder_run(m, frame_src(video, B), B, T, H, W, nullptr, nullptr, feat, ws, ws_bytes, (hipStream_t)stream, nullptr, taps);
}
int l2s_op_speaker_taps(l2s_model* m, const float* audio, int B, int n_samples, float* const* taps, float* emb, void* ws, int64_t ws_bytes, void* stream) {
    L2S_MODEL_READY(m);
    L2S_REQUIRE(m->has_spk, "model holds no speaker_encoder.* weights");
    L2S_REQUIRE(audio && taps && emb && ws && B > 0, "bad arguments");
    return speaker_run(m, audio, B, n_samples, emb, ws, ws_bytes, (hipStream_t)stream, taps);
}
int l2s_op_speaker_taps_packed(l2s_model* m, const float* audio_packed, const int64_t* offsets, const int64_t* n_samples, int B, float* const* taps, float* emb,
                               void* ws, int64_t ws_bytes, void* stream) {
    L2S_REQUIRE(taps, "bad arguments");
    return speaker_packed_entry(m, audio_packed, offsets, n_samples, B, emb, ws, ws_bytes, (hipStream_t)stream, taps);
}

#endif

int l2s_train_set_bn(l2s_model* m, int batch_stats, float momentum) {
    L2S_REQUIRE(m != nullptr && momentum >= 0.f && momentum <= 1.f, "bad arguments");
    m->bn_batch = batch_stats != 0;
    m->bn_momentum = momentum;
    return 0;
}

int l2s_train_refresh_weights(l2s_model* m, void* stream) {
    L2S_REQUIRE(m != nullptr, "null model");
    return refresh_weights(m, (hipStream_t)stream);
}

int l2s_set_option(const char* name, int value) {
    L2S_REQUIRE(name != nullptr, "null option name");
    if (set_option_field(g_default_opt, name, value)) { set_error(std::string("unknown option ") + name); return 1; }
    if (!std::strcmp(name, "persist_decode") && value > 0) pdecode_rearm();
    return 0;
}
int l2s_model_set_option(l2s_model* m, const char* name, int value) {
    L2S_REQUIRE(m != nullptr && name != nullptr, "bad arguments");
    if (set_option_field(m->opt, name, value)) { set_error(std::string("unknown option ") + name); return 1; }
    if (!std::strcmp(name, "persist_decode") && value > 0) pdecode_rearm();      // asking for the persistent forms (again) forgives the device's earlier time-outs
    return 0;
}

#ifdef L2S_DIAG      // chain microbenches, timelines, probes: libl2s_diag.so (include/l2s_diag.h)
// Average duration of the decoder LSTM-cell kernel (the kernel with the largest share of GPU time) measured with ONE pair of HIP
// events around a chain of n_pairs x {layer 0 (K=1536), layer 1 (K=1024)} launches on `stream` - the same launches the decode loop
// issues, on zeroed state.  Per-launch event brackets (l2s_profile_*) add ~1.8 us to a 6 us kernel; this does not.  Synchronises.
int l2s_op_lstm_cell_chain(l2s_model* m, int B, int n_pairs, void* ws, int64_t ws_bytes, void* stream, double* avg_us) {
    L2S_DEC_READY(m);
    L2S_REQUIRE(ws && avg_us && B > 0 && n_pairs > 0, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const Weights& w = m->w;
    const int Bp = pad16(B);
    constexpr int CHAIN_M = 4;                             // the chain has no clips: the content slots of the benchmark's 29-frame clips stand for them
    const StepForm form = step_form(w, m->opt, true, CHAIN_M);      // phases D and E of the folded step under the model's options (decode_step.h)
    Bump bp(ws, ws_bytes);
    const StepBufs d = step_carve(bp, B, true);
    const int cp_pitch = content_hoist_pitch(CHAIN_M);
    float* const cp = form.choist() ? bp.f((int64_t)B * 2048 * cp_pitch) : nullptr;      // the K = 768 form reads its table and its soft-max weights: zeros, like the state
    L2S_REQUIRE(!bp.overflow, "workspace too small");
    for (float* z : {d.h0[0], d.h0[1], d.h1[0], d.h1[1], d.c0, d.c1, d.av}) if (launch_fill(z, (int64_t)Bp * 512, 0.f, s)) return 1;
    for (float* z : {d.cc, d.p2f}) if (launch_fill(z, (int64_t)Bp * 256, 0.f, s)) return 1;
    if (cp && (launch_fill(cp, (int64_t)B * 2048 * cp_pitch, 0.f, s) || launch_fill(d.al, step_alpha_floats(B), 0.f, s))) return 1;
    hipEvent_t e0, e1;
    L2S_CHECK_HIP(hipEventCreate(&e0));
    L2S_CHECK_HIP(hipEventCreate(&e1));
    auto pair = [&](int i) -> int {
        if (launch_skinny(step_phase_d(form, w, d, B, i, cp, cp_pitch), s, "step_lstm_cell", m->opt)) return 1;
        return launch_skinny(step_phase_e(form, w, d, B, i), s, "step_lstm_cell", m->opt);
    };
    for (int i = 0; i < 8; ++i) if (pair(i)) return 1;                   // warm-up
    L2S_CHECK_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < n_pairs; ++i) if (pair(i)) return 1;
    L2S_CHECK_HIP(hipEventRecord(e1, s));
    L2S_CHECK_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    L2S_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_us = (double)ms * 1e3 / (2.0 * n_pairs);
    return 0;
}

/* measurement: ts_dev != NULL routes every skinny launch to the stamped build (8 wall-clock stamps per block into ts_dev); NULL restores */
// measurement: n back-to-back launches of the step's attention kernel alone (same K / V / content state every launch, zero queries) - does a
// clip's 119 KB of K / V stay in its XCD's L2 from one launch to the next when no weight stream runs in between?  (tools/attn_l2_probe.py)
int l2s_op_step_attn_chain(l2s_model* m, float* state, int B, int T, int n_launches, void* ws, int64_t ws_bytes, void* stream) {
    L2S_DEC_READY(m);
    L2S_REQUIRE(state && ws && B >= 1 && n_launches >= 1, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const Weights& w = m->w;
    StateLayout sl = state_layout(B, T);
    const int Bp = pad16(B);
    const StepForm form = step_form(w, m->opt, true, sl.m);      // phase B of the folded step under the model's options (decode_step.h)
    Bump bp(ws, ws_bytes);
    const StepBufs d = step_carve(bp, B, true);
    L2S_REQUIRE(!bp.overflow, "workspace too small");
    if (launch_fill(d.q, (int64_t)B * 512, 0.f, s) || launch_fill(d.qc, (int64_t)B * 256, 0.f, s) || launch_fill(d.p1, (int64_t)Bp * 256, 0.f, s)) return 1;
    for (int i = 0; i < n_launches; ++i) {
        const StepAttn b = step_phase_b(form, w, d, state, sl, B, T, 0, 1, nullptr, 0);
        if (launch_step_attn(b.at, b.pre2, b.pre2_tiles, s, m->opt.attn_lds, m->opt.attn_skip0)) return 1;
    }
    return 0;
}
int l2s_op_skinny_timeline(void* ts_dev) { skinny_set_timeline((unsigned long long*)ts_dev); return 0; }
int l2s_op_attn_timeline(void* ts_dev) { attn_set_timeline((unsigned long long*)ts_dev); return 0; }
int l2s_op_flat_timeline(void* ts_dev) { skinny_set_flat_timeline((unsigned long long*)ts_dev); return 0; }
int l2s_op_pdecode_timeline(void* ts_dev, int step) { pdecode_set_timeline((unsigned long long*)ts_dev, step); return 0; }
int l2s_op_gemm_x3_timeline(void* ts_dev, int block) { gemm_x3_set_timeline((unsigned long long*)ts_dev, block); return 0; }
int l2s_op_fused_unit_timeline(void* ts_dev, int h) { shuffle_set_timeline((unsigned long long*)ts_dev, h); return 0; }
int l2s_op_stamp_log(void* log_dev, int64_t capacity) {
    L2S_REQUIRE(set_stamp_log((unsigned long long*)log_dev, (long long)capacity) == 0, "stamp log: hipMemcpyToSymbol failed");
    return 0;
}

// which kernel launch_skinny picks for a batch described by integers; no device is touched
int l2s_op_skinny_form(l2s_model* m, int count, const int* groups, int B, int chains, int stamped_skinny, int stamped_flat, char* out, int cap) {
    L2S_REQUIRE(m && groups && out && cap > 0 && count >= 1 && count <= SKINNY_MAX_GROUP && B >= 1, "bad arguments");
    static float a[1];      // stands for every operand: the rule asks only whether W3 / a_sum are set
    SkinnyBatch sb{};
    for (int i = 0; i < count; ++i) {
        const int* g = groups + 8 * i;      // nchunks[4], ntiles, epi, W3 set, a_sum set
        SkinnyP& p = sb.p[i];
        for (int j = 0; j < 4; ++j) { p.seg[j] = {a, g[j]}; p.K += 16 * g[j]; }
        p.nseg = 4; p.B = B; p.epi = g[5]; p.W3 = g[6] ? a : nullptr; p.a_sum = g[7] ? a : nullptr;
        sb.ntiles[i] = g[4];
    }
    sb.count = count;
    dim3 grid; int block = 0, lds = 0;
    g_err.clear();
    const void* fn = skinny_form_kernel(sb, m->opt, chains, stamped_skinny != 0, stamped_flat != 0, grid, block, lds);
    if (!fn && !g_err.empty()) { std::snprintf(out, cap, "ERROR %s", g_err.c_str()); return 0; }      // the text a caller of the refused launch reads from l2s_last_error
    // The kernel is named by its symbol: this needs the kernel handles in the library's dynamic symbol table (default visibility, external linkage - true of
    // this build, not under -fvisibility=hidden), no '>' in a kernel's parameter types, and the early-stop flag as the last template argument of every
    // kernel template but the stamped "_timed" ones.  tests/test_skinny_form_host.py fails on every row if one of these stops holding.
    Dl_info di{};
    L2S_REQUIRE(fn && dladdr(fn, &di) && di.dli_sname, "the form names no kernel instance");
    char* const dm = abi::__cxa_demangle(di.dli_sname, nullptr, nullptr, nullptr);      // "[void ]l2s::name<args, ES>(parameters)"
    std::string k(dm ? dm : di.dli_sname);
    std::free(dm);
    k = k.substr(0, k.find('<') == std::string::npos ? k.find('(') : k.rfind('>') + 1);
    k.erase(0, k.find("l2s::") + 5);
    if (k.find("_timed") == std::string::npos) k = k.substr(0, k.rfind(", ")) + ">";      // every other batch-row kernel template ends in the early-stop flag
    std::snprintf(out, cap, "%s grid=(%u,%u,%u) block=%d lds=%d", k.c_str(), grid.x, grid.y, grid.z, block, lds);
    return 0;
}

// the batch that the builders of decode_step.h make for a named call site, as l2s_op_skinny_form's integers; nothing is launched
int l2s_op_step_site(l2s_model* m, const char* site, int B, int* groups, int* count) {
    L2S_REQUIRE(m && m->finalized && site && groups && count && B >= 1, "bad arguments");
    struct Site { const char* name; int fold, hoist, step; char phase; };      // hoist < 0: the model's own "hoist_vproj"; the sites stand for 29-frame clips (four content slots)
    static const Site sites[] = {
        {"bilstm_step", 1, -1, 0, 'L'}, {"phase_a_unfolded", 0, -1, 1, 'A'}, {"phase_a_folded_step0", 1, -1, 0, 'A'}, {"phase_a_folded", 1, -1, 1, 'A'},
        {"step_attention_proj", 0, -1, 1, 'C'}, {"phase_d_k1536", 1, 0, 1, 'D'}, {"phase_d_k1280", 1, 1, 1, 'D'}, {"phase_d_k1024_sum", 1, 2, 1, 'D'},
        {"phase_d_k1024_unfolded", 0, -1, 1, 'D'}, {"phase_e", 1, -1, 1, 'E'}, {"step_fc_out_stop", 1, -1, 1, 'F'}, {"spk_lstm_step", 1, -1, 0, 'S'},
        {"phase_d_k768_hoist", 1, 3, 1, 'D'}};
    const Site* st = nullptr;
    for (const Site& t : sites) if (!std::strcmp(site, t.name)) st = &t;
    L2S_REQUIRE(st, "step site: unknown name");
    L2S_REQUIRE(st->phase == 'S' ? m->has_spk : m->has_dec, "step site: the model holds no weights of that recurrence");
    static float a[1];      // stands for every buffer, as in l2s_op_skinny_form
    StepBufs d;
    for (float** p : {&d.h0[0], &d.h0[1], &d.h1[0], &d.h1[1], &d.c0, &d.c1, &d.av, &d.p1, &d.cc, &d.uu, &d.p2f, &d.yf, &d.q, &d.qc, &d.p2, &d.al}) *p = a;
    Options o = m->opt;
    if (st->hoist >= 0) o.hoist_vproj = st->hoist;
    const Weights& w = m->w;
    const StepForm form = step_form(w, o, st->fold != 0, 4);
    const StepOut out{a, a, a, 2};
    const int i = st->step;
    SkinnyBatch sb{};
    switch (st->phase) {
    case 'L': for (int dir = 0; dir < 2; ++dir) bilstm_step_group(sb, dir, w, true, B, 7, 0, a, a, a, a, a); sb.count = 2; break;
    case 'A': sb = step_phase_a(form, w, d, B, i, step_from_frame(form, i, false), out); break;
    case 'C': sb = step_phase_c(form, w, d, B); break;
    case 'D': sb = step_phase_d(form, w, d, B, i, a, 4); break;
    case 'E': sb = step_phase_e(form, w, d, B, i); break;
    case 'F': sb = step_phase_f(form, w, d, B, i, out); break;
    default:  sb = spk_lstm_step(w, 0, B, a, a, a, a, 1024, a, 256); break;
    }
    for (int g = 0; g < sb.count; ++g) {
        const SkinnyP& p = sb.p[g];
        int* r = groups + 8 * g;      // nchunks[4], ntiles, epi, W3 set, a_sum set
        for (int j = 0; j < 4; ++j) r[j] = j < p.nseg ? p.seg[j].nchunks : 0;
        r[4] = sb.ntiles[g]; r[5] = p.epi; r[6] = p.W3 != nullptr; r[7] = p.a_sum != nullptr;
    }
    *count = sb.count;
    return 0;
}

// one batch-row launch described by the caller (include/l2s_diag.h l2s_skinny_group): the batch is filled field by field and handed to launch_skinny
static int op_skinny_batch(int count, const l2s_skinny_group* groups, int B, hipStream_t s, SkinnyBatch& sb) {
    for (int i = 0; i < count; ++i) {
        const l2s_skinny_group& g = groups[i];
        SkinnyP& p = sb.p[i];
        for (int j = 0; j < 4; ++j) {
            L2S_REQUIRE(g.nchunks[j] >= 0 && (g.nchunks[j] == 0 || g.seg_a[j]), "skinny op: a K segment without activations");
            p.seg[j] = {g.seg_a[j], g.nchunks[j]}; p.K += 16 * g.nchunks[j];
            if (g.nchunks[j]) p.nseg = j + 1;
        }
        L2S_REQUIRE(g.W && g.ntiles >= 1 && g.N >= 1 && g.N <= 16 * g.ntiles, "skinny op: weight / output columns");
        p.a_sum = g.a_sum; p.W = g.W; p.bias = g.bias; p.actw = g.actw; p.add = g.add; p.ld_add = g.ld_add; p.addrow = g.addrow;
        p.out = g.out; p.ldo = g.ldo; p.B = B; p.N = g.N; p.act = g.act; p.epi = g.epi;
        p.pre = g.pre; p.ld_pre = g.ld_pre; p.c_in = g.c_in; p.c_out = g.c_out; p.h_out = g.h_out; p.h_out_K = g.h_out_K; p.h_out_off = g.h_out_off;
        p.h_seq = g.h_seq; p.ld_hseq = g.ld_hseq; p.h_plain = g.h_plain; p.ld_hplain = g.ld_hplain; p.H = g.H;
        p.mel = g.mel; p.ld_mel_b = g.ld_mel_b; p.stop = g.stop; p.ld_stop_b = g.ld_stop_b; p.stop_const = g.stop_const; p.yfrag = g.yfrag;
        if (g.planes) {
            if (launch_skx_planes(g.W, g.ntiles, p.K, g.planes, s)) return 1;
            p.W3 = g.planes;
        }
        sb.ntiles[i] = g.ntiles;
    }
    sb.count = count;
    return 0;
}
int l2s_op_skinny(l2s_model* m, int count, const l2s_skinny_group* groups, int B, const int* es_end, int es_step, void* stream) {
    L2S_REQUIRE(m && groups && count >= 1 && count <= SKINNY_MAX_GROUP && B >= 1, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    SkinnyBatch sb{};
    if (op_skinny_batch(count, groups, B, s, sb)) return 1;
    sb.es_end = es_end; sb.es_step = es_step;
    return launch_skinny(sb, s, "op_skinny", m->opt);
}
// the same for ONE LSTM group that carries the hoisted content term (SkinnyP::hoist_p / hoist_alpha / hoist_pitch)
int l2s_op_skinny_hoist(l2s_model* m, const l2s_skinny_group* group, const float* hoist_p, const float* hoist_alpha, int hoist_pitch, int B, void* stream) {
    L2S_REQUIRE(m && group && hoist_p && hoist_alpha && B >= 1, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    SkinnyBatch sb{};
    if (op_skinny_batch(1, group, B, s, sb)) return 1;
    sb.p[0].hoist_p = hoist_p; sb.p[0].hoist_alpha = hoist_alpha; sb.p[0].hoist_pitch = hoist_pitch;
    return launch_skinny(sb, s, "op_skinny", m->opt);
}

int l2s_op_launch_chain(int kind, int n_launches, int blocks, int n_per_block, const float* in, float* out, void* stream) {
    for (int i = 0; i < n_launches; ++i)
        if (launch_probe(kind, blocks, n_per_block, in, out, (hipStream_t)stream)) return 1;
    return 0;
}

int l2s_op_launch_chain2(int kind, int n_launches, int blocks, int n_per_block, const float* in, float* out, void* stream_a, void* stream_b) {
    for (int i = 0; i < n_launches; ++i) {
        if (launch_probe(kind, blocks, n_per_block, in, out, (hipStream_t)stream_a)) return 1;
        if (launch_probe(kind, blocks, n_per_block, in + (int64_t)(1 << 24), out + 2048, (hipStream_t)stream_b)) return 1;
    }
    return 0;
}
#endif      // L2S_DIAG

int l2s_set_thread_chains(int n) { chains_hint() = n < 1 ? 1 : n; return 0; }
int l2s_persist_available(void) { return pdecode_device_ok() ? 1 : 0; }
int l2s_persist_timeouts(void) { return pdecode_timeouts(); }

int l2s_profile_enable(int on) { g_prof_on = on != 0; return 0; }
int l2s_profile_reset(void) { prof_drain(); g_prof.clear(); g_prof_idx.clear(); return 0; }
int l2s_profile_count(void) { prof_drain(); return (int)g_prof.size(); }
int l2s_profile_get(int idx, const char** name, int64_t* launches, double* total_ms) {
    prof_drain();
    L2S_REQUIRE(idx >= 0 && idx < (int)g_prof.size(), "profile index");
    if (name) *name = g_prof[idx].name.c_str();
    if (launches) *launches = g_prof[idx].launches;
    if (total_ms) *total_ms = g_prof[idx].total_ms;
    return 0;
}

}  // extern "C"
