// The weight blob of a model: built on the host from the checkpoint (pack_model), kept current on the device from the bound training
// tensors (refresh_weights).  The refresh must reproduce the host packer bit for bit (tests/test_train_loop.py), so everything that is
// computed rather than copied - the eval-BatchNorm fold, the front-end's bf16 operand planes - is ONE element function that the host
// packer and the refresh kernels both call.
#include "l2s_common.h"
#include "l2s_model.h"
#include "post_wino.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace l2s {

// ------------------------------------------------------------------------------------------------ element functions (host packer and device refresh)
// BatchNorm (eval) as scale / shift, absorbing a conv bias (0 where there is none): v = (acc + bias - mu) * scale + beta.  A fold without a
// bias written as beta - mu * scale gives the same bits: 0 - mu is exact, negation commutes with the rounding of the product, and
// (-p) + beta is beta - p (only a shift of zero can differ in sign, where mu is +0 and beta is -0).
// Host and device agree to the last bit or the one before: the host rounds every operation once (x86-64 has no fused multiply-add to contract
// to, its square root is correctly rounded); the device contracts the shift's product and sum into one fused multiply-add and takes the
// hardware's square root (__fsqrt_rn is the native one here).  The tests of the refresh allow that ulp; making the two sides equal
// would change the bits a refresh writes today.
__host__ __device__ inline void bn_fold(float g, float beta, float mu, float var, float bias, float eps, float* scale, float* shift) {
#ifdef __HIP_DEVICE_COMPILE__
    const float root = __fsqrt_rn(var + eps);
#else
    const float root = std::sqrt(var + eps);
#endif
    const float s = g / root;
    *scale = s;
    *shift = (bias - mu) * s + beta;
}

// The front-end conv's weights as bf16 operand planes (frontend3d_x3_kernel): per slab (ci, kt), step st = kernel rows 2st, 2st+1 (row 7:
// zeros), 16 columns k = 8 taps per row = one zero tap + the 7 real ones, 32 rows n = the 24 output channels + 8 zero rows.  Element
// (slab, st, n, k) of the Conv3d weight w (24,3,5,7,7), as the exact truncation split hi + mid + lo (FrontendW::w3) and as one bf16 rounded
// to nearest even (FrontendW::w1, the bf16 leg).  The subtractions are exact and stand alone: nothing to contract.
struct FePlaneElem { uint16_t split[3], rne; };
__host__ __device__ inline FePlaneElem fe_plane_elem(const float* w, int slab, int st, int n, int k) {
    const int kh = 2 * st + (k >> 3), kw = (k & 7) - 1, ci = slab / 5, kt = slab % 5;
    float x = 0.f;
    if (n < 24 && kh < 7 && kw >= 0) x = w[(((int64_t)n * 3 + ci) * 5 + kt) * 49 + kh * 7 + kw];
    const uint32_t xb = __builtin_bit_cast(uint32_t, x), hb = xb & 0xFFFF0000u;
    const float r1 = x - __builtin_bit_cast(float, hb);
    const uint32_t mb = __builtin_bit_cast(uint32_t, r1) & 0xFFFF0000u;
    const float r2 = r1 - __builtin_bit_cast(float, mb);
    const uint32_t lb = __builtin_bit_cast(uint32_t, r2);
    return {{(uint16_t)(hb >> 16), (uint16_t)(mb >> 16), (uint16_t)(lb >> 16)}, (uint16_t)((xb + 0x7FFFu + ((xb >> 16) & 1u)) >> 16)};
}
// where the element lives, in bf16 units: w3 in 18432-byte slabs, w1 in 6144-byte slabs, rows of 48 bytes (16 values + padding)
constexpr int FE_W3_SLAB = 9216, FE_W1_SLAB = 3072, FE_PLANE_ELEMS = 15 * 4 * 32 * 16;
__host__ __device__ inline void fe_plane_store(const FePlaneElem& e, int slab, int st, int n, int k, uint16_t* w3, uint16_t* w1) {
    for (int pl = 0; pl < 3; ++pl) w3[(int64_t)slab * FE_W3_SLAB + ((st * 3 + pl) * 32 + n) * 24 + k] = e.split[pl];
    w1[(int64_t)slab * FE_W1_SLAB + (st * 32 + n) * 24 + k] = e.rne;
}
// element idx of the FE_PLANE_ELEMS: k fastest, then n, st, slab
__host__ __device__ inline void fe_plane_fill(const float* w, int idx, uint16_t* w3, uint16_t* w1) {
    const int k = idx & 15, n = (idx >> 4) & 31, st = (idx >> 9) & 3, slab = idx >> 11;
    fe_plane_store(fe_plane_elem(w, slab, st, n, k), slab, st, n, k, w3, w1);
}

// ------------------------------------------------------------------------------------------------ host packer
// host-side blob builder: every sub-array 64-float (256 B) aligned
struct Blob {
    std::vector<float> data;
    int64_t alloc(int64_t n) {
        int64_t off = align_up((int64_t)data.size(), 64);
        data.resize(off + n, 0.f);
        return off;
    }
};

struct Parts { bool enc = false, dec = false, spk = false, face = false; };      // which towers the checkpoint holds

struct Packer {
    l2s_model* m;
    Blob blob;
    Parts parts;
    std::vector<std::pair<const float**, int64_t>> fixups;   // pointer slots to patch once the device address is known
    std::string missing;

    const std::vector<float>* get(const std::string& key, int64_t numel) {
        auto it = m->host.find(key);
        if (it == m->host.end()) { if (missing.empty()) missing = "missing tensor " + key; return nullptr; }
        if ((int64_t)it->second.size() != numel) {
            if (missing.empty()) missing = "tensor " + key + " has " + std::to_string(it->second.size()) + " elements, expected " + std::to_string(numel);
            return nullptr;
        }
        return &it->second;
    }
    void bind(const float** slot, int64_t off) { fixups.emplace_back(slot, off); }

    // BatchNorm (eval) folded to scale / shift (bn_fold), optionally absorbing a conv bias; record: the device-side refresh recomputes it
    std::vector<l2s_model::RefreshBn> bn_rec;
    std::vector<l2s_model::RefreshSum> sum_rec;
    void fold(int64_t so, int64_t ho, int c, const std::vector<float>& g, const std::vector<float>& b, const std::vector<float>& mu, const std::vector<float>& var,
              const std::vector<float>* bias, float eps) {
        for (int i = 0; i < c; ++i) bn_fold(g[i], b[i], mu[i], var[i], bias ? (*bias)[i] : 0.f, eps, &blob.data[so + i], &blob.data[ho + i]);
    }
    void bn(const std::string& p, int c, const std::vector<float>* bias, const float** scale, const float** shift, const std::string& bias_key = std::string(),
            float eps = BN_EPS, bool record = true) {
        auto g = get(p + ".weight", c), b = get(p + ".bias", c), mu = get(p + ".running_mean", c), var = get(p + ".running_var", c);
        if (!g || !b || !mu || !var) return;
        int64_t so = blob.alloc(c), ho = blob.alloc(c);
        fold(so, ho, c, *g, *b, *mu, *var, bias, eps);
        bind(scale, so);
        bind(shift, ho);
        if (record) bn_rec.push_back({p, bias_key, c, so, ho});
    }
    void copy(const std::string& key, int64_t n, const float** slot) {
        auto v = get(key, n);
        if (!v) return;
        int64_t o = blob.alloc(n);
        std::memcpy(&blob.data[o], v->data(), n * sizeof(float));
        bind(slot, o);
    }
    // Conv1d weight (co, ci, k) -> [co][k*ci] (tap-major K)
    void conv1d_w(const std::string& key, int co, int ci, int k, const float** slot) {
        auto v = get(key, (int64_t)co * ci * k);
        if (!v) return;
        int64_t o = blob.alloc((int64_t)co * ci * k);
        for (int n = 0; n < co; ++n)
            for (int c = 0; c < ci; ++c)
                for (int t = 0; t < k; ++t) blob.data[o + ((int64_t)n * k + t) * ci + c] = (*v)[((int64_t)n * ci + c) * k + t];
        bind(slot, o);
    }
    // depthwise (c,1,3,3) -> [9][c]
    void dw_w(const std::string& key, int c, const float** slot) {
        auto v = get(key, (int64_t)c * 9);
        if (!v) return;
        int64_t o = blob.alloc((int64_t)c * 9);
        for (int ch = 0; ch < c; ++ch)
            for (int t = 0; t < 9; ++t) blob.data[o + (int64_t)t * c + ch] = (*v)[(int64_t)ch * 9 + t];
        bind(slot, o);
    }
    // frag16 packing of rows[n] (each K long) of a virtual [Npad][K] matrix; row_of(n) returns nullptr for zero rows
    template <typename RowFn>
    void frag16(int Npad, int K, RowFn row_of, const float** slot) {
        int64_t o = blob.alloc((int64_t)Npad * K);
        const int NC = K / 16;
        std::vector<float> row(K);
        for (int n = 0; n < Npad; ++n) {
            bool nz = row_of(n, row.data());
            if (!nz) continue;
            for (int k = 0; k < K; ++k) {
                int tile = n >> 4, i = n & 15, c = k >> 4, g = (k >> 2) & 3, e = k & 3;
                blob.data[o + ((int64_t)(tile * NC + c) * 64 + g * 16 + i) * 4 + e] = row[k];
            }
        }
        bind(slot, o);
    }
};

static int lstm_perm_row(int np, int H) {      // packed row (unit-major: 4*unit + gate) -> PyTorch row gate*H + unit
    int unit = np >> 2, gate = np & 3;
    return gate * H + unit;
}

// The four towers are packed independently so that a VideoExtractor or a Decoder used on its own (as the reference allows: net.encoder /
// net.decoder) needs only its own keys.  The order of the blob.alloc calls, here and in pack_host, IS the blob layout.
static const std::string E = "encoder.", Dk = "decoder.", Sk = "speaker_encoder.", Fk = "vgg_face.";

static void pack_encoder(Packer& P, Weights& w) {
    // ---- frontend: Conv3d (24,3,5,7,7) -> [slab = ci*5+kt][50][32]
    {
        auto v = P.get(E + "frontend3D.0.weight", 24 * 3 * 5 * 49);
        if (v) {
            int64_t o = P.blob.alloc(15 * 50 * 32);
            for (int co = 0; co < 24; ++co)
                for (int ci = 0; ci < 3; ++ci)
                    for (int kt = 0; kt < 5; ++kt)
                        for (int tap = 0; tap < 49; ++tap)
                            P.blob.data[o + ((int64_t)(ci * 5 + kt) * 50 + tap) * 32 + co] = (*v)[(((int64_t)co * 3 + ci) * 5 + kt) * 49 + tap];
            P.bind(&w.fe.w, o);
            // the same weights as bf16 operand planes (fe_plane_elem): the exact three-way split, and ONE plane rounded to nearest even for the
            // bf16 leg (option "infer_bf16")
            const int64_t o3 = P.blob.alloc(15 * FE_W3_SLAB / 2), o1 = P.blob.alloc(15 * FE_W1_SLAB / 2);
            std::vector<uint16_t> w3(15 * FE_W3_SLAB, 0), w1(15 * FE_W1_SLAB, 0);
            for (int idx = 0; idx < FE_PLANE_ELEMS; ++idx) fe_plane_fill(v->data(), idx, w3.data(), w1.data());
            std::memcpy(&P.blob.data[o3], w3.data(), w3.size() * 2);
            std::memcpy(&P.blob.data[o1], w1.data(), w1.size() * 2);
            P.bind(&w.fe.w3, o3);
            P.bind(&w.fe.w1, o1);
        }
        P.bn(E + "frontend3D.1", 24, nullptr, &w.fe.scale, &w.fe.shift);
        P.copy(E + "frontend3D.2.weight", 24, &w.fe.slope);
    }
    // ---- ShuffleNet units
    {
        int u = 0, cin = STAGE_CH[0];
        for (int st = 0; st < 3; ++st) {
            int cout = STAGE_CH[st + 1], half = cout / 2;
            for (int r = 0; r < STAGE_REP[st]; ++r, ++u) {
                UnitW& U = w.unit[u];
                std::string p = E + "trunk.0." + std::to_string(u) + ".";
                U.stride2 = (r == 0);
                U.cin = cin;
                U.half = half;
                int pw1_in = U.stride2 ? cin : half;
                if (U.stride2) {
                    P.dw_w(p + "banch1.0.weight", cin, &U.b1_dw.w9);
                    P.bn(p + "banch1.1", cin, nullptr, &U.b1_dw.scale, &U.b1_dw.shift);
                    P.copy(p + "banch1.2.weight", (int64_t)half * cin, &U.b1_pw.W);
                    P.bn(p + "banch1.3", half, nullptr, &U.b1_pw.scale, &U.b1_pw.shift);
                }
                P.copy(p + "banch2.0.weight", (int64_t)half * pw1_in, &U.pw1.W);
                P.bn(p + "banch2.1", half, nullptr, &U.pw1.scale, &U.pw1.shift);
                P.dw_w(p + "banch2.3.weight", half, &U.dw.w9);
                P.bn(p + "banch2.4", half, nullptr, &U.dw.scale, &U.dw.shift);
                P.copy(p + "banch2.5.weight", (int64_t)half * half, &U.pw2.W);
                P.bn(p + "banch2.6", half, nullptr, &U.pw2.scale, &U.pw2.shift);
                {   // fused-unit operands: the pointwise weights in frag16 layout, K zero-padded to a multiple of 16
                    U.kpad = pad16(half);
                    U.kin = pad16(pw1_in);
                    struct { const char* key; int K, Kp; const float** slot; } fr[3] = {
                        {"banch2.0.weight", pw1_in, U.stride2 ? U.kin : U.kpad, &U.pw1_frag},
                        {"banch2.5.weight", half, U.kpad, &U.pw2_frag},
                        {"banch1.2.weight", cin, U.kin, &U.b1_frag}};
                    for (int which = 0; which < (U.stride2 ? 3 : 2); ++which) {
                        const int K = fr[which].K, Kp = fr[which].Kp;
                        auto wv = P.get(p + fr[which].key, (int64_t)half * K);
                        if (!wv) continue;
                        P.frag16(pad16(half), Kp, [&](int n, float* row) {
                            if (n >= half) return false;
                            std::memset(row, 0, sizeof(float) * Kp);
                            std::memcpy(row, wv->data() + (int64_t)n * K, sizeof(float) * K);
                            return true;
                        }, fr[which].slot);
                    }
                }
                cin = cout;
            }
        }
        P.copy(E + "trunk.1.0.weight", (int64_t)LAST_CH * STAGE_CH[3], &w.conv_last.W);
        P.bn(E + "trunk.1.1", LAST_CH, nullptr, &w.conv_last.scale, &w.conv_last.shift);
    }
}

static void pack_decoder(Packer& P, Weights& w) {
    // ---- decoder prologue
    auto linear = [&](const std::string& p, int co, int ci, ConvW& c) {
        P.copy(p + ".weight", (int64_t)co * ci, &c.W);
        P.copy(p + ".bias", co, &c.shift);
    };
    P.conv1d_w(Dk + "residual_bottleneck.weight", D, 1024, 1, &w.resid.W);
    P.copy(Dk + "residual_bottleneck.bias", D, &w.resid.shift);
    linear(Dk + "encoder_site.0.linear_layer", D, 256, w.enc_site);
    P.copy(Dk + "encoder_site.1.w", D, &w.enc_site.actw);
    linear(Dk + "attention_site.0.linear_layer", D, 256, w.attn_site);
    P.copy(Dk + "attention_site.1.w", D, &w.attn_site.actw);
    linear(Dk + "E_C.linear_layer", D, 1024, w.e_c);
    linear(Dk + "encoder_proj.linear_layer", D, 1024, w.enc_proj);
    {   // BiLSTM: input weights of both directions stacked [4096][1024]; b_ih + b_hh folded into the GEMM shift
        const char* suf[2] = {"l0", "l0_reverse"};
        int64_t wo = P.blob.alloc((int64_t)4096 * 1024), bo = P.blob.alloc(4096);
        for (int d = 0; d < 2; ++d) {
            auto wi = P.get(Dk + "encoder_rnn.weight_ih_" + suf[d], (int64_t)2048 * 1024);
            auto bi = P.get(Dk + "encoder_rnn.bias_ih_" + suf[d], 2048), bh = P.get(Dk + "encoder_rnn.bias_hh_" + suf[d], 2048);
            auto wh = P.get(Dk + "encoder_rnn.weight_hh_" + suf[d], (int64_t)2048 * 512);
            if (!wi || !bi || !bh || !wh) continue;
            std::memcpy(&P.blob.data[wo + (int64_t)d * 2048 * 1024], wi->data(), sizeof(float) * 2048 * 1024);
            for (int i = 0; i < 2048; ++i) P.blob.data[bo + d * 2048 + i] = (*bi)[i] + (*bh)[i];
            P.sum_rec.push_back({Dk + "encoder_rnn.bias_ih_" + suf[d], Dk + "encoder_rnn.bias_hh_" + suf[d], 2048, 0, bo + d * 2048});
            P.frag16(2048, 512, [&](int np, float* row) {
                std::memcpy(row, wh->data() + (int64_t)lstm_perm_row(np, 512) * 512, sizeof(float) * 512);
                return true;
            }, &w.whh[d].W);
            w.whh[d].N = 2048; w.whh[d].K = 512; w.whh[d].tiles = 128;
        }
        P.bind(&w.wih_cat, wo);
        P.bind(&w.bih_cat, bo);
    }
    for (int kv = 0; kv < 2; ++kv) {
        std::string p = Dk + (kv == 0 ? "K" : "V");
        for (int j = 0; j < 4; ++j) {
            std::string c = p + ".0.conv." + std::to_string(j);
            P.conv1d_w(c + ".0.weight", D, D, MH_KS[j], &w.mh_branch[kv][j].W);
            P.bn(c + ".1", D, P.get(c + ".0.bias", D), &w.mh_branch[kv][j].scale, &w.mh_branch[kv][j].shift, c + ".0.bias");
        }
        P.conv1d_w(p + ".0.bottleneck.weight", D, 5 * D, 1, &w.mh_bott[kv].W);
        P.copy(p + ".0.bottleneck.bias", D, &w.mh_bott[kv].shift);
        P.copy(p + ".1.w", D, &w.mh_bott[kv].actw);
    }
    P.copy(Dk + "positional_encodings.pos_table", (int64_t)L2S_MAX_STEPS * D, &w.pos);
    for (int j = 0; j < 4; ++j) {
        std::string c = Dk + "content.agg." + std::to_string(j);
        P.conv1d_w(c + ".0.weight", D, D, CT_KS[j], &w.ct_branch[j].W);
        P.bn(c + ".1", D, P.get(c + ".0.bias", D), &w.ct_branch[j].scale, &w.ct_branch[j].shift, c + ".0.bias");
    }
    P.conv1d_w(Dk + "content.bottleneck.weight", 256, 5 * D, 1, &w.ct_bott.W);
    P.copy(Dk + "content.bottleneck.bias", 256, &w.ct_bott.shift);
    linear(Dk + "content.K.0", 256, 256, w.ct_k0);
    linear(Dk + "content.K.2", 256, 256, w.ct_k2);
    linear(Dk + "content.location_fc.0", 256, 256, w.ct_fc0);
    linear(Dk + "content.location_fc.2", 256, 256, w.ct_fc2);
    linear(Dk + "content.location_fc.4", VOC, 256, w.ct_fc4);
    {   // word_embeddings (501,256) -> transposed, K padded: [256][504]
        auto v = P.get(Dk + "content.word_embeddings", (int64_t)VOC * 256);
        if (v) {
            int64_t o = P.blob.alloc((int64_t)256 * VOCP);
            for (int n = 0; n < 256; ++n)
                for (int k = 0; k < VOC; ++k) P.blob.data[o + (int64_t)n * VOCP + k] = (*v)[(int64_t)k * 256 + n];
            P.bind(&w.ct_emb.W, o);
        }
    }
    // ---- decode-step weights in frag16 layout
    auto sk_linear = [&](const std::string& wkey, const std::string& bkey, int N, int K, SkW& s) {
        auto wv = P.get(wkey, (int64_t)N * K);
        int Np = pad16(N);
        if (wv)
            P.frag16(Np, K, [&](int n, float* row) {
                if (n >= N) return false;
                std::memcpy(row, wv->data() + (int64_t)n * K, sizeof(float) * K);
                return true;
            }, &s.W);
        auto bv = P.get(bkey, N);
        if (bv) {
            int64_t o = P.blob.alloc(Np);
            std::memcpy(&P.blob.data[o], bv->data(), sizeof(float) * N);
            P.bind(&s.bias, o);
        }
        s.N = N; s.K = K; s.tiles = Np / 16;
    };
    sk_linear(Dk + "prenet.0.linear_layer.weight", Dk + "prenet.0.linear_layer.bias", 256, NM, w.pre1);
    P.copy(Dk + "prenet.1.w", 256, &w.pre1.actw);
    sk_linear(Dk + "prenet.3.linear_layer.weight", Dk + "prenet.3.linear_layer.bias", 256, 256, w.pre2);
    P.copy(Dk + "prenet.4.w", 256, &w.pre2.actw);
    sk_linear(Dk + "Q.0.linear_layer.weight", Dk + "Q.0.linear_layer.bias", D, 1024, w.q);
    P.copy(Dk + "Q.1.w", D, &w.q.actw);
    sk_linear(Dk + "content.Q.0.weight", Dk + "content.Q.0.bias", 256, 1024, w.cq);
    sk_linear(Dk + "attention_proj.linear_layer.weight", Dk + "attention_proj.linear_layer.bias", 256, D, w.aproj);
    int64_t lstm0_bias = -1;         // where LSTM0's b_ih + b_hh went: lstm0v shares it
    for (int l = 0; l < 2; ++l) {
        SkW& s = l == 0 ? w.lstm0 : w.lstm1;
        std::string sl = "l" + std::to_string(l);
        auto wi = P.get(Dk + "decoder_rnn.weight_ih_" + sl, (int64_t)2048 * 512), wh = P.get(Dk + "decoder_rnn.weight_hh_" + sl, (int64_t)2048 * 512);
        auto bi = P.get(Dk + "decoder_rnn.bias_ih_" + sl, 2048), bh = P.get(Dk + "decoder_rnn.bias_hh_" + sl, 2048);
        if (!wi || !wh || !bi || !bh) continue;
        P.frag16(2048, 1024, [&](int np, float* row) {
            int r = lstm_perm_row(np, 512);
            std::memcpy(row, wi->data() + (int64_t)r * 512, sizeof(float) * 512);
            std::memcpy(row + 512, wh->data() + (int64_t)r * 512, sizeof(float) * 512);
            return true;
        }, &s.W);
        int64_t o = P.blob.alloc(2048);
        for (int np = 0; np < 2048; ++np) { int r = lstm_perm_row(np, 512); P.blob.data[o + np] = (*bi)[r] + (*bh)[r]; }
        P.bind(&s.bias, o);
        if (l == 0) lstm0_bias = o;
        P.sum_rec.push_back({Dk + "decoder_rnn.bias_ih_" + sl, Dk + "decoder_rnn.bias_hh_" + sl, 2048, 512, o});
        s.N = 2048; s.K = 1024; s.tiles = 128;
        if (l == 0) {
            // layer 0 without its content columns (K = 768), and those columns as the GEMM weight of the prologue's P = value W_ih[:, content]^T, rows in the
            // packed order: verbatim copies of the parameters only (the device-side refresh keeps them current by itself), the plain LSTM0 bias
            P.frag16(2048, 768, [&](int np, float* row) {
                int r = lstm_perm_row(np, 512);
                std::memcpy(row, wi->data() + (int64_t)r * 512 + 256, sizeof(float) * 256);      // u = prenet + o columns of W_ih
                std::memcpy(row + 256, wh->data() + (int64_t)r * 512, sizeof(float) * 512);      // h0 columns
                return true;
            }, &w.lstm0c.W);
            P.bind(&w.lstm0c.bias, lstm0_bias);
            w.lstm0c.N = 2048; w.lstm0c.K = 768; w.lstm0c.tiles = 128;
            int64_t c = P.blob.alloc((int64_t)2048 * 256);
            for (int np = 0; np < 2048; ++np) std::memcpy(&P.blob.data[c + (int64_t)np * 256], wi->data() + (int64_t)lstm_perm_row(np, 512) * 512, sizeof(float) * 256);
            P.bind(&w.cproj.W, c);
        }
    }
    {   // fc_out (80 rows) + stop-token row over h1 (row 80) in one weight: [96][512]
        auto wf = P.get(Dk + "fc_out.linear_layer.weight", (int64_t)NM * D), bf = P.get(Dk + "fc_out.linear_layer.bias", NM);
        auto ws = P.get(Dk + "stop_token_layer.linear_layer.weight", 1024);
        if (wf && bf && ws) {
            P.frag16(96, D, [&](int n, float* row) {
                if (n < NM) std::memcpy(row, wf->data() + (int64_t)n * D, sizeof(float) * D);
                else if (n == NM) std::memcpy(row, ws->data(), sizeof(float) * D);
                else return false;
                return true;
            }, &w.fc.W);
            int64_t o = P.blob.alloc(96);
            std::memcpy(&P.blob.data[o], bf->data(), sizeof(float) * NM);
            P.bind(&w.fc.bias, o);
            int64_t t = P.blob.alloc(D);
            std::memcpy(&P.blob.data[t], ws->data() + D, sizeof(float) * D);
            P.bind(&w.stop_tail, t);
        }
        w.fc.N = NM + 1; w.fc.K = D; w.fc.tiles = 6;
        P.copy(Dk + "stop_token_layer.linear_layer.bias", 1, &w.stop_bias);
    }
    {   // Phase merging: two linear maps that are applied back to back with nothing in between are
        // pre-multiplied once, in fp64, and rounded to fp32:
        //   prenet1(fc_out(h1)) = PSine(W_p1 (W_out h1 + b_out) + b_p1) = PSine((W_p1 W_out) h1 + (W_p1 b_out + b_p1))
        //   LSTM0 gates on u = p2 + W_ap av + b_ap:  W_ih[:,256:] u = W_ih[:,256:] p2 + (W_ih[:,256:] W_ap) av + W_ih[:,256:] b_ap
        auto wp1 = P.get(Dk + "prenet.0.linear_layer.weight", (int64_t)256 * NM), bp1 = P.get(Dk + "prenet.0.linear_layer.bias", 256);
        auto wo = P.get(Dk + "fc_out.linear_layer.weight", (int64_t)NM * D), bo = P.get(Dk + "fc_out.linear_layer.bias", NM);
        if (wp1 && bp1 && wo && bo) {
            std::vector<float> wf((size_t)256 * D);
            int64_t bo_off = P.blob.alloc(256);
            std::vector<double> row(D);
            for (int n = 0; n < 256; ++n) {
                std::fill(row.begin(), row.end(), 0.0);
                double bacc = (*bp1)[n];
                for (int k = 0; k < NM; ++k) {
                    const double a = (*wp1)[(int64_t)n * NM + k];
                    const float* wr = wo->data() + (int64_t)k * D;
                    for (int j = 0; j < D; ++j) row[j] += a * wr[j];
                    bacc += a * (*bo)[k];
                }
                for (int j = 0; j < D; ++j) wf[(size_t)n * D + j] = (float)row[j];
                P.blob.data[bo_off + n] = (float)bacc;
            }
            P.frag16(256, D, [&](int n, float* r) { std::memcpy(r, wf.data() + (size_t)n * D, sizeof(float) * D); return true; }, &w.pre1f.W);
            P.bind(&w.pre1f.bias, bo_off);
            P.copy(Dk + "prenet.1.w", 256, &w.pre1f.actw);
            w.pre1f.N = 256; w.pre1f.K = D; w.pre1f.tiles = 16;
        }
        auto wi = P.get(Dk + "decoder_rnn.weight_ih_l0", (int64_t)2048 * 512), wh = P.get(Dk + "decoder_rnn.weight_hh_l0", (int64_t)2048 * 512);
        auto bi = P.get(Dk + "decoder_rnn.bias_ih_l0", 2048), bh = P.get(Dk + "decoder_rnn.bias_hh_l0", 2048);
        auto wap = P.get(Dk + "attention_proj.linear_layer.weight", (int64_t)256 * D), bap = P.get(Dk + "attention_proj.linear_layer.bias", 256);
        if (wi && wh && bi && bh && wap && bap) {
            std::vector<float> prod((size_t)2048 * D);      // (W_ih[:,256:512] @ W_ap) in PyTorch row order
            std::vector<float> badd(2048);
            std::vector<double> row(D);
            for (int r = 0; r < 2048; ++r) {
                std::fill(row.begin(), row.end(), 0.0);
                double bacc = 0.0;
                for (int k = 0; k < 256; ++k) {
                    const double a = (*wi)[(int64_t)r * 512 + 256 + k];
                    const float* wr = wap->data() + (int64_t)k * D;
                    for (int j = 0; j < D; ++j) row[j] += a * wr[j];
                    bacc += a * (*bap)[k];
                }
                for (int j = 0; j < D; ++j) prod[(size_t)r * D + j] = (float)row[j];
                badd[r] = (float)((double)(*bi)[r] + (double)(*bh)[r] + bacc);
            }
            P.frag16(2048, 1536, [&](int np, float* rowp) {
                int r = lstm_perm_row(np, 512);
                std::memcpy(rowp, wi->data() + (int64_t)r * 512, sizeof(float) * 512);          // [cc | p2] columns of W_ih
                std::memcpy(rowp + 512, prod.data() + (size_t)r * D, sizeof(float) * D);         // av columns
                std::memcpy(rowp + 1024, wh->data() + (int64_t)r * 512, sizeof(float) * 512);   // h0 columns
                return true;
            }, &w.lstm0f.W);
            int64_t o = P.blob.alloc(2048);
            for (int np = 0; np < 2048; ++np) P.blob.data[o + np] = badd[lstm_perm_row(np, 512)];
            P.bind(&w.lstm0f.bias, o);
            w.lstm0f.N = 2048; w.lstm0f.K = 1536; w.lstm0f.tiles = 128;
            // the same step with attention_proj applied to the VALUES once, in the prologue (V' = V W_ap^T + b_ap; the attention weights sum
            // to one, so a @ V' = W_ap (a @ v) + b_ap): LSTM0 then reads o = a @ V' (256 wide) through a second copy of W_ih's u columns -
            // K = 1280 instead of 1536, verbatim copies of the parameters only (the device-side refresh keeps them current by itself)
            P.frag16(2048, 1280, [&](int np, float* rowp) {
                int r = lstm_perm_row(np, 512);
                std::memcpy(rowp, wi->data() + (int64_t)r * 512, sizeof(float) * 512);                 // [cc | p2] columns of W_ih
                std::memcpy(rowp + 512, wi->data() + (int64_t)r * 512 + 256, sizeof(float) * 256);     // o: the u columns again
                std::memcpy(rowp + 768, wh->data() + (int64_t)r * 512, sizeof(float) * 512);           // h0 columns
                return true;
            }, &w.lstm0v.W);
            P.bind(&w.lstm0v.bias, lstm0_bias);      // the plain LSTM0 bias (b_ih + b_hh, kept current by the refresh's bias-sum records): packed above from these same four tensors
            w.lstm0v.N = 2048; w.lstm0v.K = 1280; w.lstm0v.tiles = 128;
            P.copy(Dk + "attention_proj.linear_layer.weight", (int64_t)256 * D, &w.vproj.W);
            P.copy(Dk + "attention_proj.linear_layer.bias", 256, &w.vproj.shift);
        }
    }
    P.copy(Dk + "BOS", NM, &w.bos);
    P.copy(Dk + "temperature", 1, &w.tau);
    P.copy(Dk + "content.temperature", 1, &w.tau_c);
    // ---- postnet
    for (int i = 0; i < 5; ++i) {
        int ci = i == 0 ? NM : D, co = i == 4 ? NM : D;
        std::string c = Dk + "postnet.convolutions." + std::to_string(i);
        P.conv1d_w(c + ".0.conv.weight", co, ci, 5, &w.post[i].W);
        P.bn(c + ".1", co, P.get(c + ".0.conv.bias", co), &w.post[i].scale, &w.post[i].shift, c + ".0.conv.bias");
        if (i < 4) P.copy(Dk + "postnet.sin_activation." + std::to_string(i) + ".w", D, &w.post[i].actw);
    }
}

static void pack_speaker(Packer& P, Weights& w) {
    constexpr int NFFT = 400, NF = 201, NMEL = 40, NFP = 204;
    {   // hann window (periodic), real-DFT matrix [cos | sin] and HTK mel filterbank, all computed in fp64
        const double PI = 3.14159265358979323846;
        int64_t wo = P.blob.alloc(NFFT), dof = P.blob.alloc((int64_t)2 * NF * NFFT), fo = P.blob.alloc((int64_t)NMEL * NFP);
        for (int j = 0; j < NFFT; ++j) P.blob.data[wo + j] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * j / NFFT));
        for (int k = 0; k < NF; ++k)
            for (int j = 0; j < NFFT; ++j) {
                const double ang = 2.0 * PI * (double)((int64_t)k * j % NFFT) / NFFT;
                P.blob.data[dof + (int64_t)k * NFFT + j] = (float)std::cos(ang);
                P.blob.data[dof + (int64_t)(NF + k) * NFFT + j] = (float)std::sin(ang);
            }
        // torchaudio.functional.create_fb_matrix(n_freqs=201, f_min=0, f_max=8000, n_mels=40, sample_rate=16000, norm=None), HTK scale
        std::vector<double> fpts(NMEL + 2);
        const double m_min = 0.0, m_max = 2595.0 * std::log10(1.0 + 8000.0 / 700.0);
        for (int i = 0; i < NMEL + 2; ++i) {
            const double mpt = m_min + (m_max - m_min) * i / (NMEL + 1);
            fpts[i] = 700.0 * (std::pow(10.0, mpt / 2595.0) - 1.0);
        }
        for (int k = 0; k < NF; ++k) {
            const double f = 8000.0 * k / (NF - 1);
            for (int mm = 0; mm < NMEL; ++mm) {
                const double down = (f - fpts[mm]) / (fpts[mm + 1] - fpts[mm]);
                const double up = (fpts[mm + 2] - f) / (fpts[mm + 2] - fpts[mm + 1]);
                P.blob.data[fo + (int64_t)mm * NFP + k] = (float)std::max(0.0, std::min(down, up));
            }
        }
        P.bind(&w.spk_window, wo); P.bind(&w.spk_dft, dof); P.bind(&w.spk_fbT, fo);
    }
    for (int l = 0; l < 3; ++l) {
        const int in = l == 0 ? 40 : 256;
        const std::string sl = "l" + std::to_string(l);
        auto wi = P.get(Sk + "lstm.weight_ih_" + sl, (int64_t)1024 * in), wh = P.get(Sk + "lstm.weight_hh_" + sl, (int64_t)1024 * 256);
        auto bi = P.get(Sk + "lstm.bias_ih_" + sl, 1024), bh = P.get(Sk + "lstm.bias_hh_" + sl, 1024);
        if (!wi || !wh || !bi || !bh) continue;
        P.copy(Sk + "lstm.weight_ih_" + sl, (int64_t)1024 * in, &w.spk_ih[l].W);
        int64_t bo = P.blob.alloc(1024);
        for (int i = 0; i < 1024; ++i) P.blob.data[bo + i] = (*bi)[i] + (*bh)[i];
        P.bind(&w.spk_ih[l].shift, bo);
        P.frag16(1024, 256, [&](int np, float* row) {
            std::memcpy(row, wh->data() + (int64_t)lstm_perm_row(np, 256) * 256, sizeof(float) * 256);
            return true;
        }, &w.spk_hh[l].W);
        w.spk_hh[l].N = 1024; w.spk_hh[l].K = 256; w.spk_hh[l].tiles = 64;
    }
    P.copy(Sk + "linear.weight", (int64_t)256 * 256, &w.spk_linear.W);
    P.copy(Sk + "linear.bias", 256, &w.spk_linear.shift);
}

// face tower (vgg_face.py:28-60; face_tower.hip): every convolution of the layer table re-laid as [Cout][kh][kw][Cin] (fused heads: the
// parts' rows one after the other), BasicConv2d's BatchNorm (eps 1e-3) folded into scale / shift, the blocks' up-projections as
// scale = block scale, shift = bias * scale; resnet.logits is held by the caller and not packed.  The tower is not trained: no refresh records
static int pack_face(Packer& P, Weights& w) {
    const auto& layers = face_layers();
    if ((int)layers.size() != FACE_N_CONVS) { set_error("l2s_model_finalize: face layer table has " + std::to_string(layers.size()) + " entries"); return 1; }
    for (int li = 0; li < FACE_N_CONVS; ++li) {
        const FaceLayer& L = layers[li];
        const int np = (int)L.parts.size(), N = L.cout * np, taps = L.kh * L.kw, K = taps * L.cin;
        const int64_t wn = (int64_t)L.cout * K;
        std::vector<const std::vector<float>*> wt(np), g(np), b(np), mu(np), var(np);
        bool ok = true;
        for (int j = 0; j < np; ++j) {
            const std::string pre = Fk + L.parts[j];
            if (L.res_scale == 0.f) {
                wt[j] = P.get(pre + ".conv.weight", wn);
                g[j] = P.get(pre + ".bn.weight", L.cout); b[j] = P.get(pre + ".bn.bias", L.cout);
                mu[j] = P.get(pre + ".bn.running_mean", L.cout); var[j] = P.get(pre + ".bn.running_var", L.cout);
                ok = ok && wt[j] && g[j] && b[j] && mu[j] && var[j];
            } else {
                wt[j] = P.get(pre + ".weight", wn); b[j] = P.get(pre + ".bias", L.cout);
                ok = ok && wt[j] && b[j];
            }
        }
        if (!ok) continue;
        const int64_t wo = P.blob.alloc((int64_t)N * K), so = P.blob.alloc(N), ho = P.blob.alloc(N);
        for (int j = 0; j < np; ++j) {
            const std::vector<float>& v = *wt[j];
            for (int n = 0; n < L.cout; ++n) {
                const int64_t row = wo + (int64_t)(j * L.cout + n) * K;
                for (int ci = 0; ci < L.cin; ++ci)
                    for (int t = 0; t < taps; ++t) P.blob.data[row + (int64_t)t * L.cin + ci] = v[((int64_t)n * L.cin + ci) * taps + t];
                if (L.res_scale != 0.f) {
                    P.blob.data[so + j * L.cout + n] = L.res_scale;
                    P.blob.data[ho + j * L.cout + n] = (*b[j])[n] * L.res_scale;
                }
            }
            if (L.res_scale == 0.f) P.fold(so + j * L.cout, ho + j * L.cout, L.cout, *g[j], *b[j], *mu[j], *var[j], nullptr, FACE_BN_EPS);
        }
        P.bind(&w.face.convs[li].w, wo); P.bind(&w.face.convs[li].scale, so); P.bind(&w.face.convs[li].shift, ho);
    }
    auto transposed = [&](const std::string& key, int out, int in, const float** slot) {      // nn.Linear weight (out, in) -> [in][out]
        auto v = P.get(key, (int64_t)out * in);
        if (!v) return;
        const int64_t o = P.blob.alloc((int64_t)out * in);
        for (int r = 0; r < out; ++r)
            for (int c = 0; c < in; ++c) P.blob.data[o + (int64_t)c * out + r] = (*v)[(int64_t)r * in + c];
        P.bind(slot, o);
    };
    transposed(Fk + "resnet.last_linear.weight", 512, 1792, &w.face.tail.llT);
    P.bn(Fk + "resnet.last_bn", 512, nullptr, &w.face.tail.bn_s, &w.face.tail.bn_h, std::string(), FACE_BN_EPS, /*record=*/false);
    transposed(Fk + "projection_layer.0.weight", 512, 512, &w.face.tail.p0T);
    P.copy(Fk + "projection_layer.0.bias", 512, &w.face.tail.p0b);
    transposed(Fk + "projection_layer.2.weight", 256, 512, &w.face.tail.p2T);
    P.copy(Fk + "projection_layer.2.bias", 256, &w.face.tail.p2b);
    return 0;
}

static int pack_host(l2s_model* m, Packer& P) {
    m->w = Weights{};
    Weights& w = m->w;
    auto has_prefix = [&](const std::string& pre) {
        for (auto& kv : m->host) if (kv.first.compare(0, pre.size(), pre) == 0) return true;
        return false;
    };
    P.parts = Parts{has_prefix(E), has_prefix(Dk), has_prefix(Sk), has_prefix(Fk)};
    if (!P.parts.enc && !P.parts.dec && !P.parts.spk && !P.parts.face) {
        set_error("l2s_model_finalize: no encoder.* / decoder.* / speaker_encoder.* / vgg_face.* tensors were set");
        return 1;
    }
    if (P.parts.enc) pack_encoder(P, w);
    if (P.parts.dec) pack_decoder(P, w);
    if (P.parts.spk) pack_speaker(P, w);
    if (P.parts.face && pack_face(P, w)) return 1;
    if (!P.missing.empty()) { set_error("l2s_model_finalize: " + P.missing); return 1; }
    return 0;
}

static int build_refresh_map(l2s_model* m, const Packer& P, hipStream_t stream);

// ------------------------------------------------------------------------------------------------ derived bf16 planes
// Four pools of derived operands (three of bf16 operand planes, one of the post-net's Winograd weights with their planes) are derived on the device from the packed fp32 weights, after every pack and every device-side refresh.
// One item = one weight (a x b: tiles x K for the LSTM fragments, N x K otherwise) and the slot that receives its planes.
struct PlaneItem { const float* W; int a, b; const void** slot; };
typedef int64_t (*PlaneBytesFn)(int a, int b);
typedef int (*PlaneLaunchFn)(const float* W, int a, int b, void* out, hipStream_t s);
// gives up quietly (slots stay null: the callers take their fp32 forms) if a source is missing; the pool is allocated once, at its first use
static int derive_planes(const std::vector<PlaneItem>& items, PlaneBytesFn bytes, PlaneLaunchFn launch, void** pool, hipStream_t s) {
    int64_t total = 0;
    for (const PlaneItem& it : items) { if (!it.W) return 0; total += bytes(it.a, it.b); }
    if (!total) return 0;
    if (!*pool) L2S_CHECK_HIP(hipMalloc(pool, total));
    char* base = reinterpret_cast<char*>(*pool);
    for (const PlaneItem& it : items) {
        if (launch(it.W, it.a, it.b, base, s)) return 1;
        *it.slot = base;
        base += bytes(it.a, it.b);
    }
    return 0;
}

// the decoder LSTM weights (layer 0 in its unmerged [content | u | h0] form and without its content columns, layer 1) and the BiLSTM's two directions, from the packed fp32
// fragments, for the split-bf16 LSTM blocks (option "lstm_x3")
static int derive_lstm_planes(l2s_model* m, hipStream_t s) {
    Weights& w = m->w;
    std::vector<PlaneItem> items;
    for (SkW* k : {&w.lstm0, &w.lstm1, &w.whh[0], &w.whh[1], &w.lstm0c}) {
        k->W3 = nullptr;
        items.push_back({k->W, k->tiles, k->K, &k->W3});
    }
    if (!m->has_dec) return 0;
    for (const PlaneItem& it : items) if (it.b % 256) return 0;
    return derive_planes(items, [](int tiles, int K) { return (int64_t)tiles * K * 96; }, launch_skx_planes, &m->lstm_planes, s);      // 16 columns x K x 6 bytes per tile
}

// the constant weights that meet the split-bf16 GEMM's wide tile (post-net layers 0-3, the BiLSTM input matrix, the eight MultiHop convs, conv_last),
// from the packed fp32 [N][K] matrices, for its LDS-DMA weight operand (option "gemm_x3_dma")
static int derive_gemm_planes(l2s_model* m, hipStream_t s) {
    Weights& w = m->w;
    for (int i = 0; i < 5; ++i) w.post[i].W3 = nullptr;
    w.wih_cat3 = nullptr; w.conv_last.W3 = nullptr;
    for (int kv = 0; kv < 2; ++kv) for (int j = 0; j < 4; ++j) w.mh_branch[kv][j].W3 = nullptr;
    std::vector<PlaneItem> items;
    if (m->has_dec) {
        const int Ks[4] = {5 * NM, 5 * 512, 5 * 512, 5 * 512};
        for (int i = 0; i < 4; ++i) items.push_back({w.post[i].W, 512, Ks[i], &w.post[i].W3});
        items.push_back({w.wih_cat, 4096, 1024, &w.wih_cat3});
        for (int kv = 0; kv < 2; ++kv)
            for (int j = 0; j < 4; ++j) items.push_back({w.mh_branch[kv][j].W, 512, 512 * MH_KS[j], &w.mh_branch[kv][j].W3});      // k = 1, 3, 7, 11; K and V
    }
    if (m->has_enc) items.push_back({w.conv_last.W, LAST_CH, STAGE_CH[3], &w.conv_last.W3});
    return derive_planes(items, gemm_planes_bytes, launch_gemm_planes, &m->gemm_planes, s);      // no part that has any: nothing to do
}

// the fused ShuffleNet units' pointwise convs, from the packed [N][K] matrices (option "trunk_x3")
static int derive_unit_planes(l2s_model* m, hipStream_t s) {
    std::vector<PlaneItem> items;
    for (UnitW& U : m->w.unit) {
        U.pw1_p3 = nullptr; U.pw2_p3 = nullptr; U.b1_p3 = nullptr;
        items.push_back({U.pw1.W, U.half, U.stride2 ? U.cin : U.half, &U.pw1_p3});
        items.push_back({U.pw2.W, U.half, U.half, &U.pw2_p3});
        if (U.stride2) items.push_back({U.b1_pw.W, U.half, U.cin, &U.b1_p3});
    }
    if (!m->has_enc) return 0;
    return derive_planes(items, su_planes_bytes, launch_su_planes, &m->unit_planes, s);
}

// post-net layers 1-3 in their Winograd F(4,5) form (option "post_wino"): per layer the eight transformed matrices U_p in fp32 - for the split-bf16 GEMM's
// staged-weights form - and their bf16 planes - the exact split of the stored U_p, for its LDS-DMA form - from the packed fp32 [512][5 * 512] weight
static int derive_wino_weights(l2s_model* m, hipStream_t s) {
    Weights& w = m->w;
    for (int i = 0; i < 5; ++i) w.post_wino[i] = nullptr;
    if (!m->has_dec) return 0;
    std::vector<PlaneItem> items;
    for (int i = 1; i <= 3; ++i) items.push_back({w.post[i].W, D, D, &w.post_wino[i]});
    return derive_planes(items, [](int C, int) { return wino_weights_bytes(C); }, [](const float* W, int C, int, void* out, hipStream_t st) { return launch_post_wino_weights(W, C, out, st); },
                         &m->wino_weights, s);
}

// fresh (after a pack: the blob moved, the parts may have changed): every pool is freed and derived anew; otherwise (after a device-side
// refresh: the planes are splits of the old weights) the pools that exist are refilled in place
static int derive_all_planes(l2s_model* m, hipStream_t s, bool fresh) {
    struct { void** pool; int (*derive)(l2s_model*, hipStream_t); } kinds[4] = {
        {&m->lstm_planes, derive_lstm_planes}, {&m->gemm_planes, derive_gemm_planes}, {&m->unit_planes, derive_unit_planes}, {&m->wino_weights, derive_wino_weights}};
    for (auto& k : kinds) {
        if (fresh && *k.pool) { (void)hipFree(*k.pool); *k.pool = nullptr; }
        if ((fresh || *k.pool) && k.derive(m, s)) return 1;
    }
    return 0;
}

void drop_graphs(l2s_model* m) {
    for (auto& g : m->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
    m->graphs.clear();
}

// everything this file allocates on the device for a model that is about to be deleted
void free_model_device(l2s_model* m) {
    for (void* p : {(void*)m->blob, (void*)m->r_key, (void*)m->r_idx, m->r_tables, (void*)m->merge_scratch, m->lstm_planes, m->gemm_planes, m->unit_planes, m->wino_weights})
        if (p) (void)hipFree(p);
}

int pack_model(l2s_model* m, hipStream_t stream) {
    Packer P{m};
    if (pack_host(m, P)) return 1;
    if (m->opt.refresh_map && build_refresh_map(m, P, stream)) return 1;
    m->folded_valid = true;

    // upload and patch pointers
    drop_graphs(m);
    if (m->blob) { (void)hipFree(m->blob); m->blob = nullptr; }
    m->blob_floats = (int64_t)P.blob.data.size();
    L2S_CHECK_HIP(hipMalloc(&m->blob, m->blob_floats * sizeof(float)));
    L2S_CHECK_HIP(hipMemcpyAsync(m->blob, P.blob.data.data(), m->blob_floats * sizeof(float), hipMemcpyHostToDevice, stream));
    L2S_CHECK_HIP(hipStreamSynchronize(stream));     // the host staging vector dies with this scope
    for (auto& f : P.fixups) *f.first = m->blob + f.second;
    m->finalized = true;
    m->has_enc = P.parts.enc;
    m->has_dec = P.parts.dec;
    m->has_spk = P.parts.spk;
    m->has_face = P.parts.face;
    return derive_all_planes(m, stream, /*fresh=*/true);
}

// ------------------------------------------------------------------------------------------------ device-side refresh (training)
// Which checkpoint element does each blob float copy?  Pack a shadow checkpoint whose elements carry their own global id as raw bits
// (ids < 2^31 - 2^23 are finite positive floats, so plain copies preserve them; arithmetic on them produces other patterns), then keep an
// entry only if the real blob holds exactly the value of the element the id names.  Computed entries (BatchNorm folds, bias sums) are
// refreshed from the records the packer left; the phase-merged step weights are fp64 products and are invalidated instead.
static int build_refresh_map(l2s_model* m, const Packer& P, hipStream_t stream) {
    std::vector<std::string> keys;
    for (auto& kv : m->host) keys.push_back(kv.first);
    std::sort(keys.begin(), keys.end());
    std::vector<int64_t> base(keys.size() + 1, 0);
    for (size_t i = 0; i < keys.size(); ++i) base[i + 1] = base[i] + (int64_t)m->host[keys[i]].size();
    L2S_REQUIRE(base.back() < 0x7F000000LL, "too many checkpoint elements for the refresh map");
    std::unordered_map<std::string, std::vector<float>> shadow;
    for (size_t i = 0; i < keys.size(); ++i) {
        std::vector<float> v(m->host[keys[i]].size());
        for (size_t j = 0; j < v.size(); ++j) { const uint32_t id = (uint32_t)(base[i] + (int64_t)j + 1); std::memcpy(&v[j], &id, 4); }
        shadow.emplace(keys[i], std::move(v));
    }
    Weights saved = m->w;
    m->host.swap(shadow);
    Packer P2{m};
    const int rc = pack_host(m, P2);
    m->host.swap(shadow);
    m->w = saved;
    if (rc) return 1;
    L2S_REQUIRE(P2.blob.data.size() == P.blob.data.size(), "refresh map: shadow pack differs in size");
    const int64_t n = (int64_t)P.blob.data.size();
    std::vector<int32_t> rk(n, -1), ri(n, 0);
    size_t cur = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t id; std::memcpy(&id, &P2.blob.data[i], 4);
        if (id == 0 || (int64_t)id > base.back()) continue;
        const int64_t g = (int64_t)id - 1;
        if (!(g >= base[cur] && g < base[cur + 1])) cur = (size_t)(std::upper_bound(base.begin(), base.end(), g) - base.begin()) - 1;
        const std::vector<float>& src = m->host[keys[cur]];
        const int64_t j = g - base[cur];
        uint32_t a, b; std::memcpy(&a, &P.blob.data[i], 4); std::memcpy(&b, &src[j], 4);
        if (a != b) continue;
        rk[i] = (int32_t)cur; ri[i] = (int32_t)j;
    }
    if (m->r_key) { (void)hipFree(m->r_key); m->r_key = nullptr; }
    if (m->r_idx) { (void)hipFree(m->r_idx); m->r_idx = nullptr; }
    L2S_CHECK_HIP(hipMalloc(&m->r_key, n * sizeof(int32_t)));
    L2S_CHECK_HIP(hipMalloc(&m->r_idx, n * sizeof(int32_t)));
    L2S_CHECK_HIP(hipMemcpyAsync(m->r_key, rk.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    L2S_CHECK_HIP(hipMemcpyAsync(m->r_idx, ri.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    L2S_CHECK_HIP(hipStreamSynchronize(stream));
    m->r_keys = keys;
    m->r_bn = P.bn_rec;
    m->r_sum = P.sum_rec;
    return 0;
}

struct RBn { const float *g, *b, *mu, *var, *bias; float *scale, *shift; int c; };
struct RSum { const float *a, *b; float* dst; int n, perm_H; };

__global__ __launch_bounds__(256) void refresh_gather_kernel(float* __restrict__ blob, const int32_t* __restrict__ rk, const int32_t* __restrict__ ri,
                                                             const float* const* __restrict__ ptrs, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int k = rk[i];
        if (k < 0) continue;
        const float* src = ptrs[k];
        if (src) blob[i] = src[ri[i]];
    }
}
__global__ __launch_bounds__(256) void refresh_bn_kernel(const RBn* __restrict__ recs) {
    const RBn r = recs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.c) return;
    bn_fold(r.g[i], r.b[i], r.mu[i], r.var[i], r.bias ? r.bias[i] : 0.f, BN_EPS, &r.scale[i], &r.shift[i]);      // Packer::bn
}
__global__ __launch_bounds__(256) void refresh_sum_kernel(const RSum* __restrict__ recs) {
    const RSum r = recs[blockIdx.y];
    const int np = blockIdx.x * 256 + threadIdx.x;
    if (np >= r.n) return;
    const int src = r.perm_H ? (np & 3) * r.perm_H + (np >> 2) : np;
    r.dst[np] = r.a[src] + r.b[src];
}

// ---- the front-end conv's bf16 operand planes (FrontendW::w3 / w1), re-derived from the bound Conv3d weight: pack_encoder's loop, one element a thread
__global__ __launch_bounds__(256) void refresh_frontend_planes_kernel(const float* __restrict__ w, uint16_t* __restrict__ w3, uint16_t* __restrict__ w1) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < FE_PLANE_ELEMS) fe_plane_fill(w, idx, w3, w1);
}

// ---- device-side re-merge of the two pre-multiplied step matrices (the host packer's fp64 products, here as fp32 MFMA products of the bound
// parameters): prenet1 o fc_out -> w.pre1f, LSTM0 with attention_proj folded in -> w.lstm0f, both in the frag16 weight layout of the blob
struct MergeSeg { const float* src; int ld, col0, k_lo, k_hi; };
__global__ __launch_bounds__(256) void merge_pack_kernel(float* __restrict__ dst, int N, int K, MergeSeg s0, MergeSeg s1, MergeSeg s2, int perm_H) {
    const int64_t total = (int64_t)N * K;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int k = idx % K, np = idx / K;
        const int r = perm_H ? (np & 3) * perm_H + (np >> 2) : np;
        const MergeSeg* segs[3] = {&s0, &s1, &s2};
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const MergeSeg& g = *segs[q];
            if (g.src && k >= g.k_lo && k < g.k_hi) v = g.src[(int64_t)r * g.ld + g.col0 + (k - g.k_lo)];
        }
        dst[frag16_index(np, k, K)] = v;
    }
}
// out[np] = a[r] (+ b[r]) + sum_k W[r*ld + col0 + k] * x[k],  r = perm(np)
__global__ __launch_bounds__(256) void merge_bias_kernel(float* __restrict__ out, int N, const float* __restrict__ a, const float* __restrict__ b,
                                                         const float* __restrict__ W, int ld, int col0, int K, const float* __restrict__ x, int perm_H) {
    const int np = blockIdx.x * 256 + threadIdx.x;
    if (np >= N) return;
    const int r = perm_H ? (np & 3) * perm_H + (np >> 2) : np;
    double acc = (double)a[r] + (b ? (double)b[r] : 0.0);
    for (int k = 0; k < K; ++k) acc += (double)W[(int64_t)r * ld + col0 + k] * (double)x[k];
    out[np] = (float)acc;
}
static int remerge_step_weights(l2s_model* m, hipStream_t s) {
    const std::string D = "decoder.";
    auto P = [&](const char* k) { return m->canon(D + k); };
    const float *wp1 = P("prenet.0.linear_layer.weight"), *bp1 = P("prenet.0.linear_layer.bias"), *wfc = P("fc_out.linear_layer.weight"), *bfc = P("fc_out.linear_layer.bias");
    const float *wih = P("decoder_rnn.weight_ih_l0"), *whh = P("decoder_rnn.weight_hh_l0"), *bih = P("decoder_rnn.bias_ih_l0"), *bhh = P("decoder_rnn.bias_hh_l0");
    const float *wap = P("attention_proj.linear_layer.weight"), *bap = P("attention_proj.linear_layer.bias");
    if (!(wp1 && bp1 && wfc && bfc && wih && whh && bih && bhh && wap && bap) || !m->w.pre1f.W || !m->w.lstm0f.W) return 0;      // decoder not bound: stays invalid
    if (!m->merge_scratch) L2S_CHECK_HIP(hipMalloc(&m->merge_scratch, sizeof(float) * ((int64_t)2048 * 512 + (int64_t)256 * 512)));
    float* prod_ap = m->merge_scratch; float* prod_p1 = prod_ap + (int64_t)2048 * 512;
    // (W_ih[:,256:512] @ W_ap) (2048 x 512) and (W_p1 @ W_out) (256 x 512): C = A . B with B row-major is the input-gradient form of the backward GEMM
    if (launch_gemm_bwd(bwd_dx(wih + 256, 512, wap, prod_ap, 512, 1, 2048, 2048, 256, 512, 1, 0, false), s, "train_merge_step_weights")) return 1;
    if (launch_gemm_bwd(bwd_dx(wp1, NM, wfc, prod_p1, 512, 1, 256, 256, NM, 512, 1, 0, false), s, "train_merge_step_weights")) return 1;
    ProfScope ps("train_merge_step_weights", s);
    const MergeSeg none{nullptr, 0, 0, 0, 0};
    hipLaunchKernelGGL(merge_pack_kernel, dim3(4096), dim3(256), 0, s, const_cast<float*>(m->w.lstm0f.W), 2048, 1536, MergeSeg{wih, 512, 0, 0, 512},
                       MergeSeg{prod_ap, 512, 0, 512, 1024}, MergeSeg{whh, 512, 0, 1024, 1536}, 512);
    hipLaunchKernelGGL(merge_pack_kernel, dim3(512), dim3(256), 0, s, const_cast<float*>(m->w.pre1f.W), 256, 512, MergeSeg{prod_p1, 512, 0, 0, 512}, none, none, 0);
    hipLaunchKernelGGL(merge_bias_kernel, dim3(8), dim3(256), 0, s, const_cast<float*>(m->w.lstm0f.bias), 2048, bih, bhh, wih, 512, 256, 256, bap, 512);
    hipLaunchKernelGGL(merge_bias_kernel, dim3(1), dim3(256), 0, s, const_cast<float*>(m->w.pre1f.bias), 256, bp1, (const float*)nullptr, wp1, NM, 0, NM, bfc, 0);
    L2S_CHECK_HIP(hipGetLastError());
    m->folded_valid = true;
    return 0;
}

int refresh_weights(l2s_model* m, hipStream_t s) {
    L2S_REQUIRE(m->finalized && m->r_key && m->r_idx, "no refresh map: set option refresh_map=1 before l2s_model_finalize");
    const size_t nk = m->r_keys.size(), nb = m->r_bn.size(), ns = m->r_sum.size();
    const size_t off_bn = align_up((int64_t)(nk * sizeof(float*)), 64), off_sum = off_bn + align_up((int64_t)(nb * sizeof(RBn)), 64);
    const size_t total = off_sum + ns * sizeof(RSum) + 64;
    m->r_tables_host.assign(total, 0);
    const float** ptrs = reinterpret_cast<const float**>(m->r_tables_host.data());
    for (size_t i = 0; i < nk; ++i) ptrs[i] = m->canon(m->r_keys[i]);
    RBn* bn = reinterpret_cast<RBn*>(m->r_tables_host.data() + off_bn);
    size_t nb_live = 0;
    int maxc = 1;
    for (const auto& r : m->r_bn) {
        RBn d{m->canon(r.p + ".weight"), m->canon(r.p + ".bias"), m->canon(r.p + ".running_mean"), m->canon(r.p + ".running_var"),
              r.bias_key.empty() ? nullptr : m->canon(r.bias_key), m->blob + r.so, m->blob + r.ho, r.c};
        if (!d.g && !d.b && !d.mu && !d.var) continue;                   // a module that is not bound at all (e.g. frozen) keeps its packed values
        L2S_REQUIRE(d.g && d.b && d.mu && d.var && (r.bias_key.empty() || d.bias), "refresh: BatchNorm tensors of a layer are only partly bound");
        bn[nb_live++] = d; maxc = std::max(maxc, r.c);
    }
    RSum* sm = reinterpret_cast<RSum*>(m->r_tables_host.data() + off_sum);
    size_t ns_live = 0;
    int maxn = 1;
    for (const auto& r : m->r_sum) {
        RSum d{m->canon(r.a), m->canon(r.b), m->blob + r.dst, r.n, r.perm_H};
        if (!d.a && !d.b) continue;
        L2S_REQUIRE(d.a && d.b, "refresh: bias pair only partly bound");
        sm[ns_live++] = d; maxn = std::max(maxn, r.n);
    }
    if ((int64_t)total > m->r_tables_bytes) {
        if (m->r_tables) (void)hipFree(m->r_tables);
        L2S_CHECK_HIP(hipMalloc(&m->r_tables, total));
        m->r_tables_bytes = (int64_t)total;
        m->r_tables_uploaded.clear();
    }
    // the tables only change when tensors are (re)bound: upload them then, not on every optimizer step (the upload comes from a pageable vector,
    // so it ends in a stream synchronise - once per step that drained the pipeline between steps)
    if (m->r_tables_host != m->r_tables_uploaded) {
        L2S_CHECK_HIP(hipMemcpyAsync(m->r_tables, m->r_tables_host.data(), total, hipMemcpyHostToDevice, s));
        L2S_CHECK_HIP(hipStreamSynchronize(s));                         // pageable staging buffer: the copy must have left the host vector
        m->r_tables_uploaded = m->r_tables_host;
    }
    char* T = (char*)m->r_tables;
    {
        ProfScope ps("train_refresh_gather", s);
        hipLaunchKernelGGL(refresh_gather_kernel, dim3(4096), dim3(256), 0, s, m->blob, m->r_key, m->r_idx, reinterpret_cast<const float* const*>(T), m->blob_floats);
    }
    if (nb_live) hipLaunchKernelGGL(refresh_bn_kernel, dim3((maxc + 255) / 256, (unsigned)nb_live), dim3(256), 0, s, reinterpret_cast<const RBn*>(T + off_bn));
    if (ns_live) hipLaunchKernelGGL(refresh_sum_kernel, dim3((maxn + 255) / 256, (unsigned)ns_live), dim3(256), 0, s, reinterpret_cast<const RSum*>(T + off_sum));
    L2S_CHECK_HIP(hipGetLastError());
    // the front-end's bf16 operand planes are splits of the old weights: re-split them from the bound Conv3d weight (an encoder that is not
    // bound keeps its packed planes, like every other unbound module)
    if (const float* w3d = m->canon("encoder.frontend3D.0.weight"); w3d && m->w.fe.w3 && m->w.fe.w1) {
        ProfScope ps("train_refresh_frontend_planes", s);
        hipLaunchKernelGGL(refresh_frontend_planes_kernel, dim3(FE_PLANE_ELEMS / 256), dim3(256), 0, s, w3d,
                           reinterpret_cast<uint16_t*>(const_cast<float*>(m->w.fe.w3)), reinterpret_cast<uint16_t*>(const_cast<float*>(m->w.fe.w1)));
        L2S_CHECK_HIP(hipGetLastError());
    }
    if (derive_all_planes(m, s, /*fresh=*/false)) return 1;      // the derived pools are splits of the old weights too
    m->folded_valid = false;        // W_p1 W_out and W_ih W_ap are products of the old parameters ...
    if (remerge_step_weights(m, s)) return 1;      // ... rebuilt here when the decoder's tensors are bound (then the 4-launch step stays valid)
    drop_graphs(m);
    return 0;
}

}  // namespace l2s
