// Per-clip MEL lengths on the training path (include/l2s.h "training with per-clip mel lengths"): the length-aware loss (l2s_loss_lengths) and the pieces the
// masked post-net (l2s_train_postnet_masked_fwd / _masked_bwd, train_decoder.hip) lays over its unmasked launches.  The row-major activations and gradients
// (B*S, 512) / (B*S, 80) are zeroed past S_b by launch_zero_pad_rows of masked_train.hip, whose table segment 0 is the per-clip row count; here is the
// channel-first form for mel_post (B, 80, S).
//   length table (device, int32): lens[0..B) = S_b, lens[B..2B) = m_b = the clip's content rows (l2s_min_T(len_b); all m rows without video lengths)
#include "../../include/l2s.h"
#include "host_table.h"
#include "l2s_model.h"      // align_up

#include <algorithm>

namespace l2s {

int check_mel_lengths(const int32_t* mel_lengths, int B, int S) {
    if (B < 1 || B > 96) { set_error("l2s: mel_lengths: B = " + std::to_string(B) + " is outside [1, 96]"); return 1; }
    L2S_REQUIRE(mel_lengths, "mel_lengths is null");
    for (int b = 0; b < B; ++b)
        if (mel_lengths[b] < 1 || mel_lengths[b] > S) {
            set_error("l2s: mel_lengths[" + std::to_string(b) + "] = " + std::to_string(mel_lengths[b]) + " is outside [1, S = " + std::to_string(S) + "]");
            return 1;
        }
    return 0;
}

static void mel_len_table(HostTable& t, const int32_t* mel_lengths, const int32_t* video_lengths, int B, int m) {
    t.i32(mel_lengths, B);
    int32_t* mb = t.host<int32_t>(t.i32(nullptr, B));
    for (int b = 0; mb && b < B; ++b) mb[b] = video_lengths ? video_lengths[b] / 7 : m;
}
int64_t mel_len_table_words(int B) { HostTable t(false); mel_len_table(t, nullptr, nullptr, B, 0); return t.words(); }

int launch_mel_len_table(const int32_t* mel_lengths, const int32_t* video_lengths, int B, int m, int* table, hipStream_t s) {
    HostTable t;
    mel_len_table(t, mel_lengths, video_lengths, B, m);
    return t.upload(table, s);
}

// ---- x (B, C, S) channel-first: positions s >= S_b := 0
__global__ __launch_bounds__(256) void zero_cf_past_len_kernel(float* __restrict__ x, const int* __restrict__ lens, int C, int S, int64_t total) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int sidx = (int)(idx % S);
        const int b = (int)(idx / ((int64_t)C * S));
        if (sidx >= lens[b]) x[idx] = 0.f;
    }
}

int launch_zero_cf_past_len(float* x, const int* lens, int B, int C, int S, hipStream_t s) {
    const int64_t total = (int64_t)B * C * S;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 8192));
    ProfScope ps("train_zero_cf_past_len", s);
    hipLaunchKernelGGL(zero_cf_past_len_kernel, dim3(blocks), dim3(256), 0, s, x, lens, C, S, total);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the loss over each clip's own extent.  Block (chunk, clip): the clip's 80 x S mel positions, S gate positions and m x V content entries, strided over
// the clip's LL_BLOCKS blocks; a position s >= S_b or a content row >= m_b is never read and gets an exact-zero gradient.  The element arithmetic and the
// reciprocals (1.f / (float)n) are loss_partial_kernel's, so equal lengths give its gradient bits.  partials[(b * 4 + term) * LL_BLOCKS + chunk], fp64.
constexpr int LL_BLOCKS = 16;

struct LossLenP {
    LossP p;
    int B, S, m;      // m: content rows per clip (R = B * m)
};

__device__ __forceinline__ double block_sum_d4(double x, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void loss_len_partial_kernel(const LossLenP q, const int* __restrict__ lens, double* __restrict__ partials) {
    __shared__ double sh[4];
    const LossP& p = q.p;
    const int b = blockIdx.y, Sb = lens[b], mb = lens[q.B + b];
    const int start = blockIdx.x * 256 + threadIdx.x, stride = LL_BLOCKS * 256;
    const float inv_mel = 1.f / (float)((int64_t)q.B * L2S_N_MELS * Sb), inv_stop = 1.f / (float)((int64_t)q.B * Sb), inv_R = 1.f / (float)((int64_t)q.B * mb);
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    const int64_t mel0 = (int64_t)b * L2S_N_MELS * q.S;
    for (int i = start; i < L2S_N_MELS * q.S; i += stride) {
        const int sidx = i % q.S;
        float g0 = 0.f, g1 = 0.f;
        if (sidx < Sb) {
            const float t = p.mel_tgt[mel0 + i];
            const float d0 = p.mel[mel0 + i] - t, d1 = p.mel_post[mel0 + i] - t;
            a0 += (double)d0 * d0;
            a1 += (double)d1 * d1;
            g0 = 2.f * d0 * inv_mel; g1 = 20.f * d1 * inv_mel;
        }
        if (p.dmel) p.dmel[mel0 + i] = g0;
        if (p.dmel_post) p.dmel_post[mel0 + i] = g1;
    }
    const int64_t st0 = (int64_t)b * q.S;
    for (int i = start; i < q.S; i += stride) {
        float g = 0.f;
        if (i < Sb) {
            const float x = p.stop[st0 + i], y = p.gate[st0 + i];
            a2 += (double)(fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))));
            g = (1.f / (1.f + expf(-x)) - y) * inv_stop;
        }
        if (p.dstop) p.dstop[st0 + i] = g;
    }
    const int64_t dis0 = (int64_t)b * q.m * p.V;
    for (int i = start; i < q.m * p.V; i += stride) {
        float g = 0.f;
        if (i / p.V < mb) {
            const float v = p.dis[dis0 + i];
            const float arg = v * (float)p.V + 1e-20f;
            const float lr = logf(arg);
            a3 += (double)(v * lr);
            g = (lr + v * (float)p.V / arg) * inv_R;
        }
        if (p.ddis) p.ddis[dis0 + i] = g;
    }
    a0 = block_sum_d4(a0, sh); a1 = block_sum_d4(a1, sh); a2 = block_sum_d4(a2, sh); a3 = block_sum_d4(a3, sh);
    if (threadIdx.x == 0) {
        double* dst = partials + (int64_t)b * 4 * LL_BLOCKS + blockIdx.x;
        dst[0 * LL_BLOCKS] = a0; dst[1 * LL_BLOCKS] = a1; dst[2 * LL_BLOCKS] = a2; dst[3 * LL_BLOCKS] = a3;
    }
}

// finish: each clip's four terms over its own extent (per_clip, may be null), then their mean over the B clips (out5, may be null).  One block; a thread
// takes the clips b = tid, tid + 256, ..: a fixed order, the same result run to run
__global__ __launch_bounds__(256) void loss_len_final_kernel(const double* __restrict__ partials, const int* __restrict__ lens, int B, float* __restrict__ out5,
                                                             float* __restrict__ per_clip) {
    __shared__ double sh[4];
    double acc[4] = {0, 0, 0, 0};
    for (int b = threadIdx.x; b < B; b += 256) {
        const double Sb = (double)lens[b], mb = (double)lens[B + b];
        const double den[4] = {(double)L2S_N_MELS * Sb, (double)L2S_N_MELS * Sb, Sb, mb};
        for (int t = 0; t < 4; ++t) {
            double tot = 0.0;
            for (int i = 0; i < LL_BLOCKS; ++i) tot += partials[((int64_t)b * 4 + t) * LL_BLOCKS + i];
            const double term = (t == 1 ? 10.0 : 1.0) * tot / den[t];
            if (per_clip) per_clip[b * 4 + t] = (float)term;
            acc[t] += term;
        }
    }
    double tot[4];
    for (int t = 0; t < 4; ++t) tot[t] = block_sum_d4(acc[t], sh);
    if (threadIdx.x == 0 && out5) {
        for (int t = 0; t < 4; ++t) out5[t] = (float)(tot[t] / (double)B);
        out5[4] = out5[0] + out5[1] + out5[2] + out5[3];
    }
}

static int64_t loss_len_partials_bytes(int B) { return align_up((int64_t)B * 4 * LL_BLOCKS * (int64_t)sizeof(double), 256); }

}  // namespace l2s

using namespace l2s;

extern "C" {

int l2s_loss_lengths_check(const int32_t* mel_lengths, const int32_t* video_lengths, int B, int S, int T) {
    if (check_mel_lengths(mel_lengths, B, S)) return 1;
    return video_lengths ? check_lengths(video_lengths, B, T) : 0;
}

// [0, l2s_train_scratch_bytes()): what l2s_loss takes (equal lengths run its launches); then the per-(clip, term) partials and the device length table
int64_t l2s_train_scratch_bytes_lengths(int B) {
    if (B < 1 || B > 96) return -1;
    return align_up(l2s_train_scratch_bytes(), 256) + loss_len_partials_bytes(B) + align_up(mel_len_table_words(B), 64) * (int64_t)sizeof(int32_t);
}

int l2s_loss_lengths(const float* mel, const float* mel_post, const float* mel_target, const float* stop, const float* gate_target, const float* content_dis,
                     int B, int S, int R, float* losses5, float* dmel, float* dmel_post, float* dstop, float* ddis, void* scratch, void* stream,
                     const int32_t* mel_lengths, const int32_t* video_lengths, int T, float* per_clip) {
    if (l2s_loss_lengths_check(mel_lengths, video_lengths, B, S, T)) return 1;
    L2S_REQUIRE(mel && mel_post && mel_target && stop && gate_target && content_dis && losses5 && scratch, "bad arguments");
    L2S_REQUIRE(R >= B && R % B == 0 && (!video_lengths || R / B == T / 7), "content_dis must hold R = B * l2s_min_T(T) rows, clip b's at b * R / B");
    hipStream_t s = (hipStream_t)stream;
    const int m = R / B;
    LossLenP q{};
    LossP& p = q.p;
    p.mel = mel; p.mel_post = mel_post; p.mel_tgt = mel_target; p.stop = stop; p.gate = gate_target; p.dis = content_dis;
    p.dmel = dmel; p.dmel_post = dmel_post; p.dstop = dstop; p.ddis = ddis;
    p.n_mel = (int64_t)B * L2S_N_MELS * S; p.n_stop = (int64_t)B * S; p.R = R; p.V = L2S_VOCAB; p.n_dis = (int64_t)R * L2S_VOCAB;
    q.B = B; q.S = S; q.m = m;
    bool full = true;
    for (int b = 0; b < B; ++b) full = full && mel_lengths[b] == S && (!video_lengths || video_lengths[b] / 7 == m);
    // every clip of full extent: the batch means ARE the per-clip means, and l2s_loss's own launches give its bits (terms and gradients); the length-aware
    // pass then only runs for per_clip, with no gradient or batch output
    if (full) {
        if (launch_loss(p, (double*)scratch, losses5, s)) return 1;
        if (!per_clip) return 0;
        p.dmel = p.dmel_post = p.dstop = p.ddis = nullptr;
        losses5 = nullptr;
    }
    char* base = (char*)scratch + align_up(l2s_train_scratch_bytes(), 256);
    double* partials = (double*)base;
    int* lens = (int*)(base + loss_len_partials_bytes(B));
    if (launch_mel_len_table(mel_lengths, video_lengths, B, m, lens, s)) return 1;
    ProfScope ps("loss_lengths_fwd_bwd", s);
    hipLaunchKernelGGL(loss_len_partial_kernel, dim3(LL_BLOCKS, B), dim3(256), 0, s, q, lens, partials);
    hipLaunchKernelGGL(loss_len_final_kernel, dim3(1), dim3(256), 0, s, partials, lens, B, losses5, per_clip);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
