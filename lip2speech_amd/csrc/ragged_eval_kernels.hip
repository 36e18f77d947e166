// Evaluate-shaped ragged groups (l2s_forward_eval_ragged, include/l2s.h): batches of unequal B, T AND step count S as rows of one launch chain.  The
// chain decodes every row for Smax steps into buffers at pitch Smax / Tmax; the small kernels here give every row the S of its own batch.  The GEMMs,
// the convolutions and the step kernels stay the unmasked ones (the house style of masked_kernels.hip):
//   - rows j >= S_c of the decoded mel and of the post-net layers' outputs become zeros, so that the next layer's taps read past a row's end the zeros
//     the batch's own call reads as padding;
//   - the staged outputs are moved into the packed per-batch blocks, each with the layout l2s_forward_eval_masked gives that batch alone.
// Per-clip table (EvalClip, l2s_common.h): S_c, T_g, the row in its batch, min_T(T_g) and the float offsets of its batch's four blocks.
#include "../../include/l2s.h"      // L2S_N_MELS, L2S_VOCAB
#include "host_table.h"

#include <algorithm>

namespace l2s {

// ---- the table (host_table.h)
int64_t eval_table_words(int N) { HostTable t(false); t.rec<EvalClip>(nullptr, N); return t.words(); }

int launch_eval_table(const EvalClip* clips_host, int N, EvalClip* clips_dev, hipStream_t s) {
    HostTable t;
    t.rec(clips_host, N);
    return t.upload(reinterpret_cast<int32_t*>(clips_dev), s);
}

// ---- rows j >= S_c of x (N * Smax rows of cols floats, dense, 16-byte aligned) become zeros.  Block (tile of ZERO_ROWS rows, clip); a block whose rows
// are all kept returns at once.  The rows of a clip are contiguous, so the tail of a tile is one run of float4 stores.
constexpr int ZERO_ROWS = 16;
__global__ __launch_bounds__(256) void zero_rows_past_s_kernel(float* __restrict__ x, int cols4, int Smax, const EvalClip* __restrict__ clips) {
    const int c = blockIdx.y, j0 = blockIdx.x * ZERO_ROWS, j1 = min(j0 + ZERO_ROWS, Smax);
    const int S = clips[c].S;      // block-uniform
    if (j1 <= S) return;
    const int first = max(j0, S);
    float4* p = reinterpret_cast<float4*>(x) + ((int64_t)c * Smax + first) * cols4;
    const int n = (j1 - first) * cols4;
    for (int i = threadIdx.x; i < n; i += 256) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

int launch_zero_rows_past_s(float* x, int cols, const EvalTab& ev, hipStream_t s) {
    L2S_REQUIRE(x && ev.clips && cols % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0, "zero_rows_past_s: float4 rows");
    ProfScope ps("eval_zero_rows_past_s", s);
    hipLaunchKernelGGL(zero_rows_past_s_kernel, dim3((ev.Smax + ZERO_ROWS - 1) / ZERO_ROWS, ev.N), dim3(256), 0, s, x, cols / 4, ev.Smax, ev.clips);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- one staged output -> the packed blocks.  Clip c's part of a field is rows x cols floats, read at the staging pitch and written dense:
//   EV_STOP      (N, Smax)          -> (B_g, S_g)          1 x S_c
//   EV_ATTN      (N, Smax, Tmax)    -> (B_g, S_g, T_g)     S_c x T_g
//   EV_DIS       (N * mTmax, 501)   -> (B_g * mT_g, 501)   mT_g x 501 (the clip's first min_T(T_g) slot rows; those past min_T(len_c) are zeros already)
//   EV_MEL_POST  (N, 80, Smax)      -> (B_g, 80, S_g)      80 x S_c
// The dense side has whatever alignment S_g and T_g give it, so both sides move as 4-byte accesses: consecutive lanes write consecutive floats and read
// runs of `cols` consecutive floats.  Block (chunk of SCATTER_CHUNK floats of the clip's part, clip); the blocks past a clip's part return at once.
constexpr int SCATTER_CHUNK = 1024;
__global__ __launch_bounds__(256) void eval_scatter_kernel(const float* __restrict__ src, const EvalClip* __restrict__ clips, int field, int Smax, int Tmax,
                                                           int mTmax, float* __restrict__ dst) {
    const int c = blockIdx.y;
    const EvalClip k = clips[c];      // block-uniform
    int rows, cols, ld;
    int64_t src0, dst0;
    if (field == EV_STOP) {
        rows = 1; cols = k.S; ld = Smax; src0 = (int64_t)c * Smax; dst0 = k.stop_off + (int64_t)k.row * k.S;
    } else if (field == EV_ATTN) {
        rows = k.S; cols = k.T; ld = Tmax; src0 = (int64_t)c * Smax * Tmax; dst0 = k.attn_off + (int64_t)k.row * k.S * k.T;
    } else if (field == EV_DIS) {
        rows = k.mT; cols = L2S_VOCAB; ld = L2S_VOCAB; src0 = (int64_t)c * mTmax * L2S_VOCAB; dst0 = k.dis_off + (int64_t)k.row * k.mT * L2S_VOCAB;
    } else {
        rows = L2S_N_MELS; cols = k.S; ld = Smax; src0 = (int64_t)c * L2S_N_MELS * Smax; dst0 = k.mel_off + (int64_t)k.row * L2S_N_MELS * k.S;
    }
    const int n = rows * cols, i0 = blockIdx.x * SCATTER_CHUNK, i1 = min(n, i0 + SCATTER_CHUNK);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const int r = i / cols, t = i - r * cols;
        dst[dst0 + i] = src[src0 + (int64_t)r * ld + t];
    }
}

int launch_eval_scatter(int field, const float* src, const EvalTab& ev, float* dst, hipStream_t s) {
    L2S_REQUIRE(src && dst && ev.clips && field >= EV_STOP && field <= EV_MEL_POST, "eval_scatter: bad arguments");
    const int64_t part = field == EV_STOP ? ev.Smax : field == EV_ATTN ? (int64_t)ev.Smax * ev.Tmax : field == EV_DIS ? (int64_t)ev.mTmax * L2S_VOCAB
                                                                                                                      : (int64_t)L2S_N_MELS * ev.Smax;
    ProfScope ps("eval_scatter_blocks", s);
    hipLaunchKernelGGL(eval_scatter_kernel, dim3((unsigned)((part + SCATTER_CHUNK - 1) / SCATTER_CHUNK), ev.N), dim3(256), 0, s, src, ev.clips, field, ev.Smax,
                       ev.Tmax, ev.mTmax, dst);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the pre-post-net mel: row-major (N, Smax, 80) -> channel-first (B_g, 80, S_g) blocks.  Block (tile of 32 steps, clip): the tile's 32 x 80 floats are
// one contiguous run (float4 loads), turned in LDS (pitch 81: a wave's 32 steps of one channel fall into 32 banks), and written as 32 consecutive steps per
// channel.  Tiles past S_c return before the barrier (the whole block does).
__global__ __launch_bounds__(256) void eval_mel_cf_kernel(const float* __restrict__ mel, const EvalClip* __restrict__ clips, int Smax, float* __restrict__ mel_cf) {
    __shared__ float tile[32][L2S_N_MELS + 1];
    const int c = blockIdx.y, j0 = blockIdx.x * 32;
    const EvalClip k = clips[c];      // block-uniform
    if (j0 >= k.S) return;
    const int nj = min(32, k.S - j0);
    const float4* src = reinterpret_cast<const float4*>(mel + ((int64_t)c * Smax + j0) * L2S_N_MELS);
    for (int i = threadIdx.x; i < nj * (L2S_N_MELS / 4); i += 256) {
        const float4 v = src[i];
        const int j = i / (L2S_N_MELS / 4), ch = (i - j * (L2S_N_MELS / 4)) * 4;
        tile[j][ch] = v.x; tile[j][ch + 1] = v.y; tile[j][ch + 2] = v.z; tile[j][ch + 3] = v.w;
    }
    __syncthreads();
    float* dst = mel_cf + k.mel_off + (int64_t)k.row * L2S_N_MELS * k.S + j0;
    const int j = threadIdx.x & 31;
    if (j < nj)
        for (int ch = threadIdx.x >> 5; ch < L2S_N_MELS; ch += 8) dst[(int64_t)ch * k.S + j] = tile[j][ch];
}

int launch_eval_mel_cf(const float* mel, const EvalTab& ev, float* mel_cf, hipStream_t s) {
    L2S_REQUIRE(mel && mel_cf && ev.clips && (reinterpret_cast<uintptr_t>(mel) & 15u) == 0, "eval_mel_cf: bad arguments");
    ProfScope ps("eval_scatter_mel_cf", s);
    hipLaunchKernelGGL(eval_mel_cf_kernel, dim3((ev.Smax + 31) / 32, ev.N), dim3(256), 0, s, mel, ev.clips, ev.Smax, mel_cf);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace l2s
