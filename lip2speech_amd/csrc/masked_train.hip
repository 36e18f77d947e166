// Per-clip video lengths on the training path (the l2s_train_*_masked_fwd / _masked_bwd entry points of include/l2s.h): the row kernels that the masked forward and its
// backward lay over the unmasked training launches (train_encoder.hip, train_decoder.hip).  Forward pieces shared with inference are in masked_kernels.hip;
// here are the frame gather / scatter of the encoder, the taped BiLSTM reset, the adjoints of capture and reset, the masked pool_cat backward and the
// pad-row zeroing of a gradient.
//   length table (device, int32): lens[0..B) = len_b, lens[B..2B) = m_b = l2s_min_T(len_b) (the layout the masked attention blocks read), then
//   lens[2B..3B) = frame0_b = sum of len_c over c < b: clip b's first frame in the compact frame list of the encoder trunk
#include "host_table.h"

namespace l2s {

static void train_len_table(HostTable& t, const int32_t* lens_host, int B) {
    t.i32(lens_host, B);
    int32_t* m = t.host<int32_t>(t.i32(nullptr, B));
    for (int b = 0; m && b < B; ++b) m[b] = lens_host[b] / 7;
    int32_t* f0 = t.host<int32_t>(t.i32(nullptr, B));
    int32_t acc = 0;
    for (int b = 0; f0 && b < B; ++b) { f0[b] = acc; acc += lens_host[b]; }
}
int64_t train_len_table_words(int B) { HostTable t(false); train_len_table(t, nullptr, B); return t.words(); }

int launch_train_len_table(const int32_t* lens_host, int B, int* table, hipStream_t s) {
    HostTable t;
    train_len_table(t, lens_host, B);
    return t.upload(table, s);
}

// ---- encoder: rows of `cols4` float4 between the padded layout (row b*T + t) and the compact one (row frame0_b + t, t < len_b).
// to_compact: compact := the real rows of padded.  Otherwise padded := compact at real rows, ZEROS at rows t >= len_b.  Grid-stride over the padded rows.
__global__ __launch_bounds__(256) void frame_rows_kernel(const float4* __restrict__ src, float4* __restrict__ dst, const int* __restrict__ lens, int B, int T,
                                                         int64_t cols4, int to_compact) {
    const int64_t total = (int64_t)B * T * cols4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t c = idx % cols4, r = idx / cols4;
        const int b = (int)(r / T), t = (int)(r - (int64_t)b * T);
        const bool real = t < lens[b];
        const int64_t rc = (int64_t)lens[2 * B + b] + t;
        if (to_compact) { if (real) dst[rc * cols4 + c] = src[r * cols4 + c]; }
        else dst[r * cols4 + c] = real ? src[rc * cols4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

int launch_frame_rows(const float* src, float* dst, const int* lens, int B, int T, int64_t cols, bool to_compact, hipStream_t s) {
    L2S_REQUIRE(cols % 4 == 0 && lens, "frame_rows: float4 rows and a length table");
    const int64_t total = (int64_t)B * T * (cols / 4);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 16384));
    ProfScope ps(to_compact ? "train_gather_real_frames" : "train_scatter_real_frames", s);
    hipLaunchKernelGGL(frame_rows_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), lens, B, T, cols / 4,
                       to_compact ? 1 : 0);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- encoder output: the compact normalised features (sum len, C) -> vis rows [feat | emb_b] (ldv floats) and / or feat rows (C) of the padded batch;
// the C feature columns of rows t >= len_b are zeros (the embedding columns are the clip's, as on real rows).  One block per padded row.
__global__ __launch_bounds__(256) void feat_rows_store_kernel(const float* __restrict__ featc, int C, const float* __restrict__ emb, int E, const int* __restrict__ lens,
                                                              int B, int T, float* __restrict__ vis, int ldv, float* __restrict__ feat) {
    const int row = blockIdx.x, b = row / T, t = row - b * T;
    const bool real = t < lens[b];
    const float* src = featc + ((int64_t)lens[2 * B + b] + t) * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float v = real ? src[c] : 0.f;
        if (vis) vis[(int64_t)row * ldv + c] = v;
        if (feat) feat[(int64_t)row * C + c] = v;
    }
    if (vis && emb)
        for (int e = threadIdx.x; e < E; e += 256) vis[(int64_t)row * ldv + C + e] = emb[(int64_t)b * E + e];
}

int launch_feat_rows_store(const float* featc, int C, const float* emb, int E, const int* lens, int B, int T, float* vis, int ldv, float* feat, hipStream_t s) {
    L2S_REQUIRE(featc && lens && (vis || feat) && (!vis || C + E <= ldv), "feat_rows_store: bad arguments");
    ProfScope ps("train_feat_rows_store", s);
    hipLaunchKernelGGL(feat_rows_store_kernel, dim3(B * T), dim3(256), 0, s, featc, C, emb, E, lens, B, T, vis, ldv, feat);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// dfeat rows (stride ld_df) of the real frames -> compact (sum len, C).  One block per padded row; rows t >= len_b are never read
__global__ __launch_bounds__(256) void feat_rows_gather_kernel(const float* __restrict__ dfeat, int ld_df, int C, const int* __restrict__ lens, int B, int T,
                                                               float* __restrict__ out) {
    const int row = blockIdx.x, b = row / T, t = row - b * T;
    if (t >= lens[b]) return;
    float* dst = out + ((int64_t)lens[2 * B + b] + t) * C;
    for (int c = threadIdx.x; c < C; c += 256) dst[c] = dfeat[(int64_t)row * ld_df + c];
}

int launch_feat_rows_gather(const float* dfeat, int ld_df, int C, const int* lens, int B, int T, float* out, hipStream_t s) {
    ProfScope ps("train_feat_rows_gather", s);
    hipLaunchKernelGGL(feat_rows_gather_kernel, dim3(B * T), dim3(256), 0, s, dfeat, ld_df, C, lens, B, T, out);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- BiLSTM, backward direction, with the tape: the rows whose clip's last frame is t start there from h = c = s_e (bilstm_reset_kernel's rows), and the
// tape records that post-reset state as the step's predecessor (hprev / cprev: the (B,512) plain rows the step's backward reads)
__global__ __launch_bounds__(256) void bilstm_reset_tape_kernel(float* __restrict__ h_frag, float* __restrict__ c_frag, float* __restrict__ hprev,
                                                                float* __restrict__ cprev, const int* __restrict__ lens, int t, const float* __restrict__ s_e) {
    const int b = blockIdx.x;
    if (lens[b] - 1 != t) return;
    for (int k = threadIdx.x; k < 512; k += 256) {
        const int64_t i = frag16_index(b, k, 512);
        const float v = s_e[(int64_t)b * 512 + k];
        h_frag[i] = v; c_frag[i] = v;
        hprev[(int64_t)b * 512 + k] = v; cprev[(int64_t)b * 512 + k] = v;
    }
}

int launch_bilstm_reset_tape(float* h_frag, float* c_frag, float* hprev, float* cprev, const int* lens, int B, int t, const float* s_e, hipStream_t s) {
    ProfScope ps("train_bilstm_reset_rows", s);
    hipLaunchKernelGGL(bilstm_reset_tape_kernel, dim3(B), dim3(256), 0, s, h_frag, c_frag, hprev, cprev, lens, t, s_e);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- adjoint of the forward direction's capture.  The finals of a clip with len_b < T were taken after step len_b - 1, so their gradients enter there:
// before the recurrence's backward, rows with len_b < T get dh_last = 0 and dc_carry = 0 (nothing flows through their pad steps: every gate gradient
// there is then exactly 0) and d rnn_out[b][len_b - 1][0:512] += dh_init[b] (the cell backward of that step adds d rnn_out to the carried dh).
// dh_last (B,512) is written for every row: dh_init[b] where len_b == T.
__global__ __launch_bounds__(256) void bilstm_capture_adj_init_kernel(const float* __restrict__ dh_init, float* __restrict__ dh_last, float* __restrict__ dc_carry,
                                                                      float* __restrict__ drnn, int ld_rnn, const int* __restrict__ lens, int T) {
    const int b = blockIdx.x, len = lens[b];
    for (int k = threadIdx.x; k < 512; k += 256) {
        const float g = dh_init[(int64_t)b * 512 + k];
        if (len == T) { dh_last[(int64_t)b * 512 + k] = g; continue; }
        dh_last[(int64_t)b * 512 + k] = 0.f;
        dc_carry[(int64_t)b * 512 + k] = 0.f;
        drnn[((int64_t)b * T + len - 1) * ld_rnn + k] += g;
    }
}
// ... and the cell gradient of the captured c: dc_carry[b] = dcell[b] for the rows with len_b == len, just before the launch whose epilogue runs the
// cell backward of step len - 1 (dc_carry of those rows is exactly 0 until then)
__global__ __launch_bounds__(256) void bilstm_capture_adj_cell_kernel(const float* __restrict__ dcell, int ld_dcell, float* __restrict__ dc_carry,
                                                                      const int* __restrict__ lens, int len) {
    const int b = blockIdx.x;
    if (lens[b] != len) return;
    for (int k = threadIdx.x; k < 512; k += 256) dc_carry[(int64_t)b * 512 + k] = dcell[(int64_t)b * ld_dcell + k];
}

int launch_bilstm_capture_adj_init(const float* dh_init, float* dh_last, float* dc_carry, float* drnn, int ld_rnn, const int* lens, int B, int T, hipStream_t s) {
    ProfScope ps("train_bwd_bilstm_capture_rows", s);
    hipLaunchKernelGGL(bilstm_capture_adj_init_kernel, dim3(B), dim3(256), 0, s, dh_init, dh_last, dc_carry, drnn, ld_rnn, lens, T);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}
int launch_bilstm_capture_adj_cell(const float* dcell, int ld_dcell, float* dc_carry, const int* lens, int B, int len, hipStream_t s) {
    ProfScope ps("train_bwd_bilstm_capture_rows", s);
    hipLaunchKernelGGL(bilstm_capture_adj_cell_kernel, dim3(B), dim3(256), 0, s, dcell, ld_dcell, dc_carry, lens, len);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- adjoint of the backward direction's reset, just before the launch that multiplies the gate gradients of step `T - len` by W_hh: the predecessor of
// that step was s_e for the rows with len_b == len, so their gate gradients (frag16, K = 2048) move to dg_reset (the product with W_hh runs once, after
// the loop, into d s_e), their carried cell gradient goes to ds_e, and both are cut - the steps before, which read pad frames, get exact zeros
__global__ __launch_bounds__(256) void bilstm_reset_adj_kernel(float* __restrict__ dg_frag, float* __restrict__ dg_reset, float* __restrict__ dc_carry,
                                                               float* __restrict__ ds_e, const int* __restrict__ lens, int len) {
    const int b = blockIdx.x;
    if (lens[b] != len) return;
    for (int k = threadIdx.x; k < 2048; k += 256) {
        const int64_t i = frag16_index(b, k, 2048);
        dg_reset[i] = dg_frag[i];
        dg_frag[i] = 0.f;
    }
    for (int k = threadIdx.x; k < 512; k += 256) {
        ds_e[(int64_t)b * 512 + k] += dc_carry[(int64_t)b * 512 + k];
        dc_carry[(int64_t)b * 512 + k] = 0.f;
    }
}

int launch_bilstm_reset_adj(float* dg_frag, float* dg_reset, float* dc_carry, float* ds_e, const int* lens, int B, int len, hipStream_t s) {
    ProfScope ps("train_bwd_bilstm_reset_rows", s);
    hipLaunchKernelGGL(bilstm_reset_adj_kernel, dim3(B), dim3(256), 0, s, dg_frag, dg_reset, dc_carry, ds_e, lens, len);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- rows t >= len_b of x (B*T rows, ldx floats, `cols` columns) := 0: the forward replaced those rows by zeros (mask_copy_rows), so no gradient passes
__global__ __launch_bounds__(256) void zero_pad_rows_kernel(float* __restrict__ x, int ldx, const int* __restrict__ lens, int T, int64_t rows, int cols4) {
    const int64_t total = rows * cols4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % cols4);
        const int64_t r = idx / cols4;
        const int b = (int)(r / T), t = (int)(r - (int64_t)b * T);
        if (t >= lens[b]) reinterpret_cast<float4*>(x + r * ldx)[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

int launch_zero_pad_rows(float* x, int ldx, const int* lens, int B, int T, int cols, hipStream_t s, const char* name) {
    L2S_REQUIRE(cols % 4 == 0 && ldx % 4 == 0, "zero_pad_rows: float4 rows");
    const int64_t rows = (int64_t)B * T, total = rows * (cols / 4);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 8192));
    ProfScope ps(name, s);
    hipLaunchKernelGGL(zero_pad_rows_kernel, dim3(blocks), dim3(256), 0, s, x, ldx, lens, T, rows, cols / 4);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- backward of pool_cat_masked_kernel: map j of clip b has L = len_b / div[j] valid positions pooled into m_b bins (the bins of a solo call at
// T = len_b); position t < L receives dpooled / binsize of every bin that holds it, positions t >= L (rows laid out for the padded p.L[j]) receive 0.
// acc[j]: add to what dx[j] holds (the x columns of dcat), else overwrite.
__global__ __launch_bounds__(256) void pool_cat_masked_bwd_kernel(const PoolCatBwdP p, const PoolDiv d, const int* __restrict__ lens) {
    int64_t total = 0;
    for (int j = 0; j < p.nmaps; ++j) total += (int64_t)p.B * p.L[j] * p.C;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        int64_t r = idx; int j = 0;
        while (r >= (int64_t)p.B * p.L[j] * p.C) { r -= (int64_t)p.B * p.L[j] * p.C; ++j; }
        const int c = r % p.C; r /= p.C;
        const int Lp = p.L[j];
        const int t = r % Lp, b = r / Lp;
        const int mb = lens[p.B + b], L = lens[b] / d.div[j];
        float g = 0.f;
        if (t < L)
            for (int i = 0; i < mb; ++i) {
                const int st = (i * L) / mb, en = ((i + 1) * L + mb - 1) / mb;
                if (t >= st && t < en) g += p.dp[((int64_t)b * p.m + i) * (p.nmaps * p.C) + j * p.C + c] / (float)(en - st);
            }
        float* dst = p.dx[j] + ((int64_t)b * Lp + t) * p.ld[j] + c;
        *dst = p.acc[j] ? *dst + g : g;
    }
}

int launch_pool_cat_masked_bwd(const PoolCatBwdP& p, const PoolDiv& d, const int* lens, hipStream_t s) {
    ProfScope ps("train_bwd_pool_cat_masked", s);
    hipLaunchKernelGGL(pool_cat_masked_bwd_kernel, dim3(2048), dim3(256), 0, s, p, d, lens);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace l2s
