// Per-clip video lengths (the *_masked entry points of include/l2s.h): the small kernels that make row b of a zero-padded batch compute what
// clip b computes alone at T = len_b.  The LSTM cell kernels, the GEMMs and the convolutions are the unmasked ones; these kernels move, reset or
// zero the rows whose clip starts or ends inside the padded length.  (The length-masked attention blocks are in skinny.hip.)
//   length table (device, int32): lens[0..B) = len_b, lens[B..2B) = m_b = l2s_min_T(len_b)
#include "host_table.h"

namespace l2s {

// ---- the length table (host_table.h): len_b, then m_b = the min over the strided Content.agg branches (kernels 1, 3, 5, 7): the stride-7 one
static void len_table(HostTable& t, const int32_t* lens_host, int B) {
    t.i32(lens_host, B);
    int32_t* m = t.host<int32_t>(t.i32(nullptr, B));
    for (int b = 0; m && b < B; ++b) m[b] = lens_host[b] / 7;
}
int64_t len_table_words(int B) { HostTable t(false); len_table(t, nullptr, B); return t.words(); }

int launch_len_table(const int32_t* lens_host, int B, int* table, hipStream_t s) {
    HostTable t;
    len_table(t, lens_host, B);
    return t.upload(table, s);
}

// ---- the clip table of a ragged group (l2s_inference_ragged), and the pair map of its front-end: pair_clip[pair0[c] + j] = c
__global__ __launch_bounds__(64) void ragged_pair_map_kernel(const RaggedClip* __restrict__ clips, int* __restrict__ pair_clip) {
    const int c = blockIdx.x;
    const RaggedClip k = clips[c];
    for (int j = threadIdx.x; j < (k.len + 1) / 2; j += 64) pair_clip[k.pair0 + j] = c;
}

int64_t ragged_table_words(int N) { HostTable t(false); t.rec<RaggedClip>(nullptr, N); return t.words(); }

int launch_ragged_table(const RaggedClip* clips_host, int N, RaggedClip* clips_dev, int* pair_clip_dev, hipStream_t s) {
    HostTable t;
    t.rec(clips_host, N);
    if (t.upload(reinterpret_cast<int32_t*>(clips_dev), s)) return 1;
    hipLaunchKernelGGL(ragged_pair_map_kernel, dim3(N), dim3(64), 0, s, clips_dev, pair_clip_dev);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- BiLSTM, forward direction: the rows whose clip ends at frame t (len_b - 1 == t) hand over their finals - h (frag16) into the decoder's
// initial hidden state, c (plain) into the E_C input - right after the step that computed them.  One block per batch row.
__global__ __launch_bounds__(256) void bilstm_capture_kernel(const float* __restrict__ h_frag, const float* __restrict__ c_frag, const int* __restrict__ lens,
                                                             int t, float* __restrict__ h_dst_frag, float* __restrict__ c_dst, int ld_c) {
    const int b = blockIdx.x;
    if (lens[b] - 1 != t) return;
    for (int k = threadIdx.x; k < 512; k += 256) {
        const int64_t i = frag16_index(b, k, 512);
        h_dst_frag[i] = h_frag[i];
        c_dst[(int64_t)b * ld_c + k] = c_frag[i];
    }
}

// ---- BiLSTM, backward direction: the rows whose clip's last frame is t start there, from h = c = s_e, just before the step that reads frame t
__global__ __launch_bounds__(256) void bilstm_reset_kernel(float* __restrict__ h_frag, float* __restrict__ c_frag, const int* __restrict__ lens, int t,
                                                           const float* __restrict__ s_e) {
    const int b = blockIdx.x;
    if (lens[b] - 1 != t) return;
    for (int k = threadIdx.x; k < 512; k += 256) {
        const int64_t i = frag16_index(b, k, 512);
        const float v = s_e[(int64_t)b * 512 + k];
        h_frag[i] = v;
        c_frag[i] = v;
    }
}

int launch_bilstm_capture(const float* h_frag, const float* c_frag, const int* lens, int B, int t, float* h_dst_frag, float* c_dst, int ld_c, hipStream_t s) {
    ProfScope ps("bilstm_capture_rows", s);
    hipLaunchKernelGGL(bilstm_capture_kernel, dim3(B), dim3(256), 0, s, h_frag, c_frag, lens, t, h_dst_frag, c_dst, ld_c);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_bilstm_reset(float* h_frag, float* c_frag, const int* lens, int B, int t, const float* s_e, hipStream_t s) {
    ProfScope ps("bilstm_reset_rows", s);
    hipLaunchKernelGGL(bilstm_reset_kernel, dim3(B), dim3(256), 0, s, h_frag, c_frag, lens, t, s_e);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- enc rows t >= len_b become zeros, in place and in the copy the state buffer keeps: the same-pad K / V convolutions then read past a clip's end
// the zeros a solo call reads as padding.  x (B*T rows, ldx) -> also out (B*T rows, ldo), cols columns (a multiple of 4, 16-byte aligned rows)
__global__ __launch_bounds__(256) void mask_copy_rows_kernel(float* __restrict__ x, int ldx, float* __restrict__ out, int ldo, const int* __restrict__ lens,
                                                             int T, int64_t rows, int cols4) {
    const int64_t total = rows * cols4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % cols4);
        const int64_t r = idx / cols4;
        const int b = (int)(r / T), t = (int)(r - (int64_t)b * T);
        float4* px = reinterpret_cast<float4*>(x + r * ldx) + c;
        float4 v = *px;
        if (t >= lens[b]) { v = make_float4(0.f, 0.f, 0.f, 0.f); *px = v; }
        reinterpret_cast<float4*>(out + r * ldo)[c] = v;
    }
}

int launch_mask_copy_rows(float* x, int ldx, float* out, int ldo, const int* lens, int B, int T, int cols, hipStream_t s) {
    L2S_REQUIRE(cols % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0, "mask_copy_rows: float4 rows");
    const int64_t rows = (int64_t)B * T, total = rows * (cols / 4);
    int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
    if (blocks < 1) blocks = 1;
    ProfScope ps("mask_copy_rows", s);
    hipLaunchKernelGGL(mask_copy_rows_kernel, dim3(blocks), dim3(256), 0, s, x, ldx, out, ldo, lens, T, rows, cols / 4);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- pool_cat with per-row lengths: map j of row b has L_j(len_b) = len_b / div[j] valid positions (its rows are laid out for the padded length,
// p.L[j] positions per clip), pooled into m_b bins - the bins and the summation order of a solo call at T = len_b; slots i >= m_b are zeros
__global__ __launch_bounds__(256) void pool_cat_masked_kernel(const PoolCatP p, const PoolDiv d, const int* __restrict__ lens) {
    const int64_t total = (int64_t)p.B * p.m * p.nmaps * p.C;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = idx % p.C;
        int64_t r = idx / p.C;
        const int j = r % p.nmaps;
        r /= p.nmaps;
        const int i = r % p.m;
        const int b = r / p.m;
        const int len = lens[b], mb = lens[p.B + b];
        float res = 0.f;
        if (i < mb) {
            const int L = len / d.div[j];
            const int s = (i * L) / mb;
            const int e = ((i + 1) * L + mb - 1) / mb;
            const float* x = p.x[j] + (int64_t)b * p.L[j] * p.ld[j] + c;
            float acc = 0.f;
            for (int t = s; t < e; ++t) acc += x[(int64_t)t * p.ld[j]];
            res = acc / (float)(e - s);
        }
        p.out[((int64_t)b * p.m + i) * (p.nmaps * p.C) + j * p.C + c] = res;
    }
}

int launch_pool_cat_masked(const PoolCatP& p, const PoolDiv& d, const int* lens, hipStream_t s) {
    const int64_t total = (int64_t)p.B * p.m * p.nmaps * p.C;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    ProfScope ps("content_adaptive_pool_cat_masked", s);
    hipLaunchKernelGGL(pool_cat_masked_kernel, dim3(blocks), dim3(256), 0, s, p, d, lens);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- content slots i >= m_b: zero Gumbel soft-max (z, ldz columns) and zero content_dis (dis, n columns; may be null).  One block per slot row.
__global__ __launch_bounds__(256) void zero_slot_rows_kernel(float* __restrict__ z, int ldz, float* __restrict__ dis, int n, int m, int B,
                                                             const int* __restrict__ lens) {
    const int row = blockIdx.x, b = row / m, i = row - b * m;
    if (i < lens[B + b]) return;
    for (int j = threadIdx.x; j < ldz; j += 256) z[(int64_t)row * ldz + j] = 0.f;
    if (dis)
        for (int j = threadIdx.x; j < n; j += 256) dis[(int64_t)row * n + j] = 0.f;
}

int launch_zero_slot_rows(float* z, int ldz, float* dis, int n, int B, int m, const int* lens, hipStream_t s) {
    ProfScope ps("content_zero_slot_rows", s);
    hipLaunchKernelGGL(zero_slot_rows_kernel, dim3(B * m), dim3(256), 0, s, z, ldz, dis, n, m, B, lens);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace l2s
