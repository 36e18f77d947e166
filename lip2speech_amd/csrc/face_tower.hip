// The face speaker tower (vgg_face.py:28-60 of the reference): facenet_pytorch's InceptionResnetV1 trunk in eval mode, then last_linear +
// last_bn, the projection Linear -> GELU -> Linear, and for inference ReLU + L2 normalisation.  160 x 160 faces only.
//
// Activations are channel-last (NHWC), rows = B*H*W.  Every convolution is one implicit GEMM on the split-bf16 matrix path of gemm_x3.hip
// (fp32 operands split into three bf16 planes while they are staged into LDS, the six partial products with weight >= 2^-16, fp32
// accumulation): row m = output pixel (b, oh, ow), column n = output channel, k = (kh, kw, ci) with ci fastest - the weight is re-laid as
// [Cout][kh][kw][Cin] when the model is packed.  The epilogue applies the folded eval BatchNorm (scale / shift), adds the residual of the
// Inception-ResNet blocks BEFORE the activation (relu(conv * s + b * s + x)) and stores at a channel offset of a wider buffer, so every
// torch.cat of the tower costs nothing.  1x1 branch heads that read the same input are one GEMM with concatenated output columns.
//
// Small maps (8 x 8 and 3 x 3: B*64 and B*9 rows) are split over K into at most 8 slices, each a raw partial product, summed in slice order
// by a finish kernel that runs the epilogue.  The split depends on the layer's per-image geometry only, never on B: a face's embedding has
// the same bits whatever else is in the batch.
#include "l2s_model.h"

namespace l2s {

constexpr int FT_M = 64, FT_N = 64, FT_K = 32;
constexpr int FT_ROW = 80;                        // bytes per LDS row: 32 bf16 + 16 pad (conflict-free ds_read_b128 for the 32x32x16 operand layout)
constexpr int FT_PLANE = FT_M * FT_ROW;           // 5 120 bytes

typedef __bf16 ft_bf16x8 __attribute__((ext_vector_type(8)));

// x = hi + mid + lo exactly (gemm_x3.hip x3_split): four consecutive k, each plane as two packed bf16 pairs
__device__ __forceinline__ void ft_split(const float4& v, uint2& hi, uint2& mid, uint2& lo) {
    const float f[4] = {v.x, v.y, v.z, v.w};
    unsigned h[4], m[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned xb = __float_as_uint(f[e]);
        const float r1 = f[e] - __uint_as_float(xb & 0xFFFF0000u);
        const float r2 = r1 - __uint_as_float(__float_as_uint(r1) & 0xFFFF0000u);
        h[e] = xb; m[e] = __float_as_uint(r1); l[e] = __float_as_uint(r2);
    }
    hi = make_uint2(__builtin_amdgcn_perm(h[1], h[0], 0x07060302u), __builtin_amdgcn_perm(h[3], h[2], 0x07060302u));
    mid = make_uint2(__builtin_amdgcn_perm(m[1], m[0], 0x07060302u), __builtin_amdgcn_perm(m[3], m[2], 0x07060302u));
    lo = make_uint2(__builtin_amdgcn_perm(l[1], l[0], 0x07060302u), __builtin_amdgcn_perm(l[3], l[2], 0x07060302u));
}

// One 64x64 output tile per block of 256 threads (4 waves, 2 x 2 sub-tiles of 32 x 32), K tiles of 32.  Thread t stages rows t/8 and
// t/8 + 32 of both operands, four consecutive k each; the next K tile's global loads are in flight while the current tile's MFMAs issue.
// NCHW: the stem - the input is the caller's (B,3,H,W) view (image b at x + b*x_bstride), read element by element (K = 27).
template <bool NCHW>
__global__ __launch_bounds__(256) void face_conv_kernel(const FaceConvP p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[6 * FT_PLANE];     // A hi/mid/lo, B hi/mid/lo
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lg = lane >> 5;
    const int m0 = blockIdx.x * FT_M, n0 = blockIdx.y * FT_N;
    const int kbeg = blockIdx.z * p.kchunk, kend = min(p.K, kbeg + p.kchunk);
    const int HoWo = p.Ho * p.Wo;

    const int r0 = tid >> 3, kq = (tid & 7) * 4;
    int ih0[2], iw0[2], ab[2]; bool av[2], wv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = m0 + r0 + 32 * j;
        av[j] = m < p.M;
        const int mm = av[j] ? m : 0;
        const int b = mm / HoWo, pix = mm - b * HoWo, oh = pix / p.Wo, ow = pix - oh * p.Wo;
        ab[j] = b; ih0[j] = oh * p.stride - p.ph; iw0[j] = ow * p.stride - p.pw;
        wv[j] = n0 + r0 + 32 * j < p.N;
    }
    auto load_a = [&](int j, int k) -> float4 {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!av[j]) return v;
        if constexpr (NCHW) {
            float e[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int kk = k + q;
                e[q] = 0.f;
                if (kk < kend) {
                    const int tap = kk / p.Cin, ci = kk - tap * p.Cin, kh = tap / p.kw, kw = tap - kh * p.kw;
                    const int ih = ih0[j] + kh, iw = iw0[j] + kw;
                    if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) e[q] = p.x[(int64_t)ab[j] * p.x_bstride + ((int64_t)ci * p.H + ih) * p.W + iw];
                }
            }
            return make_float4(e[0], e[1], e[2], e[3]);
        } else {
            if (k >= kend) return v;                                        // Cin % 4 == 0: a quad is one tap, all in or all out
            const int tap = k / p.Cin, ci = k - tap * p.Cin, kh = tap / p.kw, kw = tap - kh * p.kw;
            const int ih = ih0[j] + kh, iw = iw0[j] + kw;
            if (ih < 0 || ih >= p.H || iw < 0 || iw >= p.W) return v;
            return *reinterpret_cast<const float4*>(p.x + (((int64_t)ab[j] * p.H + ih) * p.W + iw) * p.ldx + p.xoff + ci);
        }
    };
    auto load_w = [&](int j, int k) -> float4 {
        const int n = n0 + r0 + 32 * j;
        if (!wv[j]) return make_float4(0.f, 0.f, 0.f, 0.f);
        const float* w = p.w + (int64_t)n * p.K;
        if constexpr (NCHW) {
            float e[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) e[q] = k + q < kend ? w[k + q] : 0.f;
            return make_float4(e[0], e[1], e[2], e[3]);
        } else {
            return k < kend ? *reinterpret_cast<const float4*>(w + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float4 ra[2], rw[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) { ra[j] = load_a(j, kbeg + kq); rw[j] = load_w(j, kbeg + kq); }
    const unsigned char* a_rd = smem + (wm * 32 + li) * FT_ROW + lg * 16;
    const unsigned char* b_rd = smem + 3 * FT_PLANE + (wn * 32 + li) * FT_ROW + lg * 16;
    for (int k0 = kbeg; k0 < kend; k0 += FT_K) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            unsigned char* ad = smem + (r0 + 32 * j) * FT_ROW + kq * 2;
            unsigned char* bd = ad + 3 * FT_PLANE;
            uint2 h, md, l;
            ft_split(ra[j], h, md, l);
            *reinterpret_cast<uint2*>(ad) = h; *reinterpret_cast<uint2*>(ad + FT_PLANE) = md; *reinterpret_cast<uint2*>(ad + 2 * FT_PLANE) = l;
            ft_split(rw[j], h, md, l);
            *reinterpret_cast<uint2*>(bd) = h; *reinterpret_cast<uint2*>(bd + FT_PLANE) = md; *reinterpret_cast<uint2*>(bd + 2 * FT_PLANE) = l;
        }
        __syncthreads();
        if (k0 + FT_K < kend) {
#pragma unroll
            for (int j = 0; j < 2; ++j) { ra[j] = load_a(j, k0 + FT_K + kq); rw[j] = load_w(j, k0 + FT_K + kq); }
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const ft_bf16x8 ah = *reinterpret_cast<const ft_bf16x8*>(a_rd + st * 32);
            const ft_bf16x8 am = *reinterpret_cast<const ft_bf16x8*>(a_rd + FT_PLANE + st * 32);
            const ft_bf16x8 al = *reinterpret_cast<const ft_bf16x8*>(a_rd + 2 * FT_PLANE + st * 32);
            const ft_bf16x8 bh = *reinterpret_cast<const ft_bf16x8*>(b_rd + st * 32);
            const ft_bf16x8 bm = *reinterpret_cast<const ft_bf16x8*>(b_rd + FT_PLANE + st * 32);
            const ft_bf16x8 bl = *reinterpret_cast<const ft_bf16x8*>(b_rd + 2 * FT_PLANE + st * 32);
            // smallest partial products first, as in gemm_x3.hip
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D layout of a 32x32 tile: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int col = n0 + wn * 32 + li;
    if (col >= p.N) return;
    if (p.part) {
        float* dst = p.part + (int64_t)blockIdx.z * p.M * p.N;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg;
            if (row < p.M) dst[(int64_t)row * p.N + col] = acc[r];
        }
        return;
    }
    const float sc = p.scale[col], sh = p.shift[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg;
        if (row >= p.M) continue;
        float v = acc[r] * sc + sh;
        if (p.res) v += p.res[(int64_t)row * p.ldr + col];
        if (p.relu) v = fmaxf(v, 0.f);
        p.y[(int64_t)row * p.ldy + p.yoff + col] = v;
    }
}

// the K slices of a split launch, added in slice order, then the epilogue above
__global__ __launch_bounds__(256) void face_conv_finish_kernel(const FaceConvP p, int nsplit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)p.M * p.N;
    if (i >= total) return;
    const int row = (int)(i / p.N), col = (int)(i - (int64_t)row * p.N);
    float acc = p.part[i];
    for (int z = 1; z < nsplit; ++z) acc += p.part[(int64_t)z * total + i];
    float v = acc * p.scale[col] + p.shift[col];
    if (p.res) v += p.res[(int64_t)row * p.ldr + col];
    if (p.relu) v = fmaxf(v, 0.f);
    p.y[(int64_t)row * p.ldy + p.yoff + col] = v;
}

// K slices of a layer: by its per-image output size only (never by B).  Maps of <= 9 pixels take up to 8 slices, <= 64 up to 4, each >= 128 deep.
int face_conv_splits(int HoWo, int K, int* kchunk) {
    const int want = HoWo <= 9 ? 8 : (HoWo <= 64 ? 4 : 1);
    int kc = (K + want - 1) / want;
    kc = std::max(kc, 128);
    kc = (kc + FT_K - 1) / FT_K * FT_K;
    if (kc >= K) kc = K;
    *kchunk = kc;
    return (K + kc - 1) / kc;
}

int launch_face_conv(FaceConvP p, float* part, int64_t part_floats, hipStream_t s) {
    L2S_REQUIRE(p.nchw || (p.Cin % 4 == 0 && p.ldx % 4 == 0 && p.xoff % 4 == 0 && p.K % 4 == 0), "face conv: channel counts / offsets must be multiples of 4");
    L2S_REQUIRE(p.K == p.kh * p.kw * p.Cin && p.M > 0 && p.N > 0, "face conv: bad shape");
    L2S_REQUIRE((p.nchw || p.xoff + p.Cin <= p.ldx) && p.yoff + p.N <= p.ldy && (!p.res || p.N <= p.ldr), "face conv: channel slice outside its buffer");
    const int nsplit = face_conv_splits(p.Ho * p.Wo, p.K, &p.kchunk);
    p.part = nullptr;
    if (nsplit > 1) {
        L2S_REQUIRE(part && (int64_t)nsplit * p.M * p.N <= part_floats, "face conv: split-K scratch too small");
        p.part = part;
    }
    dim3 grid((p.M + FT_M - 1) / FT_M, (p.N + FT_N - 1) / FT_N, nsplit);
    if (p.nchw) hipLaunchKernelGGL(face_conv_kernel<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(face_conv_kernel<false>, grid, dim3(256), 0, s, p);
    L2S_CHECK_HIP(hipGetLastError());
    if (nsplit > 1) {
        const int64_t total = (int64_t)p.M * p.N;
        hipLaunchKernelGGL(face_conv_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, nsplit);
        L2S_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

// MaxPool2d(3, stride 2), no padding: x (B,H,W,C) channel-last -> y[row*ldy + yoff + c]
__global__ __launch_bounds__(256) void face_maxpool_kernel(const float* __restrict__ x, int B, int H, int W, int C, int Ho, int Wo,
                                                          float* __restrict__ y, int ldy, int yoff) {
    const int C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)B * Ho * Wo * C4;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const int64_t row = i / C4;
    const int b = (int)(row / (Ho * Wo)), pix = (int)(row - (int64_t)b * Ho * Wo), oh = pix / Wo, ow = pix - oh * Wo;
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int dh = 0; dh < 3; ++dh)
        for (int dw = 0; dw < 3; ++dw) {
            const float4 v = *reinterpret_cast<const float4*>(x + (((int64_t)b * H + oh * 2 + dh) * W + ow * 2 + dw) * C + c4 * 4);
            mx.x = fmaxf(mx.x, v.x); mx.y = fmaxf(mx.y, v.y); mx.z = fmaxf(mx.z, v.z); mx.w = fmaxf(mx.w, v.w);
        }
    *reinterpret_cast<float4*>(y + row * ldy + yoff + c4 * 4) = mx;
}

static int launch_face_maxpool(const float* x, int B, int H, int W, int C, float* y, int ldy, int yoff, hipStream_t s) {
    L2S_REQUIRE(C % 4 == 0 && ldy % 4 == 0 && yoff % 4 == 0, "face maxpool: channel counts must be multiples of 4");
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(face_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, B, H, W, C, Ho, Wo, y, ldy, yoff);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// The tail, one block of 512 threads per face: AdaptiveAvgPool2d(1) over the 3 x 3 map -> last_linear (1792 -> 512) -> last_bn (folded)
// -> Linear(512, 512) -> GELU (erf) -> Linear(512, 256) = proj (forward's output) -> ReLU -> x / max(||x||, 1e-12) = emb (inference).
// Weights are stored transposed ([in][out]): thread n walks column n, consecutive threads read consecutive floats.
__global__ __launch_bounds__(512) void face_tail_kernel(const float* __restrict__ x /*(B,9,1792)*/, FaceTailW w, float* __restrict__ proj,
                                                        float* __restrict__ emb, float* __restrict__ pooled_out, float* __restrict__ bn_out) {
    __shared__ float pooled[1792];
    __shared__ float h1[512], h2[512];
    __shared__ float red[8];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* xb = x + (int64_t)b * 9 * 1792;
    for (int c = t; c < 1792; c += 512) {
        float s = 0.f;
        for (int q = 0; q < 9; ++q) s += xb[q * 1792 + c];
        pooled[c] = s / 9.0f;
        if (pooled_out) pooled_out[(int64_t)b * 1792 + c] = pooled[c];
    }
    __syncthreads();
    {
        float a = 0.f;
        for (int k = 0; k < 1792; ++k) a = fmaf(pooled[k], w.llT[(int64_t)k * 512 + t], a);
        const float v = a * w.bn_s[t] + w.bn_h[t];
        h1[t] = v;
        if (bn_out) bn_out[(int64_t)b * 512 + t] = v;
    }
    __syncthreads();
    {
        float a = w.p0b[t];
        for (int k = 0; k < 512; ++k) a = fmaf(h1[k], w.p0T[(int64_t)k * 512 + t], a);
        h2[t] = 0.5f * a * (1.0f + erff(a * 0.70710678118654752f));
    }
    __syncthreads();
    float r = 0.f;
    if (t < 256) {
        float a = w.p2b[t];
        for (int k = 0; k < 512; ++k) a = fmaf(h2[k], w.p2T[(int64_t)k * 256 + t], a);
        if (proj) proj[(int64_t)b * 256 + t] = a;
        r = fmaxf(a, 0.f);
    }
    float sq = r * r;
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if ((t & 63) == 0) red[t >> 6] = sq;
    __syncthreads();
    if (t < 256) {
        float tot = 0.f;
        for (int i = 0; i < 8; ++i) tot += red[i];
        emb[(int64_t)b * 256 + t] = r / fmaxf(sqrtf(tot), 1e-12f);
    }
}

// ------------------------------------------------------------------------------------------------ layer table
// The order in which the packer (l2s_api.hip) lays out the convolutions and face_run consumes them.  A layer with several parts is a fused
// head: one GEMM whose output columns are the parts' columns, concatenated in part order.
const std::vector<FaceLayer>& face_layers() {
    static const std::vector<FaceLayer> L = [] {
        std::vector<FaceLayer> v;
        auto bc = [&](std::vector<std::string> parts, int cin, int cout, int kh, int kw, int stride, int ph, int pw) {
            for (auto& s : parts) s = "resnet." + s;
            v.push_back({parts, cin, cout, kh, kw, stride, ph, pw, 0.f});
        };
        auto up = [&](const std::string& name, int cin, int cout, float scale) { v.push_back({{"resnet." + name}, cin, cout, 1, 1, 1, 0, 0, scale}); };
        bc({"conv2d_1a"}, 3, 32, 3, 3, 2, 0, 0);
        bc({"conv2d_2a"}, 32, 32, 3, 3, 1, 0, 0);
        bc({"conv2d_2b"}, 32, 64, 3, 3, 1, 1, 1);
        bc({"conv2d_3b"}, 64, 80, 1, 1, 1, 0, 0);
        bc({"conv2d_4a"}, 80, 192, 3, 3, 1, 0, 0);
        bc({"conv2d_4b"}, 192, 256, 3, 3, 2, 0, 0);
        for (int i = 0; i < 5; ++i) {
            const std::string p = "repeat_1." + std::to_string(i) + ".";
            bc({p + "branch0", p + "branch1.0", p + "branch2.0"}, 256, 32, 1, 1, 1, 0, 0);
            bc({p + "branch1.1"}, 32, 32, 3, 3, 1, 1, 1);
            bc({p + "branch2.1"}, 32, 32, 3, 3, 1, 1, 1);
            bc({p + "branch2.2"}, 32, 32, 3, 3, 1, 1, 1);
            up(p + "conv2d", 96, 256, 0.17f);
        }
        bc({"mixed_6a.branch0"}, 256, 384, 3, 3, 2, 0, 0);
        bc({"mixed_6a.branch1.0"}, 256, 192, 1, 1, 1, 0, 0);
        bc({"mixed_6a.branch1.1"}, 192, 192, 3, 3, 1, 1, 1);
        bc({"mixed_6a.branch1.2"}, 192, 256, 3, 3, 2, 0, 0);
        for (int i = 0; i < 10; ++i) {
            const std::string p = "repeat_2." + std::to_string(i) + ".";
            bc({p + "branch0", p + "branch1.0"}, 896, 128, 1, 1, 1, 0, 0);
            bc({p + "branch1.1"}, 128, 128, 1, 7, 1, 0, 3);
            bc({p + "branch1.2"}, 128, 128, 7, 1, 1, 3, 0);
            up(p + "conv2d", 256, 896, 0.10f);
        }
        bc({"mixed_7a.branch0.0", "mixed_7a.branch1.0", "mixed_7a.branch2.0"}, 896, 256, 1, 1, 1, 0, 0);
        bc({"mixed_7a.branch0.1"}, 256, 384, 3, 3, 2, 0, 0);
        bc({"mixed_7a.branch1.1"}, 256, 256, 3, 3, 2, 0, 0);
        bc({"mixed_7a.branch2.1"}, 256, 256, 3, 3, 1, 1, 1);
        bc({"mixed_7a.branch2.2"}, 256, 256, 3, 3, 2, 0, 0);
        for (int i = 0; i < 6; ++i) {
            const std::string p = i < 5 ? "repeat_3." + std::to_string(i) + "." : std::string("block8.");
            bc({p + "branch0", p + "branch1.0"}, 1792, 192, 1, 1, 1, 0, 0);
            bc({p + "branch1.1"}, 192, 192, 1, 3, 1, 0, 1);
            bc({p + "branch1.2"}, 192, 192, 3, 1, 1, 1, 0);
            up(p + "conv2d", 384, 1792, i < 5 ? 0.20f : 1.0f);
        }
        return v;
    }();
    return L;
}

// ------------------------------------------------------------------------------------------------ the tower
namespace {
constexpr int64_t FACE_BIG = 64 * 77 * 77;       // per image: the largest map (conv2d_2b's output)
constexpr int64_t FACE_SMALL = 192 * 17 * 17;    // per image: the largest branch temporary (mixed_6a branch1)

struct FaceRun {
    const FaceConvW* convs;
    size_t next = 0;
    int B;
    float* part; int64_t part_floats;
    bool dry; int64_t part_need = 0;            // dry: no launches, only the split-K scratch the layers need
    hipStream_t s;
    // conv from x (B,H,W,ldx) channels [xoff, xoff + Cin) into y[row*ldy + yoff + n], optional residual (ldr), ReLU
    int conv(const float* x, int H, int W, int ldx, int xoff, float* y, int ldy, int yoff, const float* res = nullptr, int ldr = 0, bool relu = true,
             int64_t x_bstride = 0, int* HoOut = nullptr) {
        L2S_REQUIRE(next < (size_t)FACE_N_CONVS, "face tower: layer table exhausted");
        const FaceLayer& L = face_layers()[next];
        const FaceConvW* c = convs ? &convs[next] : nullptr;
        ++next;
        L2S_REQUIRE(dry || (c && c->w), "face tower: weights not packed");
        FaceConvP p{};
        p.x = x; p.x_bstride = x_bstride; p.nchw = x_bstride > 0; p.H = H; p.W = W; p.ldx = ldx; p.xoff = xoff;
        if (c) { p.w = c->w; p.scale = c->scale; p.shift = c->shift; }
        p.res = res; p.ldr = ldr; p.relu = relu ? 1 : 0;
        p.y = y; p.ldy = ldy; p.yoff = yoff;
        p.Cin = L.cin; p.kh = L.kh; p.kw = L.kw; p.stride = L.stride; p.ph = L.ph; p.pw = L.pw;
        p.Ho = (H + 2 * L.ph - L.kh) / L.stride + 1; p.Wo = (W + 2 * L.pw - L.kw) / L.stride + 1;
        p.M = B * p.Ho * p.Wo; p.N = L.cout * (int)L.parts.size(); p.K = L.kh * L.kw * L.cin;
        if (HoOut) *HoOut = p.Ho;
        int kc;
        const int ns = face_conv_splits(p.Ho * p.Wo, p.K, &kc);
        if (ns > 1) part_need = std::max(part_need, (int64_t)ns * p.M * p.N);
        if (dry) return 0;
        return launch_face_conv(p, part, part_floats, s);
    }
    int pool(const float* x, int H, int W, int C, float* y, int ldy, int yoff) { return dry ? 0 : launch_face_maxpool(x, B, H, W, C, y, ldy, yoff, s); }
    int copy(const float* in, int ldi, int off_i, float* out, int ldo, int off_o, int64_t rows, int cols) {
        return dry ? 0 : launch_copy_cols(in, ldi, off_i, out, ldo, off_o, 1, rows, cols, s);
    }
    int tap(float* dst, const float* src, int64_t floats) {
        if (dry || !dst) return 0;
        L2S_CHECK_HIP(hipMemcpyAsync(dst, src, floats * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
};
}  // namespace

// the whole trunk; with r.dry only the split-K scratch the layers need is counted (no launches, the pointers are not touched)
static int face_walk(FaceRun& r, const float* faces, int64_t bstride, float* A, float* P, float* S0, float* S1, float* const* taps) {
    const int B = r.B;
    auto tapf = [&](int i) -> float* { return taps ? taps[i] : nullptr; };
    const int64_t R17 = (int64_t)B * 289, R8 = (int64_t)B * 64, R3 = (int64_t)B * 9;
    // stem: (B,3,160,160) view -> 79 x 79 x 32 -> 77 x 77 x 32 -> 77 x 77 x 64 -> max-pool 38 x 38 x 64 -> 80 -> 36 x 36 x 192 -> 17 x 17 x 256
    if (r.conv(faces, 160, 160, 3, 0, A, 32, 0, nullptr, 0, true, bstride)) return 1;
    if (r.conv(A, 79, 79, 32, 0, P, 32, 0)) return 1;
    if (r.conv(P, 77, 77, 32, 0, A, 64, 0)) return 1;
    if (r.pool(A, 77, 77, 64, P, 64, 0)) return 1;
    if (r.conv(P, 38, 38, 64, 0, A, 80, 0)) return 1;
    if (r.conv(A, 38, 38, 80, 0, P, 192, 0)) return 1;
    if (r.conv(P, 36, 36, 192, 0, A, 256, 0)) return 1;
    if (r.tap(tapf(0), A, R17 * 256)) return 1;
    // repeat_1: Block35 x 5 on A in place.  S0 = [branch0 | branch1.0 | branch2.0] (heads), branch1 -> S1, branch2 through S0's dead columns
    for (int i = 0; i < 5; ++i) {
        if (r.conv(A, 17, 17, 256, 0, S0, 96, 0)) return 1;
        if (r.conv(S0, 17, 17, 96, 32, S1, 32, 0)) return 1;          // branch1.1: S0[32:64] -> S1
        if (r.conv(S0, 17, 17, 96, 64, S0, 96, 32)) return 1;         // branch2.1: S0[64:96] -> S0[32:64] (consumed above)
        if (r.conv(S0, 17, 17, 96, 32, S0, 96, 64)) return 1;         // branch2.2: S0[32:64] -> S0[64:96]
        if (r.copy(S1, 32, 0, S0, 96, 32, R17, 32)) return 1;          // cat = [branch0 | branch1 | branch2]
        if (r.conv(S0, 17, 17, 96, 0, A, 256, 0, A, 256)) return 1;    // relu(conv(cat) * 0.17 + x)
    }
    if (r.tap(tapf(1), A, R17 * 256)) return 1;
    // mixed_6a -> P (8 x 8 x 896) = [branch0 384 | branch1 256 | max-pool 256]
    if (r.conv(A, 17, 17, 256, 0, P, 896, 0)) return 1;
    if (r.conv(A, 17, 17, 256, 0, S0, 192, 0)) return 1;
    if (r.conv(S0, 17, 17, 192, 0, S1, 192, 0)) return 1;
    if (r.conv(S1, 17, 17, 192, 0, P, 896, 384)) return 1;
    if (r.pool(A, 17, 17, 256, P, 896, 640)) return 1;
    if (r.tap(tapf(2), P, R8 * 896)) return 1;
    // repeat_2: Block17 x 10 on P in place.  S0 = [branch0 | branch1.0]; branch1.1 -> S1; branch1.2 -> S0[128:256]
    for (int i = 0; i < 10; ++i) {
        if (r.conv(P, 8, 8, 896, 0, S0, 256, 0)) return 1;
        if (r.conv(S0, 8, 8, 256, 128, S1, 128, 0)) return 1;
        if (r.conv(S1, 8, 8, 128, 0, S0, 256, 128)) return 1;
        if (r.conv(S0, 8, 8, 256, 0, P, 896, 0, P, 896)) return 1;
    }
    if (r.tap(tapf(3), P, R8 * 896)) return 1;
    // mixed_7a -> A (3 x 3 x 1792) = [branch0 384 | branch1 256 | branch2 256 | max-pool 896]; S0 = the three 1x1 heads
    if (r.conv(P, 8, 8, 896, 0, S0, 768, 0)) return 1;
    if (r.conv(S0, 8, 8, 768, 0, A, 1792, 0)) return 1;
    if (r.conv(S0, 8, 8, 768, 256, A, 1792, 384)) return 1;
    if (r.conv(S0, 8, 8, 768, 512, S1, 256, 0)) return 1;
    if (r.conv(S1, 8, 8, 256, 0, A, 1792, 640)) return 1;
    if (r.pool(P, 8, 8, 896, A, 1792, 896)) return 1;
    if (r.tap(tapf(4), A, R3 * 1792)) return 1;
    // repeat_3 (Block8 x 5) and block8 (scale 1, no ReLU) on A in place.  S0 = [branch0 | branch1.0]; branch1.1 -> S1; branch1.2 -> S0[192:384]
    for (int i = 0; i < 6; ++i) {
        if (r.conv(A, 3, 3, 1792, 0, S0, 384, 0)) return 1;
        if (r.conv(S0, 3, 3, 384, 192, S1, 192, 0)) return 1;
        if (r.conv(S1, 3, 3, 192, 0, S0, 384, 192)) return 1;
        if (r.conv(S0, 3, 3, 384, 0, A, 1792, 0, A, 1792, i < 5)) return 1;
    }
    if (r.tap(tapf(5), A, R3 * 1792)) return 1;
    L2S_REQUIRE(r.next == (size_t)FACE_N_CONVS, "face tower: layer table not consumed");
    return 0;
}

static int64_t face_part_floats(int B) {
    FaceRun r{nullptr, 0, B, nullptr, 0, true};
    if (face_walk(r, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr)) return -1;
    return r.part_need;
}

int64_t face_ws_floats(int B) {
    const int64_t part = face_part_floats(B);
    if (part < 0) return -1;
    return (int64_t)B * (2 * FACE_BIG + 2 * FACE_SMALL) + part + 64 * 6;
}

int face_run(l2s_model* m, const float* faces, int64_t bstride, int B, float* proj, float* emb, void* ws, int64_t ws_bytes, hipStream_t s,
             float* const* taps) {
    const int64_t part_floats = face_part_floats(B);
    L2S_REQUIRE(part_floats >= 0, "face tower: bad layer table");
    Bump bp(ws, ws_bytes);
    float* A = bp.f((int64_t)B * FACE_BIG); float* P = bp.f((int64_t)B * FACE_BIG);
    float* S0 = bp.f((int64_t)B * FACE_SMALL); float* S1 = bp.f((int64_t)B * FACE_SMALL);
    float* part = bp.f(std::max<int64_t>(part_floats, 1));
    L2S_REQUIRE(!bp.overflow, "face-tower workspace too small (l2s_face_workspace_bytes)");
    FaceRun r{m->w.face.convs, 0, B, part, part_floats, false};
    r.s = s;
    if (face_walk(r, faces, bstride, A, P, S0, S1, taps)) return 1;
    hipLaunchKernelGGL(face_tail_kernel, dim3(B), dim3(512), 0, s, A, m->w.face.tail, proj, emb, taps ? taps[6] : nullptr, taps ? taps[7] : nullptr);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace l2s
