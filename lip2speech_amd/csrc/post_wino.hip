// The transforms of the post-net's Winograd F(4,5) route (post_wino.h): weights once per pack / refresh, activations in and out once per layer.  The
// eight products between them are one grouped launch of the split-bf16 GEMM (gemm_x3.hip).  All three kernels are element-wise over (tile, channel quad):
// every load and store is a float4 of 128 consecutive threads = one 2-KB row, nothing is shared between threads, and the order of the sums is fixed
// by the unrolled loops below (coefficients that are exactly zero are skipped, at compile time).
#include "post_wino.h"
#include "gemm_dev.h"

namespace l2s {

int64_t wino_weights_bytes(int C) { return (int64_t)WINO_P * C * C * 4 + WINO_P * gemm_planes_bytes(C, C); }

// U[p][n][ci] = sum_k G[p][k] W[n][k * C + ci] in fp64 (a chain of fused multiply-adds, k ascending), rounded once
__global__ __launch_bounds__(256) void post_wino_weights_kernel(const float* __restrict__ W, int C, float* __restrict__ U) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)C * C) return;
    const int n = (int)(idx / C), ci = (int)(idx - (int64_t)n * C);
    double g[WINO_R];
#pragma unroll
    for (int k = 0; k < WINO_R; ++k) g[k] = (double)W[((int64_t)n * WINO_R + k) * C + ci];
#pragma unroll
    for (int p = 0; p < WINO_P; ++p) {
        double u = 0.0;
#pragma unroll
        for (int k = 0; k < WINO_R; ++k)
            if (WINO_G[p][k] != 0.0) u = fma(WINO_G[p][k], g[k], u);
        U[(int64_t)p * C * C + idx] = (float)u;
    }
}

int launch_post_wino_weights(const float* W, int C, void* out, hipStream_t s) {
    L2S_REQUIRE(W && out && C % 256 == 0, "winograd weights: C a multiple of 256");
    float* U = reinterpret_cast<float*>(out);
    {
        ProfScope ps("post_wino_weights", s);
        hipLaunchKernelGGL(post_wino_weights_kernel, dim3((unsigned)(((int64_t)C * C + 255) / 256)), dim3(256), 0, s, W, C, U);
        L2S_CHECK_HIP(hipGetLastError());
    }
    for (int p = 0; p < WINO_P; ++p)
        if (launch_gemm_planes(wino_u(out, C, p), C, C, const_cast<void*>(wino_u3(out, C, p)), s)) return 1;
    return 0;
}

// The transforms' sums run in fp64 and are rounded ONCE: a term is a dyadic constant of at most five bits times a float, so unless the terms are more than
// 2^20 apart the fp64 sum is exact and V (the GEMM's fp32 operand) and the fp32 value handed to the epilogue are the correctly rounded sums.  In fp32 the
// partial sums - up to 10x an input in BT, 8x a product in AT, cancelling in the result - were rounded at every step (measured at B = 3, S = 4 against fp64:
// 4.4x the direct layer's error with fp32 chains).  Both kernels move 384 bytes per thread for 160 fp64 FMAs: the arithmetic hides under the memory traffic.
struct Dbl4 { double x, y, z, w; };
__device__ __forceinline__ Dbl4 wino_fma(double c, const float4& x, const Dbl4& a) {
    return Dbl4{fma(c, (double)x.x, a.x), fma(c, (double)x.y, a.y), fma(c, (double)x.z, a.z), fma(c, (double)x.w, a.w)};
}

// thread = (row = clip * nt + tile, channel quad): d[i] = x[clip][4 tile - 2 + i], V_p[row] = sum_i BT[p][i] d[i], i ascending
__global__ __launch_bounds__(256) void post_wino_in_kernel(const float* __restrict__ x, int B, int S, int C, int nt, float* __restrict__ V) {
    const int cq = C >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, R = (int64_t)B * nt;
    if (idx >= R * cq) return;
    const int row = (int)(idx / cq), c = 4 * (int)(idx - (int64_t)row * cq);
    const int b = row / nt, t0 = WINO_M * (row - b * nt) - WINO_R / 2;
    float4 d[WINO_P];
#pragma unroll
    for (int i = 0; i < WINO_P; ++i) {
        const int t = t0 + i;
        d[i] = (t >= 0 && t < S) ? *reinterpret_cast<const float4*>(x + ((int64_t)b * S + t) * C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int p = 0; p < WINO_P; ++p) {
        Dbl4 v{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < WINO_P; ++i)
            if (WINO_BT[p][i] != 0.0) v = wino_fma(WINO_BT[p][i], d[i], v);
        *reinterpret_cast<float4*>(V + ((int64_t)p * R + row) * C + c) = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
    }
}

int launch_post_wino_in(const float* x, int B, int S, int C, float* V, hipStream_t s) {
    L2S_REQUIRE(x && V && B > 0 && S > 0 && C % 4 == 0, "winograd input transform: bad arguments");
    const int nt = wino_tiles(S);
    const int64_t n = (int64_t)B * nt * (C / 4);
    L2S_REQUIRE((n + 255) / 256 < (1ll << 31), "winograd input transform: too many rows");
    ProfScope ps("postnet_wino_in", s);
    hipLaunchKernelGGL(post_wino_in_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, B, S, C, nt, V);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// thread = (row, channel quad): y[clip][4 tile + i] = PSine((sum_p AT[i][p] M_p[row]) * scale + shift) + resid, p ascending; frames >= S are not written
__global__ __launch_bounds__(256) void post_wino_out_kernel(const float* __restrict__ M, int B, int S, int C, int nt, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, const float* __restrict__ actw, const float* __restrict__ resid,
                                                            float* __restrict__ y) {
    const int cq = C >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, R = (int64_t)B * nt;
    if (idx >= R * cq) return;
    const int row = (int)(idx / cq), c = 4 * (int)(idx - (int64_t)row * cq);
    const int b = row / nt, t0 = WINO_M * (row - b * nt);
    float4 m[WINO_P];
#pragma unroll
    for (int p = 0; p < WINO_P; ++p) m[p] = *reinterpret_cast<const float4*>(M + ((int64_t)p * R + row) * C + c);
    const float4 sc = *reinterpret_cast<const float4*>(scale + c), sh = *reinterpret_cast<const float4*>(shift + c);
#pragma unroll
    for (int i = 0; i < WINO_M; ++i) {
        const int t = t0 + i;
        if (t >= S) break;
        Dbl4 a{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int p = 0; p < WINO_P; ++p)
            if (WINO_AT[i][p] != 0.0) a = wino_fma(WINO_AT[i][p], m[p], a);
        const int64_t o = ((int64_t)b * S + t) * C + c;
        const float4 r = *reinterpret_cast<const float4*>(resid + o);
        float4 v;      // gemm_store's epilogue: v = acc * scale + shift (here still in fp64, rounded once), the activation, then the addend
        v.x = apply_act((float)fma(a.x, (double)sc.x, (double)sh.x), ACT_PSINE, actw, c) + r.x;
        v.y = apply_act((float)fma(a.y, (double)sc.y, (double)sh.y), ACT_PSINE, actw, c + 1) + r.y;
        v.z = apply_act((float)fma(a.z, (double)sc.z, (double)sh.z), ACT_PSINE, actw, c + 2) + r.z;
        v.w = apply_act((float)fma(a.w, (double)sc.w, (double)sh.w), ACT_PSINE, actw, c + 3) + r.w;
        *reinterpret_cast<float4*>(y + o) = v;
    }
}

int launch_post_wino_out(const float* M, int B, int S, int C, const float* scale, const float* shift, const float* actw, const float* resid, float* y, hipStream_t s) {
    L2S_REQUIRE(M && scale && shift && actw && resid && y && B > 0 && S > 0 && C % 4 == 0, "winograd output transform: bad arguments");
    const int nt = wino_tiles(S);
    const int64_t n = (int64_t)B * nt * (C / 4);
    L2S_REQUIRE((n + 255) / 256 < (1ll << 31), "winograd output transform: too many rows");
    ProfScope ps("postnet_wino_out", s);
    hipLaunchKernelGGL(post_wino_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, M, B, S, C, nt, scale, shift, actw, resid, y);
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace l2s
