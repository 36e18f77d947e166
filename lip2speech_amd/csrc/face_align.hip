// Face alignment on the device: what the GRID / AVSpeech / in-the-wild loaders do between "decoded frame" and "aligned face" (reference:
// datasets/face_utils.py:12-103, called per frame at datasets/grid/dataset.py:216 and its avspeech / wild twins): the face box is cut out of the frame and the cut
// is rotated about its centre by the angle of the eye line, with cv2.getRotationMatrix2D and cv2.warpAffine.  Here the loader uploads the UNROTATED face-box crops,
// packed as l2s_resize_normalise reads them, and one call warps every image into a second packed buffer of the same layout: a JOB names an image and the six
// float64 of its destination-to-source map, which the host derives from the frame's landmarks (lip2speech_amd/datasets/face_utils.py).  OpenCV is absent from the
// build image: the transform is the fixed-point bilinear path of OpenCV 4.x's generic warpAffine (INTER_LINEAR, constant border 0; not its IPP or OpenCL path) as
// lip2speech_amd/datasets/face_utils.py::warp_affine_u8 restates it - PARITY UNPINNED against the package; the kernel is tested bit for bit against that
// restatement (tests/test_face_align_gpu.py).
//
// Per output pixel (x, y), rn = float64 to the nearest integer, ties to even:
//   ad = rn(m0 x 1024), bd = rn(m3 x 1024), X0 = rn((m1 y + m2) 1024) + 16, Y0 = rn((m4 y + m5) 1024) + 16, X = (X0 + ad) >> 5, Y = (Y0 + bd) >> 5,
//   sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31, weights 32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy (sum 32768),
//   out = (w00 s[sy][sx] + w01 s[sy][sx+1] + w10 s[sy+1][sx] + w11 s[sy+1][sx+1] + 16384) >> 15, a tap outside the image counting 0.
// The float64 products and sums inside rn must round one by one: contraction into fma is off for this file.
#include "l2s_common.h"
#include "../../include/l2s.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace l2s {

constexpr int AL_BAND_PIX = 1024;           // output pixels per block: whole groups of 4 (below), one per thread.  16 x 75 faces of 130 x 130 at +-15 degrees,
                                            // a call (22 launches): 245 us, 270 with 2 048 pixels, 408 with 4 096 - a launch is one wave of short blocks
constexpr int AL_LDS_DW = 15360;            // at most 60 KiB of staged source rows per block
constexpr int AL_MAX_DIM = 4096;            // H, W of an image
constexpr double AL_MAX_COORD = 16384.0;    // source coordinates of the output's corners: inside it every integer below fits 32 bits with room to spare

struct AlignTab { l2s_align_job j[L2S_ALIGN_JOBS_PER_LAUNCH]; };
static_assert(sizeof(l2s_align_job) == 64 && sizeof(AlignTab) <= 3840, "the job table travels in the kernel arguments (4 KiB with the rest)");
static_assert(AL_BAND_PIX % 4 == 0, "a band's first pixel is the first of a group of 4");

__host__ __device__ __forceinline__ int al_rn(double v) { return (int)rint(v); }

// the row terms of the map: X0, Y0 of output row y
__host__ __device__ __forceinline__ void al_row(const double* m, int y, int& X0, int& Y0) {
    const double yd = (double)y;
    X0 = al_rn((m[1] * yd + m[2]) * 1024.0) + 16;
    Y0 = al_rn((m[4] * yd + m[5]) * 1024.0) + 16;
}

// The source rows [r0, r1] inside the image that the taps of output rows [y0, y1) name (r0 > r1: none).  sy = (Y0(y) + bd(x)) >> 10 is monotonic in x and in y
// (a product by a constant, a sum with one and rn all are), so its extremes over the band lie at the band's four corners: exact, not an estimate.
__host__ __device__ __forceinline__ void al_band_rows(const double* m, int H, int W, int y0, int y1, int& r0, int& r1) {
    int lo = INT_MAX, hi = INT_MIN;
    for (int i = 0; i < 2; ++i) {
        int X0, Y0;
        al_row(m, i ? y1 - 1 : y0, X0, Y0);
        for (int k = 0; k < 2; ++k) {
            const int sy = ((Y0 + al_rn(m[3] * (double)(k ? W - 1 : 0) * 1024.0)) >> 5) >> 5;
            lo = sy < lo ? sy : lo;
            hi = sy > hi ? sy : hi;
        }
    }
    r0 = lo > 0 ? lo : 0;
    r1 = hi + 1 < H - 1 ? hi + 1 : H - 1;
}

// dwords of the aligned span that holds source rows [r0, r1] of an image of row pitch `pitch` bytes (the image starts on a 4-byte boundary, its rows follow one
// another without gaps: the rows are ONE span of bytes); lo: the span's first byte, relative to the image
__host__ __device__ __forceinline__ int al_span_dwords(int pitch, int r0, int r1, int& lo) {
    lo = (r0 * pitch) & ~3;
    return (((r1 + 1) * pitch + 3 - lo) >> 2);
}

// the aligned dword at byte a of the packed buffer; the last, partial dword of a buffer whose size is no multiple of 4 is put together from its bytes
__device__ __forceinline__ uint32_t al_load(const uint8_t* __restrict__ packed, int64_t a, int64_t packed_bytes) {
    if (a + 4 <= packed_bytes) return *reinterpret_cast<const uint32_t*>(packed + a);
    uint32_t v = 0;
    for (int i = 0; i < 4 && a + i < packed_bytes; ++i) v |= (uint32_t)packed[a + i] << (8 * i);
    return v;
}

// one output pixel, three channels.  src[i - bias] is byte i of the image: the staged span of LDS (bias = the span's first byte) or the image in global memory
// (bias = 0); the two routes read the same bytes and do the same integer arithmetic.
__device__ __forceinline__ void al_pixel(const uint8_t* __restrict__ src, int bias, int H, int W, int pitch, const double* m, int X0, int Y0, int x, int (&o)[3]) {
    const double xd = (double)x;
    const int X = (X0 + al_rn(m[0] * xd * 1024.0)) >> 5, Y = (Y0 + al_rn(m[3] * xd * 1024.0)) >> 5;
    const int sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
    const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
    const bool xa = sx >= 0 && sx < W, xb = sx + 1 >= 0 && sx + 1 < W, ya = sy >= 0 && sy < H, yb = sy + 1 >= 0 && sy + 1 < H;
    const int i0 = sy * pitch + sx * 3 - bias, i1 = i0 + pitch;
    if (xa && xb && ya && yb) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            o[c] = (w00 * (int)src[i0 + c] + w01 * (int)src[i0 + 3 + c] + w10 * (int)src[i1 + c] + w11 * (int)src[i1 + 3 + c] + 16384) >> 15;
    } else {                                           // constant border 0: a tap outside the image is never read
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int t00 = ya && xa ? (int)src[i0 + c] : 0, t01 = ya && xb ? (int)src[i0 + 3 + c] : 0;
            const int t10 = yb && xa ? (int)src[i1 + c] : 0, t11 = yb && xb ? (int)src[i1 + 3 + c] : 0;
            o[c] = (w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11 + 16384) >> 15;
        }
    }
}

struct alignas(4) AlDword3 { uint32_t a, b, c; };

// one GROUP: pixels 4 g .. 4 g + 3 of the image in row-major order, which are exactly its aligned dwords 3 g .. 3 g + 2
__device__ __forceinline__ void al_group(const uint8_t* __restrict__ src, int bias, const l2s_align_job& j, int pitch, int npix, int span4, int g,
                                         uint8_t* __restrict__ out, int64_t packed_bytes) {
    const int H = j.H, W = j.W, p = 4 * g;
    int y = p / W, x = p - y * W, X0, Y0;
    al_row(j.m, y, X0, Y0);
    int o[4][3] = {};
    if (x + 3 < W) {                                   // the four pixels lie in one row: no branch between them, their loads overlap
#pragma unroll
        for (int i = 0; i < 4; ++i) al_pixel(src, bias, H, W, pitch, j.m, X0, Y0, x + i, o[i]);
    } else {                                           // a row ends inside the group, or the image does: the pixels past its last one are the pad zeros
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (p + i < npix) {
                al_pixel(src, bias, H, W, pitch, j.m, X0, Y0, x, o[i]);
                if (++x == W) {
                    x = 0;
                    al_row(j.m, ++y, X0, Y0);
                }
            }
        }
    }
    uint32_t d[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k) d[k >> 2] |= (uint32_t)o[k / 3][k % 3] << (8 * (k & 3));
    const int a = 12 * g;
    const int64_t ga = j.offset + a;
    if (a + 12 <= span4 && ga + 12 <= packed_bytes) {
        *reinterpret_cast<AlDword3*>(out + ga) = AlDword3{d[0], d[1], d[2]};
    } else {                                           // the image's last group, or the buffer's last, partial dword
        for (int k = 0; k < 3; ++k) {
            if (a + 4 * k >= span4) break;
            if (ga + 4 * k + 4 <= packed_bytes) *reinterpret_cast<uint32_t*>(out + ga + 4 * k) = d[k];
            else
                for (int b = 0; b < 4 && ga + 4 * k + b < packed_bytes; ++b) out[ga + 4 * k + b] = (uint8_t)(d[k] >> (8 * b));
        }
    }
}

// block (x: a band of the image's output rows, y: a job of the table).  The image is one span of interleaved bytes, 3 per pixel in row-major order, that starts
// on a 4-byte boundary, so a thread that makes a group of 4 consecutive pixels of that order - wherever the rows break - makes 3 whole aligned dwords and stores
// them as such.  A band is AL_BAND_PIX consecutive pixels, whole groups: a few rows that need not start or end at a row's first pixel, so that every block has
// the same work whatever the width.  Of the image's last group only the dwords inside the image's span rounded up to 4 bytes are stored.
//   stage    the source rows that the taps of the band's rows name (al_band_rows), ONE span of bytes, by aligned dword loads, where AL_LDS_DW of LDS hold it:
//            R + W |m3| + 2 rows or so for R output rows - a few dozen for the +-15 degrees of real eye lines.  The span lies inside the image's own span
//            rounded out to 4 bytes.
//   direct   otherwise (steep angles on large images) the four taps are read from global memory.
__global__ __launch_bounds__(256) void align_faces_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t packed_bytes, const AlignTab tab,
                                                          int lds_dw) {
    extern __shared__ uint32_t s_src[];
    const l2s_align_job j = tab.j[blockIdx.y];
    const int H = j.H, W = j.W, tid = threadIdx.x;
    const int pitch = W * 3, npix = H * W, span4 = (npix * 3 + 3) & ~3;
    const int p0 = blockIdx.x * AL_BAND_PIX;
    if (p0 >= npix) return;                            // an image smaller than the launch's largest
    const int p1 = p0 + AL_BAND_PIX < npix ? p0 + AL_BAND_PIX : npix;
    const int g0 = p0 >> 2, g1 = (p1 + 3) >> 2;
    int r0, r1, lo = 0;
    al_band_rows(j.m, H, W, p0 / W, (p1 - 1) / W + 1, r0, r1);
    const int ndw = r0 <= r1 ? al_span_dwords(pitch, r0, r1, lo) : 0;
    if (ndw <= lds_dw) {                               // ndw = 0, no source row at all: every tap is the border
        // whole dwords first, with nothing between the loads, so that a thread has several in flight; only the buffer's last dword can be a partial one
        const int64_t s0 = j.offset + lo, room = (packed_bytes - s0) >> 2;
        const int nfull = room < ndw ? (int)room : ndw;
        const uint32_t* __restrict__ gsrc = reinterpret_cast<const uint32_t*>(in + s0);
#pragma unroll 8
        for (int k = tid; k < nfull; k += 256) s_src[k] = gsrc[k];
        for (int k = nfull + tid; k < ndw; k += 256) s_src[k] = al_load(in, s0 + 4 * (int64_t)k, packed_bytes);
        __syncthreads();
        for (int g = g0 + tid; g < g1; g += 256) al_group(reinterpret_cast<const uint8_t*>(s_src), lo, j, pitch, npix, span4, g, out, packed_bytes);
    } else {
        for (int g = g0 + tid; g < g1; g += 256) al_group(in + j.offset, 0, j, pitch, npix, span4, g, out, packed_bytes);
    }
}

int align_check(const l2s_align_job* jobs, int n, int64_t packed_bytes) {
    L2S_REQUIRE(n >= 0 && (n == 0 || jobs) && packed_bytes >= 0, "align: bad job table");
    std::vector<std::pair<int64_t, int>> spans;        // (offset, job)
    spans.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        const l2s_align_job& q = jobs[i];
        const std::string job = "l2s: align: job " + std::to_string(i) + ": ";
        auto fail = [&](const std::string& what) { set_error(job + what); return 1; };
        if (q.H < 1 || q.H > AL_MAX_DIM || q.W < 1 || q.W > AL_MAX_DIM)
            return fail("image " + std::to_string(q.H) + " x " + std::to_string(q.W) + " is outside [1, 4096] x [1, 4096]");
        if (q.offset < 0 || q.offset % 4 != 0) return fail("offset " + std::to_string(q.offset) + " is not a non-negative multiple of 4");
        const int64_t end = q.offset + (int64_t)q.H * q.W * 3;
        if (end > packed_bytes)
            return fail("image bytes [" + std::to_string(q.offset) + ", " + std::to_string(end) + ") lie outside the packed buffer of " + std::to_string(packed_bytes) + " bytes");
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(q.m[k])) return fail("m[" + std::to_string(k) + "] is not finite");
        for (int c = 0; c < 4; ++c) {
            const double x = (c & 1) ? q.W - 1 : 0, y = (c & 2) ? q.H - 1 : 0;
            const double u = q.m[0] * x + q.m[1] * y + q.m[2], v = q.m[3] * x + q.m[4] * y + q.m[5];
            if (!(std::fabs(u) <= AL_MAX_COORD && std::fabs(v) <= AL_MAX_COORD))
                return fail("the map sends output corner (" + std::to_string((int)x) + ", " + std::to_string((int)y) + ") to source (" + std::to_string(u) + ", " +
                            std::to_string(v) + "), outside [-16384, 16384]");
        }
        spans.emplace_back(q.offset, i);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k) {
        const l2s_align_job& p = jobs[spans[k - 1].second];
        const int64_t pend = (p.offset + (int64_t)p.H * p.W * 3 + 3) & ~(int64_t)3;
        if (spans[k].first < pend) {
            const int a = std::min(spans[k - 1].second, spans[k].second), b = std::max(spans[k - 1].second, spans[k].second);
            set_error("l2s: align: job " + std::to_string(b) + ": its bytes from " + std::to_string(jobs[b].offset) + " overlap the span of job " + std::to_string(a) +
                      ", [" + std::to_string(jobs[a].offset) + ", " + std::to_string((jobs[a].offset + (int64_t)jobs[a].H * jobs[a].W * 3 + 3) & ~(int64_t)3) +
                      ") rounded up to 4 bytes");
            return 1;
        }
    }
    return 0;
}

int launch_align_faces(const uint8_t* packed_in, int64_t packed_bytes, const l2s_align_job* jobs, int n, uint8_t* packed_out, hipStream_t s) {
    if (align_check(jobs, n, packed_bytes)) return 1;
    if (n == 0) return 0;
    L2S_REQUIRE(packed_in && packed_out, "align: null buffer");
    L2S_REQUIRE((reinterpret_cast<uintptr_t>(packed_in) & 3u) == 0 && (reinterpret_cast<uintptr_t>(packed_out) & 3u) == 0, "align: packed_in and packed_out must be 4-byte aligned");
    const uintptr_t a = reinterpret_cast<uintptr_t>(packed_in), b = reinterpret_cast<uintptr_t>(packed_out);
    L2S_REQUIRE(a + (uintptr_t)packed_bytes <= b || b + (uintptr_t)packed_bytes <= a, "align: packed_in and packed_out overlap");
    ProfScope ps("align_faces", s);
    for (int j0 = 0; j0 < n; j0 += L2S_ALIGN_JOBS_PER_LAUNCH) {
        const int nj = n - j0 < L2S_ALIGN_JOBS_PER_LAUNCH ? n - j0 : L2S_ALIGN_JOBS_PER_LAUNCH;
        AlignTab tab{};
        int pmax = 1, lds_dw = 0;
        for (int i = 0; i < nj; ++i) {
            const l2s_align_job& q = tab.j[i] = jobs[j0 + i];
            const int npix = q.H * q.W;
            pmax = std::max(pmax, npix);
            // the launch's LDS: the largest staged span of any of its bands that fits (the kernel makes the same decision from the same integers)
            for (int p0 = 0; p0 < npix; p0 += AL_BAND_PIX) {
                int r0, r1, lo;
                al_band_rows(q.m, q.H, q.W, p0 / q.W, (std::min(p0 + AL_BAND_PIX, npix) - 1) / q.W + 1, r0, r1);
                const int ndw = r0 <= r1 ? al_span_dwords(q.W * 3, r0, r1, lo) : 0;
                if (ndw <= AL_LDS_DW) lds_dw = std::max(lds_dw, ndw);
            }
        }
        const dim3 grid((pmax + AL_BAND_PIX - 1) / AL_BAND_PIX, nj);
        hipLaunchKernelGGL(align_faces_kernel, grid, dim3(256), (size_t)lds_dw * 4, s, packed_in, packed_out, packed_bytes, tab, lds_dw);
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace l2s
