// Face crops on the device: the tail of the GRID / AVSpeech / in-the-wild loaders' __getitem__ (reference: datasets/grid/dataset.py:216-236 and its avspeech / wild
// twins; LRW's face crops, datasets/lrw/dataset.py:76-79,139-141).  Every frame of those loaders yields one aligned face of its OWN size; two of them go through
// Resize((160,160)) and (x - 127.5) / 128 to the face tower, and the lower half of every one goes through Resize((96,96)), / 255 and the ImageNet Normalize to the
// model.  Here the uint8 faces cross the bus once, packed back to back, and one kernel does resize, crop, flip, rounding back to uint8 and either epilogue: a JOB
// names a source rectangle of one image, a flip bit and an output slot.  torchvision is absent from the build image: the resize is the published tensor path as
// lip2speech_amd/datasets/lrw.py::face_recog_resize restates it (bilinear, half-pixel centres, no antialias, rounded half-to-even back to uint8) - PARITY UNPINNED
// against the package; the kernel is tested against that restatement (tests/test_frame_resize_gpu.py).
#include "l2s_common.h"
#include "../../include/l2s.h"

#include <algorithm>
#include <vector>

namespace l2s {

constexpr int RS_BAND = 8;                  // output rows per block
constexpr int RS_LDS_DW = 15360;            // at most 60 KiB of staged source rows per block: with the epilogue's 3 KiB table under the 64 KiB of a block
constexpr int RS_MAX_DIM = 4096;            // H, W of an image
constexpr int64_t RS_MAX_SLOTS = 1 << 24;   // B * T

// One table entry per OUTPUT SLOT of the launch, in slot order (entry i is slot s0 + i): 16 bytes, 240 of them in the kernel arguments.  w = 0: no job names
// the slot, the block writes zeros.
struct ResizeSlot {
    int64_t base;        // byte offset in the packed buffer of the rectangle's pixel (y0, x0)
    uint16_t W;          // the image's width: the row pitch is 3 W bytes
    uint16_t h, w;       // the rectangle
    uint16_t flip;
};
struct ResizeTab { ResizeSlot s[L2S_RESIZE_JOBS_PER_LAUNCH]; };
static_assert(sizeof(ResizeTab) == 16 * L2S_RESIZE_JOBS_PER_LAUNCH && sizeof(ResizeTab) <= 3840, "the slot table travels in the kernel arguments (4 KiB with the rest)");

// torch's upsample_bilinear2d source index (align_corners = False): src = scale (dst + 0.5) - 0.5 clamped at 0, lower tap = floor, upper tap clamped at the
// last row / column, weight of the upper tap = the fraction.  fp32, no fma contraction.  i0 is clamped too, so that no rounding can index past the rectangle.
__device__ __forceinline__ void rs_tap(float scale, int d, int n, int& i0, int& i1, float& l1) {
    float s = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)d, 0.5f)), 0.5f);
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i0 = i0 > n - 1 ? n - 1 : i0;
    i1 = i0 < n - 1 ? i0 + 1 : i0;
    l1 = __fsub_rn(s, (float)i0);
}

// the aligned dword at byte a of the packed buffer; the last, partial dword of a buffer whose size is no multiple of 4 is put together from its bytes
__device__ __forceinline__ uint32_t rs_load(const uint8_t* __restrict__ packed, int64_t a, int64_t packed_bytes) {
    if (a + 4 <= packed_bytes) return *reinterpret_cast<const uint32_t*>(packed + a);
    uint32_t v = 0;
    for (int i = 0; i < 4 && a + i < packed_bytes; ++i) v |= (uint32_t)packed[a + i] << (8 * i);
    return v;
}

// block (x: a band of RS_BAND output rows, y: a slot of the table).  The band is walked in groups of rs rows, as many as the staged rows of LDS hold:
//   stage    the source rows the group's taps name, each ONCE, by aligned dword loads (one wave per row, 256 contiguous bytes per wave instruction).  Where
//            the group's tap rows are dense - upsampling, or ratios up to 2 - that is the whole span [first lower tap, last upper tap], at most 2 rs rows,
//            so a source row shared by several output rows is fetched once; at larger ratios the span has holes, and the two tap rows of every output row
//            are staged in their own pair of LDS rows instead.  A staged row starts at the dword that holds the rectangle's first byte of that source row
//            and ends at the one that holds its last: inside the image's own 4-byte-rounded span, since the image starts on a 4-byte boundary.
//   compute  a thread makes 4 consecutive output pixels of one row, all three channels: 3 x 16-byte stores, one plane per channel.
template <int MODE>
__global__ __launch_bounds__(256) void resize_normalise_kernel(const uint8_t* __restrict__ packed, int64_t packed_bytes, const ResizeTab tab, int s0, int T,
                                                               int oh, int ow, int lds_dw, float* __restrict__ out) {
    extern __shared__ uint32_t s_rows[];
    const ResizeSlot j = tab.s[blockIdx.y];
    const int slot = s0 + blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int band0 = blockIdx.x * RS_BAND;
    const int nband = oh - band0 < RS_BAND ? oh - band0 : RS_BAND;
    const int ow4 = ow >> 2;
    const int64_t P = (int64_t)oh * ow;
    float* o;
    int64_t cstride;
    if (MODE == L2S_RESIZE_MOUTH) {                    // (B,3,T,oh,ow), slot = b T + t
        const int b = slot / T, t = slot - b * T;
        o = out + ((int64_t)b * 3 * T + t) * P;
        cstride = (int64_t)T * P;
    } else {                                           // (B,2,3,oh,ow), slot = 2 b + k
        o = out + (int64_t)slot * 3 * P;
        cstride = P;
    }
    o += (int64_t)band0 * ow;
    if (j.w == 0) {                                    // a slot that no job names: exact zeros
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int it = tid; it < nband * ow4; it += 256)
            for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + c * cstride + (int64_t)it * 4) = z;
        return;
    }
    const int h = j.h, w = j.w;
    const int64_t pitch = (int64_t)j.W * 3;
    const int stride = (w * 3 + 6) >> 2;               // dwords per staged row: the rectangle's row bytes, up to 3 bytes before and 3 after
    int rs = lds_dw / (2 * stride);
    rs = rs > RS_BAND ? RS_BAND : rs;                  // >= 2 by the launch's lds_dw
    const float sy = __fdiv_rn((float)h, (float)oh), sx = __fdiv_rn((float)w, (float)ow);
    // the mouth epilogue as a table of the 3 x 256 values it can take, made by normalise_pad_kernel's three operations (IEEE division, no contraction): the same
    // bits as dividing per output value, at a twelfth of the divisions - the kernel is bound by its instructions, not by memory
    __shared__ float s_epi[MODE == L2S_RESIZE_MOUTH ? 3 * 256 : 1];
    if (MODE == L2S_RESIZE_MOUTH) {
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
        for (int c = 0; c < 3; ++c) s_epi[c * 256 + tid] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)tid, 255.0f), mean[c]), stdv[c]);
    }                                                  // read after the first barrier below
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(s_rows);
    for (int r0 = 0; r0 < nband; r0 += rs) {
        const int nr = nband - r0 < rs ? nband - r0 : rs;
        int ylo, yhi, ti;
        float tf;
        rs_tap(sy, band0 + r0, h, ylo, ti, tf);
        rs_tap(sy, band0 + r0 + nr - 1, h, ti, yhi, tf);
        const bool dense = yhi - ylo + 1 <= 2 * nr;
        const int nslots = dense ? yhi - ylo + 1 : 2 * nr;
        for (int s = wave; s < nslots; s += 4) {
            int y = ylo + s;
            if (!dense) {
                int ya, yb;
                rs_tap(sy, band0 + r0 + (s >> 1), h, ya, yb, tf);
                y = (s & 1) ? yb : ya;
            }
            const int64_t row = j.base + (int64_t)y * pitch;
            const int64_t a0 = row & ~(int64_t)3;
            const int ndw = ((int)(row - a0) + w * 3 + 3) >> 2;        // <= stride
            for (int k = lane; k < ndw; k += 64) s_rows[s * stride + k] = rs_load(packed, a0 + 4 * (int64_t)k, packed_bytes);
        }
        __syncthreads();
        for (int it = tid; it < nr * ow4; it += 256) {
            const int r = it / ow4, q = it - r * ow4;
            int ya, yb;
            float ly;
            rs_tap(sy, band0 + r0 + r, h, ya, yb, ly);
            const float hy0 = __fsub_rn(1.f, ly);
            const uint8_t* ra = sb + (dense ? ya - ylo : 2 * r) * stride * 4 + (int)((j.base + (int64_t)ya * pitch) & 3);
            const uint8_t* rb = sb + (dense ? yb - ylo : 2 * r + 1) * stride * 4 + (int)((j.base + (int64_t)yb * pitch) & 3);
            float v[3][4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                int xa, xb;
                float lx;
                rs_tap(sx, 4 * q + p, w, xa, xb, lx);
                const float wx0 = __fsub_rn(1.f, lx);
                if (j.flip) { xa = w - 1 - xa; xb = w - 1 - xb; }      // the mirrored rectangle's columns: flip, then resize
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float top = __fadd_rn(__fmul_rn(wx0, (float)ra[xa * 3 + c]), __fmul_rn(lx, (float)ra[xb * 3 + c]));
                    const float bot = __fadd_rn(__fmul_rn(wx0, (float)rb[xa * 3 + c]), __fmul_rn(lx, (float)rb[xb * 3 + c]));
                    // back to the uint8 the reference's Resize returns: round half to even, clamp
                    const float u = fminf(fmaxf(rintf(__fadd_rn(__fmul_rn(hy0, top), __fmul_rn(ly, bot))), 0.f), 255.f);
                    v[c][p] = MODE == L2S_RESIZE_MOUTH ? s_epi[c * 256 + (int)u] : __fmul_rn(__fsub_rn(u, 127.5f), 0.0078125f);      // x / 128 exactly
                }
            }
            float* dst = o + (int64_t)(r0 + r) * ow + 4 * q;
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(dst + c * cstride) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        }
        __syncthreads();
    }
}

// The host check of a job table: 0, or 1 with an error that names the job and the limit.  slot_job (optional): B T entries, the job that names each slot or -1.
static int resize_check_map(const l2s_resize_job* jobs, int n, int64_t packed_bytes, int mode, int B, int T, int oh, int ow, std::vector<int32_t>* slot_job) {
    L2S_REQUIRE(mode == L2S_RESIZE_MOUTH || mode == L2S_RESIZE_FACE, "resize: mode is not built (0 = mouth crops, 1 = face crops)");
    if (mode == L2S_RESIZE_MOUTH) L2S_REQUIRE(oh == ow && (oh == 96 || oh == 88), "resize: mouth crops are built for 96 x 96 and 88 x 88 outputs");
    else L2S_REQUIRE(oh == 160 && ow == 160 && T == 2, "resize: face crops are built for two 160 x 160 outputs per clip (T = 2)");
    L2S_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T <= RS_MAX_SLOTS, "resize: B and T must be positive and B * T at most 2^24");
    L2S_REQUIRE(n >= 0 && (n == 0 || jobs) && packed_bytes >= 0, "resize: bad job table");
    const int64_t slots = (int64_t)B * T;
    std::vector<int32_t> local;
    std::vector<int32_t>& seen = slot_job ? *slot_job : local;
    seen.assign((size_t)slots, -1);
    for (int i = 0; i < n; ++i) {
        const l2s_resize_job& q = jobs[i];
        const std::string job = "l2s: resize: job " + std::to_string(i) + ": ";
        auto fail = [&](const std::string& what) { set_error(job + what); return 1; };
        if (q.H < 1 || q.H > RS_MAX_DIM || q.W < 1 || q.W > RS_MAX_DIM)
            return fail("image " + std::to_string(q.H) + " x " + std::to_string(q.W) + " is outside [1, 4096] x [1, 4096]");
        if (q.offset < 0 || q.offset % 4 != 0) return fail("offset " + std::to_string(q.offset) + " is not a non-negative multiple of 4");
        const int64_t end = q.offset + (int64_t)q.H * q.W * 3;
        if (end > packed_bytes)
            return fail("image bytes [" + std::to_string(q.offset) + ", " + std::to_string(end) + ") lie outside the packed buffer of " + std::to_string(packed_bytes) + " bytes");
        if (q.h < 1 || q.w < 1) return fail("rectangle " + std::to_string(q.h) + " x " + std::to_string(q.w) + " is empty");
        if (q.y0 < 0 || q.x0 < 0 || (int64_t)q.y0 + q.h > q.H || (int64_t)q.x0 + q.w > q.W)
            return fail("rectangle rows [" + std::to_string(q.y0) + ", " + std::to_string((int64_t)q.y0 + q.h) + ") columns [" + std::to_string(q.x0) + ", " +
                        std::to_string((int64_t)q.x0 + q.w) + ") lies outside its " + std::to_string(q.H) + " x " + std::to_string(q.W) + " image");
        if (q.flip != 0 && q.flip != 1) return fail("flip = " + std::to_string(q.flip) + " is neither 0 nor 1");
        if (q.slot < 0 || q.slot >= slots) return fail("slot " + std::to_string(q.slot) + " is outside the output's " + std::to_string(slots) + " slots (B * T)");
        if (seen[q.slot] >= 0) return fail("slot " + std::to_string(q.slot) + " is already named by job " + std::to_string(seen[q.slot]));
        seen[q.slot] = i;
    }
    return 0;
}

int resize_check(const l2s_resize_job* jobs, int n, int64_t packed_bytes, int mode, int B, int T, int oh, int ow) {
    return resize_check_map(jobs, n, packed_bytes, mode, B, T, oh, ow, nullptr);
}

int launch_resize_normalise(const uint8_t* packed, int64_t packed_bytes, const l2s_resize_job* jobs, int n, int mode, int B, int T, int oh, int ow, float* out,
                            hipStream_t s) {
    std::vector<int32_t> slot_job;
    if (resize_check_map(jobs, n, packed_bytes, mode, B, T, oh, ow, &slot_job)) return 1;
    L2S_REQUIRE(out && (packed || n == 0), "resize: null buffer");
    L2S_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0, "resize: packed must be 4-byte, out 16-byte aligned");
    ProfScope ps("resize_normalise", s);
    const int slots = B * T;
    for (int s0 = 0; s0 < slots; s0 += L2S_RESIZE_JOBS_PER_LAUNCH) {
        const int ns = slots - s0 < L2S_RESIZE_JOBS_PER_LAUNCH ? slots - s0 : L2S_RESIZE_JOBS_PER_LAUNCH;
        ResizeTab tab{};
        int stride = 1;
        for (int i = 0; i < ns; ++i) {
            ResizeSlot& d = tab.s[i];
            if (slot_job[s0 + i] < 0) continue;
            const l2s_resize_job& q = jobs[slot_job[s0 + i]];
            d.base = q.offset + ((int64_t)q.y0 * q.W + q.x0) * 3;
            d.W = (uint16_t)q.W; d.h = (uint16_t)q.h; d.w = (uint16_t)q.w; d.flip = (uint16_t)q.flip;
            stride = std::max(stride, (q.w * 3 + 6) >> 2);
        }
        // staged rows for the launch's widest rectangle: a whole band's 2 RS_BAND rows where 60 KiB hold them, never fewer than two output rows' worth
        const int lds_dw = std::min(RS_LDS_DW, 2 * RS_BAND * stride);
        const dim3 grid((oh + RS_BAND - 1) / RS_BAND, ns);
        if (mode == L2S_RESIZE_MOUTH)
            hipLaunchKernelGGL(resize_normalise_kernel<L2S_RESIZE_MOUTH>, grid, dim3(256), (size_t)lds_dw * 4, s, packed, packed_bytes, tab, s0, T, oh, ow, lds_dw, out);
        else
            hipLaunchKernelGGL(resize_normalise_kernel<L2S_RESIZE_FACE>, grid, dim3(256), (size_t)lds_dw * 4, s, packed, packed_bytes, tab, s0, T, oh, ow, lds_dw, out);
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace l2s
