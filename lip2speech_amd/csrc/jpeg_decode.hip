// Baseline JPEG decoding on the device: the first step of the LRW and in-the-wild loaders (reference: datasets/lrw/dataset.py:62-70 and its wild twin, which call
// cv2.imdecode per frame on the host).  The loader uploads the COMPRESSED byte strings, all in one buffer, and one call decodes every image into a packed buffer
// of interleaved (H_i, W_i, 3) uint8 images, the layout l2s_normalise_pad_frames, l2s_resize_normalise and l2s_align_faces read.  libjpeg's default decoder is
// integer arithmetic throughout (jidctint "islow" IDCT, triangle "fancy" chroma upsampling, fixed-point YCbCr -> RGB), so it is restated exactly:
// lip2speech_amd/datasets/jpeg.py is that restatement, equal to Pillow / libjpeg-turbo bit for bit on the committed cases, and these kernels are tested bit for bit
// against it (tests/test_jpeg_decode_gpu.py).  Parity with cv2.imdecode itself stays UNPINNED: OpenCV is absent from the build image.
//
// Three launches per call, after the tables:
//   entropy  one LANE per image: the Huffman stream is serial, the parallelism is across the call's images.  A block (one wave) takes up to JD_LANES images of ONE
//            table set, whose derived lookup tables it holds in LDS; few images per wave, so that the call spreads over the chip's compute units.  The lane writes all 64 int16 of every coefficient block of its image (zeros first, then the non-zero ones).
//            The core is ONE __host__ __device__ function, jd_entropy_image; its host instantiation is the diagnostic l2s_op_jpeg_entropy_host, through which
//            corrupt streams are tested - never on the device.
//   idct     one thread per 8 x 8 block: dequantise, columns then rows, clamp -> the component's uint8 sample plane (whole MCUs) in the workspace.  The planes are
//            staged because fancy upsampling reads the chroma row above and below, which at an MCU-row boundary is another MCU row's.
//   colour   one thread per 4 output pixels = 3 aligned dwords of the image's byte span: upsample, convert, store whole dwords (as face_align.hip does).
// Every loop is bounded by counts from the header, never by the data: at most blocks x 64 symbols per image, at most 16 bits per code, at most 8 bytes per refill,
// and a bit reader that yields zeros past its image's span or past a marker - a hostile or truncated stream costs a wrong picture and a status word.
//
// The tables - one 56-byte record per image, the entropy blocks' work list, the table sets of 4 040 bytes each - travel through the carrier of host_table.h into the
// call's workspace, not in kernel arguments: one table set alone fills the 4 KB of arguments, and the records of an LRW batch (928 images) are 52 KB; with the
// carrier all three kernels index ONE table by image whatever the call's size, at 960 words per table-writing launch.
#include "l2s_common.h"
#include "host_table.h"
#include "../../include/l2s.h"
#ifdef L2S_DIAG
#include "../../include/l2s_diag.h"
#endif

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

namespace l2s {

constexpr int JD_THREADS = 64;              // an entropy block: one wave, all of it copies the table set to LDS
constexpr int JD_LANES = 8;                 // images per entropy block, one per lane of its first lanes.  A lane's time is its own chain of dependent instructions,
                                            // whatever the other lanes do, and every store of a wave of 64 images is 64 scattered cache lines: 32 x 29 mouth frames
                                            // decode in 3.46 ms at 64 images per block, 2.76 at 16, 2.37 at 8, 2.06 at 4, 1.88 at 1; 16 x 75 faces of 146 x 120 (a
                                            // quarter of them noise, 4 x a face's bytes: the longest stream sets the time) in 11.3 ms from 64 down to 8, 12.4 at 4,
                                            // 15.3 at 1, where the blocks outnumber what the chip holds at once (profiles/jpeg_decode_times.txt)
constexpr int JD_MAX_DIM = 4096;
constexpr int JD_SET_WORDS = (int)(sizeof(l2s_jpeg_tables) / 4);
static_assert(sizeof(l2s_jpeg_huff) == 912 && sizeof(l2s_jpeg_tables) == 4040 && sizeof(l2s_jpeg_tables) % 4 == 0, "a table set is whole 32-bit words");
static_assert(sizeof(l2s_jpeg_image) == 40, "the plan's record");

// what the kernels read per image
struct JdImage {
    int64_t scan_abs;       // first byte of the entropy-coded segment in the stream buffer
    int64_t out_off;        // the image's first byte in packed_out
    int64_t blk0;           // its first 8 x 8 block in the call: coefficients at 64 blk0 int16, sample planes at 64 blk0 bytes
    int32_t scan_bytes, H, W, layout, restart, set, eoi, pad;
};
struct JdWork { int32_t set, first, count, pad; };      // an entropy block: images order[first .. first + count) share table set `set`
static_assert(sizeof(JdImage) == 56, "14 words");

// natural (row-major) position of the k-th coefficient in zigzag order: the host's copy and the device's
#define JD_ZIGZAG_LIST                                                                                                                                      \
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, \
        15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63
static const uint8_t JD_ZIGZAG[64] = {JD_ZIGZAG_LIST};
__constant__ uint8_t JD_ZIGZAG_DEV[64] = {JD_ZIGZAG_LIST};
static inline int64_t jd_align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// MCUs across and down, blocks per MCU
__host__ __device__ __forceinline__ void jd_geom(int layout, int H, int W, int& mcus_x, int& mcus_y, int& mcu_blocks) {
    const int m = layout == L2S_JPEG_420 ? 16 : 8;
    mcus_x = (W + m - 1) / m;
    mcus_y = (H + m - 1) / m;
    mcu_blocks = layout == L2S_JPEG_420 ? 6 : layout == L2S_JPEG_444 ? 3 : 1;
}
__host__ __device__ __forceinline__ int64_t jd_blocks(int layout, int H, int W) {
    int mx, my, mb;
    jd_geom(layout, H, W, mx, my, mb);
    return (int64_t)mx * my * mb;
}

struct alignas(16) JdQuad { uint32_t a, b, c, d; };
struct alignas(4) JdChunk { uint32_t a, b, c, d; };

// The bit reader of one image: bytes [0, len) of its entropy-coded segment, most significant bit first, FF 00 unstuffed on the fly.  Past the segment, and from a
// marker (FF followed by anything but 00) on, it yields zero bits and counts them in `pad`; consuming more bits than the real ones shows as nbits < pad.
// The bytes come in CHUNKS of 16, four dwords from a 4-byte boundary (the stream buffer's base is 4-byte aligned), held in four named registers: one load per 16
// bytes of stream.  The buffer's last chunk, where it is a partial one, is put together from its bytes: no byte outside [0, bytes) is read.
struct JdBits {
    const uint8_t* base;
    int64_t a0, bytes;          // a0: the segment's first byte rounded down to 4
    int32_t skew, len, pos, nbits, pad, chunk;
    uint64_t buf;
    uint32_t c0, c1, c2, c3;
    bool stopped;

    __host__ __device__ __forceinline__ void init(const uint8_t* streams, int64_t stream_bytes, int64_t scan_abs, int32_t scan_bytes) {
        base = streams, bytes = stream_bytes, a0 = scan_abs & ~(int64_t)3, skew = (int32_t)(scan_abs & 3), len = scan_bytes;
        pos = 0, nbits = 0, pad = 0, chunk = -1, buf = 0, c0 = c1 = c2 = c3 = 0, stopped = false;
    }
    __host__ __device__ __forceinline__ uint32_t byte_at(int32_t p) {      // p in [0, len)
        const int32_t q = p + skew, j = q >> 4;
        if (j != chunk) {
            chunk = j;
            const int64_t a = a0 + 16 * (int64_t)j;
            if (a + 16 <= bytes) {
                const JdChunk v = *static_cast<const JdChunk*>(__builtin_assume_aligned(base + a, 4));
                c0 = v.a, c1 = v.b, c2 = v.c, c3 = v.d;
            } else {
                c0 = c1 = c2 = c3 = 0;
#pragma unroll 1
                for (int i = 0; i < 16 && a + i < bytes; ++i) {
                    const uint32_t v = (uint32_t)base[a + i] << (8 * (i & 3));
                    if ((i >> 2) == 0) c0 |= v; else if ((i >> 2) == 1) c1 |= v; else if ((i >> 2) == 2) c2 |= v; else c3 |= v;
                }
            }
        }
        const int k = (q >> 2) & 3;
        const uint32_t w = k == 0 ? c0 : k == 1 ? c1 : k == 2 ? c2 : c3;
        return (w >> (8 * (q & 3))) & 255u;
    }
    // at least 57 bits in buf (real or zeros) - a code of up to 16 bits and its up to 15 extra bits: at most 8 bytes are taken
    __host__ __device__ __forceinline__ void refill() {
#pragma unroll 1
        for (int i = 0; i < 8 && nbits <= 56; ++i) {
            uint32_t b = 0;
            bool real = false;
            if (!stopped && pos < len) {
                b = byte_at(pos);
                real = true;
                pos += 1;
                if (b == 0xFFu) {
                    if (pos < len && byte_at(pos) == 0u) {
                        pos += 1;
                    } else {                    // a marker, or an FF that ends the segment: not data
                        pos -= 1;
                        stopped = true, real = false, b = 0;
                    }
                }
            }
            if (!real) pad += 8;
            buf |= (uint64_t)b << (56 - nbits);
            nbits += 8;
        }
    }
    __host__ __device__ __forceinline__ void drop(int n) {      // n <= 16
        buf <<= n;
        nbits -= n;
    }
};

enum { JD_ST_CODE = 1, JD_ST_END = 2, JD_ST_RESTART = 4, JD_ST_RUN = 8, JD_ST_EXTRA = 16 };      // L2S_JPEG_STATUS_* of include/l2s.h

// One image's entropy-coded segment -> its quantised coefficients: per component a plane of whole MCUs, block after block in row-major order, 64 int16 per block in
// natural (row-major) order; component after component.  `t` is the image's table set (LDS on the device), zz the zigzag table, coef the image's first block
// (16-byte aligned).  Returns the status word.  At most blocks x 64 iterations; no access outside the image's segment or its blocks x 64 coefficients.
__host__ __device__ inline int jd_entropy_image(const uint8_t* __restrict__ streams, int64_t stream_bytes, const JdImage& im, const l2s_jpeg_tables* t,
                                                const uint8_t* zz, int16_t* __restrict__ coef) {
    int mcus_x, mcus_y, mcu_blocks;
    jd_geom(im.layout, im.H, im.W, mcus_x, mcus_y, mcu_blocks);
    const int n_mcu = mcus_x * mcus_y;
    const int total = n_mcu * mcu_blocks * 64;              // <= 512 x 512 x 1.5 x 64 = 25 165 824
    const bool is420 = im.layout == L2S_JPEG_420;
    JdBits br;
    br.init(streams, stream_bytes, im.scan_abs, im.scan_bytes);
    int status = im.eoi ? 0 : JD_ST_END;
    int pred0 = 0, pred1 = 0, pred2 = 0;                      // the DC predictors, in named registers
    int mcu = 0, mx = 0, my = 0, b = 0, k = 0, comp = 0, rst_left = im.restart, rst_k = 0;
    int16_t* blk = coef;
    auto zero_block = [](int16_t* p) {
        JdQuad* q = static_cast<JdQuad*>(__builtin_assume_aligned(p, 16));
        for (int i = 0; i < 8; ++i) q[i] = JdQuad{0u, 0u, 0u, 0u};
    };
    zero_block(blk);
    for (int it = 0; it < total; ++it) {                     // one Huffman symbol per iteration: k advances by at least 1, a block ends at k = 64
        const l2s_jpeg_huff& h = t->huff[k == 0 ? (t->dc[comp] & 1) : 2 + (t->ac[comp] & 1)];
        br.refill();
        const uint32_t peek = (uint32_t)(br.buf >> 48);
        int len, sym;
        const uint32_t e = h.lut[peek >> 8];
        if (e) {
            len = (int)(e >> 8);
            sym = (int)(e & 255u);
        } else {
            int code = 0;
#pragma unroll 1
            for (len = 9; len <= 16; ++len) {
                code = (int)(peek >> (16 - len));
                if (code <= h.maxcode[len]) break;
            }
            if (len <= 16) {
                sym = h.vals[(h.valoff[len] + code) & 255];
            } else {
                status |= JD_ST_CODE;
                len = 16;
                sym = 0;
            }
        }
        br.drop(len);
        const int s = sym & 15, r = k == 0 ? 0 : sym >> 4;
        int v = 0;
        if (s) {
            v = (int)(br.buf >> (64 - s));
            br.drop(s);
            if (v < (1 << (s - 1))) v = v - (1 << s) + 1;
        }
        if (k == 0) {
            int p = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
            p = (int)((uint32_t)p + (uint32_t)v);
            if (comp == 0) pred0 = p; else if (comp == 1) pred1 = p; else pred2 = p;
            blk[0] = (int16_t)p;
            k = 1;
        } else if (s == 0) {
            k = r == 15 ? k + 16 : 64;
        } else {
            k += r;
            if (k < 64) blk[zz[k]] = (int16_t)v;
            else status |= JD_ST_RUN;
            k += 1;
        }
        if (k >= 64) {                                       // the next block
            k = 0;
            if (++b == mcu_blocks) {
                b = 0;
                if (++mcu == n_mcu) break;
                if (++mx == mcus_x) mx = 0, ++my;
                if (im.restart > 0 && --rst_left == 0) {     // byte-align, take RSTn, reset the predictors
                    if (br.nbits < br.pad) status |= JD_ST_END;
                    if (br.nbits - br.pad >= 8) status |= JD_ST_EXTRA;      // a whole data byte that nothing decoded
                    br.buf = 0, br.nbits = 0, br.pad = 0;
                    if (br.pos + 1 < br.len && br.byte_at(br.pos) == 0xFFu && br.byte_at(br.pos + 1) == (uint32_t)(0xD0 + (rst_k & 7))) {
                        br.pos += 2;
                        br.stopped = false;
                    } else {
                        status |= JD_ST_RESTART;
                    }
                    rst_k += 1;
                    rst_left = im.restart;
                    pred0 = pred1 = pred2 = 0;
                }
            }
            int64_t bi;
            if (is420) {
                comp = b < 4 ? 0 : b - 3;
                bi = b < 4 ? (int64_t)(2 * my + (b >> 1)) * (2 * mcus_x) + 2 * mx + (b & 1) : (int64_t)(b) * n_mcu + mcu;      // Cb from 4 n_mcu, Cr from 5 n_mcu
            } else {
                comp = b;
                bi = (int64_t)b * n_mcu + mcu;
            }
            blk = coef + bi * 64;
            zero_block(blk);
        }
    }
    if (mcu != n_mcu) status |= JD_ST_END;                   // cannot happen: every block ends within 64 symbols
    if (br.nbits < br.pad) status |= JD_ST_END;
    if (br.pos < br.len || br.nbits - br.pad >= 8) status |= JD_ST_EXTRA;
    return status;
}

__global__ __launch_bounds__(JD_THREADS) void jpeg_entropy_kernel(const uint8_t* __restrict__ streams, int64_t stream_bytes, const JdImage* __restrict__ imgs,
                                                                const JdWork* __restrict__ work, const int32_t* __restrict__ order,
                                                                const l2s_jpeg_tables* __restrict__ sets, int16_t* __restrict__ coef, int32_t* __restrict__ status) {
    __shared__ l2s_jpeg_tables s_set;
    __shared__ uint8_t s_zz[64];
    const JdWork w = work[blockIdx.x];
    const int tid = threadIdx.x;
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(sets + w.set);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&s_set);
    for (int i = tid; i < JD_SET_WORDS; i += JD_THREADS) dst[i] = src[i];
    s_zz[tid & 63] = JD_ZIGZAG_DEV[tid & 63];
    __syncthreads();
    if (tid < w.count) {
        const int i = order[w.first + tid];
        const JdImage im = imgs[i];
        const int st = jd_entropy_image(streams, stream_bytes, im, &s_set, s_zz, coef + im.blk0 * 64);
        if (status) status[i] = st;
    }
}

// ---- reconstruction ------------------------------------------------------------------------------------------------------------------------------------------------

constexpr int JD_FIX_0_298631336 = 2446, JD_FIX_0_390180644 = 3196, JD_FIX_0_541196100 = 4433, JD_FIX_0_765366865 = 6270, JD_FIX_0_899976223 = 7373,
              JD_FIX_1_175875602 = 9633, JD_FIX_1_501321110 = 12299, JD_FIX_1_847759065 = 15137, JD_FIX_1_961570560 = 16069, JD_FIX_2_053119869 = 16819,
              JD_FIX_2_562915447 = 20995, JD_FIX_3_072711026 = 25172;      // int(x 8192 + 0.5)

// one 1-D pass of libjpeg's jidctint over v[0..7], in place, descaled by D bits (arithmetic shifts); 32-bit arithmetic that wraps, as the restatement's does
template <int D> __host__ __device__ __forceinline__ void jd_idct_pass(int (&v)[8]) {
    auto mul = [](int a, int c) { return (int)((uint32_t)a * (uint32_t)c); };
    auto add = [](int a, int c) { return (int)((uint32_t)a + (uint32_t)c); };
    auto sub = [](int a, int c) { return (int)((uint32_t)a - (uint32_t)c); };
    auto shl13 = [](int a) { return (int)((uint32_t)a << 13); };
    int z1 = mul(add(v[2], v[6]), JD_FIX_0_541196100);
    const int t2 = sub(z1, mul(v[6], JD_FIX_1_847759065)), t3 = add(z1, mul(v[2], JD_FIX_0_765366865));
    const int t0 = shl13(add(v[0], v[4])), t1 = shl13(sub(v[0], v[4]));
    const int t10 = add(t0, t3), t13 = sub(t0, t3), t11 = add(t1, t2), t12 = sub(t1, t2);
    int a0 = v[7], a1 = v[5], a2 = v[3], a3 = v[1];
    z1 = add(a0, a3);
    int z2 = add(a1, a2), z3 = add(a0, a2), z4 = add(a1, a3);
    const int z5 = mul(add(z3, z4), JD_FIX_1_175875602);
    a0 = mul(a0, JD_FIX_0_298631336), a1 = mul(a1, JD_FIX_2_053119869), a2 = mul(a2, JD_FIX_3_072711026), a3 = mul(a3, JD_FIX_1_501321110);
    z1 = mul(z1, -JD_FIX_0_899976223), z2 = mul(z2, -JD_FIX_2_562915447);
    z3 = add(mul(z3, -JD_FIX_1_961570560), z5), z4 = add(mul(z4, -JD_FIX_0_390180644), z5);
    a0 = add(a0, add(z1, z3)), a1 = add(a1, add(z2, z4)), a2 = add(a2, add(z2, z3)), a3 = add(a3, add(z1, z4));
    constexpr int R = 1 << (D - 1);
    v[0] = add(add(t10, a3), R) >> D, v[7] = add(sub(t10, a3), R) >> D;
    v[1] = add(add(t11, a2), R) >> D, v[6] = add(sub(t11, a2), R) >> D;
    v[2] = add(add(t12, a1), R) >> D, v[5] = add(sub(t12, a1), R) >> D;
    v[3] = add(add(t13, a0), R) >> D, v[4] = add(sub(t13, a0), R) >> D;
}

// where block bi of an image lies: its component, and its rows and columns in that component's sample plane
struct JdBlockPos { int comp, brow, bcol, pitch; int64_t plane; };      // plane: the component plane's first byte, relative to the image's planes
__host__ __device__ __forceinline__ JdBlockPos jd_block_pos(int layout, int mcus_x, int mcus_y, int bi) {
    const int n_mcu = mcus_x * mcus_y;
    JdBlockPos p;
    if (layout == L2S_JPEG_420 && bi < 4 * n_mcu) {
        p.comp = 0, p.pitch = 16 * mcus_x, p.plane = 0, p.brow = bi / (2 * mcus_x), p.bcol = bi - p.brow * (2 * mcus_x);
    } else {
        const int c = layout == L2S_JPEG_420 ? bi / n_mcu - 3 : bi / n_mcu, m = bi - (layout == L2S_JPEG_420 ? c + 3 : c) * n_mcu;
        p.comp = c, p.pitch = 8 * mcus_x, p.plane = (int64_t)(layout == L2S_JPEG_420 ? c + 3 : c) * n_mcu * 64, p.brow = m / mcus_x, p.bcol = m - p.brow * mcus_x;
    }
    return p;
}

struct alignas(8) JdPair { uint32_t a, b; };

// block bi of image im: dequantise, IDCT, clamp -> its 8 x 8 samples in the component's plane
__host__ __device__ __forceinline__ void jd_idct_block(const JdImage& im, const l2s_jpeg_tables* __restrict__ sets, const int16_t* __restrict__ coef,
                                                       uint8_t* __restrict__ planes, int bi) {
    int mcus_x, mcus_y, mcu_blocks;
    jd_geom(im.layout, im.H, im.W, mcus_x, mcus_y, mcu_blocks);
    if (bi >= mcus_x * mcus_y * mcu_blocks) return;
    const JdBlockPos bp = jd_block_pos(im.layout, mcus_x, mcus_y, bi);
    const uint16_t* __restrict__ q = sets[im.set].quant[bp.comp];
    const JdQuad* __restrict__ src = reinterpret_cast<const JdQuad*>(coef + (im.blk0 + bi) * 64);
    int x[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const JdQuad c = src[r];
        const uint32_t w[4] = {c.a, c.b, c.c, c.d};
#pragma unroll
        for (int j = 0; j < 8; ++j) x[r][j] = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1))) * (int)q[r * 8 + j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {                             // columns first
        int v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = x[r][j];
        jd_idct_pass<11>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r][j] = v[r];
    }
    uint8_t* __restrict__ dst = planes + im.blk0 * 64 + bp.plane + (int64_t)(bp.brow * 8) * bp.pitch + bp.bcol * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {                             // then rows; beyond +-512 of the centre libjpeg's C path wraps where its SIMD paths saturate: this saturates
        jd_idct_pass<18>(x[r]);
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int s = (int)((uint32_t)x[r][j] + 128u);
            w[j >> 2] |= (uint32_t)(s < 0 ? 0 : s > 255 ? 255 : s) << (8 * (j & 3));
        }
        *reinterpret_cast<JdPair*>(dst + (int64_t)r * bp.pitch) = JdPair{w[0], w[1]};
    }
}
// block (x: 256 of an image's 8 x 8 blocks, y: an image): one thread per block
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JdImage* __restrict__ imgs, int img0, const l2s_jpeg_tables* __restrict__ sets,
                                                        const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
    jd_idct_block(imgs[img0 + blockIdx.y], sets, coef, planes, blockIdx.x * 256 + threadIdx.x);
}

constexpr int JD_FX_1_40200 = 91881, JD_FX_1_77200 = 116130, JD_FX_0_34414 = 22554, JD_FX_0_71414 = 46802;      // int(x 65536 + 0.5)

// libjpeg's h2v2_fancy_upsample at output pixel (y, x) of a chroma plane p (row pitch `pitch`) with ch x cw real samples, edge rows and columns replicated
__host__ __device__ __forceinline__ int jd_upsample(const uint8_t* __restrict__ p, int pitch, int ch, int cw, int y, int x) {
    const int r = y >> 1, c = x >> 1;
    const int rn = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
    const int cn = (x & 1) ? (c + 1 < cw ? c + 1 : cw - 1) : (c > 0 ? c - 1 : 0);
    const uint8_t* __restrict__ a = p + (int64_t)r * pitch;
    const uint8_t* __restrict__ b = p + (int64_t)rn * pitch;
    const int cs = 3 * (int)a[c] + (int)b[c], csn = 3 * (int)a[cn] + (int)b[cn];
    return (3 * cs + csn + ((x & 1) ? 7 : 8)) >> 4;          // at the first / last column csn = cs: (4 cs + 8) >> 4, (4 cs + 7) >> 4
}

struct alignas(4) JdDword3 { uint32_t a, b, c; };

// Group g of image im.  The image is one span of interleaved bytes that starts on a 4-byte boundary, so pixels 4 g .. 4 g + 3 of its
// row-major order are exactly its aligned dwords 3 g .. 3 g + 2, wherever the rows break.  Of the last group only the dwords inside the image's span rounded up
// to 4 bytes are stored, the pad bytes as zeros; the buffer's last, partial dword is stored byte by byte.
__host__ __device__ __forceinline__ void jd_colour_group(const JdImage& im, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, int64_t packed_bytes,
                                                         int g) {
    const int H = im.H, W = im.W, npix = H * W, span4 = (npix * 3 + 3) & ~3;
    if (4 * g >= npix) return;
    int mcus_x, mcus_y, mcu_blocks;
    jd_geom(im.layout, H, W, mcus_x, mcus_y, mcu_blocks);
    const int n_mcu = mcus_x * mcus_y;
    const uint8_t* __restrict__ yp = planes + im.blk0 * 64;
    const int ypitch = (im.layout == L2S_JPEG_420 ? 16 : 8) * mcus_x, cpitch = 8 * mcus_x;
    const uint8_t* __restrict__ cbp = yp + (int64_t)(im.layout == L2S_JPEG_420 ? 4 : 1) * n_mcu * 64;
    const uint8_t* __restrict__ crp = cbp + (int64_t)n_mcu * 64;
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    uint32_t d[3] = {0u, 0u, 0u};
    int y = (4 * g) / W, x = 4 * g - y * W;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (4 * g + i < npix) {
            const int Y = yp[(int64_t)y * ypitch + x];
            int R = Y, G = Y, B = Y;
            if (im.layout != L2S_JPEG_GREY) {
                int cb, cr;
                if (im.layout == L2S_JPEG_420) {
                    cb = jd_upsample(cbp, cpitch, ch, cw, y, x), cr = jd_upsample(crp, cpitch, ch, cw, y, x);
                } else {
                    cb = cbp[(int64_t)y * cpitch + x], cr = crp[(int64_t)y * cpitch + x];
                }
                cb -= 128, cr -= 128;
                R = Y + ((JD_FX_1_40200 * cr + 32768) >> 16);
                B = Y + ((JD_FX_1_77200 * cb + 32768) >> 16);
                G = Y + ((-JD_FX_0_34414 * cb + 32768 - JD_FX_0_71414 * cr) >> 16);
                R = R < 0 ? 0 : R > 255 ? 255 : R, G = G < 0 ? 0 : G > 255 ? 255 : G, B = B < 0 ? 0 : B > 255 ? 255 : B;
            }
            d[(3 * i) >> 2] |= (uint32_t)R << (8 * ((3 * i) & 3));
            d[(3 * i + 1) >> 2] |= (uint32_t)G << (8 * ((3 * i + 1) & 3));
            d[(3 * i + 2) >> 2] |= (uint32_t)B << (8 * ((3 * i + 2) & 3));
            if (++x == W) x = 0, ++y;
        }
    }
    const int a = 12 * g;
    const int64_t ga = im.out_off + a;
    if (a + 12 <= span4 && ga + 12 <= packed_bytes) {
        *reinterpret_cast<JdDword3*>(out + ga) = JdDword3{d[0], d[1], d[2]};
    } else {
        for (int k = 0; k < 3; ++k) {
            if (a + 4 * k >= span4) break;
            if (ga + 4 * k + 4 <= packed_bytes) *reinterpret_cast<uint32_t*>(out + ga + 4 * k) = d[k];
            else
                for (int b = 0; b < 4 && ga + 4 * k + b < packed_bytes; ++b) out[ga + 4 * k + b] = (uint8_t)(d[k] >> (8 * b));
        }
    }
}
// block (x: 256 groups of an image, y: an image): one thread per group
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JdImage* __restrict__ imgs, int img0, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out,
                                                          int64_t packed_bytes) {
    jd_colour_group(imgs[img0 + blockIdx.y], planes, out, packed_bytes, blockIdx.x * 256 + threadIdx.x);
}

// ---- host: the plan ------------------------------------------------------------------------------------------------------------------------------------------------

namespace {

struct ParsedHuff { bool have = false; uint8_t counts[16] = {}; uint8_t vals[256] = {}; int n = 0; };

void derive_huff(const ParsedHuff& p, l2s_jpeg_huff& h) {
    memset(&h, 0, sizeof(h));
    int code = 0, k = 0;
    h.maxcode[0] = h.maxcode[17] = -1;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = k - code;
        for (int i = 0; i < p.counts[l - 1]; ++i, ++code, ++k) {
            if (l <= 8)
                for (int f = 0; f < (1 << (8 - l)); ++f) h.lut[(code << (8 - l)) + f] = (uint16_t)((l << 8) | p.vals[k]);
        }
        h.maxcode[l] = p.counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    memcpy(h.vals, p.vals, 256);
}

const char* sof_name(int m) {
    switch (m) {
        case 0xC1: return "extended sequential (SOF1)";
        case 0xC2: return "progressive (SOF2)";
        case 0xC3: return "lossless (SOF3)";
        case 0xC5: return "differential sequential (SOF5)";
        case 0xC6: return "differential progressive (SOF6)";
        case 0xC7: return "differential lossless (SOF7)";
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: return "arithmetic coding (SOF9-15)";
        default: return nullptr;
    }
}

// One stream's headers -> its record (scan_offset relative to the stream) and its table set; "" or the reason it is refused.  Mirrors datasets/jpeg.py::parse_jpeg.
std::string parse_one(const uint8_t* d, int64_t n, l2s_jpeg_image& im, l2s_jpeg_tables& ts) {
    const std::string past = "a header runs past the stream";
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return "no SOI marker at the start of the stream";
    int64_t p = 2, L = 0;
    bool have_q[4] = {false, false, false, false}, have_sof = false;
    uint16_t q[4][64] = {};
    ParsedHuff ht[4];
    int nc = 0, cid[3] = {}, ch[3] = {}, cv[3] = {}, ctq[3] = {}, H = 0, W = 0, restart = 0, adobe = -1;
    const uint8_t* seg = nullptr;
    int64_t sl = 0;
    for (;;) {
        if (p + 2 > n) return past;
        if (d[p] != 0xFF) return "no marker at byte " + std::to_string(p);
        const int m = d[p + 1];
        if (m == 0xFF) { p += 1; continue; }
        p += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9) return "EOI before any scan";
        if (p + 2 > n) return past;
        L = ((int64_t)d[p] << 8) | d[p + 1];
        if (L < 2 || p + L > n) return past;
        seg = d + p + 2, sl = L - 2;
        if (const char* name = sof_name(m)) return std::string(name) + " is not supported: baseline sequential (SOF0) only";
        if (m == 0xC0) {
            if (have_sof) return "more than one frame header";
            if (sl < 6) return past;
            if (seg[0] != 8) return std::to_string((int)seg[0]) + "-bit samples are not supported: 8-bit only";
            H = (seg[1] << 8) | seg[2], W = (seg[3] << 8) | seg[4], nc = seg[5];
            if (H == 0) return "the frame header leaves the height to a DNL marker: not supported";
            if (nc == 4) return "four components (CMYK / YCCK) are not supported";
            if (nc != 1 && nc != 3) return std::to_string(nc) + " components are not supported: one (grey) or three (YCbCr)";
            if (sl < 6 + 3 * nc) return past;
            if (H < 1 || H > JD_MAX_DIM || W < 1 || W > JD_MAX_DIM) return "image " + std::to_string(H) + " x " + std::to_string(W) + " is outside [1, 4096] x [1, 4096]";
            for (int i = 0; i < nc; ++i) cid[i] = seg[6 + 3 * i], ch[i] = seg[7 + 3 * i] >> 4, cv[i] = seg[7 + 3 * i] & 15, ctq[i] = seg[8 + 3 * i];
            have_sof = true;
        } else if (m == 0xDB) {
            for (int64_t o = 0; o < sl;) {
                const int pq = seg[o] >> 4, tq = seg[o] & 15;
                if (pq != 0) return "16-bit quantisation tables are not supported: 8-bit only";
                if (tq > 3) return "quantisation table id " + std::to_string(tq) + " is outside [0, 3]";
                if (o + 65 > sl) return past;
                for (int k = 0; k < 64; ++k) q[tq][JD_ZIGZAG[k]] = seg[o + 1 + k];      // natural order
                have_q[tq] = true;
                o += 65;
            }
        } else if (m == 0xC4) {
            for (int64_t o = 0; o < sl;) {
                const int tc = seg[o] >> 4, th = seg[o] & 15;
                if (tc > 1 || th > 1) return "Huffman table class " + std::to_string(tc) + " id " + std::to_string(th) + ": baseline has classes 0 / 1 and ids 0 / 1";
                if (o + 17 > sl) return past;
                ParsedHuff& t = ht[tc * 2 + th];
                t = ParsedHuff();
                int nv = 0, code = 0;
                for (int l = 0; l < 16; ++l) t.counts[l] = seg[o + 1 + l], nv += t.counts[l];
                if (nv > 256) return "a Huffman table holds more than 256 codes";
                if (o + 17 + nv > sl) return past;
                for (int l = 0; l < 16; ++l) {
                    code += t.counts[l];
                    if (code > (2 << l)) return "a Huffman table assigns more codes than its lengths allow";
                    code <<= 1;
                }
                for (int k = 0; k < nv; ++k) {
                    t.vals[k] = seg[o + 17 + k];
                    if (tc == 0 && t.vals[k] > 15) return "a DC Huffman table names a category above 15";
                }
                t.n = nv, t.have = true;
                o += 17 + nv;
            }
        } else if (m == 0xDD) {
            if (sl < 2) return past;
            restart = (seg[0] << 8) | seg[1];
        } else if (m == 0xDC) {
            return "a DNL marker is not supported";
        } else if (m == 0xEE && sl >= 12 && memcmp(seg, "Adobe", 5) == 0) {
            adobe = seg[11];
        } else if (m == 0xDA) {
            break;
        }
        p += L;
    }
    if (!have_sof) return "a scan before the frame header";
    const int ns = sl >= 1 ? seg[0] : 0;
    if (sl < 1 + 2 * ns + 3) return past;
    if (ns != nc) return "the scan holds " + std::to_string(ns) + " of the frame's " + std::to_string(nc) + " components: more than one scan is not supported";
    int td[3] = {}, ta[3] = {};
    for (int i = 0; i < nc; ++i) {
        if (seg[1 + 2 * i] != cid[i]) return "the scan's components are not the frame's, in order";
        td[i] = seg[2 + 2 * i] >> 4, ta[i] = seg[2 + 2 * i] & 15;
    }
    if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) return "the scan is not a whole sequential one (Ss, Se, Ah / Al = 0, 63, 0)";
    int layout = L2S_JPEG_GREY;
    if (nc == 3) {
        if (adobe == 0 || (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B'))
            return "RGB-coded components (Adobe transform 0, or component ids R, G, B) are not supported: YCbCr only";
        const bool c11 = ch[1] == 1 && cv[1] == 1 && ch[2] == 1 && cv[2] == 1;
        if (c11 && ch[0] == 2 && cv[0] == 2) layout = L2S_JPEG_420;
        else if (c11 && ch[0] == 1 && cv[0] == 1) layout = L2S_JPEG_444;
        else {
            std::string s = "sampling factors ";
            for (int i = 0; i < 3; ++i) s += std::to_string(ch[i]) + "x" + std::to_string(cv[i]) + (i < 2 ? " / " : "");
            return s + " are not supported: 2x2 / 1x1 / 1x1 (4:2:0) or all 1x1 (4:4:4)";
        }
    }
    memset(&ts, 0, sizeof(ts));
    for (int i = 0; i < nc; ++i) {
        if (ctq[i] > 3 || !have_q[ctq[i]])
            return "component " + std::to_string(cid[i]) + " names quantisation table " + std::to_string(ctq[i]) + ", which was never defined";
        if (td[i] > 1 || ta[i] > 1 || !ht[td[i]].have || !ht[2 + ta[i]].have)
            return "the scan names Huffman table DC " + std::to_string(td[i]) + " / AC " + std::to_string(ta[i]) + " for component " + std::to_string(cid[i]) +
                   ", which was never defined";
        memcpy(ts.quant[i], q[ctq[i]], sizeof(ts.quant[i]));
        ts.dc[i] = (uint8_t)td[i], ts.ac[i] = (uint8_t)ta[i];
    }
    for (int i = 0; i < nc; ++i) {                           // only the tables the scan uses: two streams that differ in an unused table share a set
        derive_huff(ht[td[i]], ts.huff[td[i]]);
        derive_huff(ht[2 + ta[i]], ts.huff[2 + ta[i]]);
    }
    const int64_t s0 = p + L;
    int64_t e = s0;
    bool eoi = false;
    for (;;) {                                               // the entropy-coded segment ends at the first marker that is neither a stuffed FF 00 nor RSTn
        const uint8_t* f = e < n ? (const uint8_t*)memchr(d + e, 0xFF, (size_t)(n - e)) : nullptr;
        if (!f || f + 1 >= d + n) { e = f ? f - d : n; break; }
        e = f - d;
        const int m = f[1];
        if (m == 0 || (m >= 0xD0 && m <= 0xD7)) { e += 2; continue; }
        if (m == 0xD9) eoi = true;
        else if (m == 0xDC) return "a DNL marker is not supported";
        else if (m == 0xDA || m == 0xC4 || m == 0xDB || (m >= 0xC0 && m <= 0xCF && m != 0xC8)) return "more than one scan is not supported";
        break;
    }
    if (e - s0 > INT32_MAX) return "the scan is longer than 2^31 bytes";
    im.scan_offset = s0, im.scan_bytes = (int32_t)(e - s0), im.H = H, im.W = W, im.layout = layout, im.restart = restart, im.table_set = -1, im.eoi = eoi ? 1 : 0,
    im.reserved = 0;
    return "";
}

// what every entry point that takes records refuses: `what` names the entry point
int check_images(const char* what, const l2s_jpeg_image* images, int n, int n_sets, int64_t stream_bytes) {
    L2S_REQUIRE(n >= 0 && (n == 0 || images) && n_sets >= 0, "jpeg: bad record table");
    for (int i = 0; i < n; ++i) {
        const l2s_jpeg_image& r = images[i];
        auto fail = [&](const std::string& why) { set_error(std::string("l2s: ") + what + ": image " + std::to_string(i) + ": " + why); return 1; };
        if (r.H < 1 || r.H > JD_MAX_DIM || r.W < 1 || r.W > JD_MAX_DIM)
            return fail("image " + std::to_string(r.H) + " x " + std::to_string(r.W) + " is outside [1, 4096] x [1, 4096]");
        if (r.layout != L2S_JPEG_GREY && r.layout != L2S_JPEG_444 && r.layout != L2S_JPEG_420) return fail("layout " + std::to_string(r.layout) + " is not one of L2S_JPEG_*");
        if (r.restart < 0 || r.restart > 65535) return fail("restart interval " + std::to_string(r.restart) + " is outside [0, 65535]");
        if (r.table_set < 0 || r.table_set >= n_sets) return fail("table set " + std::to_string(r.table_set) + " is outside [0, " + std::to_string(n_sets) + ")");
        if (r.scan_offset < 0 || r.scan_bytes < 0 || (stream_bytes >= 0 && r.scan_offset + r.scan_bytes > stream_bytes))
            return fail("scan bytes [" + std::to_string(r.scan_offset) + ", " + std::to_string(r.scan_offset + r.scan_bytes) + ") lie outside the stream buffer of " +
                        std::to_string(stream_bytes) + " bytes");
    }
    return 0;
}

// The call's layout: the table (records, work list, order, sets) at the head of the workspace, then the coefficients, then the sample planes.
struct JdLayout {
    int64_t off_img = 0, off_work = 0, off_order = 0, off_sets = 0, n_work = 0, blocks = 0, coef_off = 0, plane_off = 0, bytes = 0;
};
JdLayout build_layout(HostTable& t, const l2s_jpeg_image* images, int n, const l2s_jpeg_tables* sets, int n_sets, const int64_t* out_offsets) {
    JdLayout lay;
    std::vector<JdImage> recs((size_t)n);
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return images[a].table_set < images[b].table_set; });
    std::vector<JdWork> work;
    for (int i = 0; i < n;) {
        int j = i;
        while (j < n && j - i < JD_LANES && images[order[j]].table_set == images[order[i]].table_set) ++j;
        work.push_back(JdWork{images[order[i]].table_set, i, j - i, 0});
        i = j;
    }
    for (int i = 0; i < n; ++i) {
        const l2s_jpeg_image& r = images[i];
        recs[i] = JdImage{r.scan_offset, out_offsets ? out_offsets[i] : 0, lay.blocks, r.scan_bytes, r.H, r.W, r.layout, r.restart, r.table_set, r.eoi, 0};
        lay.blocks += jd_blocks(r.layout, r.H, r.W);
    }
    lay.n_work = (int64_t)work.size();
    lay.off_img = t.rec<JdImage>(recs.data(), n);
    lay.off_work = t.rec<JdWork>(work.data(), lay.n_work);
    lay.off_order = t.i32(order.data(), n);
    lay.off_sets = t.rec<l2s_jpeg_tables>(sets, n_sets);
    lay.coef_off = jd_align_up(t.words() * 4, 256);
    lay.plane_off = lay.coef_off + jd_align_up(lay.blocks * 128, 256);
    lay.bytes = lay.plane_off + jd_align_up(lay.blocks * 64, 256);
    return lay;
}

}  // namespace
}  // namespace l2s

using namespace l2s;

extern "C" {

int l2s_jpeg_plan(const uint8_t* streams, const int64_t* offsets, const int64_t* sizes, int n, l2s_jpeg_image* images, l2s_jpeg_tables* sets, int sets_cap,
                  int* n_sets) {
    L2S_REQUIRE(n >= 0 && sets_cap >= 0 && n_sets && (n == 0 || (streams && offsets && sizes && images)) && (sets_cap == 0 || sets), "jpeg plan: bad arguments");
    int ns = 0;
    l2s_jpeg_tables ts;
    for (int i = 0; i < n; ++i) {
        auto fail = [&](const std::string& why) { set_error("l2s: jpeg plan: image " + std::to_string(i) + ": " + why); return 1; };
        if (offsets[i] < 0 || sizes[i] < 0) return fail("negative offset or size");
        const std::string why = parse_one(streams + offsets[i], sizes[i], images[i], ts);
        if (!why.empty()) return fail(why);
        images[i].scan_offset += offsets[i];
        int s = 0;
        while (s < ns && memcmp(&sets[s], &ts, sizeof(ts)) != 0) ++s;
        if (s == ns) {
            if (ns >= sets_cap) return fail("its tables are the call's table set " + std::to_string(ns) + ", and there is room for " + std::to_string(sets_cap));
            sets[ns++] = ts;
        }
        images[i].table_set = s;
    }
    *n_sets = ns;
    return 0;
}

int64_t l2s_jpeg_workspace_bytes(const l2s_jpeg_image* images, int n, int n_sets) {
    if (check_images("jpeg workspace", images, n, n_sets, -1)) return -1;
    HostTable t(false);
    return build_layout(t, images, n, nullptr, n_sets, nullptr).bytes;
}

int l2s_jpeg_decode(const uint8_t* streams, int64_t stream_bytes, const l2s_jpeg_image* images, int n, const l2s_jpeg_tables* sets, int n_sets,
                    const int64_t* out_offsets, uint8_t* packed_out, int64_t packed_bytes, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L2S_REQUIRE(stream_bytes >= 0 && packed_bytes >= 0 && (n_sets == 0 || sets) && (n <= 0 || out_offsets), "jpeg decode: bad arguments");
    if (check_images("jpeg decode", images, n, n_sets, stream_bytes)) return 1;
    if (n == 0) return 0;
    std::vector<std::pair<int64_t, int>> spans;        // (offset, image)
    spans.reserve((size_t)n);
    auto end4 = [&](int i) { return (out_offsets[i] + (int64_t)images[i].H * images[i].W * 3 + 3) & ~(int64_t)3; };
    for (int i = 0; i < n; ++i) {
        const std::string img = "l2s: jpeg decode: image " + std::to_string(i) + ": ";
        const int64_t o = out_offsets[i], end = o + (int64_t)images[i].H * images[i].W * 3;
        if (o < 0 || o % 4 != 0) { set_error(img + "output offset " + std::to_string(o) + " is not a non-negative multiple of 4"); return 1; }
        if (end > packed_bytes) {
            set_error(img + "output bytes [" + std::to_string(o) + ", " + std::to_string(end) + ") lie outside the packed buffer of " + std::to_string(packed_bytes) + " bytes");
            return 1;
        }
        spans.emplace_back(o, i);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k) {
        if (spans[k].first < end4(spans[k - 1].second)) {
            const int a = std::min(spans[k - 1].second, spans[k].second), b = std::max(spans[k - 1].second, spans[k].second);
            set_error("l2s: jpeg decode: image " + std::to_string(b) + ": its output bytes from " + std::to_string(out_offsets[b]) + " overlap the span of image " +
                      std::to_string(a) + ", [" + std::to_string(out_offsets[a]) + ", " + std::to_string(end4(a)) + ") rounded up to 4 bytes");
            return 1;
        }
    }
    L2S_REQUIRE(streams && packed_out && ws, "jpeg decode: null buffer");
    L2S_REQUIRE((reinterpret_cast<uintptr_t>(streams) & 3u) == 0 && (reinterpret_cast<uintptr_t>(packed_out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 255u) == 0,
                "jpeg decode: streams and packed_out must be 4-byte aligned, the workspace 256-byte aligned");
    HostTable t;
    const JdLayout lay = build_layout(t, images, n, sets, n_sets, out_offsets);
    L2S_REQUIRE(ws_bytes >= lay.bytes, "jpeg decode: workspace too small (l2s_jpeg_workspace_bytes)");
    auto disjoint = [](const void* p, int64_t pn, const void* q, int64_t qn) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
        return a + (uintptr_t)pn <= b || b + (uintptr_t)qn <= a;
    };
    L2S_REQUIRE(disjoint(streams, stream_bytes, packed_out, packed_bytes), "jpeg decode: the stream buffer and packed_out overlap");
    L2S_REQUIRE(disjoint(streams, stream_bytes, ws, lay.bytes) && disjoint(packed_out, packed_bytes, ws, lay.bytes), "jpeg decode: the workspace overlaps a buffer");
    L2S_REQUIRE(!status || (disjoint(status, (int64_t)n * 4, ws, lay.bytes) && disjoint(status, (int64_t)n * 4, packed_out, packed_bytes)),
                "jpeg decode: status overlaps a buffer");
    ProfScope ps("jpeg_decode", s);
    int32_t* tab = reinterpret_cast<int32_t*>(ws);
    if (t.upload(tab, s)) return 1;
    const JdImage* imgs = table_seg<JdImage>(tab, lay.off_img);
    const l2s_jpeg_tables* dsets = table_seg<l2s_jpeg_tables>(tab, lay.off_sets);
    int16_t* coef = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(ws) + lay.coef_off);
    uint8_t* planes = reinterpret_cast<uint8_t*>(ws) + lay.plane_off;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)lay.n_work), dim3(JD_THREADS), 0, s, streams, stream_bytes, imgs, table_seg<JdWork>(tab, lay.off_work),
                       table_seg<int32_t>(tab, lay.off_order), dsets, coef, status);
    constexpr int JD_IMAGES_PER_LAUNCH = 32768;            // grid.y
    for (int i0 = 0; i0 < n; i0 += JD_IMAGES_PER_LAUNCH) {
        const int ni = std::min(n - i0, JD_IMAGES_PER_LAUNCH);
        int64_t bmax = 1, gmax = 1;
        for (int i = i0; i < i0 + ni; ++i) {
            bmax = std::max(bmax, jd_blocks(images[i].layout, images[i].H, images[i].W));
            gmax = std::max(gmax, ((int64_t)images[i].H * images[i].W + 3) / 4);
        }
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((bmax + 255) / 256), ni), dim3(256), 0, s, imgs, i0, dsets, coef, planes);
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((gmax + 255) / 256), ni), dim3(256), 0, s, imgs, i0, planes, packed_out, packed_bytes);
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

#ifdef L2S_DIAG
int l2s_op_jpeg_entropy_host(const uint8_t* streams, int64_t stream_bytes, const l2s_jpeg_image* images, int n, const l2s_jpeg_tables* sets, int n_sets,
                             int16_t* coefs, int64_t coef_count, int32_t* status) {
    L2S_REQUIRE(stream_bytes >= 0 && (n_sets == 0 || sets), "jpeg entropy (host): bad arguments");
    if (check_images("jpeg entropy (host)", images, n, n_sets, stream_bytes)) return 1;
    if (n == 0) return 0;
    L2S_REQUIRE(streams && coefs && status, "jpeg entropy (host): null buffer");
    L2S_REQUIRE((reinterpret_cast<uintptr_t>(streams) & 3u) == 0 && (reinterpret_cast<uintptr_t>(coefs) & 15u) == 0,
                "jpeg entropy (host): streams must be 4-byte aligned, coefs 16-byte aligned");
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) blocks += jd_blocks(images[i].layout, images[i].H, images[i].W);
    L2S_REQUIRE(coef_count >= blocks * 64, "jpeg entropy (host): coefs is smaller than the images' blocks x 64");
    blocks = 0;
    for (int i = 0; i < n; ++i) {
        const l2s_jpeg_image& r = images[i];
        const JdImage im{r.scan_offset, 0, blocks, r.scan_bytes, r.H, r.W, r.layout, r.restart, r.table_set, r.eoi, 0};
        status[i] = jd_entropy_image(streams, stream_bytes, im, sets + r.table_set, JD_ZIGZAG, coefs + blocks * 64);
        blocks += jd_blocks(r.layout, r.H, r.W);
    }
    return 0;
}
#endif

}  // extern "C"
