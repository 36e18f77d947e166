// Vocoder + metric of evaluate.py on the device:
//   MelSpec2Audio (datasets/spectograms.py:76-95) = exp -> torchaudio 0.9.0 InverseMelScale (SGD on spec @ fb = mel) -> GriffinLim
//   ESTOI         (evaluate.py:41-45: pystoi.stoi(clean, pred, fs, extended=True))
// torchaudio and pystoi are absent from the build image: what these kernels implement is the published algorithm as restated in
// lip2speech_amd/datasets/spectrograms.py and lip2speech_amd/metrics.py - PARITY UNPINNED against the third-party packages; the kernels
// are tested against those restatements with the random initial iterates passed in explicitly.
#include "fft_dev.h"
#include "host_table.h"
#include "../../include/l2s.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace l2s {

// =====================================================================================================================================
// InverseMelScale: minimise mean_{rows} |mel - spec @ fb|^2 over spec >= 0 by SGD (lr 0.1, momentum 0.9), `iters` iterations, from a
// given start.  A row (one mel frame of one clip) meets the others only through the loss that drives the two stopping rules, and the
// filterbank is banded (a frequency bin feeds at most a few mel bands): ONE WAVE PER ROW keeps spec and velocity in registers (bin
// f = lane + 64 j), exchanges spec / diff through 2.4 KB of LDS and walks only the non-zero band of each filter - no GEMM: the dense
// 513 x 80 product would be 97 % zeros.  Per-iteration per-row losses go to `loss_rows` [iter][row]; inverse_mel_stop_kernel then
// evaluates the reference's rules per call (new_loss < 1e-5, |loss - new_loss| < 1e-8; the update of the stopping iteration is still
// applied) and a second pass re-runs only the calls that stop early, with their iteration count.
// =====================================================================================================================================
constexpr int IM_ROWS = 8;        // rows (waves) per block: they share the compact filterbank tables in LDS (IM_MAXF / IM_MAXM / IM_NNZ: l2s_common.h)

struct InvMelP {
    const float* mel;        // (N, n_mels, L) power mel, or log-mel when log_input
    const float* init;       // (N*L, n_freqs) start iterate, row = n*L + l
    const int* tab;          // ws: [n_mels][3] first bin / last+1 / offset into fwd; [n_freqs][3] first band / last+1 / offset into bwd; then nnz_fwd, nnz_bwd
    const float* fwd;        // ws: the non-zeros of fb, band-major (band m: fb[flo..fhi) [m])
    const float* bwd;        // ws: the same non-zeros, bin-major (bin f: fb[f][mlo..mhi))
    float* spec;             // (N, n_freqs, L) out
    float* loss_rows;        // [iters][N*L] or null
    const int* iters_call;   // per call: iterations to run in THIS pass (null: `iters` for all); a call whose entry equals `iters` is skipped when `second`
    int N, L, n_mels, n_freqs, rows_per_call, iters, log_input, second;
    // the ragged form only (RAG): clip n is its own call of row_off[n + 1] - row_off[n] rows; its mel frame l, band m is mel[mel_off[n] + m mel_pitch[n] + l]
    const int* row_off;      // ws: [N + 1] prefix sums of the clips' frame counts
    const int64_t* mel_off;  // ws: [N]
    const int64_t* mel_pitch;// ws: [N]
};

// one block: band structure of the filterbank + its non-zeros in the two orders the SGD walks them
__global__ __launch_bounds__(256) void inverse_mel_bands_kernel(const float* fb, int n_freqs, int n_mels, int* tab, float* fwd, float* bwd) {
    __shared__ int cnt[IM_MAXM + IM_MAXF];
    const int tid = threadIdx.x;
    for (int i = tid; i < n_mels + n_freqs; i += 256) {
        int lo = 0, hi = 0;
        if (i < n_mels) {
            lo = n_freqs;
            for (int f = 0; f < n_freqs; ++f) if (fb[(int64_t)f * n_mels + i] != 0.f) { lo = f < lo ? f : lo; hi = f + 1; }
        } else {
            const int f = i - n_mels;
            lo = n_mels;
            for (int m = 0; m < n_mels; ++m) if (fb[(int64_t)f * n_mels + m] != 0.f) { lo = m < lo ? m : lo; hi = m + 1; }
        }
        if (hi == 0) lo = 0;
        tab[3 * i] = lo; tab[3 * i + 1] = hi;
        cnt[i] = hi - lo;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int m = 0; m < n_mels; ++m) { tab[3 * m + 2] = o; o += cnt[m]; }
        tab[3 * (n_mels + n_freqs)] = o;
        o = 0;
        for (int f = 0; f < n_freqs; ++f) { tab[3 * (n_mels + f) + 2] = o; o += cnt[n_mels + f]; }
        tab[3 * (n_mels + n_freqs) + 1] = o;
    }
    __syncthreads();
    for (int i = tid; i < n_mels + n_freqs; i += 256) {
        const int lo = tab[3 * i], hi = tab[3 * i + 1], o = tab[3 * i + 2];
        if (i < n_mels) { for (int f = lo; f < hi; ++f) if (o + f - lo < IM_NNZ) fwd[o + f - lo] = fb[(int64_t)f * n_mels + i]; }
        else { const int f = i - n_mels; for (int m = lo; m < hi; ++m) if (o + m - lo < IM_NNZ) bwd[o + m - lo] = fb[(int64_t)f * n_mels + m]; }
    }
}

int launch_mel_bands(const float* fb, int n_freqs, int n_mels, int* tab, float* fwd, float* bwd, hipStream_t s) {
    L2S_REQUIRE(n_mels > 0 && n_mels <= IM_MAXM && n_freqs > 0 && n_freqs <= IM_MAXF, "mel bands: at most 128 mel bands and 576 frequency bins");
    hipLaunchKernelGGL(inverse_mel_bands_kernel, dim3(1), dim3(256), 0, s, fb, n_freqs, n_mels, tab, fwd, bwd);
    return 0;
}

// RAG: row -> (clip, frame) by a search of the prefix table; L, the gradient scale, the mel address and the clip's block of `spec` are the clip's own, and
// the arithmetic of the row is the other instantiation's at N = 1, L = L_b, rows_per_call = 1
template <bool RAG>
__global__ __launch_bounds__(IM_ROWS * 64) void inverse_mel_kernel(const InvMelP p) {
    __shared__ float s_fwd[IM_NNZ], s_bwd[IM_NNZ];
    __shared__ float s_specs[IM_ROWS][IM_MAXF];
    __shared__ float s_diffs[IM_ROWS][IM_MAXM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = p.n_mels, F = p.n_freqs;
    {
        const int nf = p.tab[3 * (M + F)], nb = p.tab[3 * (M + F) + 1];
        for (int i = tid; i < nf && i < IM_NNZ; i += IM_ROWS * 64) s_fwd[i] = p.fwd[i];
        for (int i = tid; i < nb && i < IM_NNZ; i += IM_ROWS * 64) s_bwd[i] = p.bwd[i];
    }
    __syncthreads();                                   // the only block barrier: from here on every wave runs its own row
    const int64_t row = (int64_t)blockIdx.x * IM_ROWS + wave;
    const int64_t rows_total = RAG ? (int64_t)p.row_off[p.N] : (int64_t)p.N * p.L;
    if (row >= rows_total) return;
    float* s_spec = s_specs[wave];
    float* s_diff = s_diffs[wave];
    int L, n, l, call;
    const float* mel_row;                              // band m of this row's frame: mel_row[m * mel_pitch]
    int64_t mel_pitch;
    float* spec_out;                                   // bin f of this row's frame: spec_out[f * L]
    if constexpr (RAG) {
        int lo = 0, hi = p.N;                          // the clip whose rows hold `row`: row_off[lo] <= row < row_off[lo + 1] (wave-uniform: scalar loads)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.row_off[mid] <= row) lo = mid; else hi = mid; }
        n = call = lo;
        const int r0 = p.row_off[n];
        L = p.row_off[n + 1] - r0; l = (int)row - r0;
        mel_pitch = p.mel_pitch[n];
        mel_row = p.mel + p.mel_off[n] + l;
        spec_out = p.spec + (int64_t)r0 * F + l;
    } else {
        L = p.L;
        n = (int)(row / L); l = (int)(row - (int64_t)n * L);
        call = (int)(row / ((int64_t)p.rows_per_call * L));
        mel_pitch = L;
        mel_row = p.mel + (int64_t)n * M * L + l;
        spec_out = p.spec + (int64_t)n * F * L + l;
    }
    int iters = p.iters;
    if (p.iters_call) {
        iters = p.iters_call[call];
        if (p.second && iters >= p.iters) return;             // this call ran to the end in the first pass
    }
    const float gscale = -2.0f / (float)((RAG ? 1 : p.rows_per_call) * L);
    float spec[9], vel[9];
    int mlo[9], mcnt[9], boff[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int f = lane + 64 * j;
        spec[j] = f < F ? p.init[row * F + f] : 0.f;
        vel[j] = 0.f;
        mlo[j] = f < F ? p.tab[3 * (M + f)] : 0;
        mcnt[j] = f < F ? p.tab[3 * (M + f) + 1] - mlo[j] : 0;
        boff[j] = f < F ? p.tab[3 * (M + f) + 2] : 0;
    }
    float target[2];
    int flo[2], fcnt[2], foff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = lane + 64 * i;
        float t = m < M ? mel_row[(int64_t)m * mel_pitch] : 0.f;
        if (p.log_input && m < M) t = expf(t);
        target[i] = t;
        flo[i] = m < M ? p.tab[3 * m] : 0;
        fcnt[i] = m < M ? p.tab[3 * m + 1] - flo[i] : 0;
        foff[i] = m < M ? p.tab[3 * m + 2] : 0;
    }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 9; ++j) s_spec[lane + 64 * j] = spec[j];
        wave_lds_sync();
        float lsum = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = lane + 64 * i;
            float acc = 0.f;
            for (int c = 0; c < fcnt[i]; ++c) acc = fmaf(s_spec[flo[i] + c], s_fwd[foff[i] + c], acc);      // bins ascending
            const float d = target[i] - acc;
            if (m < M) { s_diff[m] = d; lsum = fmaf(d, d, lsum); }
        }
        wave_lds_sync();
        if (p.loss_rows) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o);
            if (lane == 0) p.loss_rows[(int64_t)it * rows_total + row] = lsum;
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            float g = 0.f;
            for (int c = 0; c < mcnt[j]; ++c) g = fmaf(s_diff[mlo[j] + c], s_bwd[boff[j] + c], g);          // bands ascending
            const float nv = 0.9f * vel[j] + gscale * g;                 // torch.optim.SGD(lr 0.1, momentum 0.9): buf = 0.9 buf + grad
            vel[j] = nv;
            spec[j] = fmaxf(spec[j] - 0.1f * nv, 0.f);                   // p -= lr buf; clamp_(min=0)
        }
        wave_lds_sync();
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int f = lane + 64 * j;
        if (f < F) spec_out[(int64_t)f * L] = spec[j];
    }
}

// per call: the mean loss of every iteration (rows summed in index order, fp64) -> the iteration count the reference's stopping rules leave
// row_off (the ragged form; else null): call c is the rows [row_off[c], row_off[c + 1])
__global__ __launch_bounds__(256) void inverse_mel_stop_kernel(const float* loss_rows, int rows_total, int rows_call, int iters, int* iters_call, float* loss_out,
                                                               const int* row_off) {
    __shared__ double red[256];
    __shared__ int stop_at;
    const int call = blockIdx.x, tid = threadIdx.x;
    const int64_t row0 = row_off ? (int64_t)row_off[call] : (int64_t)call * rows_call;
    if (row_off) rows_call = row_off[call + 1] - row_off[call];
    if (tid == 0) stop_at = iters;
    float prev = INFINITY;
    __syncthreads();
    for (int it = 0; it < iters; ++it) {
        double s = 0.0;
        const float* lr = loss_rows + (int64_t)it * rows_total + row0;
        for (int r = tid; r < rows_call; r += 256) s += (double)lr[r];
        red[tid] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
        const float nl = (float)(red[0] / (double)rows_call);
        __syncthreads();
        if (tid == 0 && loss_out) loss_out[(int64_t)call * iters + it] = nl;
        const bool stop = nl < 1e-5f || fabsf(prev - nl) < 1e-8f;        // prev = inf at it = 0: |inf - x| = inf
        prev = nl;
        if (stop) { if (tid == 0) stop_at = it + 1; break; }             // block-uniform: every thread computed the same nl
    }
    __syncthreads();
    if (tid == 0) iters_call[call] = stop_at;
}

// =====================================================================================================================================
// Griffin-Lim (torchaudio 0.9.0 functional.griffinlim: power 2, momentum 0.99, given start angles), n_fft = win = 1024, hop = 256:
//   repeat n_iter times:  rebuilt = stft(istft(mag * ang));  ang = rebuilt - prev * (0.99 / 1.99);  ang /= |ang| + 1e-16;  prev = rebuilt
//   wave = istft(mag * ang)
// ONE BLOCK PER CLIP, NW waves, one wave per STFT frame at a time.  The clip's waveform (hop (L-1) samples) lives in LDS for the whole
// loop: the inverse transforms overlap-add into it in four barrier-separated phases (frames t = p mod 4 do not overlap each other, so
// the order of the additions is fixed: deterministic), the forward transforms read it back with the reflect padding of
// torch.stft(center=True) folded into the index.  The half spectra (L x 513 complex: 316 KB per clip) do not fit next to it: the last
// two `rebuilt` spectra live in the caller's workspace (ping-pong; ang is recomputed from them where it is consumed and never stored),
// frame-major so that a wave's 64 lanes touch consecutive bins.  FFTs: fft_dev.h (three radix-8 stages per 1024-point real transform).
// =====================================================================================================================================
constexpr int GL_NFFT = 1024, GL_HOP = 256, GL_NBIN = 513, GL_LDK = 520;      // bins per frame padded to 520 in the workspace

struct GriffinP {
    const float* power;      // (N, 513, L) power spectrogram (>= 0; clamped)
    const float* init;       // (N, 513, L, 2) start angles (complex, used as given)
    float* mag;              // ws: (N, L, 520) sqrt(power), frame-major
    float2* reb;             // ws: (N, 2, L, 520) the last two rebuilt spectra (slot 0 starts as the transposed init)
    float* wave;             // (N, hop (L-1)) out
    int N, L, iters;
    float momentum;          // 0.99 / 1.99
    // the ragged form only (RAG): block j runs clip list[j]; the clip's frames are [frame_off[clip], frame_off[clip + 1]) of the packed arrays (three
    // workspace slots per frame there, whatever the form) and its waveform row starts at wave + clip wave_pitch
    const int* frame_off;    // ws: [N + 1] prefix sums of the clips' frame counts
    const int* list;         // ws: the clips this launch's form takes
    int64_t wave_pitch;
};

// RAG: the clip, its L and its blocks of the packed arrays come from the tables; the rest of the row past the clip's samples is written as zeros
template <int NW, int YCAP, bool RAG>
__global__ __launch_bounds__(NW * 64) void griffin_lim_kernel(const GriffinP p) {
    __shared__ __attribute__((aligned(16))) float y[YCAP];
    __shared__ __attribute__((aligned(16))) float2 scratch[NW][GL_LDK];
    __shared__ float w2[GL_NFFT];                                  // window^2 for the overlap-add envelope
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int clip = RAG ? p.list[blockIdx.x] : (int)blockIdx.x;
    const int L = RAG ? p.frame_off[clip + 1] - p.frame_off[clip] : p.L, ylen = GL_HOP * (L - 1);
    const int64_t f0 = RAG ? (int64_t)p.frame_off[clip] : (int64_t)clip * L;      // the clip's first frame in the packed arrays
    float2* sc = scratch[wave];
    float* mag = p.mag + f0 * GL_LDK;
    float2* reb0 = p.reb + f0 * (RAG ? 3 : 2) * GL_LDK;
    float2* reb1 = reb0 + (int64_t)L * GL_LDK;
    // ---- prologue: frame-major copies of sqrt(power) and of the start angles; window constants
    {
        const float* pw = p.power + f0 * GL_NBIN;
        const float2* in = reinterpret_cast<const float2*>(p.init) + f0 * GL_NBIN;
        for (int i = tid; i < GL_NBIN * L; i += NW * 64) {
            const int k = i / L, t = i - k * L;
            mag[(int64_t)t * GL_LDK + k] = sqrtf(fmaxf(pw[i], 0.f));
            reb0[(int64_t)t * GL_LDK + k] = in[i];
        }
        for (int i = tid; i < GL_NFFT; i += NW * 64) { const float w = 0.5f - 0.5f * cospif((float)i / 512.0f); w2[i] = w * w; }
    }
    Fft512Tw tw;
    tw.init(lane);
    float wn[8][2];                                                  // hann(periodic) at samples 2 n, 2 n + 1 of a frame, n = lane + 64 r
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int m = 2 * (lane + 64 * r);
        wn[r][0] = 0.5f - 0.5f * cospif((float)m / 512.0f);
        wn[r][1] = 0.5f - 0.5f * cospif((float)(m + 1) / 512.0f);
    }
    __threadfence_block();
    __syncthreads();

    for (int it = 0; it <= p.iters; ++it) {
        const float2* cur = (it & 1) ? reb1 : reb0;                  // written by phase B of iteration it - 1 (it = 0: the start angles)
        const float2* prv = (it & 1) ? reb0 : reb1;                  // written at it - 2; not read for it < 2
        // ---------------- phase A: y = istft(mag * ang)
        for (int i = tid; i < ylen; i += NW * 64) y[i] = 0.f;
        __syncthreads();
        for (int ph = 0; ph < 4; ++ph) {
            for (int t = ph + 4 * wave; t < L; t += 4 * NW) {
                const float* mg = mag + (int64_t)t * GL_LDK;
                const float2* c = cur + (int64_t)t * GL_LDK;
                const float2* q = prv + (int64_t)t * GL_LDK;
                float2 v[8];
                auto spec_at = [&](int k) -> float2 {
                    float2 a = c[k];
                    if (it >= 1) {
                        if (it >= 2) { const float2 b = q[k]; a.x -= p.momentum * b.x; a.y -= p.momentum * b.y; }
                        const float inv = 1.0f / (sqrtf(a.x * a.x + a.y * a.y) + 1e-16f);
                        a.x *= inv; a.y *= inv;
                    }
                    const float g = mg[k];
                    return make_float2(g * a.x, g * a.y);
                };
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = spec_at(lane + 64 * r);
                float2 s512 = make_float2(0.f, 0.f);
                if (lane == 0) s512 = spec_at(512);
                irfft1024_pre(v, s512, sc, lane, tw);
                fft512<+1>(v, sc, lane, tw);
                const int base = t * GL_HOP - GL_NFFT / 2;           // output index of the frame's sample 0 (istft trims n_fft / 2)
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int idx = base + 2 * (lane + 64 * r);
                    if (idx >= 0 && idx < ylen) {                    // idx is even and ylen is even: both samples in or out together
                        float2 o = *reinterpret_cast<float2*>(y + idx);
                        o.x += v[r].x * (1.0f / 1024.0f) * wn[r][0];
                        o.y += v[r].y * (1.0f / 1024.0f) * wn[r][1];
                        *reinterpret_cast<float2*>(y + idx) = o;
                    }
                }
            }
            __syncthreads();
        }
        // overlap-add envelope: sum of window^2 over the frames that cover the sample
        for (int i = tid; i < ylen; i += NW * 64) {
            const int pp = i + GL_NFFT / 2;
            int t0 = (pp - (GL_NFFT - 1) + GL_HOP - 1) / GL_HOP; t0 = t0 < 0 ? 0 : t0;
            int t1 = pp / GL_HOP; t1 = t1 > L - 1 ? L - 1 : t1;
            float env = 0.f;
            for (int t = t0; t <= t1; ++t) env += w2[pp - t * GL_HOP];
            y[i] = y[i] / env;
        }
        __syncthreads();
        if (it == p.iters) break;
        // ---------------- phase B: rebuilt = stft(y) (centre, reflect), into the slot phase A of the next iteration reads as `cur`
        float2* dst = (it & 1) ? reb0 : reb1;
        for (int t = wave; t < L; t += NW) {
            float2 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                int s0 = t * GL_HOP + 2 * (lane + 64 * r) - GL_NFFT / 2, s1 = s0 + 1;
                s0 = s0 < 0 ? -s0 : s0; s0 = s0 >= ylen ? 2 * (ylen - 1) - s0 : s0;
                s1 = s1 < 0 ? -s1 : s1; s1 = s1 >= ylen ? 2 * (ylen - 1) - s1 : s1;
                v[r] = make_float2(y[s0] * wn[r][0], y[s1] * wn[r][1]);
            }
            fft512<-1>(v, sc, lane, tw);
            const float nyq = rfft1024_post(v, sc, lane, tw);
            float2* d = dst + (int64_t)t * GL_LDK;
#pragma unroll
            for (int r = 0; r < 8; ++r) d[lane + 64 * r] = v[r];
            if (lane == 0) d[512] = make_float2(nyq, 0.f);
        }
        __threadfence_block();                                       // the spectra go through global memory: this block's own stores, re-read by other waves
        __syncthreads();
    }
    float* out = p.wave + (int64_t)clip * (RAG ? p.wave_pitch : (int64_t)ylen);
    for (int i = tid; i < ylen; i += NW * 64) out[i] = y[i];
    if constexpr (RAG)
        for (int64_t i = ylen + tid; i < p.wave_pitch; i += NW * 64) out[i] = 0.f;
}

// =====================================================================================================================================
// Griffin-Lim, long form (L >= 122: the waveform no longer fits one block's LDS).  ONE LAUNCH PER ITERATION, one block per (clip, tile of
// F consecutive STFT frames), no barrier or wait between blocks inside a launch.  A block recomputes the waveform samples its own forward
// transforms read - [t0 hop - 512, (t1 - 1) hop + 512) plus the indices torch.stft's reflect padding mirrors into at the clip's two ends -
// from the inverse transforms of every frame that covers them (a halo of three frames each side), with the short kernel's arithmetic: the
// same spec_at, the same FFTs, the overlap-add in four barrier-separated phases ordered by the ABSOLUTE t mod 4 (so a sample's sum does not
// depend on the tiling) and the same envelope division.  It then writes the forward transforms of its own frames, or on the last iteration
// its own partition [t0 hop, t1 hop) of the waveform: every spectrum value and every sample has exactly one writer.
// Other blocks of the launch still read rebuilt[it - 1] and rebuilt[it - 2] while this one writes rebuilt[it]: THREE rotating slots
// (rebuilt[k] in slot k % 3; the start angles in slot 2, which it = 0 reads as "rebuilt[-1]").
// =====================================================================================================================================
// built tile: 24 own + 6 halo frames = at most 8 inverse transforms per overlap-add phase, one per wave.  174 VGPRs: one block per compute unit, so a launch
// of up to 256 blocks (32 clips of 188 frames) is one round of blocks; smaller tiles are 10 % faster below that and 70 % slower at it (profiles/vocoder_long_times.txt)
constexpr int GLT_F = 24, GLT_NW = 8;

struct GriffinTileP {
    const float* mag;        // ws: (N, L, 520) sqrt(power), frame-major
    float2* reb;             // ws: (N, 3, L, 520) rotating rebuilt spectra
    float* wave;             // (N, hop (L-1)) out
    int N, L, it, iters;
    float momentum;          // 0.99 / 1.99
    // the ragged form only (RAG): a 1-D grid over the (clip, tile) pairs of the n_long clips in `list`; block x is tile x - tile_off[j] of clip list[j]
    const int* frame_off;    // ws: [N + 1] prefix sums of the clips' frame counts
    const int* list;         // ws: [n_long] the clips past 121 frames, in clip order
    const int* tile_off;     // ws: [n_long + 1] prefix sums of their tile counts
    int n_long;
    int64_t wave_pitch;
};

// frame-major copies of sqrt(power) and of the start angles (what the short kernel's prologue writes), the angles into slot 2.
// frame_off / list (the ragged form; else null): block row y is clip list[y] with its own L (the grid's x is sized by the longest)
__global__ __launch_bounds__(256) void griffin_lim_tile_prologue_kernel(const float* power, const float* init, float* mag_all, float2* reb_all, int L,
                                                                        const int* frame_off, const int* list) {
    const int clip = list ? list[blockIdx.y] : (int)blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (list) L = frame_off[clip + 1] - frame_off[clip];
    if (i >= GL_NBIN * L) return;
    const int64_t f0 = list ? (int64_t)frame_off[clip] : (int64_t)clip * L;
    const int k = i / L, t = i - k * L;
    const float* pw = power + f0 * GL_NBIN;
    const float2* in = reinterpret_cast<const float2*>(init) + f0 * GL_NBIN;
    mag_all[(f0 + t) * GL_LDK + k] = sqrtf(fmaxf(pw[i], 0.f));
    reb_all[(f0 * 3 + 2 * (int64_t)L + t) * GL_LDK + k] = in[i];
}

// RAG: (clip, tile) by a search of the tile prefix table - block-uniform, so the lookup lives in scalar registers; the last tile of a clip also writes the
// zeros past the clip's samples on the last iteration
template <int NW, int F, bool RAG>
__global__ __launch_bounds__(NW * 64) void griffin_lim_tile_kernel(const GriffinTileP p) {
    constexpr int YCAP = (F + 3) * GL_HOP;                           // (F - 1) hop + n_fft samples; the clip-end extensions stay below it (F >= 2)
    static_assert(F >= 2, "a tile's sample range is sized for at least two frames");
    __shared__ __attribute__((aligned(16))) float y[YCAP];
    __shared__ __attribute__((aligned(16))) float2 scratch[NW][GL_LDK];
    __shared__ float w2[GL_NFFT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int clip = blockIdx.y, tile = blockIdx.x, L = p.L;
    int64_t f0;                                                      // the clip's first frame in the packed workspace
    if constexpr (RAG) {
        int lo = 0, hi = p.n_long;                                   // tile_off[lo] <= blockIdx.x < tile_off[lo + 1]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.tile_off[mid] <= (int)blockIdx.x) lo = mid; else hi = mid; }
        tile = (int)blockIdx.x - p.tile_off[lo];
        clip = p.list[lo];
        f0 = p.frame_off[clip];
        L = p.frame_off[clip + 1] - p.frame_off[clip];
    } else {
        f0 = (int64_t)clip * L;
    }
    const int ylen = GL_HOP * (L - 1), it = p.it;
    const int t0 = tile * F, t1 = t0 + F < L ? t0 + F : L;
    float2* sc = scratch[wave];
    const float* mag = p.mag + f0 * GL_LDK;
    float2* reb = p.reb + f0 * 3 * GL_LDK;
    const float2* cur = reb + (int64_t)((it + 2) % 3) * L * GL_LDK;  // rebuilt[it - 1] (it = 0: the start angles)
    const float2* prv = reb + (int64_t)((it + 1) % 3) * L * GL_LDK;  // rebuilt[it - 2]; not read for it < 2
    // ---- the samples [lo, hi) this block holds: what its forward transforms read, the reflect padding's mirrored indices included
    const int smin = t0 * GL_HOP - GL_NFFT / 2, smax = (t1 - 1) * GL_HOP + GL_NFFT / 2 - 1;
    int lo = smin < 0 ? 0 : smin, hi = smax > ylen - 1 ? ylen - 1 : smax;
    if (smin < 0 && -smin > hi) hi = -smin;
    if (smax > ylen - 1 && 2 * (ylen - 1) - smax < lo) lo = 2 * (ylen - 1) - smax;
    lo &= ~1; hi = (hi + 2) & ~1;                                    // both even (ylen is): a frame's sample pair is in or out together; hi exclusive
    int ta = (lo + GL_NFFT / 2) / GL_HOP - 3; ta = ta < 0 ? 0 : ta;  // frames [ta, tb) cover a sample of [lo, hi): frame t spans [t hop - 512, t hop + 512)
    int tb = (hi + GL_NFFT / 2 + GL_HOP - 1) / GL_HOP; tb = tb > L ? L : tb;
    for (int i = tid; i < GL_NFFT; i += NW * 64) { const float w = 0.5f - 0.5f * cospif((float)i / 512.0f); w2[i] = w * w; }
    for (int i = tid; i < hi - lo; i += NW * 64) y[i] = 0.f;
    Fft512Tw tw;
    tw.init(lane);
    float wn[8][2];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int m = 2 * (lane + 64 * r);
        wn[r][0] = 0.5f - 0.5f * cospif((float)m / 512.0f);
        wn[r][1] = 0.5f - 0.5f * cospif((float)(m + 1) / 512.0f);
    }
    __syncthreads();
    // ---------------- phase A: y[lo, hi) = istft(mag * ang)
    for (int ph = 0; ph < 4; ++ph) {
        for (int t = ta + ((ph - ta) & 3) + 4 * wave; t < tb; t += 4 * NW) {
            const float* mg = mag + (int64_t)t * GL_LDK;
            const float2* c = cur + (int64_t)t * GL_LDK;
            const float2* q = prv + (int64_t)t * GL_LDK;
            float2 v[8];
            auto spec_at = [&](int k) -> float2 {
                float2 a = c[k];
                if (it >= 1) {
                    if (it >= 2) { const float2 b = q[k]; a.x -= p.momentum * b.x; a.y -= p.momentum * b.y; }
                    const float inv = 1.0f / (sqrtf(a.x * a.x + a.y * a.y) + 1e-16f);
                    a.x *= inv; a.y *= inv;
                }
                const float g = mg[k];
                return make_float2(g * a.x, g * a.y);
            };
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = spec_at(lane + 64 * r);
            float2 s512 = make_float2(0.f, 0.f);
            if (lane == 0) s512 = spec_at(512);
            irfft1024_pre(v, s512, sc, lane, tw);
            fft512<+1>(v, sc, lane, tw);
            const int base = t * GL_HOP - GL_NFFT / 2;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int idx = base + 2 * (lane + 64 * r);
                if (idx >= lo && idx < hi) {
                    float2 o = *reinterpret_cast<float2*>(y + idx - lo);
                    o.x += v[r].x * (1.0f / 1024.0f) * wn[r][0];
                    o.y += v[r].y * (1.0f / 1024.0f) * wn[r][1];
                    *reinterpret_cast<float2*>(y + idx - lo) = o;
                }
            }
        }
        __syncthreads();
    }
    for (int j = tid; j < hi - lo; j += NW * 64) {
        const int pp = lo + j + GL_NFFT / 2;
        int e0 = (pp - (GL_NFFT - 1) + GL_HOP - 1) / GL_HOP; e0 = e0 < 0 ? 0 : e0;
        int e1 = pp / GL_HOP; e1 = e1 > L - 1 ? L - 1 : e1;
        float env = 0.f;
        for (int t = e0; t <= e1; ++t) env += w2[pp - t * GL_HOP];
        y[j] = y[j] / env;
    }
    __syncthreads();
    if (it == p.iters) {                                             // the waveform: this tile's own partition
        float* out = p.wave + (int64_t)clip * (RAG ? p.wave_pitch : (int64_t)ylen);
        const int o1 = t1 * GL_HOP < ylen ? t1 * GL_HOP : ylen;
        for (int i = t0 * GL_HOP + tid; i < o1; i += NW * 64) out[i] = y[i - lo];
        if constexpr (RAG)
            if (t1 == L) for (int64_t i = ylen + tid; i < p.wave_pitch; i += NW * 64) out[i] = 0.f;
        return;
    }
    // ---------------- phase B: rebuilt[it] = stft(y) (centre, reflect) for the tile's own frames
    float2* dst = reb + (int64_t)(it % 3) * L * GL_LDK;
    for (int t = t0 + wave; t < t1; t += NW) {
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            int s0 = t * GL_HOP + 2 * (lane + 64 * r) - GL_NFFT / 2, s1 = s0 + 1;
            s0 = s0 < 0 ? -s0 : s0; s0 = s0 >= ylen ? 2 * (ylen - 1) - s0 : s0;
            s1 = s1 < 0 ? -s1 : s1; s1 = s1 >= ylen ? 2 * (ylen - 1) - s1 : s1;
            v[r] = make_float2(y[s0 - lo] * wn[r][0], y[s1 - lo] * wn[r][1]);
        }
        fft512<-1>(v, sc, lane, tw);
        const float nyq = rfft1024_post(v, sc, lane, tw);
        float2* d = dst + (int64_t)t * GL_LDK;
#pragma unroll
        for (int r = 0; r < 8; ++r) d[lane + 64 * r] = v[r];
        if (lane == 0) d[512] = make_float2(nyq, 0.f);
    }
}

// =====================================================================================================================================
// ESTOI (pystoi 0.3.3 stoi(x, y, fs, extended=True) as restated in lip2speech_amd/metrics.py), one block per clip:
//   resample_poly(., 10000 / g, fs / g) with the caller's polyphase FIR (pystoi's resample_oct window) -> drop the frames of the clean signal more than 40 dB below its
//   loudest frame (256-sample hann frames, hop 128) from both signals and overlap-add the rest -> 512-point spectra of 256-sample frames ->
//   15 one-third octave bands -> every run of 30 frames: rows and columns normalised to zero mean / unit norm -> mean correlation.
// The work per clip is small (two signals x ~93 frames x 257 bins): the spectra are direct sums against a 512-entry twiddle table.
// =====================================================================================================================================
constexpr int ES_FRAME = 256, ES_HOP = 128, ES_NFFT = 512, ES_BANDS = 15, ES_SEG = 30, ES_MAXFRAMES = 128, ES_MAXLEN = ES_HOP * (ES_MAXFRAMES + 1);
constexpr int ES_NBIN = ES_NFFT / 2 + 1;

// the ragged forms only (RAG): block (or grid layer) j scores clip list[j] and uses workspace slot j; the clip's signals are the first n_samples[clip] floats
// of row clip (pitch floats apart), its filter the first n_fir[clip] taps of the call's one table, its resampled length n_res[clip]
struct EstoiRag {
    const int* n_samples; const int* n_fir; const int* n_res;      // ws: [N] each
    const int* list;                                               // ws: the clips this launch's form takes
    int64_t pitch;
};

struct EstoiP {
    const float* clean; const float* pred;    // (N, n_samples)
    const float* fir;                          // resampling filter h (already scaled by `up`, pre-padded), n_fir taps; null when fs == 10000
    const int* band_lo; const int* band_hi;    // third-octave band edges (bins), 15 each
    float* rs;                                 // ws: (N, 2, ES_MAXLEN) resampled signals
    float* pw;                                 // ws: (N, 2, ES_MAXFRAMES, ES_NBIN) power spectra of the frames
    float* score;                              // (N)
    int N, n_samples, n_fir, up, down, n_pre_remove, n_res;
    EstoiRag rag;
};

template <bool RAG>
__global__ __launch_bounds__(1024) void estoi_kernel(const EstoiP p) {
    __shared__ float sig[2][ES_MAXLEN];                               // the silent-frame-free signals (x = clean, y = pred); later: row statistics + contributions
    __shared__ float tob[2][ES_BANDS][ES_MAXFRAMES];
    __shared__ float2 twd[ES_NFFT];
    __shared__ float win[ES_FRAME];
    __shared__ float energy[ES_MAXFRAMES];
    __shared__ int keep_pos[ES_MAXFRAMES];
    __shared__ float red[1024];
    __shared__ int n_keep_s;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int clip = RAG ? p.rag.list[slot] : slot;
    float* rs = p.rs + (int64_t)slot * 2 * ES_MAXLEN;
    float* pw = p.pw + (int64_t)slot * 2 * ES_MAXFRAMES * ES_NBIN;
    const int nr = RAG ? p.rag.n_res[clip] : p.n_res;
    const int n_samples = RAG ? p.rag.n_samples[clip] : p.n_samples, n_fir = RAG ? p.rag.n_fir[clip] : p.n_fir;
    const int64_t pitch = RAG ? p.rag.pitch : (int64_t)p.n_samples;
    constexpr float EPS = 2.220446049250313e-16f;
    // ---- tables
    for (int i = tid; i < ES_NFFT; i += 1024) { float s, c; sincospif((float)i / 256.0f, &s, &c); twd[i] = make_float2(c, -s); }      // exp(-2 pi i n / 512)
    for (int i = tid; i < ES_FRAME; i += 1024) win[i] = 0.5f - 0.5f * cospif(2.0f * (float)(i + 1) / (float)(ES_FRAME + 1));          // np.hanning(258)[1:-1]
    // ---- resample (upfirdn, zero-padded ends): out[n] = sum_i x[i] h[(n + n_pre_remove) down - i up]
    for (int s = 0; s < 2; ++s) {
        const float* x = (s ? p.pred : p.clean) + (int64_t)clip * pitch;
        for (int n = tid; n < nr; n += 1024) {
            float acc;
            if (p.fir) {
                const int64_t c = (int64_t)(n + p.n_pre_remove) * p.down;
                int64_t ihi = c / p.up; if (ihi > n_samples - 1) ihi = n_samples - 1;
                int64_t ilo = c - (n_fir - 1) <= 0 ? 0 : (c - (n_fir - 1) + p.up - 1) / p.up;
                double a = 0.0;
                for (int64_t i = ilo; i <= ihi; ++i) a += (double)x[i] * (double)p.fir[c - i * p.up];
                acc = (float)a;
            } else {
                acc = x[n];
            }
            rs[s * ES_MAXLEN + n] = acc;
        }
    }
    __syncthreads();
    // ---- silent-frame removal: energies of the clean signal's windowed frames
    // pystoi 0.3.3 frames with range(0, len - framelen, hop): ceil((len - framelen) / hop) frames - the one ending on the last sample is not taken
    const int nf = nr > ES_FRAME ? (nr - ES_FRAME + ES_HOP - 1) / ES_HOP : 0;
    {
        const int wv = tid >> 6, ln = tid & 63;
        for (int f = wv; f < nf; f += 16) {
            float e = 0.f;
            for (int i = ln; i < ES_FRAME; i += 64) { const float v = rs[f * ES_HOP + i] * win[i]; e = fmaf(v, v, e); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
            if (ln == 0) energy[f] = 20.0f * log10f(sqrtf(e) + EPS);
        }
    }
    __syncthreads();
    if (tid == 0) {
        float mx = -INFINITY;
        for (int f = 0; f < nf; ++f) mx = fmaxf(mx, energy[f]);
        int k = 0;
        for (int f = 0; f < nf; ++f) if (mx - 40.0f - energy[f] < 0.f) keep_pos[k++] = f;
        n_keep_s = k;
    }
    __syncthreads();
    const int nk = n_keep_s;
    const int len2 = nk > 0 ? (nk - 1) * ES_HOP + ES_FRAME : 0;
    // overlap-add of the kept frames: output sample i is covered by kept frames j = i / hop - 1 and i / hop
    for (int s = 0; s < 2; ++s)
        for (int i = tid; i < len2; i += 1024) {
            const int j1 = i / ES_HOP, j0 = j1 - 1;
            float acc = 0.f;
            if (j0 >= 0 && j0 < nk) { const int o = i - j0 * ES_HOP; acc += rs[s * ES_MAXLEN + keep_pos[j0] * ES_HOP + o] * win[o]; }
            if (j1 < nk) { const int o = i - j1 * ES_HOP; acc += rs[s * ES_MAXLEN + keep_pos[j1] * ES_HOP + o] * win[o]; }
            sig[s][i] = acc;
        }
    __syncthreads();
    // ---- power spectra of the bins the bands use (direct sums against the twiddle table), then the band magnitudes
    const int nf2 = len2 > ES_FRAME ? (len2 - ES_FRAME + ES_HOP - 1) / ES_HOP : 0;      // = nk - 1: the same rule on the overlap-added signal
    if (nf2 < ES_SEG) { if (tid == 0) p.score[clip] = 1e-5f; return; }      // pystoi: not enough frames -> 1e-5 (with a warning)
    const int k_lo = p.band_lo[0], k_hi = p.band_hi[ES_BANDS - 1], nkb = k_hi - k_lo;
    for (int item = tid; item < 2 * nf2 * nkb; item += 1024) {
        const int s = item / (nf2 * nkb), rem = item - s * nf2 * nkb, f = rem / nkb, k = k_lo + rem - f * nkb;
        const float* fr = sig[s] + f * ES_HOP;
        float re = 0.f, im = 0.f;
        for (int i = 0; i < ES_FRAME; ++i) {
            const float v = fr[i] * win[i];
            const float2 w = twd[(k * i) & (ES_NFFT - 1)];
            re = fmaf(v, w.x, re); im = fmaf(v, w.y, im);
        }
        pw[(s * ES_MAXFRAMES + f) * ES_NBIN + k] = re * re + im * im;
    }
    __syncthreads();
    for (int item = tid; item < 2 * nf2 * ES_BANDS; item += 1024) {
        const int s = item / (nf2 * ES_BANDS), rem = item - s * nf2 * ES_BANDS, f = rem / ES_BANDS, b = rem - f * ES_BANDS;
        float a = 0.f;
        for (int k = p.band_lo[b]; k < p.band_hi[b]; ++k) a += pw[(s * ES_MAXFRAMES + f) * ES_NBIN + k];
        tob[s][b][f] = sqrtf(a);
    }
    __syncthreads();
    // ---- segments of 30 frames.  Row (band) statistics per (signal, segment, band): mean and 1 / (norm + eps) over the 30 frames
    const int nseg = nf2 - ES_SEG + 1;
    float* rstat = &sig[0][0];                                          // [2][nseg][15][2]   (the signals are dead)
    float* contrib = rstat + 2 * ES_MAXFRAMES * ES_BANDS * 2;           // [nseg][30]
    for (int item = tid; item < 2 * nseg * ES_BANDS; item += 1024) {
        const int s = item / (nseg * ES_BANDS), rem = item - s * nseg * ES_BANDS, seg = rem / ES_BANDS, b = rem - seg * ES_BANDS;
        float mean = 0.f;
        for (int i = 0; i < ES_SEG; ++i) mean += tob[s][b][seg + i];
        mean /= (float)ES_SEG;
        float nrm = 0.f;
        for (int i = 0; i < ES_SEG; ++i) { const float v = tob[s][b][seg + i] - mean; nrm = fmaf(v, v, nrm); }
        rstat[item * 2] = mean; rstat[item * 2 + 1] = 1.0f / (sqrtf(nrm) + EPS);
    }
    __syncthreads();
    // column (frame) normalisation over the 15 bands of the row-normalised values, and the frame's share of the correlation
    for (int item = tid; item < nseg * ES_SEG; item += 1024) {
        const int seg = item / ES_SEG, i = item - seg * ES_SEG;
        float v[2][ES_BANDS];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float mean = 0.f;
#pragma unroll
            for (int b = 0; b < ES_BANDS; ++b) {
                const float* st = rstat + ((s * nseg + seg) * ES_BANDS + b) * 2;
                v[s][b] = (tob[s][b][seg + i] - st[0]) * st[1];
                mean += v[s][b];
            }
            mean /= (float)ES_BANDS;
            float nrm = 0.f;
#pragma unroll
            for (int b = 0; b < ES_BANDS; ++b) { v[s][b] -= mean; nrm = fmaf(v[s][b], v[s][b], nrm); }
            const float inv = 1.0f / (sqrtf(nrm) + EPS);
#pragma unroll
            for (int b = 0; b < ES_BANDS; ++b) v[s][b] *= inv;
        }
        float c = 0.f;
#pragma unroll
        for (int b = 0; b < ES_BANDS; ++b) c = fmaf(v[0][b], v[1][b], c);
        contrib[item] = c / (float)ES_SEG;
    }
    __syncthreads();
    float part = 0.f;
    for (int item = tid; item < nseg * ES_SEG; item += 1024) part += contrib[item];
    red[tid] = part;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) p.score[clip] = red[0] / (float)nseg;
}

// =====================================================================================================================================
// ESTOI, long form (more than 16 512 samples at 10 kHz: the two signals no longer fit one block's LDS).  The same algorithm and the same
// order of every per-clip sum as estoi_kernel; what changes is where things live.  The resampler is a grid-wide kernel of its own over
// (chunk, signal, clip) into the workspace; then one block per clip: the overlap-added signals go to the workspace too (one clip's stay in
// L2) and are staged into LDS 64 frames at a time for the spectra, the row statistics take the staging buffer's place once the spectra are
// done, and a thread adds up the contributions of its (segment, frame) items as it computes them - in the order estoi_kernel sums them.
// =====================================================================================================================================
constexpr int ESL_MAXFRAMES = 376, ESL_MAXLEN = ES_HOP * (ESL_MAXFRAMES + 1), ESL_CHUNK = 64;      // 48 256 samples at 10 kHz

struct EstoiLongP {
    const float* clean; const float* pred;    // (N, n_samples)
    const float* fir;
    const int* band_lo; const int* band_hi;
    float* rs;                                 // ws: (N, 2, ESL_MAXLEN) resampled signals
    float* oa;                                 // ws: (N, 2, ESL_MAXLEN) the silent-frame-free signals
    float* pw;                                 // ws: (N, 2, ESL_MAXFRAMES, ES_NBIN) power spectra of the frames
    float* score;                              // (N)
    int N, n_samples, n_fir, up, down, n_pre_remove, n_res;
    EstoiRag rag;
};

template <bool RAG>
__global__ __launch_bounds__(256) void estoi_resample_kernel(const EstoiLongP p) {
    const int n = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, slot = blockIdx.z;
    const int clip = RAG ? p.rag.list[slot] : slot;
    if (n >= (RAG ? p.rag.n_res[clip] : p.n_res)) return;            // the ragged grid's x is sized by the longest clip
    const int n_samples = RAG ? p.rag.n_samples[clip] : p.n_samples, n_fir = RAG ? p.rag.n_fir[clip] : p.n_fir;
    const float* x = (s ? p.pred : p.clean) + (int64_t)clip * (RAG ? p.rag.pitch : (int64_t)p.n_samples);
    float acc;
    if (p.fir) {                               // upfirdn, zero-padded ends: out[n] = sum_i x[i] h[(n + n_pre_remove) down - i up]
        const int64_t c = (int64_t)(n + p.n_pre_remove) * p.down;
        int64_t ihi = c / p.up; if (ihi > n_samples - 1) ihi = n_samples - 1;
        int64_t ilo = c - (n_fir - 1) <= 0 ? 0 : (c - (n_fir - 1) + p.up - 1) / p.up;
        double a = 0.0;
        for (int64_t i = ilo; i <= ihi; ++i) a += (double)x[i] * (double)p.fir[c - i * p.up];
        acc = (float)a;
    } else {
        acc = x[n];
    }
    p.rs[((int64_t)slot * 2 + s) * ESL_MAXLEN + n] = acc;
}

template <bool RAG>
__global__ __launch_bounds__(1024) void estoi_long_kernel(const EstoiLongP p) {
    __shared__ float buf[2 * ESL_MAXFRAMES * ES_BANDS * 2];           // ESL_CHUNK frames of one signal for the spectra; later the row statistics
    __shared__ float tob[2][ES_BANDS][ESL_MAXFRAMES];
    __shared__ float2 twd[ES_NFFT];
    __shared__ float win[ES_FRAME];
    __shared__ float energy[ESL_MAXFRAMES];
    __shared__ int keep_pos[ESL_MAXFRAMES];
    __shared__ float red[1024];
    __shared__ int n_keep_s;
    static_assert(ES_HOP * (ESL_CHUNK + 1) <= 2 * ESL_MAXFRAMES * ES_BANDS * 2, "the staged frames fit the buffer the row statistics use later");
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int clip = RAG ? p.rag.list[slot] : slot;
    const float* rs = p.rs + (int64_t)slot * 2 * ESL_MAXLEN;
    float* oa = p.oa + (int64_t)slot * 2 * ESL_MAXLEN;
    float* pw = p.pw + (int64_t)slot * 2 * ESL_MAXFRAMES * ES_NBIN;
    const int nr = RAG ? p.rag.n_res[clip] : p.n_res;
    constexpr float EPS = 2.220446049250313e-16f;
    for (int i = tid; i < ES_NFFT; i += 1024) { float s, c; sincospif((float)i / 256.0f, &s, &c); twd[i] = make_float2(c, -s); }
    for (int i = tid; i < ES_FRAME; i += 1024) win[i] = 0.5f - 0.5f * cospif(2.0f * (float)(i + 1) / (float)(ES_FRAME + 1));
    __syncthreads();
    // ---- silent-frame removal: energies of the clean signal's windowed frames (pystoi 0.3.3's frame rule: estoi_kernel)
    const int nf = nr > ES_FRAME ? (nr - ES_FRAME + ES_HOP - 1) / ES_HOP : 0;
    {
        const int wv = tid >> 6, ln = tid & 63;
        for (int f = wv; f < nf; f += 16) {
            float e = 0.f;
            for (int i = ln; i < ES_FRAME; i += 64) { const float v = rs[f * ES_HOP + i] * win[i]; e = fmaf(v, v, e); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
            if (ln == 0) energy[f] = 20.0f * log10f(sqrtf(e) + EPS);
        }
    }
    __syncthreads();
    if (tid == 0) {
        float mx = -INFINITY;
        for (int f = 0; f < nf; ++f) mx = fmaxf(mx, energy[f]);
        int k = 0;
        for (int f = 0; f < nf; ++f) if (mx - 40.0f - energy[f] < 0.f) keep_pos[k++] = f;
        n_keep_s = k;
    }
    __syncthreads();
    const int nk = n_keep_s;
    const int len2 = nk > 0 ? (nk - 1) * ES_HOP + ES_FRAME : 0;
    const int nf2 = len2 > ES_FRAME ? (len2 - ES_FRAME + ES_HOP - 1) / ES_HOP : 0;
    if (nf2 < ES_SEG) { if (tid == 0) p.score[clip] = 1e-5f; return; }
    for (int s = 0; s < 2; ++s)
        for (int i = tid; i < len2; i += 1024) {
            const int j1 = i / ES_HOP, j0 = j1 - 1;
            float acc = 0.f;
            if (j0 >= 0 && j0 < nk) { const int o = i - j0 * ES_HOP; acc += rs[s * ESL_MAXLEN + keep_pos[j0] * ES_HOP + o] * win[o]; }
            if (j1 < nk) { const int o = i - j1 * ES_HOP; acc += rs[s * ESL_MAXLEN + keep_pos[j1] * ES_HOP + o] * win[o]; }
            oa[s * ESL_MAXLEN + i] = acc;
        }
    __threadfence_block();                                             // this block's own global stores, re-read by other waves
    __syncthreads();
    // ---- power spectra of the bins the bands use, ESL_CHUNK frames of one signal staged in LDS at a time
    const int k_lo = p.band_lo[0], k_hi = p.band_hi[ES_BANDS - 1], nkb = k_hi - k_lo;
    for (int s = 0; s < 2; ++s)
        for (int f0 = 0; f0 < nf2; f0 += ESL_CHUNK) {
            const int nfc = nf2 - f0 < ESL_CHUNK ? nf2 - f0 : ESL_CHUNK;
            for (int i = tid; i < nfc * ES_HOP + ES_HOP; i += 1024) buf[i] = oa[s * ESL_MAXLEN + f0 * ES_HOP + i];      // < len2: (nf2 + 1) hop = len2
            __syncthreads();
            for (int item = tid; item < nfc * nkb; item += 1024) {
                const int f = item / nkb, k = k_lo + item - f * nkb;
                const float* fr = buf + f * ES_HOP;
                float re = 0.f, im = 0.f;
                for (int i = 0; i < ES_FRAME; ++i) {
                    const float v = fr[i] * win[i];
                    const float2 w = twd[(k * i) & (ES_NFFT - 1)];
                    re = fmaf(v, w.x, re); im = fmaf(v, w.y, im);
                }
                pw[(s * ESL_MAXFRAMES + f0 + f) * ES_NBIN + k] = re * re + im * im;
            }
            __syncthreads();
        }
    __threadfence_block();
    __syncthreads();
    for (int item = tid; item < 2 * nf2 * ES_BANDS; item += 1024) {
        const int s = item / (nf2 * ES_BANDS), rem = item - s * nf2 * ES_BANDS, f = rem / ES_BANDS, b = rem - f * ES_BANDS;
        float a = 0.f;
        for (int k = p.band_lo[b]; k < p.band_hi[b]; ++k) a += pw[(s * ESL_MAXFRAMES + f) * ES_NBIN + k];
        tob[s][b][f] = sqrtf(a);
    }
    __syncthreads();
    // ---- segments of 30 frames: row statistics, then column normalisation and the frame's share of the correlation (estoi_kernel)
    const int nseg = nf2 - ES_SEG + 1;
    float* rstat = buf;                                                // [2][nseg][15][2]
    for (int item = tid; item < 2 * nseg * ES_BANDS; item += 1024) {
        const int s = item / (nseg * ES_BANDS), rem = item - s * nseg * ES_BANDS, seg = rem / ES_BANDS, b = rem - seg * ES_BANDS;
        float mean = 0.f;
        for (int i = 0; i < ES_SEG; ++i) mean += tob[s][b][seg + i];
        mean /= (float)ES_SEG;
        float nrm = 0.f;
        for (int i = 0; i < ES_SEG; ++i) { const float v = tob[s][b][seg + i] - mean; nrm = fmaf(v, v, nrm); }
        rstat[item * 2] = mean; rstat[item * 2 + 1] = 1.0f / (sqrtf(nrm) + EPS);
    }
    __syncthreads();
    float part = 0.f;
    for (int item = tid; item < nseg * ES_SEG; item += 1024) {
        const int seg = item / ES_SEG, i = item - seg * ES_SEG;
        float v[2][ES_BANDS];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float mean = 0.f;
#pragma unroll
            for (int b = 0; b < ES_BANDS; ++b) {
                const float* st = rstat + ((s * nseg + seg) * ES_BANDS + b) * 2;
                v[s][b] = (tob[s][b][seg + i] - st[0]) * st[1];
                mean += v[s][b];
            }
            mean /= (float)ES_BANDS;
            float nrm = 0.f;
#pragma unroll
            for (int b = 0; b < ES_BANDS; ++b) { v[s][b] -= mean; nrm = fmaf(v[s][b], v[s][b], nrm); }
            const float inv = 1.0f / (sqrtf(nrm) + EPS);
#pragma unroll
            for (int b = 0; b < ES_BANDS; ++b) v[s][b] *= inv;
        }
        float c = 0.f;
#pragma unroll
        for (int b = 0; b < ES_BANDS; ++b) c = fmaf(v[0][b], v[1][b], c);
        part += c / (float)ES_SEG;
    }
    red[tid] = part;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) p.score[clip] = red[0] / (float)nseg;
}

// =====================================================================================================================================
// The ragged forms (l2s_*_ragged): clips of unequal length in one launch chain.  The per-clip tables (lengths, prefix sums, the clips each kernel form takes)
// are built on the host and reach the WORKSPACE through the carrier of host_table.h: every block of every later launch can search the whole table (the tile
// form's (clip, tile) lookup needs all of it).
// =====================================================================================================================================
static int clip_error(const char* fn, int b, const std::string& what) {
    set_error(std::string("l2s: ") + fn + ": clip " + std::to_string(b) + ": " + what);
    return 1;
}

constexpr int RAG_MAX_CLIPS = 65535, RAG_MAX_FRAMES = 1 << 20, RAG_MAX_SUM_FRAMES = 1 << 24;

// N in range, the length table present, every L_b in [5, 2^20] and their sum at most 2^24 (row and frame indices stay 32-bit)
static int ragged_lengths_check(const char* fn, const int* L, int N) {
    if (N < 1 || N > RAG_MAX_CLIPS) { set_error(std::string("l2s: ") + fn + ": N = " + std::to_string(N) + " clips is outside [1, 65535]"); return 1; }
    if (!L) { set_error(std::string("l2s: ") + fn + ": null table of clip lengths"); return 1; }
    int64_t sum = 0;
    for (int b = 0; b < N; ++b) {
        if (L[b] < 5) return clip_error(fn, b, std::to_string(L[b]) + " frames: at least 5 are needed");
        if (L[b] > RAG_MAX_FRAMES) return clip_error(fn, b, std::to_string(L[b]) + " frames: at most 2^20 per clip");
        sum += L[b];
        if (sum > RAG_MAX_SUM_FRAMES) return clip_error(fn, b, "the clips up to this one hold more than 2^24 frames");
    }
    return 0;
}

}  // namespace l2s

using namespace l2s;

extern "C" {

static int64_t im_align(int64_t x) { return (x + 255) / 256 * 256; }
int64_t l2s_inverse_mel_workspace_bytes(int N, int L, int n_mels, int n_freqs, int rows_per_call, int iters) {
    const int64_t rows = (int64_t)N * L;
    const int calls = rows_per_call > 0 ? N / rows_per_call : 1;
    return 256 + im_align((3 * (int64_t)(n_mels + n_freqs) + 2) * 4) + 2 * im_align(IM_NNZ * 4) + im_align(rows * (iters > 0 ? iters : 1) * 4) + im_align((int64_t)calls * 4);
}

// the buffers both forms of the inverse mel carve first: the band tables of launch_mel_bands and the per-row losses; `end` is what follows them
struct InvMelWs { int* tab; float *fwd, *bwd, *loss_rows; char* end; };
static InvMelWs inverse_mel_carve(void* ws, int n_mels, int n_freqs, int64_t rows, int iters) {
    char* w = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    const int64_t fwd = im_align((3 * (int64_t)(n_mels + n_freqs) + 2) * 4), bwd = fwd + im_align(IM_NNZ * 4), loss = bwd + im_align(IM_NNZ * 4);
    return InvMelWs{(int*)w, (float*)(w + fwd), (float*)(w + bwd), (float*)(w + loss), w + loss + im_align(rows * (iters > 0 ? iters : 1) * 4)};
}

int l2s_inverse_mel(const float* mel, int log_input, const float* fb, int fb_nnz, const float* init, int N, int L, int n_mels, int n_freqs, int rows_per_call,
                    int iters, float* spec, float* loss_per_iter, int* iters_run, void* ws, int64_t ws_bytes, void* stream) {
    L2S_REQUIRE(mel && fb && init && spec && ws, "inverse_mel: null argument");
    L2S_REQUIRE(N > 0 && L > 0 && iters >= 0, "inverse_mel: sizes");
    L2S_REQUIRE(n_mels > 0 && n_mels <= IM_MAXM && n_freqs > 0 && n_freqs <= IM_MAXF, "inverse_mel: at most 128 mel bands and 576 frequency bins");
    L2S_REQUIRE(fb_nnz > 0 && fb_nnz <= IM_NNZ, "inverse_mel: the filterbank's non-zero count (host-side, exact) must be given and at most 2048");
    if (rows_per_call <= 0) rows_per_call = N;
    L2S_REQUIRE(N % rows_per_call == 0, "inverse_mel: rows_per_call must divide N");
    L2S_REQUIRE(ws_bytes >= l2s_inverse_mel_workspace_bytes(N, L, n_mels, n_freqs, rows_per_call, iters), "inverse_mel: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int calls = N / rows_per_call;
    const int64_t rows = (int64_t)N * L;
    const InvMelWs c = inverse_mel_carve(ws, n_mels, n_freqs, rows, iters);
    int* iters_call = iters_run ? iters_run : (int*)c.end;
    ProfScope ps("vocoder_inverse_mel", s);
    if (launch_mel_bands(fb, n_freqs, n_mels, c.tab, c.fwd, c.bwd, s)) return 1;
    InvMelP p{mel, init, c.tab, c.fwd, c.bwd, spec, iters > 0 ? c.loss_rows : nullptr, nullptr, N, L, n_mels, n_freqs, rows_per_call, iters, log_input, 0, nullptr, nullptr, nullptr};
    const unsigned blocks = (unsigned)((rows + IM_ROWS - 1) / IM_ROWS);
    hipLaunchKernelGGL(inverse_mel_kernel<false>, dim3(blocks), dim3(IM_ROWS * 64), 0, s, p);
    if (iters > 0) {
        hipLaunchKernelGGL(inverse_mel_stop_kernel, dim3(calls), dim3(256), 0, s, c.loss_rows, (int)rows, rows_per_call * L, iters, iters_call, loss_per_iter, (const int*)nullptr);
        p.loss_rows = nullptr; p.iters_call = iters_call; p.second = 1;
        hipLaunchKernelGGL(inverse_mel_kernel<false>, dim3(blocks), dim3(IM_ROWS * 64), 0, s, p);      // only the calls a stopping rule ended early re-run
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

int64_t l2s_griffin_lim_workspace_bytes(int N, int L) {
    const int slots = GL_HOP * (L - 1) <= 30720 ? 2 : 3;      // the long form rotates three rebuilt spectra
    return (int64_t)N * L * GL_LDK * 4 + (int64_t)N * slots * L * GL_LDK * 8 + 512;
}

int l2s_griffin_lim(const float* power_spec, const float* init_angles, int N, int L, int n_fft, int hop, int iters, float momentum,
                    float* wave, void* ws, int64_t ws_bytes, void* stream) {
    L2S_REQUIRE(power_spec && init_angles && wave && ws, "griffin_lim: null argument");
    L2S_REQUIRE(n_fft == GL_NFFT && hop == GL_HOP, "griffin_lim: built for n_fft = win_length = 1024, hop 256 (hparams.py)");
    L2S_REQUIRE(N > 0 && L >= 5 && iters >= 0, "griffin_lim: sizes");
    L2S_REQUIRE(N <= 65535 && L <= (1 << 20), "griffin_lim: at most 65 535 clips and 2^20 frames per call");
    L2S_REQUIRE(ws_bytes >= l2s_griffin_lim_workspace_bytes(N, L), "griffin_lim: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    float* mag = (float*)w;
    float2* reb = (float2*)(w + (int64_t)N * L * GL_LDK * 4);
    ProfScope ps("vocoder_griffin_lim", s);
    if (GL_HOP * (L - 1) <= 30720) {
        GriffinP p{power_spec, init_angles, mag, reb, wave, N, L, iters, momentum / (1.0f + momentum), nullptr, nullptr, 0};
        if (GL_HOP * (L - 1) <= 19456) hipLaunchKernelGGL((griffin_lim_kernel<12, 19456, false>), dim3(N), dim3(768), 0, s, p);
        else hipLaunchKernelGGL((griffin_lim_kernel<8, 30720, false>), dim3(N), dim3(512), 0, s, p);
    } else {                                       // 122 frames and more: one launch per iteration over (tile, clip)
        hipLaunchKernelGGL(griffin_lim_tile_prologue_kernel, dim3((GL_NBIN * L + 255) / 256, N), dim3(256), 0, s, power_spec, init_angles, mag, reb, L,
                           (const int*)nullptr, (const int*)nullptr);
        GriffinTileP p{mag, reb, wave, N, L, 0, iters, momentum / (1.0f + momentum), nullptr, nullptr, nullptr, 0, 0};
        for (p.it = 0; p.it <= iters; ++p.it)
            hipLaunchKernelGGL((griffin_lim_tile_kernel<GLT_NW, GLT_F, false>), dim3((L + GLT_F - 1) / GLT_F, N), dim3(GLT_NW * 64), 0, s, p);
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

int64_t l2s_estoi_workspace_bytes(int N) { return 512 + 256 + (int64_t)N * 2 * ES_MAXLEN * 4 + (int64_t)N * 2 * ES_MAXFRAMES * ES_NBIN * 4; }
int64_t l2s_estoi_workspace_bytes_long(int N, int n_resampled) {
    if (n_resampled <= ES_MAXLEN) return l2s_estoi_workspace_bytes(N);
    return 512 + 256 + (int64_t)N * 4 * ESL_MAXLEN * 4 + (int64_t)N * 2 * ESL_MAXFRAMES * ES_NBIN * 4;
}

static int band_edges_check(const char* fn, const int* band_lo_hi_host) {
    for (int b = 0; b < ES_BANDS; ++b)
        L2S_REQUIRE(band_lo_hi_host[b] >= 0 && band_lo_hi_host[b] <= band_lo_hi_host[ES_BANDS + b] && band_lo_hi_host[ES_BANDS + b] <= ES_NBIN &&
                    (b == 0 || band_lo_hi_host[b] >= band_lo_hi_host[b - 1]), std::string(fn) + ": band edges");
    return 0;
}

int l2s_estoi(const float* clean, const float* pred, int N, int n_samples, const float* fir, int n_fir, int up, int down, int n_pre_remove, int n_resampled,
              const int* band_lo_hi_host, float* score, void* ws, int64_t ws_bytes, void* stream) {
    L2S_REQUIRE(clean && pred && score && ws && band_lo_hi_host, "estoi: null argument");
    L2S_REQUIRE(N > 0 && n_samples > 0, "estoi: sizes");
    L2S_REQUIRE(n_resampled > 0 && n_resampled <= ESL_MAXLEN, "estoi: at most 48 256 samples at 10 kHz per clip (4.8 s)");
    L2S_REQUIRE(fir ? (n_fir > 0 && up > 0 && down > 0 && n_pre_remove >= 0) : n_resampled == n_samples, "estoi: resampler arguments");
    L2S_REQUIRE(ws_bytes >= l2s_estoi_workspace_bytes_long(N, n_resampled), "estoi: workspace too small");
    if (band_edges_check("estoi", band_lo_hi_host)) return 1;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    int* bands = (int*)w;
    float* rs = (float*)(w + 256);
    if (table_upload(bands, band_lo_hi_host, 2 * ES_BANDS, s)) return 1;
    ProfScope ps("metric_estoi", s);
    if (n_resampled <= ES_MAXLEN) {
        float* pw = rs + (int64_t)N * 2 * ES_MAXLEN;
        EstoiP p{clean, pred, fir, bands, bands + ES_BANDS, rs, pw, score, N, n_samples, n_fir, up, down, n_pre_remove, n_resampled, EstoiRag{}};
        hipLaunchKernelGGL(estoi_kernel<false>, dim3(N), dim3(1024), 0, s, p);
    } else {                                       // the long form: the signals in the workspace, the resampler a kernel of its own
        L2S_REQUIRE(N <= 65535, "estoi: at most 65 535 clips per call");
        float* oa = rs + (int64_t)N * 2 * ESL_MAXLEN;
        float* pw = oa + (int64_t)N * 2 * ESL_MAXLEN;
        EstoiLongP p{clean, pred, fir, bands, bands + ES_BANDS, rs, oa, pw, score, N, n_samples, n_fir, up, down, n_pre_remove, n_resampled, EstoiRag{}};
        hipLaunchKernelGGL(estoi_resample_kernel<false>, dim3((n_resampled + 255) / 256, 2, N), dim3(256), 0, s, p);
        hipLaunchKernelGGL(estoi_long_kernel<false>, dim3(N), dim3(1024), 0, s, p);
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------ ragged forms
int l2s_inverse_mel_ragged_check(const int* L, const int64_t* mel_offset, const int64_t* mel_pitch, int N, int64_t mel_floats, int n_mels, int n_freqs,
                                 int fb_nnz, int iters) {
    const char* fn = "inverse_mel_ragged";
    if (ragged_lengths_check(fn, L, N)) return 1;
    L2S_REQUIRE(mel_offset && mel_pitch, "inverse_mel_ragged: null table of mel offsets or pitches");
    L2S_REQUIRE(n_mels > 0 && n_mels <= IM_MAXM && n_freqs > 0 && n_freqs <= IM_MAXF, "inverse_mel_ragged: at most 128 mel bands and 576 frequency bins");
    L2S_REQUIRE(fb_nnz > 0 && fb_nnz <= IM_NNZ, "inverse_mel_ragged: the filterbank's non-zero count (host-side, exact) must be given and at most 2048");
    L2S_REQUIRE(iters >= 0 && mel_floats >= 0, "inverse_mel_ragged: sizes");
    for (int b = 0; b < N; ++b) {
        if (mel_offset[b] < 0) return clip_error(fn, b, "mel offset " + std::to_string(mel_offset[b]) + " is negative");
        if (mel_pitch[b] < L[b]) return clip_error(fn, b, "mel pitch " + std::to_string(mel_pitch[b]) + " is below its " + std::to_string(L[b]) + " frames");
        if (mel_pitch[b] > ((int64_t)1 << 40)) return clip_error(fn, b, "mel pitch " + std::to_string(mel_pitch[b]) + " is above 2^40");
        const int64_t end = mel_offset[b] + (int64_t)(n_mels - 1) * mel_pitch[b] + L[b];
        if (end > mel_floats)
            return clip_error(fn, b, "its mel (offset " + std::to_string(mel_offset[b]) + ", pitch " + std::to_string(mel_pitch[b]) + ", " + std::to_string(L[b]) +
                              " frames) is read up to float " + std::to_string(end) + ", past the buffer of " + std::to_string(mel_floats));
    }
    return 0;
}

// table: mel_offset[N] | mel_pitch[N] (int64) | the row prefix sums [N + 1] (written by the caller)
struct ImTable { int64_t off, pitch, row_off; };
static ImTable im_table(HostTable& t, int N, const int64_t* mel_offset, const int64_t* mel_pitch) {
    return ImTable{t.i64(mel_offset, N), t.i64(mel_pitch, N), t.i32(nullptr, (int64_t)N + 1)};
}

// never below the sum of the solo sizers (N = 1, L = L_b): a caller that sized for a loop of solo calls has enough
int64_t l2s_inverse_mel_ragged_workspace_bytes(const int* L, int N, int n_mels, int n_freqs, int iters) {
    if (ragged_lengths_check("inverse_mel_ragged", L, N)) return -1;
    HostTable t(false);
    im_table(t, N, nullptr, nullptr);
    int64_t bytes = 256 + im_align(t.words() * 4) + 512;      // 512: this size once rounded the table's three segments up one by one, and never shrinks
    for (int b = 0; b < N; ++b) bytes += l2s_inverse_mel_workspace_bytes(1, L[b], n_mels, n_freqs, 1, iters);
    return bytes;
}

int l2s_inverse_mel_ragged(const float* mel, int64_t mel_floats, const int64_t* mel_offset, const int64_t* mel_pitch, const int* L, int N, int log_input,
                           const float* fb, int fb_nnz, const float* init, int n_mels, int n_freqs, int iters, float* spec, float* loss_per_iter,
                           int* iters_run, void* ws, int64_t ws_bytes, void* stream) {
    if (l2s_inverse_mel_ragged_check(L, mel_offset, mel_pitch, N, mel_floats, n_mels, n_freqs, fb_nnz, iters)) return 1;
    L2S_REQUIRE(mel && fb && init && spec && ws, "inverse_mel_ragged: null argument");
    L2S_REQUIRE(ws_bytes >= l2s_inverse_mel_ragged_workspace_bytes(L, N, n_mels, n_freqs, iters), "inverse_mel_ragged: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    HostTable t;
    const ImTable o = im_table(t, N, mel_offset, mel_pitch);
    int* row_off = t.host<int>(o.row_off);
    int64_t rows = 0;
    for (int b = 0; b < N; ++b) { row_off[b] = (int)rows; rows += L[b]; }
    row_off[N] = (int)rows;
    const InvMelWs c = inverse_mel_carve(ws, n_mels, n_freqs, rows, iters);
    float* loss_rows = c.loss_rows;
    int* table = (int*)(c.end + im_align((int64_t)N * 4));       // 256-byte aligned, behind the iteration counts
    const int64_t *d_off = table_seg<int64_t>(table, o.off), *d_pitch = table_seg<int64_t>(table, o.pitch);
    const int* d_row_off = table + o.row_off;
    int* iters_call = iters_run ? iters_run : (int*)c.end;
    ProfScope ps("vocoder_inverse_mel_ragged", s);
    if (t.upload(table, s)) return 1;
    if (launch_mel_bands(fb, n_freqs, n_mels, c.tab, c.fwd, c.bwd, s)) return 1;      // once per call, whatever N
    InvMelP p{mel, init, c.tab, c.fwd, c.bwd, spec, iters > 0 ? loss_rows : nullptr, nullptr, N, 0, n_mels, n_freqs, 1, iters, log_input, 0, d_row_off, d_off, d_pitch};
    const unsigned blocks = (unsigned)((rows + IM_ROWS - 1) / IM_ROWS);
    hipLaunchKernelGGL(inverse_mel_kernel<true>, dim3(blocks), dim3(IM_ROWS * 64), 0, s, p);
    if (iters > 0) {
        hipLaunchKernelGGL(inverse_mel_stop_kernel, dim3(N), dim3(256), 0, s, loss_rows, (int)rows, 0, iters, iters_call, loss_per_iter, d_row_off);
        p.loss_rows = nullptr; p.iters_call = iters_call; p.second = 1;
        hipLaunchKernelGGL(inverse_mel_kernel<true>, dim3(blocks), dim3(IM_ROWS * 64), 0, s, p);      // only the clips a stopping rule ended early re-run
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

int l2s_griffin_lim_ragged_check(const int* L, int N, int n_fft, int hop, int iters, int64_t wave_pitch) {
    const char* fn = "griffin_lim_ragged";
    L2S_REQUIRE(n_fft == GL_NFFT && hop == GL_HOP, "griffin_lim_ragged: built for n_fft = win_length = 1024, hop 256 (hparams.py)");
    if (ragged_lengths_check(fn, L, N)) return 1;
    L2S_REQUIRE(iters >= 0, "griffin_lim_ragged: sizes");
    for (int b = 0; b < N; ++b)
        if ((int64_t)GL_HOP * (L[b] - 1) > wave_pitch)
            return clip_error(fn, b, "its " + std::to_string((int64_t)GL_HOP * (L[b] - 1)) + " samples do not fit the row pitch of " + std::to_string(wave_pitch) +
                              ": the rows of wave would overlap");
    return 0;
}

// table: frame_off[N + 1] | clips of the 12-wave form | of the 8-wave form | of the tile form | tile_off[n_long + 1]
struct GlTable { int64_t frame_off, c12, c8, cl, tile_off; };
static GlTable gl_table(HostTable& t, int N, const int* frame_off, const int* c12, int n12, const int* c8, int n8, const int* cl, int nl, const int* tile_off) {
    return GlTable{t.i32(frame_off, (int64_t)N + 1), t.i32(c12, n12), t.i32(c8, n8), t.i32(cl, nl), t.i32(tile_off, nl ? nl + 1 : 0)};
}
// the table's slot: the largest table (every clip takes the tile form) and the one spare word this size has always counted
static int64_t gl_table_bytes(int N) { HostTable t(false); gl_table(t, N, nullptr, nullptr, 0, nullptr, 0, nullptr, N, nullptr); return im_align((t.words() + 1) * 4); }

int64_t l2s_griffin_lim_ragged_workspace_bytes(const int* L, int N) {
    if (ragged_lengths_check("griffin_lim_ragged", L, N)) return -1;
    int64_t frames = 0;
    for (int b = 0; b < N; ++b) frames += L[b];
    // three slots of rebuilt spectra per frame whatever the clip's form (one block offset serves every form), and the solo sizers' 512 bytes per clip:
    // never below their sum
    return 512 + gl_table_bytes(N) + frames * GL_LDK * 4 + frames * 3 * GL_LDK * 8 + 512 * (int64_t)N;
}

int l2s_griffin_lim_ragged(const float* power_spec, const float* init_angles, const int* L, int N, int n_fft, int hop, int iters, float momentum,
                           float* wave, int64_t wave_pitch, void* ws, int64_t ws_bytes, void* stream) {
    if (l2s_griffin_lim_ragged_check(L, N, n_fft, hop, iters, wave_pitch)) return 1;
    L2S_REQUIRE(power_spec && init_angles && wave && ws, "griffin_lim_ragged: null argument");
    L2S_REQUIRE(ws_bytes >= l2s_griffin_lim_ragged_workspace_bytes(L, N), "griffin_lim_ragged: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> foff((size_t)N + 1), l12, l8, ll, toff;
    int64_t frames = 0;
    int long_max = 0, tiles = 0;
    for (int b = 0; b < N; ++b) {
        foff[b] = (int)frames; frames += L[b];
        const int ylen = GL_HOP * (L[b] - 1);
        if (ylen <= 19456) l12.push_back(b);
        else if (ylen <= 30720) l8.push_back(b);
        else { toff.push_back(tiles); tiles += (L[b] + GLT_F - 1) / GLT_F; ll.push_back(b); long_max = std::max(long_max, L[b]); }
    }
    foff[N] = (int)frames;
    const int n12 = (int)l12.size(), n8 = (int)l8.size(), nl = (int)ll.size();
    if (nl) toff.push_back(tiles);
    HostTable t;
    const GlTable o = gl_table(t, N, foff.data(), l12.data(), n12, l8.data(), n8, ll.data(), nl, toff.data());
    char* w = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    int* table = (int*)w; w += gl_table_bytes(N);
    float* mag = (float*)w;
    float2* reb = (float2*)(w + frames * GL_LDK * 4);
    const int *d_off = table + o.frame_off, *d12 = table + o.c12, *d8 = table + o.c8, *dl = table + o.cl, *dt = table + o.tile_off;
    ProfScope ps("vocoder_griffin_lim_ragged", s);
    if (t.upload(table, s)) return 1;
    const float mom = momentum / (1.0f + momentum);
    if (n12) {
        GriffinP p{power_spec, init_angles, mag, reb, wave, N, 0, iters, mom, d_off, d12, wave_pitch};
        hipLaunchKernelGGL((griffin_lim_kernel<12, 19456, true>), dim3(n12), dim3(768), 0, s, p);
    }
    if (n8) {
        GriffinP p{power_spec, init_angles, mag, reb, wave, N, 0, iters, mom, d_off, d8, wave_pitch};
        hipLaunchKernelGGL((griffin_lim_kernel<8, 30720, true>), dim3(n8), dim3(512), 0, s, p);
    }
    if (nl) {                                      // one launch per iteration over the (clip, tile) pairs of the long clips only
        hipLaunchKernelGGL(griffin_lim_tile_prologue_kernel, dim3((GL_NBIN * long_max + 255) / 256, nl), dim3(256), 0, s, power_spec, init_angles, mag, reb, 0, d_off, dl);
        GriffinTileP p{mag, reb, wave, N, 0, 0, iters, mom, d_off, dl, dt, nl, wave_pitch};
        for (p.it = 0; p.it <= iters; ++p.it)
            hipLaunchKernelGGL((griffin_lim_tile_kernel<GLT_NW, GLT_F, true>), dim3(tiles), dim3(GLT_NW * 64), 0, s, p);
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

int l2s_estoi_ragged_check(const int* n_samples, const int* n_fir, const int* n_resampled, int N, int64_t pitch, int has_fir, int n_fir_max, int up, int down,
                           int n_pre_remove) {
    const char* fn = "estoi_ragged";
    if (N < 1 || N > RAG_MAX_CLIPS) { set_error("l2s: estoi_ragged: N = " + std::to_string(N) + " clips is outside [1, 65535]"); return 1; }
    L2S_REQUIRE(n_samples && n_resampled && (!has_fir || n_fir), "estoi_ragged: null table of sample counts, filter lengths or resampled lengths");
    L2S_REQUIRE(!has_fir || (n_fir_max > 0 && up > 0 && down > 0 && n_pre_remove >= 0), "estoi_ragged: resampler arguments");
    for (int b = 0; b < N; ++b) {
        if (n_samples[b] < 1) return clip_error(fn, b, std::to_string(n_samples[b]) + " samples: at least one is needed");
        if (n_samples[b] > pitch)
            return clip_error(fn, b, "its " + std::to_string(n_samples[b]) + " samples do not fit the row pitch of " + std::to_string(pitch) + ": the rows would overlap");
        if (n_resampled[b] < 1 || n_resampled[b] > ESL_MAXLEN)
            return clip_error(fn, b, std::to_string(n_resampled[b]) + " samples at 10 kHz: outside [1, 48256] (4.8 s)");
        if (has_fir && (n_fir[b] < 1 || n_fir[b] > n_fir_max))
            return clip_error(fn, b, "its filter of " + std::to_string(n_fir[b]) + " taps is not a prefix of the call's table of " + std::to_string(n_fir_max));
        if (!has_fir && n_resampled[b] != n_samples[b]) return clip_error(fn, b, "without a resampling filter n_resampled must equal n_samples");
    }
    return 0;
}

// table: n_samples[N] | n_fir[N] (null: zeros) | n_resampled[N] | clips of the short form [ns], then of the long form [N - ns] | band edges [30]
struct EsTable { int64_t n_samples, n_fir, n_resampled, c_short, c_long, bands; };
static EsTable es_table(HostTable& t, int N, const int* n_samples, const int* n_fir, const int* n_resampled, const int* c_short, int ns, const int* c_long,
                        const int* band_lo_hi) {
    return EsTable{t.i32(n_samples, N), t.i32(n_fir, N), t.i32(n_resampled, N), t.i32(c_short, ns), t.i32(c_long, N - ns), t.i32(band_lo_hi, 2 * ES_BANDS)};
}
static int64_t es_table_bytes(int N) { HostTable t(false); es_table(t, N, nullptr, nullptr, nullptr, nullptr, N, nullptr, nullptr); return im_align(t.words() * 4); }

// the sum of the solo sizers (each clip's form by its own n_resampled) plus the tables
int64_t l2s_estoi_ragged_workspace_bytes(const int* n_resampled, int N) {
    if (N < 1 || N > RAG_MAX_CLIPS || !n_resampled) { set_error("l2s: estoi_ragged: N outside [1, 65535] or a null table of resampled lengths"); return -1; }
    int64_t bytes = 256 + es_table_bytes(N);
    for (int b = 0; b < N; ++b) bytes += l2s_estoi_workspace_bytes_long(1, n_resampled[b]);
    return bytes;
}

int l2s_estoi_ragged(const float* clean, const float* pred, int64_t pitch, const int* n_samples, int N, const float* fir, int n_fir_max, const int* n_fir,
                     int up, int down, int n_pre_remove, const int* n_resampled, const int* band_lo_hi_host, float* score, void* ws, int64_t ws_bytes,
                     void* stream) {
    if (l2s_estoi_ragged_check(n_samples, n_fir, n_resampled, N, pitch, fir != nullptr, n_fir_max, up, down, n_pre_remove)) return 1;
    L2S_REQUIRE(clean && pred && score && ws && band_lo_hi_host, "estoi_ragged: null argument");
    L2S_REQUIRE(ws_bytes >= l2s_estoi_ragged_workspace_bytes(n_resampled, N), "estoi_ragged: workspace too small");
    if (band_edges_check("estoi_ragged", band_lo_hi_host)) return 1;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> ls, ll;
    int long_max = 0;
    for (int b = 0; b < N; ++b) {
        if (n_resampled[b] <= ES_MAXLEN) ls.push_back(b); else { ll.push_back(b); long_max = std::max(long_max, n_resampled[b]); }
    }
    const int ns = (int)ls.size(), nl = (int)ll.size();
    HostTable t;
    const EsTable o = es_table(t, N, n_samples, fir ? n_fir : nullptr, n_resampled, ls.data(), ns, ll.data(), band_lo_hi_host);
    char* w = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    int* table = (int*)w; w += es_table_bytes(N);
    const int* bands = table + o.bands;
    float* rs_s = (float*)w;                                                  // short slots: (ns, 2, ES_MAXLEN) then (ns, 2, ES_MAXFRAMES, ES_NBIN)
    float* pw_s = rs_s + (int64_t)ns * 2 * ES_MAXLEN;
    float* rs_l = pw_s + (int64_t)ns * 2 * ES_MAXFRAMES * ES_NBIN;            // long slots: rs, oa (nl, 2, ESL_MAXLEN) each, then the spectra
    float* oa_l = rs_l + (int64_t)nl * 2 * ESL_MAXLEN;
    float* pw_l = oa_l + (int64_t)nl * 2 * ESL_MAXLEN;
    ProfScope ps("metric_estoi_ragged", s);
    if (t.upload(table, s)) return 1;
    if (ns) {
        EstoiP p{clean, pred, fir, bands, bands + ES_BANDS, rs_s, pw_s, score, N, 0, 0, up, down, n_pre_remove, 0,
                 EstoiRag{table + o.n_samples, table + o.n_fir, table + o.n_resampled, table + o.c_short, pitch}};
        hipLaunchKernelGGL(estoi_kernel<true>, dim3(ns), dim3(1024), 0, s, p);
    }
    if (nl) {
        EstoiLongP p{clean, pred, fir, bands, bands + ES_BANDS, rs_l, oa_l, pw_l, score, N, 0, 0, up, down, n_pre_remove, 0,
                     EstoiRag{table + o.n_samples, table + o.n_fir, table + o.n_resampled, table + o.c_long, pitch}};
        hipLaunchKernelGGL(estoi_resample_kernel<true>, dim3((long_max + 255) / 256, 2, nl), dim3(256), 0, s, p);
        hipLaunchKernelGGL(estoi_long_kernel<true>, dim3(nl), dim3(1024), 0, s, p);
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
