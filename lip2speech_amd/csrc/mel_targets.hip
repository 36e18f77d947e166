// Mel targets on the device: the audio half of the data boundary (reference: datasets/spectograms.py:41-59 - torchaudio MelSpectrogram + log(clamp(x, 1e-5)) -
// and the audio / mel / gate padding of the collates, datasets/__init__.py:7-46).  B waveforms packed back to back become the padded (B, n_mels, M_pad) log-mel
// targets, the gates, the mel lengths and the zero-padded audio in one launch chain: the band table of the filterbank (the vocoder's inverse_mel_bands_kernel),
// the window table, one kernel over the B x M_pad frames, one copy kernel for the audio.  torchaudio is absent from the build image: what is implemented is the algorithm as
// restated in lip2speech_amd/datasets/spectrograms.py (PARITY UNPINNED against the package); the kernel is tested against that restatement in fp64.
#include "fft_dev.h"
#include "l2s_common.h"
#include "../../include/l2s.h"

#include <math.h>

namespace l2s {

constexpr int MT_NFFT = 1024, MT_HOP = 256, MT_NBIN = 513, MT_LDK = 520;      // torch.stft(center=True) of n samples: n / 256 + 1 frames of 513 bins
constexpr int MT_WAVES = 4;       // frames (waves) per block: they share the compact filterbank table in LDS.  A build with 8 timed the same within the spread
                                  // (profiles/mel_targets_times.txt, variant (c)): the smaller block stays
constexpr int MT_CLIPS = 64;      // clips per launch (the clip table travels in the kernel arguments, like the frame collate's)
constexpr int MT_MAX_SAMPLES = 1 << 30;

struct MelClips { int64_t off[MT_CLIPS]; int32_t n[MT_CLIPS]; };

// The window, once per call: torch.hann_window(1024, periodic=True) AS TORCH BUILDS IT, in fp32 - 0.5 - 0.5 cos(fl(k * fl(2 pi / 1024))).  The rounded argument
// puts torch's values up to 1.9e-7 away from the exact Hann window, which is more than rounding, and the transform this kernel is held against (the fp64
// restatement) runs on torch's table: a frame whose only energy sits at the window's foot sees that difference in full.  The cosine itself is the fp64 one
// rounded to nearest, so the table is torch's to the rounding of its fp32 cosine.
__global__ __launch_bounds__(256) void mel_window_kernel(float* win) {
    const float c = (float)(6.283185307179586 / 1024.0);
    for (int i = threadIdx.x; i < MT_NFFT; i += 256) win[i] = 0.5f + -0.5f * (float)cos((double)((float)i * c));
}

struct MelTargetsP {
    const float* audio;      // the packed waveforms
    const float* fb;         // (513, n_mels)
    const float* win;        // ws: mel_window_kernel's table
    const int* tab;          // ws: launch_mel_bands' table
    const float* fwd;        // ws: fb's values over each band's [first, last] bins, band-major
    float* mels;             // (B, n_mels, M_pad), this launch's first clip
    float* gate;             // (B, M_pad) or null
    int64_t* mel_lengths;    // (B) or null
    int B, n_mels, M_pad, log_output;
    float mel_pad;
};

// ONE WAVE PER FRAME (b, t) of the B x M_pad grid, so that every element of mels and gate has exactly one writer and a frame's value cannot depend on what
// else is in the launch.  A real frame: lane j loads the packed points z[n] = x[2n] + i x[2n+1], n = j + 64 r, of the frame's 1024 samples t*256 - 512 + i
// (the reflect padding of torch.stft(center=True) folded into the index, as in griffin_lim_kernel's phase B), times the periodic Hann window; fft512 +
// rfft1024_post give the 513 bins, whose powers go to the wave's LDS scratch; then each lane sums one or two mel bands over the band's own bins, ascending.
__global__ __launch_bounds__(MT_WAVES * 64) void mel_targets_kernel(const MelTargetsP p, const MelClips clips) {
    __shared__ __attribute__((aligned(16))) float2 scratch[MT_WAVES][MT_LDK];
    __shared__ float s_fwd[IM_NNZ];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = p.n_mels;
    // the band ranges are contiguous [first, last]: a filterbank with zeros inside a band can need more than the compact table holds - then fb itself is read
    const int nf = p.tab[3 * (M + MT_NBIN)];
    const bool compact = nf <= IM_NNZ;
    if (compact) for (int i = tid; i < nf; i += MT_WAVES * 64) s_fwd[i] = p.fwd[i];
    __syncthreads();                                   // the only block barrier: from here on every wave runs its own frame
    const int64_t w = (int64_t)blockIdx.x * MT_WAVES + wave;
    if (w >= (int64_t)p.B * p.M_pad) return;           // tail waves of the last block
    const int b = (int)(w / p.M_pad), t = (int)(w - (int64_t)b * p.M_pad);
    const int n = clips.n[b], Mb = n / MT_HOP + 1;
    float* out = p.mels + (int64_t)b * M * p.M_pad + t;
    if (lane == 0) {
        if (p.gate) p.gate[(int64_t)b * p.M_pad + t] = t >= Mb - 1 ? 1.f : 0.f;
        if (p.mel_lengths && t == 0) p.mel_lengths[b] = Mb;
    }
    if (t >= Mb) {                                     // a pad frame
        for (int m = lane; m < M; m += 64) out[(int64_t)m * p.M_pad] = p.mel_pad;
        return;
    }
    const float* x = p.audio + clips.off[b];
    const bool al8 = (reinterpret_cast<uintptr_t>(x) & 7u) == 0;      // the frame starts on an even sample: its pairs are 8-byte aligned when the clip is
    float2* sc = scratch[wave];
    Fft512Tw tw;
    tw.init(lane);
    float2 v[8];
    const int base = t * MT_HOP - MT_NFFT / 2;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int k = 2 * (lane + 64 * r);
        const int s0 = base + k, s1 = s0 + 1;
        float2 z;
        if (al8 && s0 >= 0 && s1 < n) {
            z = *reinterpret_cast<const float2*>(x + s0);
        } else {                                       // a single reflection at either end (n >= 513 > n_fft / 2)
            int a = s0 < 0 ? -s0 : s0; a = a >= n ? 2 * (n - 1) - a : a;
            int c = s1 < 0 ? -s1 : s1; c = c >= n ? 2 * (n - 1) - c : c;
            z = make_float2(x[a], x[c]);
        }
        const float2 wn = *reinterpret_cast<const float2*>(p.win + k);      // the window at samples k, k + 1
        v[r] = make_float2(z.x * wn.x, z.y * wn.y);
    }
    fft512<-1>(v, sc, lane, tw);
    const float nyq = rfft1024_post(v, sc, lane, tw);
    float* pw = reinterpret_cast<float*>(sc);          // the scratch is dead after the mirrored read: the frame's 513 powers
#pragma unroll
    for (int r = 0; r < 8; ++r) pw[lane + 64 * r] = v[r].x * v[r].x + v[r].y * v[r].y;
    if (lane == 0) pw[512] = nyq * nyq;
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = lane + 64 * i;
        if (m >= M) continue;
        const int lo = p.tab[3 * m], cnt = p.tab[3 * m + 1] - lo, o = p.tab[3 * m + 2];
        float acc = 0.f;
        if (compact) for (int c = 0; c < cnt; ++c) acc = fmaf(pw[lo + c], s_fwd[o + c], acc);                       // bins ascending
        else for (int c = 0; c < cnt; ++c) acc = fmaf(pw[lo + c], p.fb[(int64_t)(lo + c) * M + m], acc);
        // the log in fp64, rounded to nearest: the device's logf came out 2 ulp from the rounded value at the floor itself (logf(1e-5f), every silent frame)
        out[(int64_t)m * p.M_pad] = p.log_output ? (float)log((double)fmaxf(acc, 1e-5f)) : acc;
    }
}

// audio_pad[b][i] = the clip's sample i, zeros from n_b on; block (x: a stride of samples, y: clip)
__global__ __launch_bounds__(256) void mel_audio_pad_kernel(const float* __restrict__ audio, const MelClips clips, int64_t A_pad, float* __restrict__ audio_pad) {
    const int b = blockIdx.y;
    const float* x = audio + clips.off[b];
    const int64_t n = clips.n[b];
    float* dst = audio_pad + (int64_t)b * A_pad;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < A_pad; i += (int64_t)gridDim.x * 256) dst[i] = i < n ? x[i] : 0.f;
}

}  // namespace l2s

using namespace l2s;

extern "C" {

int l2s_mel_frames(int64_t n_samples) {
    if (n_samples <= MT_NFFT / 2 || n_samples > MT_MAX_SAMPLES) {
        set_error("l2s: mel_frames: n_samples = " + std::to_string(n_samples) + " is outside [513, 2^30] (the reflect padding of 512 needs more than 512 samples)");
        return 0;
    }
    return (int)(n_samples / MT_HOP) + 1;
}

static int64_t mt_align(int64_t x) { return (x + 255) / 256 * 256; }
int64_t l2s_mel_targets_workspace_bytes(int B, int n_mels) {
    (void)B;                                           // the band tables only: nothing per clip
    return 256 + mt_align((3 * (int64_t)(n_mels + MT_NBIN) + 2) * 4) + 2 * mt_align(IM_NNZ * 4) + mt_align(MT_NFFT * 4);
}

int l2s_mel_targets(const float* audio_packed, const int64_t* offsets, const int64_t* n_samples, int B, const float* fb, int fb_nnz, int n_mels, int n_fft,
                    int hop, int log_output, float mel_pad, int M_pad, int64_t A_pad, float* mels, float* gate, float* audio_pad, int64_t* mel_lengths,
                    void* ws, int64_t ws_bytes, void* stream) {
    L2S_REQUIRE(audio_packed && offsets && n_samples && fb && mels && ws, "mel_targets: null argument");
    L2S_REQUIRE(B > 0, "mel_targets: B must be positive");
    L2S_REQUIRE(n_fft == MT_NFFT && hop == MT_HOP, "mel_targets: built for n_fft = win_length = 1024, hop 256 (hparams.py)");
    L2S_REQUIRE(n_mels >= 1 && n_mels <= IM_MAXM, "mel_targets: n_mels must be in [1, 128]");
    L2S_REQUIRE(fb_nnz > 0 && fb_nnz <= IM_NNZ, "mel_targets: fb_nnz, the filterbank's non-zero count (host-side, exact), must be given and at most 2048");
    L2S_REQUIRE(M_pad > 0 && (int64_t)B * M_pad <= INT32_MAX, "mel_targets: M_pad must be positive and B * M_pad below 2^31");
    for (int b = 0; b < B; ++b) {
        const std::string row = "[" + std::to_string(b) + "] = ";
        if (n_samples[b] <= MT_NFFT / 2 || n_samples[b] > MT_MAX_SAMPLES) {
            set_error("l2s: mel_targets: n_samples" + row + std::to_string(n_samples[b]) + " is outside [513, 2^30]");
            return 1;
        }
        if (offsets[b] < 0) { set_error("l2s: mel_targets: offsets" + row + std::to_string(offsets[b]) + " is negative"); return 1; }
        const int64_t Mb = n_samples[b] / MT_HOP + 1;
        if (Mb > M_pad) {
            set_error("l2s: mel_targets: M_pad = " + std::to_string(M_pad) + " is below the " + std::to_string(Mb) + " frames of n_samples" + row + std::to_string(n_samples[b]));
            return 1;
        }
        if (audio_pad && n_samples[b] > A_pad) {
            set_error("l2s: mel_targets: A_pad = " + std::to_string(A_pad) + " is below n_samples" + row + std::to_string(n_samples[b]));
            return 1;
        }
    }
    L2S_REQUIRE(ws_bytes >= l2s_mel_targets_workspace_bytes(B, n_mels), "mel_targets: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    int* tab = (int*)w; w += mt_align((3 * (int64_t)(n_mels + MT_NBIN) + 2) * 4);
    float* fwd = (float*)w; w += mt_align(IM_NNZ * 4);
    float* bwd = (float*)w; w += mt_align(IM_NNZ * 4);
    float* win = (float*)w;
    ProfScope ps("mel_targets", s);
    if (launch_mel_bands(fb, MT_NBIN, n_mels, tab, fwd, bwd, s)) return 1;
    hipLaunchKernelGGL(mel_window_kernel, dim3(1), dim3(256), 0, s, win);
    for (int b0 = 0; b0 < B; b0 += MT_CLIPS) {
        const int nb = B - b0 < MT_CLIPS ? B - b0 : MT_CLIPS;
        MelClips clips{};
        for (int i = 0; i < nb; ++i) { clips.off[i] = offsets[b0 + i]; clips.n[i] = (int32_t)n_samples[b0 + i]; }
        MelTargetsP p{audio_packed, fb, win, tab, fwd, mels + (int64_t)b0 * n_mels * M_pad, gate ? gate + (int64_t)b0 * M_pad : nullptr,
                      mel_lengths ? mel_lengths + b0 : nullptr, nb, n_mels, M_pad, log_output, mel_pad};
        const unsigned blocks = (unsigned)(((int64_t)nb * M_pad + MT_WAVES - 1) / MT_WAVES);
        hipLaunchKernelGGL(mel_targets_kernel, dim3(blocks), dim3(MT_WAVES * 64), 0, s, p, clips);
        if (audio_pad) {
            const int64_t bx = (A_pad + 255) / 256;
            hipLaunchKernelGGL(mel_audio_pad_kernel, dim3((unsigned)(bx < 1024 ? bx : 1024), nb), dim3(256), 0, s, audio_packed, clips, A_pad,
                               audio_pad + (int64_t)b0 * A_pad);
        }
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
