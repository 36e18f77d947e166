"""What the long forms of the device vocoder and metric cost (include/l2s.h `l2s_griffin_lim` past 121 frames, `l2s_estoi` past 16 512 samples at
10 kHz; vocoder.hip) - the tail of evaluate.py / demo.py, NOT on the mel-frames/s path.  Per call, log-mel in, waveform and ESTOI scores out:
  (a) `MelSpec2Audio(max_iters=256, backend="torch")` on the device (~5 000 torch launches), the waveforms copied to the host and scored by the fp64
      numpy restatement `metrics.stoi` clip by clip - the route these shapes took before the long forms existed;
  (b) `MelSpec2Audio(max_iters=256, backend="hip")` and `metrics.estoi_device`: the waveforms never leave the GPU, one (N,) score vector comes back;
  (c) with `ALT_LIBS=name=path[,name=path...]` (other builds of this library, e.g. another GLT_F / GLT_NW in vocoder.hip): `l2s_griffin_lim` alone,
      256 iterations, from every build in the same process - the tile-size / waves-per-block A/B.
Shapes: N = 1 x 300 frames (a demo clip at the decoder's limit), N = 16 x 188 (a GRID batch), N = 32 x 188.
ROUNDS interleaved rounds, the variants rotating inside a round, wall clock around REPS synchronised calls (the host metric is host work); per variant
the median of the rounds and the whole span.
`SHAPES=NxL[,NxL...]`: other shapes; `ROUNDS=`, `REPS=`, `ITERS=`.
-> profiles/vocoder_long_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from lip2speech_amd import metrics, native
from lip2speech_amd.datasets.spectrograms import MelSpec2Audio, MelSpectrogram
from tools import abtime

ROUNDS = int(os.environ.get("ROUNDS", 5))
REPS = int(os.environ.get("REPS", 2))
ITERS = int(os.environ.get("ITERS", 256))
WORKLOADS = [("demo clip", 1, 300), ("GRID batch", 16, 188), ("two GRID batches", 32, 188)]
if os.environ.get("SHAPES"):                      # "N x L,N x L": other shapes (the smoke test runs one small one)
    WORKLOADS = [(s, int(s.split("x")[0]), int(s.split("x")[1])) for s in os.environ["SHAPES"].split(",")]
FS = 16000


def griffin_lim_call(L, power, ang):
    N, _, Lf = power.shape
    ws = torch.empty(int(L.l2s_griffin_lim_workspace_bytes(N, Lf)), dtype=torch.uint8, device="cuda")
    wave = torch.empty(N, 256 * (Lf - 1), device="cuda")

    def call():
        native.check(L.l2s_griffin_lim(power.data_ptr(), ang.data_ptr(), N, Lf, 1024, 256, ITERS, 0.99, wave.data_ptr(), ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream), L)
        return wave
    return call


def workload(title, N, L, alts):
    n = 256 * (L - 1)
    rng = np.random.default_rng(N * 1000 + L)
    t = np.arange(n) / FS
    clean = np.stack([np.sin(2 * np.pi * (110 + 20 * i) * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t)) + 0.3 * rng.standard_normal(n) for i in range(N)])
    clean = torch.from_numpy(clean.astype(np.float32) * 0.1)
    clean_dev = clean.cuda()
    mel = MelSpectrogram(backend="torch").cuda()(clean_dev)[:, :, :L].contiguous()
    voc_t, voc_h = MelSpec2Audio(max_iters=ITERS, backend="torch").cuda(), MelSpec2Audio(max_iters=ITERS, backend="hip").cuda()
    g = torch.Generator(device="cuda")

    def torch_route():
        pred = voc_t(mel, generator=g.manual_seed(1)).cpu().numpy()
        gt = clean.numpy()
        return np.array([metrics.stoi(gt[i], pred[i], FS, extended=True) for i in range(N)])

    def hip_route():
        pred = voc_h(mel, generator=g.manual_seed(1))
        return metrics.estoi_device(clean_dev, pred, FS).cpu().numpy()

    variants = [("(a) torch vocoder + host ESTOI", torch_route), ("(b) hip vocoder + device ESTOI", hip_route)]
    tt, (sa, sb) = abtime.rounds(variants, ROUNDS, (1, REPS), clock="host")          # the warm-up call covers both routes
    print(f"\n== {title}: N = {N} x {L} mel frames ({n} samples, {-(-n * 10000 // FS)} at 10 kHz), {ITERS} + {ITERS} iterations")
    print(f"mean ESTOI of the vocoded clips: (a) {sa.mean():.4f}  (b) {sb.mean():.4f}")
    abtime.report(variants, tt, ratio="the first")
    print(f"whole span of (b) below the whole span of (a): {abtime.wholly_under(tt[1], tt[0])}")
    power = torch.rand(N, 513, L, device="cuda", generator=g.manual_seed(2)) ** 4 * 3.0
    ang = torch.rand(N, 513, L, 2, device="cuda", generator=g.manual_seed(3))
    gl = [("(c) l2s_griffin_lim alone, this build", griffin_lim_call(native.lib(), power, ang))]
    gl += [(f"(c) l2s_griffin_lim alone, {name}", griffin_lim_call(lib, power, ang)) for name, lib in alts]
    tt, waves = abtime.rounds(gl, ROUNDS, REPS, clock="host")          # waves: each build's own buffer, which every call of it rewrites
    for (name, _), wave in zip(gl[1:], waves[1:]):
        print(f"{name}: waveform bit-identical to this build's: {torch.equal(wave, waves[0])}")
    abtime.report(gl, tt, ratio="the first")


def main():
    alts = abtime.libs_from_env("ALT_LIBS", native._load)
    print(f"{ROUNDS} interleaved rounds, wall clock around synchronised calls ((a) 1 call, the others {REPS}); median of the rounds, span = min .. max"
          + (f"; ALT_LIBS = {', '.join(n for n, _ in alts)}" if alts else "; ALT_LIBS not given: this build only"))
    for w in WORKLOADS:
        workload(*w, alts)


if __name__ == "__main__":
    main()
