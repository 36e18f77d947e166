"""What the device-side mel targets cost (include/l2s.h `l2s_mel_targets`, mel_targets.hip) - a data-boundary transform, NOT on the mel-frames/s path:
  (a) `MelSpectrogram(backend="torch")` on the device (rocFFT `torch.stft`, the dense 513 x 80 matmul, the elementwise launches) followed by the padding the
      host collate `_pad_audio_mels` does, written with device tensors (audio / mels / gate filled row by row);
  (b) ONE `native.mel_targets` call on the same waveforms packed back to back;
  (c) with `ALT_LIB=<path to another build of this library>` (e.g. `-DMT_WAVES=8`: eight frames per block instead of four): (b) from that build, in the same
      process - the waves-per-block A/B.
Shapes: B = 32 x 18 560 samples (LRW's clips) and B = 16 x 48 000 (GRID's 3 s).  The uploads are outside the timed region on both sides (the bytes are the same).
ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the REPS calls; per variant the median of the
rounds and the spread.  `SHAPES=Bxn[,Bxn...]`: other workloads of B clips x n samples; `ROUNDS=`, `REPS=`.
-> profiles/mel_targets_times.txt (stdout)"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native
from lip2speech_amd.datasets import MEL_PAD, MelSpectrogram, PackedAudio
from tools import abtime

REPS = int(os.environ.get("REPS", 20))
ROUNDS = int(os.environ.get("ROUNDS", 7))
WORKLOADS = (("LRW", 32, 18560), ("GRID, 3 s", 16, 48000))
if os.environ.get("SHAPES"):
    WORKLOADS = [(s, *(int(v) for v in s.split("x"))) for s in os.environ["SHAPES"].split(",")]


def torch_route(mt, waves):
    """the torch transform per item, then `_pad_audio_mels` on the device"""
    mels = [mt(w)[0] for w in waves]
    n, a_max, m_max = len(waves), max(w.shape[1] for w in waves), max(m.shape[1] for m in mels)
    audio = torch.zeros(n, a_max, device="cuda")
    out = torch.full((n, 80, m_max), MEL_PAD, device="cuda")
    gate = torch.zeros(n, m_max, device="cuda")
    for i, (w, m) in enumerate(zip(waves, mels)):
        audio[i, :w.shape[1]] = w[0]
        out[i, :, :m.shape[1]] = m
        gate[i, m.shape[1] - 1:] = 1.0
    return audio, out, gate


def torch_route_batched(mt, batch):
    """the same for equal-length clips as ONE batched transform (the cheapest form the torch path has; no padding left to do but the gate)"""
    mels = mt(batch)
    gate = torch.zeros(batch.shape[0], mels.shape[2], device="cuda")
    gate[:, -1] = 1.0
    return batch, mels, gate


def hip_call(L, buf, off, ns, fb, fb_nnz):
    """`native.mel_targets` on library L (the package's own, or ALT_LIB's)"""
    B, M, A = len(ns), max(ns) // 256 + 1, max(ns)
    ws = torch.empty(int(L.l2s_mel_targets_workspace_bytes(B, 80)), dtype=torch.uint8, device="cuda")
    offs, nss = (ctypes.c_int64 * B)(*off), (ctypes.c_int64 * B)(*ns)

    def call():
        mels = torch.empty(B, 80, M, device="cuda")
        gate = torch.empty(B, M, device="cuda")
        audio = torch.empty(B, A, device="cuda")
        lengths = torch.empty(B, dtype=torch.int64, device="cuda")
        native.check(L.l2s_mel_targets(buf.data_ptr(), offs, nss, B, fb.data_ptr(), fb_nnz, 80, 1024, 256, 1, MEL_PAD, M, A, mels.data_ptr(), gate.data_ptr(),
                                       audio.data_ptr(), lengths.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), L)
        return audio, mels, gate
    return call


def workload(title, B, n, alt):
    g = torch.Generator().manual_seed(B)
    waves_cpu = [0.1 * torch.randn(1, n, generator=g) for _ in range(B)]
    waves = [w.cuda() for w in waves_cpu]
    batch = torch.cat(waves, dim=0)
    packed = PackedAudio(waves_cpu, pin=False)
    buf = packed.data.cuda()
    mt = MelSpectrogram(backend="torch").cuda()
    variants = [("(a) torch on the device, per item + padding", lambda: torch_route(mt, waves)),
                ("(a') torch on the device, one batched transform", lambda: torch_route_batched(mt, batch)),
                ("(b) native.mel_targets, one call", lambda: native.mel_targets(buf, packed.offsets, packed.samples, mt.fb, mt.fb_nnz)),
                ("(b) the same through ctypes, this build", hip_call(native.lib(), buf, packed.offsets, packed.samples, mt.fb, mt.fb_nnz))]
    if alt is not None:
        variants.append(("(c) ALT_LIB build, one call", hip_call(alt, buf, packed.offsets, packed.samples, mt.fb, mt.fb_nnz)))
    t, outs = abtime.rounds(variants, ROUNDS, REPS)          # the warm-up call covers every route
    frames = B * (n // 256 + 1)
    print(f"\n== {title}: B = {B} x {n} samples, {frames} frames")
    print(f"(b) against (a): audio and gate identical: {torch.equal(outs[0][0], outs[2][2]) and torch.equal(outs[0][2], outs[2][1])}; "
          f"max |d log-mel| = {float((outs[0][1] - outs[2][0]).abs().max()):.3e}")
    if alt is not None:
        print(f"(c) against (b): log-mels bit-identical: {torch.equal(outs[4][1], outs[3][1])}")
    abtime.report(variants, t, unit="us", ratio="(a)", extra=lambda name, m: f"   {frames / m / 1e3:8.2f} M frames/s")


def main():
    alt_name, alt = next(iter(abtime.libs_from_env("ALT_LIB", native._load)), (None, None))
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min"
          + (f"; ALT_LIB = {alt_name}" if alt else "; ALT_LIB not given: this build only"))
    for w in WORKLOADS:
        workload(*w, alt)


if __name__ == "__main__":
    main()
