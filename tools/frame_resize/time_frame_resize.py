"""What the device-side face crops cost (include/l2s.h `l2s_resize_normalise`, frame_resize.hip) - a data-boundary transform, NOT on the mel-frames/s path:
  (a) the new call at IDENTITY size (96 x 96 frames, whole-image rectangles) against `l2s_normalise_pad_frames` on the same frames, which moves the same
      bytes - from this build and, with `ALT_LIB=<path to a build of the parent commit>`, from that build in the same process;
  (b) the new mouth + face calls on B clips of T faces against today's route written with device tensors: per face `F.interpolate` of the lower half, round,
      `/ 255`, mean / std, written into the zero-padded `(B,3,T,96,96)` batch, plus the two 160 x 160 face crops per clip;
  (c) the bytes the calls of (b) must move (rectangles read once, outputs written once) over their time, against the 8 TB/s peak.
Workloads: 16 clips x 75 faces of 130 x 130 (GRID-like) and 32 x 29 of 96 x 96.  The uploads are outside the timed region on both sides.  The native calls are
timed through ctypes with the job table built once (`native.resize_normalise` builds it per call in Python: listed separately).  ROUNDS interleaved rounds of
REPS warm calls each, the variants rotating inside a round, HIP events around the REPS calls; per variant the median of the rounds and the spread.
`SHAPES=BxTxS[,BxTxS...]`: other workloads of B clips x T faces of S x S; `ROUNDS=`, `REPS=`.
-> profiles/frame_resize_times.txt (stdout)"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.nn.functional as F

from lip2speech_amd import native
from lip2speech_amd.datasets import PackedFaces, PackedFrames
from tools import abtime

REPS = int(os.environ.get("REPS", 20))
ROUNDS = int(os.environ.get("ROUNDS", 7))
WORKLOADS = (("GRID-like", 16, 75, 130), ("LRW-like", 32, 29, 96))
if os.environ.get("SHAPES"):
    WORKLOADS = [(s, *(int(v) for v in s.split("x"))) for s in os.environ["SHAPES"].split(",")]
PEAK = 8e12


def resize_call(buf, jobs, mode, B, T, size):
    """`l2s_resize_normalise` through ctypes, the table built once"""
    L = native.lib()
    arr, n = native._resize_jobs(jobs), len(jobs)
    shape = (B, 2, 3, size, size) if mode == native.RESIZE_FACE else (B, 3, T, size, size)

    def call():
        out = torch.empty(shape, device="cuda")
        native.check(L.l2s_resize_normalise(buf.data_ptr(), buf.numel(), arr, n, mode, B, T, size, size, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return out
    return call


def pad_call(L, buf, offsets, frames, T):
    """`l2s_normalise_pad_frames` of library L through ctypes"""
    B = len(frames)
    off, fr = (ctypes.c_int64 * B)(*offsets), (ctypes.c_int32 * B)(*frames)

    def call():
        out = torch.empty(B, 3, T, 96, 96, device="cuda")
        native.check(L.l2s_normalise_pad_frames(buf.data_ptr(), off, fr, B, T, 96, 96, out.data_ptr(), torch.cuda.current_stream().cuda_stream), L)
        return out
    return call


def identity(title, B, T, alt):
    g = torch.Generator().manual_seed(B)
    clips = [torch.randint(0, 256, (T, 96, 96, 3), dtype=torch.uint8, generator=g) for _ in range(B)]
    pf = PackedFrames(clips, pin=False)
    buf = pf.data.cuda()
    jobs = [(pf.offsets[b] + t * 96 * 96 * 3, 96, 96, 0, 0, 96, 96, 0, b * T + t) for b in range(B) for t in range(T)]
    variants = [("(a) l2s_normalise_pad_frames, this build", pad_call(native.lib(), buf, pf.offsets, pf.frames, T)),
                ("(a) l2s_resize_normalise at identity size", resize_call(buf, jobs, native.RESIZE_MOUTH, B, T, 96))]
    if alt is not None:
        variants.append(("(a) l2s_normalise_pad_frames, ALT_LIB (the parent commit's build)", pad_call(alt, buf, pf.offsets, pf.frames, T)))
    t, outs = abtime.rounds(variants, ROUNDS, REPS)
    moved = B * T * 96 * 96 * 3 * (1 + 4)
    print(f"\n== identity, {title}: B = {B} x {T} frames of 96 x 96; {moved / 1e6:.1f} MB read + written; {-(-B * T // native.RESIZE_JOBS_PER_LAUNCH)} launches "
          f"against {-(-B // 64)}; bit-identical outputs: {all(torch.equal(outs[0], o) for o in outs[1:])}")
    abtime.report(variants, t, unit="us", ratio="the first", extra=lambda name, m: f"   {moved / m / 1e9:7.2f} TB/s = {moved / m * 1e3 / PEAK * 100:5.1f} % of 8 TB/s")


def torch_route(faces, idx, B, T, mean, std):
    """today's route on the device: per face interpolate + round + normalise, the collate's zero padding, the two face crops per clip"""
    video = torch.zeros(B, T, 3, 96, 96, device="cuda")
    crops = torch.empty(B, 2, 3, 160, 160, device="cuda")
    for b in range(B):
        for t, f in enumerate(faces[b]):
            u = F.interpolate(f[None, :, f.shape[1] // 2:].float(), size=(96, 96), mode="bilinear", align_corners=False)[0].round().clamp(0, 255)
            video[b, t] = (u / 255.0 - mean) / std
        for k, i in enumerate(idx[b]):
            u = F.interpolate(faces[b][i][None].float(), size=(160, 160), mode="bilinear", align_corners=False)[0].round().clamp(0, 255)
            crops[b, k] = (u - 127.5) / 128.0
    return video.permute(0, 2, 1, 3, 4), crops


def crops_workload(title, B, T, S):
    g = torch.Generator().manual_seed(B + S)
    faces_cpu = [[torch.randint(0, 256, (3, S, S), dtype=torch.uint8, generator=g) for _ in range(T)] for _ in range(B)]
    idx = [(0, T - 1)] * B
    packed = PackedFaces([(f, False, i) for f, i in zip(faces_cpu, idx)], pin=False)
    buf = packed.data.cuda()
    faces = [[f.cuda() for f in clip] for clip in faces_cpu]
    mean, std = torch.tensor((0.485, 0.456, 0.406), device="cuda").view(3, 1, 1), torch.tensor((0.229, 0.224, 0.225), device="cuda").view(3, 1, 1)
    mouth, face = resize_call(buf, packed.mouth_jobs(T), native.RESIZE_MOUTH, B, T, 96), resize_call(buf, packed.face_jobs, native.RESIZE_FACE, B, 2, 160)
    variants = [("(b) torch on the device: per-face interpolate + normalise + pad", lambda: torch_route(faces, idx, B, T, mean, std)),
                ("(b) l2s_resize_normalise, mouth + face calls (table built once)", lambda: (mouth(), face())),
                ("(b) native.resize_normalise x 2 (tables built per call in Python)",
                 lambda: (native.resize_normalise(buf, packed.mouth_jobs(T), native.RESIZE_MOUTH, B, T), native.resize_normalise(buf, packed.face_jobs, native.RESIZE_FACE, B))),
                ("    the mouth call alone", mouth), ("    the face call alone", face)]
    t, outs = abtime.rounds(variants, ROUNDS, REPS)
    diff = [float((a - b).abs().max()) for a, b in zip(outs[0], outs[1])]
    read = B * T * (S - S // 2) * S * 3 + B * 2 * S * S * 3
    moved = read + (B * T * 3 * 96 * 96 + B * 2 * 3 * 160 * 160) * 4
    print(f"\n== crops, {title}: B = {B} x {T} faces of {S} x {S}; {buf.numel() / 1e6:.1f} MB uploaded, {moved / 1e6:.1f} MB read + written by the two calls; "
          f"max |d| against the torch route: video {diff[0]:.3e}, face crops {diff[1]:.3e} (one LSB is {1 / 255 / 0.225:.3e} / {1 / 128:.3e})")
    abtime.report(variants, t, unit="us", ratio="the first",
                  extra=lambda name, m: f"   (c) {moved / m / 1e9:7.2f} TB/s = {moved / m * 1e3 / PEAK * 100:5.1f} % of 8 TB/s" if "l2s_resize" in name else "")


def main():
    alt_name, alt = next(iter(abtime.libs_from_env("ALT_LIB", native._load)), (None, None))
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min"
          + (f"; ALT_LIB = {alt_name}" if alt else "; ALT_LIB not given: this build only (encoder_kernels.hip, which holds normalise_pad_kernel, is the parent commit's)"))
    for title, B, T, S in WORKLOADS:
        identity(title, B, T, alt)
    for w in WORKLOADS:
        crops_workload(*w)
    print("\n(c) is listed on the two-call row of each crops workload: the bytes the algorithm must move / the calls' time, against the 8 TB/s peak.")


if __name__ == "__main__":
    main()
