"""What the device-side face alignment costs (include/l2s.h `l2s_align_faces`, face_align.hip) - a data-boundary transform, NOT on the mel-frames/s path:
  (a) `l2s_align_faces` alone on the packed face-box crops of a batch, eye angles uniform in +-15 degrees;
  (b) the two `l2s_resize_normalise` calls (mouth + face crops) alone, on the aligned buffer;
  (c) all three together: what `PackedFaces.to_device()` runs after the upload for items that came with landmarks;
  (d) the launches of (a), and the bytes it must move - every image read once and written once, 2 x packed_bytes - over its time, against the 8 TB/s peak.
No earlier code does this work on the device (the reference rotates each frame with OpenCV in the loader workers), so there is no yardstick to hold (a) against.
Workloads: 16 clips x 75 faces of 130 x 130 (GRID-like) and 32 x 29 of 96 x 96.  The upload is outside the timed region.  The native calls are timed through
ctypes with the job tables built once (`native.align_faces` builds its table per call in Python: listed separately).  ROUNDS interleaved rounds of REPS warm calls
each, the variants rotating inside a round, HIP events around the REPS calls; per variant the median of the rounds and the spread.
`SHAPES=BxTxS[,BxTxS...]`: other workloads of B clips x T faces of S x S; `ROUNDS=`, `REPS=`.
-> profiles/face_align_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from lip2speech_amd import native
from lip2speech_amd.datasets import PackedFaces
from lip2speech_amd.datasets.face_utils import rotation_inverse_map, warp_affine_u8
from tools import abtime

REPS = int(os.environ.get("REPS", 20))
ROUNDS = int(os.environ.get("ROUNDS", 7))
WORKLOADS = (("GRID-like", 16, 75, 130), ("LRW-like", 32, 29, 96))
if os.environ.get("SHAPES"):
    WORKLOADS = [(s, *(int(v) for v in s.split("x"))) for s in os.environ["SHAPES"].split(",")]
PEAK = 8e12


def align_call(buf, out, jobs):
    """`l2s_align_faces` through ctypes, the table built once"""
    L = native.lib()
    arr, n = native._align_jobs(jobs), len(jobs)
    return lambda: native.check(L.l2s_align_faces(buf.data_ptr(), buf.numel(), arr, n, out.data_ptr(), torch.cuda.current_stream().cuda_stream))


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


def workload(title, B, T, S):
    g = torch.Generator().manual_seed(B + S)
    faces = [[torch.randint(0, 256, (3, S, S), dtype=torch.uint8, generator=g) for _ in range(T)] for _ in range(B)]
    packed = PackedFaces([(f, False, (0, T - 1)) for f in faces], pin=False)
    angles = np.random.default_rng(B + S).uniform(-15.0, 15.0, len(packed.images))
    jobs = [(o, H, W) + tuple(rotation_inverse_map(a, H, W)) for (o, H, W), a in zip(packed.images, angles)]
    buf = packed.data.cuda()
    out = torch.zeros_like(buf)
    align = align_call(buf, out, jobs)
    mouth, face = resize_call(out, packed.mouth_jobs(T), native.RESIZE_MOUTH, B, T, 96), resize_call(out, packed.face_jobs, native.RESIZE_FACE, B, 2, 160)
    align()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    exact = all(np.array_equal(got[o:o + H * W * 3].reshape(H, W, 3), warp_affine_u8(packed.data[o:o + H * W * 3].numpy().reshape(H, W, 3), j[3:]))
                for (o, H, W), j in list(zip(packed.images, jobs))[::37])
    launches = -(-len(jobs) // native.ALIGN_JOBS_PER_LAUNCH)
    moved = 2 * buf.numel()
    print(f"\n== {title}: B = {B} x {T} faces of {S} x {S}, angles uniform in +-15 degrees; packed_bytes = {buf.numel() / 1e6:.1f} MB, {moved / 1e6:.1f} MB read + "
          f"written by the align call in {launches} launches ({native.ALIGN_JOBS_PER_LAUNCH} jobs each); every 37th image equals the host restatement to the bit: {exact}")
    variants = [("(a) l2s_align_faces alone (table built once)", align),
                ("(b) l2s_resize_normalise, mouth + face calls alone", lambda: (mouth(), face())),
                ("(c) all three: align, mouth, face", lambda: (align(), mouth(), face())),
                ("    native.align_faces (table built per call in Python)", lambda: native.align_faces(buf, jobs, out=out))]
    abtime.report(variants, abtime.rounds(variants, ROUNDS, REPS)[0], unit="us",
                  extra=lambda name, m: f"   (d) {moved / m / 1e9:7.2f} TB/s = {moved / m * 1e3 / PEAK * 100:5.1f} % of 8 TB/s" if name.startswith("(a)") else "")


def main():
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min")
    for w in WORKLOADS:
        workload(*w)
    print("\n(d) is listed on row (a): 2 x packed_bytes, the bytes the call must move, over its time, against the 8 TB/s peak.")


if __name__ == "__main__":
    main()
