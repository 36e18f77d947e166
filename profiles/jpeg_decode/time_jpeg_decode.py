"""What moving the JPEG decode of the loader frames onto the device costs and saves (include/l2s.h `l2s_jpeg_decode`, csrc/jpeg_decode.hip) - a data-boundary
transform, NOT on the mel-frames/s path of bench.py.  Per workload, from frames held in host memory to the model's normalised `(B,3,T,H,W)` input on the device:
  (a) host Pillow decode of every frame, then `PackedFrames(...)` and `.to_device()`: today's `raw_frames` route, the host decode included (one core);
  (b) `PackedFrames.to_device()` alone on frames already decoded and packed: the upload of the decoded bytes and `l2s_normalise_pad_frames`;
  (b') (b) with the packing of the decoded frames into the pinned buffer, the collate's share;
  (c) `PackedJpegFrames.to_device()` alone on strings already packed and planned: the upload of the COMPRESSED bytes, `l2s_jpeg_decode`, then the normalise;
  (c') (c) with the packing and `l2s_jpeg_plan`, the collate's share.
These are host clocks around work that ends in a device synchronise (the routes contain host work).  A second table takes the device side of (c) apart with HIP
events: the `l2s_jpeg_decode` call alone (tables built once, workspace allocated once) and `l2s_normalise_pad_frames` alone.
Workloads: `mouth` B = 32 x 29 frames of 96 x 96, the streams of tests/golden/sample_lrw repeated; `face` B = 16 x 75 frames of 146 x 120, the 146 x 120 streams of
tests/golden/jpeg_cases.npz (a ramp, a ramp with restart markers, uniform noise - the noise stream is several times the size of a real face's) repeated.
ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round; per variant the median of the rounds and the spread.
`WORKLOADS=mouth:BxT,face:BxT` for other sizes (the test suite runs `mouth:2x3,face:1x2`); `ROUNDS=`, `REPS=`.  Without Pillow (a) is left out, and said so.

Expectation, written down before the first run: (a) is dominated by the host decode, about 130 us per mouth frame and 180 us per face, so ~120 ms and ~215 ms
per batch; (b) moves 25.7 MB (mouth) over the host link and should take 1 - 2 ms; (c) moves 1.6 MB but its entropy launch is ONE wave per 64 images - 15 waves for
the mouth batch, each running ~2 500 dependent symbol iterations - so the decode call should take on the order of 1 ms and (c) should land near (b), far
below (a).  There is no speed gate on any of this.
-> profiles/jpeg_decode_times.txt (stdout)"""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from lip2speech_amd import native
from lip2speech_amd.datasets import PackedFrames, PackedJpegFrames
from lip2speech_amd.datasets.jpeg import decode_jpeg_host
from lip2speech_amd.datasets.lrw import load_jpeg_strings
from tools import abtime

REPS = int(os.environ.get("REPS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 7))
WORKLOADS = dict(w.split(":") for w in os.environ.get("WORKLOADS", "mouth:32x29,face:16x75").split(","))
GOLDEN = os.path.join(ROOT, "tests", "golden")

try:
    from PIL import Image
except ImportError:
    Image = None


def streams_of(kind):
    if kind == "mouth":
        files = sorted(f for f in os.listdir(os.path.join(GOLDEN, "sample_lrw")) if f.endswith("_mouth.npz"))
        return [s for f in files for s in load_jpeg_strings(os.path.join(GOLDEN, "sample_lrw", f))]
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    return [z["s_" + n].tobytes() for n in ("ramp_146x120_420_q75", "ramp_146x120_420_q75_rr1", "noise_146x120_420_q75", "ramp_146x120_420_q75")]


def pillow_decode(strings):
    return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in strings]))


def workload(kind, B, T):
    pool = streams_of(kind)
    clips = [[pool[(b * T + t) % len(pool)] for t in range(T)] for b in range(B)]
    pj = PackedJpegFrames(clips)
    decoded_pool = {id(s): torch.from_numpy(decode_jpeg_host(s)) for s in pool}      # the restatement: Pillow's bits, with or without Pillow
    decoded = [torch.stack([decoded_pool[id(s)] for s in c]) for c in clips]
    pf = PackedFrames(decoded)
    exact = torch.equal(pj.to_device(), pf.to_device()) and torch.equal(pj.decode().cpu(), pf.data)
    print(f"\n== {kind}: B = {B} x {T} frames of {pj.H} x {pj.W}; compressed {pj.data.numel() / 1e6:.2f} MB ({pj.data.numel() / pj.plan.n:.0f} bytes per frame, "
          f"{pj.plan.n_sets} table set(s)), decoded {pf.data.numel() / 1e6:.2f} MB; workspace {pj.plan.workspace_bytes() / 1e6:.1f} MB; "
          f"(c) and (b) equal to the bit: {exact}")
    variants = [("(b)  PackedFrames.to_device() on packed decoded frames", lambda: pf.to_device()),
                ("(b') PackedFrames(decoded) + to_device()", lambda: PackedFrames(decoded).to_device()),
                ("(c)  PackedJpegFrames.to_device() on packed, planned strings", lambda: pj.to_device()),
                ("(c') PackedJpegFrames(strings) + to_device()", lambda: PackedJpegFrames(clips).to_device())]
    if Image is not None:
        variants.insert(0, ("(a)  Pillow decode + PackedFrames + to_device()", lambda: PackedFrames([pillow_decode(c) for c in clips]).to_device()))
    else:
        print("Pillow is absent: (a) is left out")
    abtime.report(variants, abtime.rounds(variants, ROUNDS, REPS, clock="host")[0], ratio="(b)", base=1 if Image is not None else 0)
    # the device side of (c), HIP events
    dev = pj.data.cuda()
    out = torch.empty(pj.packed_bytes, dtype=torch.uint8, device="cuda")
    ws = torch.empty(pj.plan.workspace_bytes(), dtype=torch.uint8, device="cuda")
    offs, L, p = native._int64s(pj.image_offsets), native.lib(), pj.plan

    def decode():
        native.check(L.l2s_jpeg_decode(dev.data_ptr(), dev.numel(), p.images, p.n, p.sets, p.n_sets, offs, out.data_ptr(), out.numel(), None, ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream))
    parts = [("l2s_jpeg_decode alone (tables and workspace built once)", decode),
             ("l2s_normalise_pad_frames alone", lambda: native.normalise_pad_frames(out, pj.offsets, pj.frames, pj.H, pj.W))]
    abtime.report(parts, abtime.rounds(parts, ROUNDS, max(REPS, 1) * 4, clock="events")[0], unit="us",
                  extra=lambda name, m: f"   {m * 1e3 / p.n:6.2f} us per frame" if name.startswith("l2s_jpeg") else "")


def main():
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls; median of the rounds, spread = max - min.  First table: host clock around calls that end in a "
          f"synchronise; second table: HIP events")
    for kind, shape in WORKLOADS.items():
        B, T = (int(v) for v in shape.split("x"))
        workload(kind, B, T)


if __name__ == "__main__":
    main()
