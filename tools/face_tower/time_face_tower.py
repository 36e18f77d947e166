"""Time the face speaker tower (l2s_face_encoder_fwd, face_tower.hip) at B = 1, 8, 32 faces of 160 x 160, HIP events around warm calls, and
torch-ROCm's own fp32 F.conv2d chain on the same weights (the CPU-side restatement tests/face_tower_torch.py, run on the device) as the
yardstick.  TFLOP/s counts the executed FLOPs of the layer table (2 x MAC of every conv + the tail's Linears); "frac" = that rate over
the split-bf16 pipe's fp32-equivalent ceiling (2.5 PFLOP/s bf16 dense / 6 products = 416.7 TFLOP/s).
`SIZES=1,8,32` the batch sizes, `REPS=`, `YARDSTICK=0` the HIP tower only.
-> profiles/face_tower_times.txt (stdout only; tools/face_tower/profile_face_tower.sh runs it under rocprofv3 for the per-kernel breakdown)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import face_tower_torch as ft
from lip2speech_amd import synth
from model.modules import FaceRecognizer
from tools import abtime

REPS = int(os.environ.get("REPS", 20))
SIZES = [int(b) for b in os.environ.get("SIZES", "1,8,32").split(",")]
YARDSTICK = os.environ.get("YARDSTICK", "1") != "0"       # 0: the HIP tower only (profile_face_tower.sh traces its kernels alone)
X3_CEIL = 416.7e12


def macs_per_face():
    """MACs of the convolutions (from the restatement's modules at 160 x 160) and of the tail's Linears."""
    tower = ft.FaceTower().eval()
    conv = [0]

    def hook(mod, inp, out):
        conv[0] += out.numel() * mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1] // out.shape[0]

    hs = [m.register_forward_hook(hook) for m in tower.modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        tower(torch.zeros(1, 3, 160, 160))
    for h in hs:
        h.remove()
    return conv[0], 1792 * 512 + 512 * 512 + 512 * 256


def main():
    sd = synth.synth_face_state_dict()
    fr = FaceRecognizer()
    fr.load_state_dict({k[len("vgg_face."):]: v for k, v in sd.items()}, strict=True)
    fr = fr.cuda()
    nm = fr.native_model()
    tower = ft.load_tower(sd).cuda()
    conv_mac, tail_mac = macs_per_face()
    flop = 2 * (conv_mac + tail_mac)
    print(f"face tower: {conv_mac / 1e9:.3f} GMAC of convolution + {tail_mac / 1e6:.2f} M MAC of Linears per 160 x 160 face = {flop / 1e9:.2f} GFLOP; "
          f"{REPS} warm calls per size, HIP events")
    print(f"{'B':>4} {'HIP ms':>9} {'TFLOP/s':>8} {'frac':>6} {'torch fp32 ms':>14} {'speed-up':>9} {'max|d emb|':>11}")
    for B in SIZES:
        crops = synth.synth_faces(B).cuda()
        x = crops[:, 0]
        ms = abtime.timed(lambda: nm.face_encoder_fwd(x), REPS, warm=3)
        if not YARDSTICK:
            print(f"{B:4d} {ms:9.3f}")
            continue
        with torch.no_grad():
            ms_t = abtime.timed(lambda: tower.inference(x), REPS, warm=3)
            d = (nm.face_encoder_fwd(x) - tower.inference(x)).abs().max().item()
        tf = B * flop / (ms * 1e-3) / 1e12
        print(f"{B:4d} {ms:9.3f} {tf:8.1f} {tf * 1e12 / X3_CEIL:6.3f} {ms_t:14.3f} {ms_t / ms:9.2f} {d:11.2e}")


if __name__ == "__main__":
    main()
