"""Writes tests/golden/jpeg_cases.npz: JPEG streams that Pillow encodes from seeded images, and the RGB pixels Pillow decodes from them - the fixture of
tests/test_jpeg_decode_host.py and tests/test_jpeg_decode_gpu.py, which therefore need no Pillow.  Pillow and numpy only; reads nothing but this repository.

    python tests/golden/make_jpeg_cases.py

For every case `<name>`: `s_<name>` the stream (uint8) and `p_<name>` the pixels (H, W, 3); `names` lists the cases.  Before the file is written the host
restatement (lip2speech_amd/datasets/jpeg.py) must equal Pillow on every case.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lip2speech_amd.datasets.jpeg import decode_jpeg_host  # noqa: E402

SIZES = [(1, 1), (2, 2), (8, 8), (16, 16), (17, 9), (9, 17), (24, 40), (33, 31), (96, 96), (146, 120)]
SUB = {"420": 2, "444": 0}      # Pillow's `subsampling`


def image(content: str, H: int, W: int, seed: int, grey: bool) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if content == "noise":          # FF 00 stuffing, 16-bit codes, saturated pixels
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    elif content == "ramp":         # EOB and ZRL runs
        y, x = np.mgrid[0:H, 0:W]
        img = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(H + W - 2, 1)], axis=-1).astype(np.uint8)
    else:                           # DC only
        img = np.empty((H, W, 3), dtype=np.uint8)
        img[:] = rng.integers(0, 256, size=3, dtype=np.uint8)
    return img[:, :, 0] if grey else img


def cases():
    """(name, content, H, W, mode "420" / "444" / "grey", save options)"""
    out = []
    for H, W in SIZES:
        out.append((f"noise_{H}x{W}_420_q75", "noise", H, W, "420", dict(quality=75)))
        out.append((f"ramp_{H}x{W}_420_q75", "ramp", H, W, "420", dict(quality=75)))
    for H, W in [(1, 1), (17, 9), (33, 31)]:
        out.append((f"const_{H}x{W}_420_q75", "const", H, W, "420", dict(quality=75)))
    for H, W in [(1, 1), (17, 9), (24, 40), (33, 31)]:
        out.append((f"noise_{H}x{W}_444_q75", "noise", H, W, "444", dict(quality=75)))
    out.append(("ramp_96x96_444_q75", "ramp", 96, 96, "444", dict(quality=75)))
    for H, W in [(1, 1), (9, 17), (33, 31)]:
        out.append((f"noise_{H}x{W}_grey_q75", "noise", H, W, "grey", dict(quality=75)))
    out.append(("ramp_24x40_grey_q75", "ramp", 24, 40, "grey", dict(quality=75)))
    out.append(("const_16x16_grey_q75", "const", 16, 16, "grey", dict(quality=75)))
    for q in (30, 95, 100):
        out.append((f"noise_33x31_420_q{q}", "noise", 33, 31, "420", dict(quality=q)))
        out.append((f"ramp_17x9_420_q{q}", "ramp", 17, 9, "420", dict(quality=q)))
    out.append(("noise_24x40_444_q100", "noise", 24, 40, "444", dict(quality=100)))
    out.append(("noise_9x17_grey_q30", "noise", 9, 17, "grey", dict(quality=30)))
    out.append(("noise_33x31_420_q75_opt", "noise", 33, 31, "420", dict(quality=75, optimize=True)))
    out.append(("ramp_96x96_420_q95_opt", "ramp", 96, 96, "420", dict(quality=95, optimize=True)))
    out.append(("noise_9x17_grey_q75_opt", "noise", 9, 17, "grey", dict(quality=75, optimize=True)))
    out.append(("noise_17x9_444_q100_opt", "noise", 17, 9, "444", dict(quality=100, optimize=True)))
    for nb in (1, 3):
        out.append((f"noise_33x31_420_q75_rb{nb}", "noise", 33, 31, "420", dict(quality=75, restart_marker_blocks=nb)))
        out.append((f"noise_17x9_444_q75_rb{nb}", "noise", 17, 9, "444", dict(quality=75, restart_marker_blocks=nb)))
        out.append((f"ramp_24x40_grey_q75_rb{nb}", "ramp", 24, 40, "grey", dict(quality=75, restart_marker_blocks=nb)))
    out.append(("noise_96x96_420_q75_rr1", "noise", 96, 96, "420", dict(quality=75, restart_marker_rows=1)))
    out.append(("ramp_146x120_420_q75_rr1", "ramp", 146, 120, "420", dict(quality=75, restart_marker_rows=1)))
    out.append(("noise_24x40_grey_q75_rr1", "noise", 24, 40, "grey", dict(quality=75, restart_marker_rows=1)))
    out.append(("noise_33x31_444_q95_rr1_opt", "noise", 33, 31, "444", dict(quality=95, restart_marker_rows=1, optimize=True)))
    return out


def main():
    arrays, names = {}, []
    for seed, (name, content, H, W, mode, opts) in enumerate(cases()):
        img = image(content, H, W, 1000 + seed, mode == "grey")
        buf = io.BytesIO()
        if mode == "grey":
            Image.fromarray(img, "L").save(buf, "JPEG", **opts)
        else:
            Image.fromarray(img, "RGB").save(buf, "JPEG", subsampling=SUB[mode], **opts)
        stream = buf.getvalue()
        pixels = np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))
        mine = decode_jpeg_host(stream)
        assert mine.shape == pixels.shape and np.array_equal(mine, pixels), f"{name}: the restatement differs from Pillow in {int((mine != pixels).sum())} values"
        names.append(name)
        arrays["s_" + name] = np.frombuffer(stream, dtype=np.uint8)
        arrays["p_" + name] = pixels
    path = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")
    np.savez_compressed(path, names=np.array(names), **arrays)
    print(f"{len(names)} cases, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
