"""Face alignment, host side (no GPU).  `warp_affine_u8` (vectorised numpy) equals, to the byte, the scalar per-pixel restatement of the transform that lives in
this file, and both satisfy closed forms that depend on neither; the eye angle and the inverse map; the reference's `datasets.align_and_crop_face` name;
`l2s_align_check` refuses every limit it documents with a message that names the job; `PackedFaces` keeps today's tables for 3-tuple items and builds
`align_jobs` for items that come with landmarks."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((16, 16), (33, 16), (37, 29))
ANGLES = (0.0, 0.9, -0.9, 7.3, -12.0, 45.0, 90.0)


def _rn(v: float) -> int:
    """float64 to the nearest integer, ties to even: Python's round() on a float"""
    return int(round(v))


def scalar_warp(img, m):
    """The transform, one pixel at a time in plain Python: the four rn in float64, everything after them in integers."""
    H, W, C = img.shape
    out = np.zeros_like(img)

    def s(yy, xx, c):
        return int(img[yy, xx, c]) if 0 <= yy < H and 0 <= xx < W else 0

    for y in range(H):
        X0 = _rn((m[1] * y + m[2]) * 1024) + 16
        Y0 = _rn((m[4] * y + m[5]) * 1024) + 16
        for x in range(W):
            ad, bd = _rn(m[0] * x * 1024), _rn(m[3] * x * 1024)
            X, Y = (X0 + ad) >> 5, (Y0 + bd) >> 5
            sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
            w00, w01, w10, w11 = 32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy
            assert w00 + w01 + w10 + w11 == 32768
            for c in range(C):
                out[y, x, c] = (w00 * s(sy, sx, c) + w01 * s(sy, sx + 1, c) + w10 * s(sy + 1, sx, c) + w11 * s(sy + 1, sx + 1, c) + 16384) >> 15
    return out


def _image(h, w, seed=0):
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _landmarks(eye1, eye2):
    """68 integer points whose eye boxes have the given mid points (a 3 x 3 box around each)"""
    lm = np.zeros((68, 2), dtype=np.int32)
    for sl, (mx, my) in ((slice(36, 42), eye1), (slice(42, 48), eye2)):
        lm[sl] = [(mx - 1, my - 1), (mx + 1, my - 1), (mx + 1, my + 1), (mx - 1, my + 1), (mx, my), (mx, my)]
    return lm.tolist()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_vectorised_warp_equals_the_scalar_restatement(size):
    from lip2speech_amd.datasets.face_utils import rotation_inverse_map, warp_affine_u8
    img = _image(*size)
    for angle in ANGLES:
        m = rotation_inverse_map(angle, *size)
        assert np.array_equal(warp_affine_u8(img, m), scalar_warp(img, m)), f"angle {angle}"


@pytest.mark.parametrize("warp", ("vectorised", "scalar"))
def test_closed_forms(warp):
    from lip2speech_amd.datasets import face_utils as fu
    f = fu.warp_affine_u8 if warp == "vectorised" else scalar_warp
    for h, w in ((16, 16), (33, 16), (37, 29)):
        img = _image(h, w, 1)
        assert np.array_equal(f(img, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), img)                       # identity copies
        assert np.array_equal(f(img, fu.rotation_inverse_map(0.0, h, w)), img)
        for dx, dy in ((3, 0), (0, -2), (-5, 4), (w, 0), (0, -h)):                                # integer shifts: zeros are shifted in
            want = np.zeros_like(img)
            ys, xs = np.arange(h) + dy, np.arange(w) + dx
            oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
            want[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
            assert np.array_equal(f(img, [1.0, 0.0, float(dx), 0.0, 1.0, float(dy)]), want), (dx, dy)
        wide = np.concatenate([img.astype(np.int64), np.zeros((h, 1, 3), np.int64)], axis=1)      # half a pixel: the tap past the last column is 0
        assert np.array_equal(f(img, [1.0, 0.0, 0.5, 0.0, 1.0, 0.0]), ((wide[:, :-1] + wide[:, 1:] + 1) >> 1).astype(np.uint8))
    for h, w in ((33, 17), (37, 29)):                                                             # 180 degrees on odd x odd reverses both axes
        img = _image(h, w, 2)
        assert np.array_equal(f(img, fu.rotation_inverse_map(180.0, h, w)), img[::-1, ::-1])
    for n in (17, 29):                                                                            # 90 degrees on an odd square
        img = _image(n, n, 3)
        assert np.array_equal(f(img, fu.rotation_inverse_map(90.0, n, n)), np.rot90(img, 1))


def test_eye_angle_and_inverse_map():
    from lip2speech_amd.datasets.face_utils import eye_angle_degrees, rotation_inverse_map
    assert eye_angle_degrees(_landmarks((30, 40), (70, 40))) == 0.0                               # level eyes
    assert eye_angle_degrees(_landmarks((30, 40), (30, 60))) == 0.0                               # dx == 0
    assert eye_angle_degrees(_landmarks((10, 10), (20, 20))) == pytest.approx(45.0, abs=1e-12)
    assert eye_angle_degrees(_landmarks((10, 10), (20, 20))) == float(np.arctan(10 / 10) * 180 / np.pi)
    assert eye_angle_degrees(_landmarks((10, 20), (20, 10))) == pytest.approx(-45.0, abs=1e-12)
    shifted = (np.asarray(_landmarks((31, 44), (75, 39))) + (-200, 1000)).tolist()                # only differences enter
    assert eye_angle_degrees(shifted) == eye_angle_degrees(_landmarks((31, 44), (75, 39))) == float(np.arctan(-5 / 44) * 180 / np.pi)
    # the box of cv2.boundingRect: x = min, w = max - min + 1, mid = x + w // 2
    lm = np.zeros((68, 2), dtype=np.int64)
    lm[36:42] = [(10, 10), (13, 10), (13, 11), (10, 11), (11, 10), (12, 11)]                      # box x 10 w 4 -> 12, y 10 h 2 -> 11
    lm[42:48] = [(20, 10), (24, 10), (24, 14), (20, 14), (22, 12), (22, 12)]                      # box x 20 w 5 -> 22, y 10 h 5 -> 12
    assert eye_angle_degrees(lm) == float(np.arctan(1 / 10) * 180 / np.pi)
    for h, w in ((16, 16), (33, 16), (700, 900)):
        assert rotation_inverse_map(0, h, w) == [1, 0, 0, 0, 1, 0]
    m = rotation_inverse_map(30.0, 40, 60)                                                        # the inverse of getRotationMatrix2D((30, 20), 30, 1)
    a, b = math.cos(math.pi / 6), math.sin(math.pi / 6)
    assert np.allclose(m, [a, -b, 30 - a * 30 + b * 20, b, a, 20 - b * 30 - a * 20], rtol=0, atol=1e-12)
    assert np.allclose([m[0] * 30 + m[1] * 20 + m[2], m[3] * 30 + m[4] * 20 + m[5]], [30, 20], rtol=0, atol=1e-12)      # the centre stays


def test_align_and_crop_face_is_the_reference_name():
    import datasets
    from lip2speech_amd.datasets import face_utils as fu
    assert datasets.align_and_crop_face is fu.align_and_crop_face
    frame = torch.from_numpy(_image(60, 80)).permute(2, 0, 1)
    lm = _landmarks((30, 20), (52, 25))
    face = datasets.align_and_crop_face(frame, (10, 5, 70, 50), lm)
    assert face.dtype == torch.uint8 and tuple(face.shape) == (3, 45, 60)
    crop = frame[:, 5:50, 10:70].permute(1, 2, 0).contiguous().numpy()
    want = fu.warp_affine_u8(crop, fu.rotation_inverse_map(fu.eye_angle_degrees(lm), 45, 60))
    assert np.array_equal(face.permute(1, 2, 0).numpy(), want) and not np.array_equal(want, crop)
    level = datasets.align_and_crop_face(frame, (10, 5, 70, 50), _landmarks((30, 20), (52, 20)))
    assert np.array_equal(level.permute(1, 2, 0).numpy(), crop)                                    # level eyes: the crop itself


def test_face_box_crops_is_the_loaders_loop():
    from lip2speech_amd.datasets import face_box_crops
    frames = torch.from_numpy(np.stack([_image(64, 96, k) for k in range(4)])).permute(0, 3, 1, 2)
    lm = [_landmarks((30, 20), (50, 22 + k)) for k in range(4)]
    coords = [(-3, 4, 40, 50), None, (10, -1, 90, 30), (5, 5, 25, 64)]
    crops, kept = face_box_crops(frames, coords, [lm[0], None, lm[2], lm[3]])
    assert [tuple(c.shape) for c in crops] == [(3, 46, 40), (3, 30, 80), (3, 59, 20)] and kept == [lm[0], lm[2], lm[3]]
    assert torch.equal(crops[0], frames[0, :, 4:50, 0:40]) and torch.equal(crops[1], frames[2, :, 0:30, 10:90])      # negative coordinates clamp to 0
    assert face_box_crops(frames, [(0, 0, 15, 40)] + coords[1:], lm) is None                        # a face under 16 x 16: the item is unusable
    assert face_box_crops(frames, [(0, 0, 40, 15)] + coords[1:], lm) is None
    assert face_box_crops(frames, [None] * 4, [None] * 4) is None                                   # no face at all


# ---------------------------------------------------------------- the C ABI

@pytest.fixture(scope="module")
def L():
    from lip2speech_amd import native
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lip2speech_amd", "csrc"), "-j", "8"], check=True)
    return native.lib()


def test_symbols_declared_exported_bound(L):
    from lip2speech_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l2s.h")).read(), flags=re.S)
    for sym in ("l2s_align_check", "l2s_align_faces"):
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} not declared in include/l2s.h"
        assert sym in native.ABI_SYMBOLS and hasattr(L, sym) and getattr(L, sym).argtypes is not None
    assert L.l2s_abi_version() == 2                      # the change only adds symbols
    assert int(re.search(r"#define\s+L2S_ALIGN_JOBS_PER_LAUNCH\s+(\d+)", header).group(1)) == native.ALIGN_JOBS_PER_LAUNCH
    assert ctypes.sizeof(native.AlignJob) == 64 and native.ALIGN_JOBS_PER_LAUNCH * 64 <= 3840
    assert re.search(r"typedef struct l2s_align_job \{\s*int64_t offset;\s*int32_t H, W;\s*double m\[6\];\s*\}", header)
    assert [f[0] for f in native.AlignJob._fields_] == ["offset", "H", "W", "m"]


IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
BYTES = 2 * 3600                                          # two 40 x 30 images


def _job(offset=0, H=40, W=30, m=IDENT):
    return (offset, H, W) + tuple(m)


def _check(L, jobs, packed_bytes=BYTES):
    from lip2speech_amd import native
    return L.l2s_align_check(native._align_jobs(jobs), len(jobs), packed_bytes)


def test_check_accepts_and_names_the_job_it_refuses(L):
    from lip2speech_amd import native
    from lip2speech_amd.datasets.face_utils import rotation_inverse_map
    good = _job()
    assert _check(L, [good, _job(offset=3600)]) == 0
    assert _check(L, []) == 0
    assert _check(L, [_job(H=4096, W=4096)], packed_bytes=4096 * 4096 * 3) == 0
    assert _check(L, [_job(m=rotation_inverse_map(a, 40, 30)) for a in (45.0,)] + [_job(offset=3600, m=rotation_inverse_map(-173.0, 40, 30))]) == 0
    assert _check(L, [_job(H=5, W=5), _job(offset=76, H=5, W=5)], packed_bytes=151) == 0           # 75 bytes round up to 76; the buffer may end with the image
    assert _check(L, [_job(m=(1.0, 0.0, 16384.0 - 29, 0.0, 1.0, -16384.0))]) == 0                  # the corners may touch the limit
    inf, nan = float("inf"), float("nan")
    for bad, names in ((_job(offset=3602), b"offset 3602 is not"),
                       (_job(offset=-4), b"offset -4 is not"),
                       (_job(offset=3604), b"image bytes [3604, 7204) lie outside the packed buffer of 7200 bytes"),
                       (_job(offset=3600, H=0), b"image 0 x 30 is outside [1, 4096]"),
                       (_job(offset=3600, W=4097), b"image 40 x 4097 is outside [1, 4096]"),
                       (_job(offset=3600, H=-1), b"image -1 x 30 is outside"),
                       (_job(offset=3600, m=(1.0, 0.0, nan, 0.0, 1.0, 0.0)), b"m[2] is not finite"),
                       (_job(offset=3600, m=(1.0, 0.0, 0.0, 0.0, inf, 0.0)), b"m[4] is not finite"),
                       (_job(offset=3600, m=(1.0, 0.0, 0.0, -inf, 1.0, 0.0)), b"m[3] is not finite"),
                       (_job(offset=3600, m=(1.0, 0.0, 16384.0 - 28, 0.0, 1.0, 0.0)), b"output corner (29, 0)"),
                       (_job(offset=3600, m=(1.0, 0.0, 0.0, 0.0, 1.0, -16385.0)), b"output corner (0, 0)"),
                       (_job(offset=3600, m=(1.0, 0.0, 0.0, 0.0, 500.0, 0.0)), b"output corner (0, 39)"),
                       (_job(offset=3600, m=(1e300, 0.0, 0.0, 0.0, 1.0, 0.0)), b"outside [-16384, 16384]")):
        assert _check(L, [good, bad]) == 1
        err = L.l2s_last_error()
        assert b"job 1:" in err and names in err, err
        with pytest.raises(RuntimeError, match="job 1"):
            native.align_check([good, bad], BYTES)
    # two jobs whose spans, rounded up to 4 bytes, overlap: the same image twice, and a 5 x 5 image's pad byte
    assert _check(L, [good, _job(offset=3600), _job(offset=3600)]) == 1
    assert b"job 2:" in L.l2s_last_error() and b"overlap the span of job 1" in L.l2s_last_error()
    assert _check(L, [_job(offset=1800, H=20), good]) == 1
    assert b"job 1:" in L.l2s_last_error() and b"overlap the span of job 0, [1800, 3600)" in L.l2s_last_error()
    assert _check(L, [_job(H=5, W=5), _job(offset=76, H=5, W=5)], packed_bytes=200) == 0
    native.align_check([good], BYTES)


def test_align_faces_refuses_a_bad_call_before_the_device(L):
    """null and misaligned pointers, overlapping buffers, a bad table: refused on the host, nothing is launched (no GPU here)"""
    from lip2speech_amd import native
    jobs = native._align_jobs([_job()])
    assert L.l2s_align_faces(0x1000, BYTES, native._align_jobs([_job(offset=2)]), 1, 0x100000, None) == 1 and b"job 0: offset 2" in L.l2s_last_error()
    assert L.l2s_align_faces(None, BYTES, jobs, 1, 0x100000, None) == 1 and b"null buffer" in L.l2s_last_error()
    assert L.l2s_align_faces(0x1000, BYTES, jobs, 1, None, None) == 1 and b"null buffer" in L.l2s_last_error()
    assert L.l2s_align_faces(0x1002, BYTES, jobs, 1, 0x100000, None) == 1 and b"4-byte aligned" in L.l2s_last_error()
    assert L.l2s_align_faces(0x1000, BYTES, jobs, 1, 0x100001, None) == 1 and b"4-byte aligned" in L.l2s_last_error()
    for out in (0x100000, 0x100000 + BYTES - 4, 0x100000 - BYTES + 4):
        assert L.l2s_align_faces(0x100000, BYTES, jobs, 1, out, None) == 1 and b"overlap" in L.l2s_last_error()
    assert L.l2s_align_faces(None, 0, jobs, 0, None, None) == 0                                     # no job: nothing to do


# ---------------------------------------------------------------- PackedFaces

def _items():
    g = torch.Generator().manual_seed(5)
    sizes = [[(16, 16), (33, 16), (37, 29)], [(40, 35), (21, 50), (16, 19), (64, 48)]]
    faces = [[torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g) for h, w in clip] for clip in sizes]
    lms = [[_landmarks((10, 10), (30, 10 + 2 * t - 3 * b)) for t in range(len(clip))] for b, clip in enumerate(sizes)]
    return faces, lms, [False, True], [(0, 2), (3, 1)]


def test_packed_faces_keeps_its_tables_and_adds_align_jobs():
    from lip2speech_amd import native
    from lip2speech_amd.datasets import PackedFaces
    from lip2speech_amd.datasets.face_utils import eye_angle_degrees, rotation_inverse_map
    faces, lms, flips, idx = _items()
    three = PackedFaces([(f, fl, i) for f, fl, i in zip(faces, flips, idx)], pin=False)
    four = PackedFaces([(f, fl, i, lm) for f, fl, i, lm in zip(faces, flips, idx, lms)], pin=False)
    # 3-tuples: the tables as they were - offsets on 4-byte boundaries in item order, lower halves to mouth slots, drawn faces whole to face slots
    assert three.align_jobs == []
    offs, total = [], 0
    for clip in faces:
        for f in clip:
            offs.append(total)
            total += (f.numel() + 3) // 4 * 4
    dims = [(int(f.shape[1]), int(f.shape[2])) for clip in faces for f in clip]
    assert three.images == [(o, h, w) for o, (h, w) in zip(offs, dims)] and three.data.numel() == total
    assert three.mouth_jobs() == [(o, h, w, h // 2, 0, h - h // 2, w, b, b * 4 + t)
                                  for (o, (h, w)), (b, t) in zip(zip(offs, dims), [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (1, 3)])]
    assert three.face_jobs == [(offs[0], 16, 16, 0, 0, 16, 16, 0, 0), (offs[2], 37, 29, 0, 0, 37, 29, 0, 1),
                               (offs[6], 64, 48, 0, 0, 64, 48, 1, 2), (offs[4], 21, 50, 0, 0, 21, 50, 1, 3)]
    # 4-tuples: the same bytes and tables, plus one align job per image with the map of its landmarks
    assert torch.equal(four.data, three.data) and four.images == three.images and four.frames == three.frames
    assert four.mouth_jobs() == three.mouth_jobs() and four.face_jobs == three.face_jobs
    flat = [lm for clip in lms for lm in clip]
    assert four.align_jobs == [(o, h, w) + tuple(rotation_inverse_map(eye_angle_degrees(lm), h, w)) for (o, h, w), lm in zip(three.images, flat)]
    assert len({j[3:] for j in four.align_jobs}) > 3                                               # the items do carry different angles
    native.align_check(four.align_jobs, four.data.numel())
    # a batch may mix both kinds of item: only the images that came with landmarks are named
    mixed = PackedFaces([(faces[0], False, idx[0]), (faces[1], True, idx[1], lms[1])], pin=False)
    assert mixed.align_jobs == four.align_jobs[3:] and mixed.mouth_jobs() == three.mouth_jobs()


def test_collate_passes_items_with_landmarks_through():
    from lip2speech_amd.datasets import device_collate_fn_pad_faces
    faces, lms, flips, idx = _items()
    speech = [torch.zeros(1, 600), torch.zeros(1, 900)]
    batch = [((f, fl, i, lm), s, None, None) for f, fl, i, lm, s in zip(faces, flips, idx, lms, speech)]
    (packed, lengths), audio, audio2, packed2 = device_collate_fn_pad_faces(batch)
    assert packed is packed2 and audio is audio2 and lengths.tolist() == [3, 4] and len(packed.align_jobs) == 7
