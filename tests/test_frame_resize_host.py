"""Device-side face crops, host side (no GPU): the two C-ABI symbols are declared, exported and bound; `l2s_resize_check` refuses every limit it
documents with a message that names the job, and `l2s_resize_normalise` refuses a bad table before anything reaches the device; `PackedFaces` lays
the images out interleaved on 4-byte boundaries and builds the two job tables; `faces_item_host` is `face_recog_resize` plus the per-face formula of
the reference's loaders (datasets/grid/dataset.py:225-236); `LRW(raw_faces=True)` only swaps the face slot."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_lrw")
SYMBOLS = ("l2s_resize_check", "l2s_resize_normalise")
MOUTH, FACE = 0, 1


@pytest.fixture(scope="module")
def L():
    from lip2speech_amd import native
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lip2speech_amd", "csrc"), "-j", "8"], check=True)
    return native.lib()


def test_symbols_declared_exported_bound(L):
    from lip2speech_amd import native
    text = open(os.path.join(ROOT, "include", "l2s.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} not declared in include/l2s.h"
        assert sym in native.ABI_SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None, f"{sym} has no ctypes signature"
    assert L.l2s_abi_version() == 2                      # the change only adds symbols
    assert len(native.ABI_SYMBOLS) == len(set(native.ABI_SYMBOLS))
    # one set of constants on both sides of the binding
    assert int(re.search(r"#define\s+L2S_RESIZE_JOBS_PER_LAUNCH\s+(\d+)", header).group(1)) == native.RESIZE_JOBS_PER_LAUNCH
    assert re.search(r"L2S_RESIZE_MOUTH\s*=\s*0\s*,\s*L2S_RESIZE_FACE\s*=\s*1", header) and (native.RESIZE_MOUTH, native.RESIZE_FACE) == (0, 1)
    assert ctypes.sizeof(native.ResizeJob) == 40
    fields = re.search(r"typedef struct l2s_resize_job \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"\b(offset|H|W|y0|x0|h|w|flip|slot)\b", fields) == [f[0] for f in native.ResizeJob._fields_]


GOOD = (0, 40, 30, 20, 0, 20, 30, 0, 0)      # offset, H, W, y0, x0, h, w, flip, slot: the lower half of a 40 x 30 image
BYTES = 2 * 3600


def _job(**kw):
    j = dict(zip(("offset", "H", "W", "y0", "x0", "h", "w", "flip", "slot"), GOOD))
    j.update(kw)
    return tuple(j.values())


def _check(L, jobs, packed_bytes=BYTES, mode=MOUTH, B=1, T=2, size=96):
    from lip2speech_amd import native
    return L.l2s_resize_check(native._resize_jobs(jobs), len(jobs), packed_bytes, mode, B, T, size, size)


def test_check_accepts_and_names_the_job_it_refuses(L):
    second = _job(offset=3600, slot=1)
    assert _check(L, [GOOD, second]) == 0
    assert _check(L, []) == 0                                                         # no job: every slot is written as zeros
    assert _check(L, [_job(H=4096, W=4096, y0=0, h=4096, w=4096)], packed_bytes=4096 * 4096 * 3) == 0
    assert _check(L, [_job(y0=0, h=40), _job(y0=0, h=40, offset=3600, slot=1)], mode=FACE, size=160) == 0
    assert _check(L, [GOOD], size=88) == 0
    for bad, names in ((_job(offset=3602, slot=1), b"offset 3602 is not"),
                       (_job(offset=-4, slot=1), b"offset -4 is not"),
                       (_job(offset=3604, slot=1), b"image bytes [3604, 7204) lie outside the packed buffer of 7200 bytes"),
                       (_job(H=0, slot=1), b"image 0 x 30 is outside [1, 4096]"),
                       (_job(W=4097, slot=1), b"image 40 x 4097 is outside [1, 4096]"),
                       (_job(h=0, slot=1), b"rectangle 0 x 30 is empty"),
                       (_job(w=-1, slot=1), b"rectangle 20 x -1 is empty"),
                       (_job(y0=21, slot=1), b"rows [21, 41) columns [0, 30) lies outside its 40 x 30 image"),
                       (_job(x0=1, slot=1), b"columns [1, 31) lies outside"),
                       (_job(y0=-1, slot=1), b"rows [-1, 19)"),
                       (_job(flip=2, slot=1), b"flip = 2"),
                       (_job(slot=2), b"slot 2 is outside the output's 2 slots"),
                       (_job(slot=-1), b"slot -1 is outside"),
                       (_job(slot=0), b"slot 0 is already named by job 0")):
        assert _check(L, [GOOD, bad]) != 0, bad
        msg = L.l2s_last_error()
        assert b"job 1:" in msg and names in msg, (bad, msg)
    # a mode or an output size that is not built, and shapes without slots: refused whatever the table holds
    for kw, names in ((dict(mode=2), b"mode"), (dict(size=97), b"96 x 96 and 88 x 88"), (dict(mode=FACE, size=96), b"160 x 160"),
                      (dict(mode=FACE, size=160, T=3), b"T = 2"), (dict(B=0), b"B and T"), (dict(T=0), b"B and T"), (dict(B=1 << 20, T=1 << 10), b"2^24")):
        assert _check(L, [GOOD], **kw) != 0, kw
        assert names in L.l2s_last_error(), (kw, L.l2s_last_error())


def test_bad_table_is_refused_before_any_launch(L):
    """null device pointers: a call that got as far as a launch, or as reading the buffer, would not return an error code"""
    from lip2speech_amd import native
    for jobs, names in (([GOOD, _job(slot=0)], b"job 1: slot 0 is already named by job 0"), ([_job(offset=2)], b"job 0: offset 2"),
                        ([_job(H=5000)], b"job 0: image 5000 x 30")):
        assert L.l2s_resize_normalise(None, BYTES, native._resize_jobs(jobs), len(jobs), MOUTH, 1, 2, 96, 96, None, None) != 0
        assert names in L.l2s_last_error()
    assert L.l2s_resize_normalise(None, BYTES, native._resize_jobs([GOOD]), 1, 3, 1, 2, 96, 96, None, None) != 0 and b"mode" in L.l2s_last_error()
    assert L.l2s_resize_normalise(None, BYTES, native._resize_jobs([GOOD]), 1, MOUTH, 1, 2, 96, 96, None, None) != 0 and b"null buffer" in L.l2s_last_error()
    with pytest.raises(RuntimeError, match="job 0: slot 7 is outside"):
        native.resize_check([_job(slot=7)], BYTES, MOUTH, 1, 2, 96)


def _faces(seed=0, sizes=((33, 16), (40, 51), (21, 19))):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g) for H, W in sizes]


def test_packed_faces_layout_and_job_tables(L):
    from lip2speech_amd import native
    from lip2speech_amd.datasets import PackedFaces
    a, b = _faces(0), _faces(1, ((17, 23),))
    hwc = [f.permute(1, 2, 0).contiguous() for f in a]                       # the other accepted layout
    p = PackedFaces([(a, True, (2, 0)), (b, False, torch.tensor([0, 0]))], pin=False)
    q = PackedFaces([(hwc, True, (2, 0)), (b, False, (0, 0))], pin=False)
    # 33*16*3 = 1584 | 40*51*3 = 6120 | 21*19*3 = 1197 -> 1200 | 17*23*3 = 1173 -> 1176
    assert p.images == [(0, 33, 16), (1584, 40, 51), (7704, 21, 19), (8904, 17, 23)] and all(o % 4 == 0 for o, _, _ in p.images)
    assert p.data.dtype == torch.uint8 and p.data.numel() == 8904 + 1176 and torch.equal(p.data, q.data)
    for f, (o, H, W) in zip(a + b, p.images):
        assert torch.equal(p.data[o:o + H * W * 3].view(H, W, 3), f.permute(1, 2, 0))        # interleaved, verbatim
    assert p.data[7704 + 1197:8904].tolist() == [0, 0, 0] and p.data[8904 + 1173:].tolist() == [0, 0, 0]      # the alignment gaps are zeros
    assert p.frames == [3, 1] and p.lengths.tolist() == [3, 1] and p.lengths.dtype == torch.int64 and p.flips == [1, 0]
    # the lower half [H // 2, H) of every face to slot b * T + t, T = the longest clip; the whole drawn faces to slot 2 b + k
    assert p.mouth_jobs() == [(0, 33, 16, 16, 0, 17, 16, 1, 0), (1584, 40, 51, 20, 0, 20, 51, 1, 1), (7704, 21, 19, 10, 0, 11, 19, 1, 2),
                              (8904, 17, 23, 8, 0, 9, 23, 0, 3)]
    assert [j[-1] for j in p.mouth_jobs(5)] == [0, 1, 2, 5]
    assert p.face_jobs == [(7704, 21, 19, 0, 0, 21, 19, 1, 0), (0, 33, 16, 0, 0, 33, 16, 1, 1), (8904, 17, 23, 0, 0, 17, 23, 0, 2), (8904, 17, 23, 0, 0, 17, 23, 0, 3)]
    native.resize_check(p.mouth_jobs(), p.data.numel(), MOUTH, 2, 3, 96)
    native.resize_check(p.mouth_jobs(5), p.data.numel(), MOUTH, 2, 5, 88)
    native.resize_check(p.face_jobs, p.data.numel(), FACE, 2, 2, 160)
    with pytest.raises(AssertionError, match="two face indices"):
        PackedFaces([(a, False, (0, 3))], pin=False)
    with pytest.raises(AssertionError, match="uint8"):
        PackedFaces([([a[0].float()], False, (0, 0))], pin=False)


def test_faces_item_host_is_the_reference_tail():
    """against `face_recog_resize` and the per-face formula of datasets/grid/dataset.py:225-236 written out: flip every face, Resize + (x - 127.5) / 128 on
    the two drawn faces, the lower half `face[:, H // 2:, :]` through Resize, / 255 and Normalize"""
    import torch.nn.functional as F

    from lip2speech_amd.datasets import faces_item_host
    from lip2speech_amd.datasets.lrw import IMAGENET_MEAN, IMAGENET_STD, face_recog_resize
    faces = _faces(3)
    for flip in (False, True):
        for size in (96, 88):
            lower, crop = faces_item_host(faces, flip, (2, 1), size=size)
            src = [torch.flip(f, dims=(-1,)) for f in faces] if flip else faces
            assert crop.shape == (2, 3, 160, 160) and torch.equal(crop, torch.stack([face_recog_resize(src[2]), face_recog_resize(src[1])]))
            assert lower.shape == (3, 3, size, size) and lower.dtype == torch.float32
            for got, face in zip(lower, src):
                C, H, W = face.shape
                u8 = F.interpolate(face[:, H // 2:, :][None].float(), size=(size, size), mode="bilinear", align_corners=False)[0].round().clamp(0, 255).to(torch.uint8)
                x = u8.float() / 255.0
                want = (x - torch.tensor(IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(IMAGENET_STD).view(3, 1, 1)
                assert torch.equal(got, want)
    assert not torch.equal(faces_item_host(faces, True, (0, 0))[0], faces_item_host(faces, False, (0, 0))[0])
    # (H,W,3) faces give the same item
    a = faces_item_host([f.permute(1, 2, 0).contiguous() for f in faces], True, (2, 1))
    b = faces_item_host(faces, True, (2, 1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_collate_of_face_items():
    from lip2speech_amd.datasets import PackedAudio, PackedFaces, device_collate_fn_pad_faces
    g = torch.Generator().manual_seed(5)
    batch = [((_faces(7), False, (0, 1)), torch.randn(1, 1000, generator=g), None, None), ((_faces(8)[:2], True, (1, 1)), torch.randn(1, 600, generator=g), None, None)]
    (pf, vlen), pa, pa2, faces = device_collate_fn_pad_faces(batch)
    assert isinstance(pf, PackedFaces) and faces is pf and isinstance(pa, PackedAudio) and pa2 is pa
    assert vlen.tolist() == [3, 2] and pa.lengths.tolist() == [1000, 600] and pf.flips == [0, 1]
    out = device_collate_fn_pad_faces([b + ("p%d" % i,) for i, b in enumerate(batch)])
    assert len(out) == 5 and out[4] == ("p0", "p1")


def test_lrw_raw_faces_swaps_only_the_face_slot(tmp_path):
    import numpy as np

    from lip2speech_amd.datasets import LRW, PackedFaces
    from lip2speech_amd.datasets.lrw import face_recog_resize, load_frames
    d = tmp_path / "LRW_Faces" / "ABOUT" / "test"
    a = tmp_path / "lipread_audio" / "ABOUT" / "test"
    d.mkdir(parents=True); a.mkdir(parents=True)
    for i in (1, 2):
        shutil.copy(os.path.join(SAMPLE, f"ABOUT_0000{i}_mouth.npz"), d / f"ABOUT_0000{i}_mouth.npz")
        shutil.copy(os.path.join(SAMPLE, f"ABOUT_0000{i}.npz"), a / f"ABOUT_0000{i}.npz")
    shutil.copy(os.path.join(SAMPLE, "ABOUT_00001_mouth.npz"), d / "ABOUT_00001_face.npz")        # the same container holds the face frames: item 0 has a face file
    raw, ref = LRW(str(tmp_path), mode="test", raw_faces=True), LRW(str(tmp_path), mode="test")
    for i in range(2):
        torch.manual_seed(i)
        got = raw[i]
        after_raw = torch.rand(1)
        torch.manual_seed(i)
        want = ref[i]
        assert torch.equal(after_raw, torch.rand(1))                                                 # the draw stays where it is
        assert len(got) == len(want) == 4 and all(torch.equal(got[k], want[k]) for k in (0, 1, 2))
        if i == 0:
            assert got[3].dtype == torch.uint8 and got[3].shape == (2, 3, 96, 96)
            assert torch.equal(torch.stack([face_recog_resize(f) for f in got[3]]), want[3])       # the same two frames, not yet resized
            frames = torch.from_numpy(np.ascontiguousarray(load_frames(str(d / "ABOUT_00001_face.npz")))).permute(0, 3, 1, 2)
            assert any(torch.equal(got[3][0], f) for f in frames)
            p = PackedFaces([(list(got[3]), False, (0, 1))], pin=False)                              # what the device route packs
            assert p.face_jobs == [(0, 96, 96, 0, 0, 96, 96, 0, 0), (27648, 96, 96, 0, 0, 96, 96, 0, 1)]
        else:
            assert torch.equal(got[3], torch.zeros(2, 3, 160, 160))                                  # no face file: the usual zeros
