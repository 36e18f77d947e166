"""Device-side JPEG decode, the host half (no GPU): the restatement `lip2speech_amd/datasets/jpeg.py` against the pixels Pillow recorded
(tests/golden/jpeg_cases.npz, written by tests/golden/make_jpeg_cases.py) and against Pillow itself on the sample clips; `parse_jpeg` / `l2s_jpeg_plan`
on known streams, their table-set deduplication and every refusal; the entropy decoder's host instantiation (`l2s_op_jpeg_entropy_host`, diagnostic
library) on every case and on corrupted copies - corrupt streams are tested here and nowhere on the device; the loader and collate routes."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

from lip2speech_amd import native
from lip2speech_amd.datasets import jpeg
from lip2speech_amd.datasets.lrw import load_jpeg_strings

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMPLE = os.path.join(GOLDEN, "sample_lrw")


@pytest.fixture(scope="module")
def cases():
    """name -> (stream bytes, the pixels Pillow decoded)"""
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    return {str(n): (z["s_" + str(n)].tobytes(), z["p_" + str(n)]) for n in z["names"]}


def _plan(streams):
    arrays = [np.frombuffer(s, dtype=np.uint8) for s in streams]
    sizes = [a.size for a in arrays]
    offsets = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    buf = np.concatenate(arrays + [np.zeros(0, dtype=np.uint8)])
    return buf, offsets, sizes, (lambda: native.jpeg_plan(buf, offsets, sizes))


def test_fixture_covers_the_issue_list(cases):
    sizes = {n.split("_")[1] for n in cases}
    assert {"1x1", "2x2", "8x8", "16x16", "17x9", "9x17", "24x40", "33x31", "96x96", "146x120"} <= sizes
    for word in ("noise", "ramp", "const", "_420_", "_444_", "_grey_", "_q30", "_q75", "_q95", "_q100", "_opt", "_rb1", "_rb3", "_rr1"):
        assert any(word in n for n in cases), word
    assert os.path.getsize(os.path.join(GOLDEN, "jpeg_cases.npz")) < 1 << 20


def test_restatement_equals_recorded_pixels(cases):
    for name, (stream, pixels) in cases.items():
        mine = jpeg.decode_jpeg_host(stream)
        assert mine.dtype == np.uint8 and mine.shape == pixels.shape and np.array_equal(mine, pixels), name


def test_restatement_equals_pillow_on_sample_clips():
    Image = pytest.importorskip("PIL.Image")
    import io
    clips = sorted(f for f in os.listdir(SAMPLE) if f.endswith("_mouth.npz"))
    assert len(clips) == 10
    for clip in clips:
        strings = load_jpeg_strings(os.path.join(SAMPLE, clip))
        for t in (0, 14, 28):
            want = np.asarray(Image.open(io.BytesIO(strings[t])).convert("RGB"))
            assert np.array_equal(jpeg.decode_jpeg_host(strings[t]), want), (clip, t)


def test_fields_on_known_streams(cases):
    names = ["noise_33x31_420_q75_rb3", "noise_17x9_444_q75", "noise_24x40_grey_q75_rr1", "noise_146x120_420_q75"]
    want = {names[0]: (33, 31, jpeg.LAYOUT_420, 3), names[1]: (17, 9, jpeg.LAYOUT_444, 0), names[2]: (24, 40, jpeg.LAYOUT_GREY, 5),
            names[3]: (146, 120, jpeg.LAYOUT_420, 0)}
    buf, offsets, sizes, plan = _plan([cases[n][0] for n in names])
    p = plan()
    assert p.n == 4 and p.stream_bytes == buf.size
    for i, n in enumerate(names):
        h = jpeg.parse_jpeg(cases[n][0])
        assert (h.H, h.W, h.layout, h.restart_interval) == want[n], n
        assert h.eoi and h.scan_offset + h.scan_length + 2 == sizes[i]                   # the scan ends at EOI, the stream's last two bytes
        assert len(h.components) == (1 if h.layout == jpeg.LAYOUT_GREY else 3)
        assert [(c.h, c.v) for c in h.components][1:] == [(1, 1)] * (len(h.components) - 1)
        assert all(h.qtables[c.tq].shape == (64,) and len(h.htables[(0, c.td)][0]) == 16 and len(h.htables[(1, c.ta)][0]) == 16 for c in h.components)
        r = p.images[i]
        assert (r.H, r.W, r.layout, r.restart, r.eoi) == want[n] + (1,), n
        assert (r.scan_offset, r.scan_bytes) == (offsets[i] + h.scan_offset, h.scan_length), n
        assert p.blocks[i] == h.n_blocks
        # the set's quantisers are the stream's, in natural order
        ts = p.sets[r.table_set]
        for c, comp in enumerate(h.components):
            q = np.zeros(64, dtype=np.uint16)
            q[jpeg.ZIGZAG] = h.qtables[comp.tq]
            assert np.array_equal(np.asarray(ts.quant[c][:]), q) and (ts.dc[c], ts.ac[c]) == (comp.td, comp.ta)
    assert (native.JPEG_GREY, native.JPEG_444, native.JPEG_420) == (jpeg.LAYOUT_GREY, jpeg.LAYOUT_444, jpeg.LAYOUT_420)
    assert p.workspace_bytes() >= sum(p.blocks) * 192


def test_table_sets_are_deduplicated_by_content(cases):
    strings = load_jpeg_strings(os.path.join(SAMPLE, "ABOUT_00001_mouth.npz"))
    assert len(strings) == 29
    p = _plan(strings)[3]()
    assert p.n_sets == 1 and {r.table_set for r in p.images} == {0}
    p = _plan([cases["noise_33x31_420_q30"][0], cases["noise_33x31_420_q95"][0], cases["ramp_17x9_420_q30"][0]])[3]()
    assert p.n_sets == 2 and [r.table_set for r in p.images] == [0, 1, 0]


# ---- refusals: each made by editing bytes of a fixture stream ------------------------------------------------------------------------------------------------

def _segments(s: bytes):
    """marker -> offset of its FF, for the header segments up to SOS"""
    out, p = {}, 2
    while True:
        assert s[p] == 0xFF
        m = s[p + 1]
        out.setdefault(m, p)
        if m == 0xDA:
            return out
        p += 2 + ((s[p + 2] << 8) | s[p + 3])


def _edit(s: bytes, pos: int, new: bytes) -> bytes:
    return s[:pos] + new + s[pos + len(new):]


def _insert(s: bytes, pos: int, new: bytes) -> bytes:
    return s[:pos] + new + s[pos:]


def _refusals(colour: bytes, grey: bytes):
    seg, gseg = _segments(colour), _segments(grey)
    sof, sos, gsos, gsof = seg[0xC0], seg[0xDA], gseg[0xDA], gseg[0xC0]
    h = jpeg.parse_jpeg(colour)
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    yield "progressive", _edit(colour, sof + 1, b"\xc2"), "progressive"
    yield "extended", _edit(colour, sof + 1, b"\xc1"), "extended"
    yield "lossless", _edit(colour, sof + 1, b"\xc3"), "lossless"
    yield "arithmetic", _edit(colour, sof + 1, b"\xc9"), "arithmetic"
    yield "12-bit", _edit(colour, sof + 4, b"\x0c"), "12-bit"
    yield "four components", _edit(colour, sof + 9, b"\x04"), "four components"
    yield "4:2:2", _edit(colour, sof + 11, b"\x21"), "sampling factors 2x1"
    yield "4:4:0", _edit(colour, sof + 11, b"\x12"), "sampling factors 1x2"
    yield "scan of one component", _edit(colour, sos + 4, b"\x01"), "more than one scan"
    yield "second scan", _insert(colour, len(colour) - 2, colour[sos:sos + 14]), "more than one scan"
    yield "DNL", _insert(colour, sos, b"\xff\xdc\x00\x04\x00\x10"), "DNL"
    yield "DNL after the scan", _insert(colour, len(colour) - 2, b"\xff\xdc\x00\x04\x00\x10"), "DNL"
    yield "Adobe transform 0", _insert(colour, sof, adobe), "RGB-coded"
    rgb = colour
    for k, c in enumerate(b"RGB"):
        rgb = _edit(_edit(rgb, sof + 10 + 3 * k, bytes([c])), sos + 5 + 2 * k, bytes([c]))
    yield "component ids R G B", rgb, "RGB-coded"
    yield "undefined Huffman table", _edit(grey, gsos + 6, b"\x11"), "never defined"
    yield "undefined quantisation table", _edit(grey, gsof + 12, b"\x03"), "never defined"
    yield "cut inside a header", colour[:h.scan_offset - 5], "runs past the stream"
    yield "cut inside the first header", colour[:20], "runs past the stream"
    yield "too large", _edit(colour, sof + 5, b"\x13\x88"), "outside [1, 4096]"
    yield "no SOI", b"\x00" + colour[1:], "SOI"


def test_every_refusal_names_the_image_and_the_reason(cases):
    colour, grey = cases["noise_33x31_420_q75"][0], cases["noise_33x31_grey_q75"][0]
    seen = 0
    for what, stream, reason in _refusals(colour, grey):
        with pytest.raises(jpeg.JpegError, match=re.escape(reason)):
            jpeg.parse_jpeg(stream)
        with pytest.raises(RuntimeError) as e:
            _plan([colour, stream, grey])[3]()
        assert "image 1:" in str(e.value) and reason in str(e.value), (what, str(e.value))
        seen += 1
    assert seen == 20
    _plan([colour, grey])[3]()                                   # the unedited streams pass


# ---- the entropy decoder's host instantiation ----------------------------------------------------------------------------------------------------------------

def test_host_entropy_path_equals_the_restatement(cases):
    names = list(cases)
    buf, _, _, plan = _plan([cases[n][0] for n in names])
    p = plan()
    coefs, status, sentinel = native.op_jpeg_entropy_host(buf, p, sentinel_words=32)
    assert not status.any() and (sentinel == 0x5A5A).all()
    b0 = 0
    for n, nb in zip(names, p.blocks):
        want = np.concatenate([c.reshape(-1, 64) for c in jpeg.entropy_decode_host(cases[n][0])])
        assert want.shape == (nb, 64) and np.array_equal(coefs[b0:b0 + nb], want), n
        b0 += nb
    assert b0 == coefs.shape[0]


def _corrupted(plain: bytes, restarts: bytes):
    h, hr = jpeg.parse_jpeg(plain), jpeg.parse_jpeg(restarts)
    mid = h.scan_offset + h.scan_length // 2
    yield "cut at the header's end", plain[:h.scan_offset]
    yield "cut mid-scan", plain[:mid]
    yield "one byte short", plain[:-1]
    yield "a run of FF FF", _edit(plain, mid, b"\xff\xff\xff\xff")
    # a flip that breaks the code structure: the scan's first bytes become zeros, i.e. a run of the shortest codes, and the bits no longer add up to the scan
    # (a flip inside a coefficient's magnitude bits alone would be another legal stream, and no decoder could tell)
    yield "flipped bytes in the scan", _edit(plain, h.scan_offset + 2, b"\x00\x00\x00")
    first = restarts.index(b"\xff\xd0", hr.scan_offset)
    yield "a deleted restart marker", restarts[:first] + restarts[first + 2:]
    yield "a wrong restart marker", _edit(restarts, first, b"\xff\xd3")
    yield "restart markers without DRI", _edit(restarts, _segments(restarts)[0xDD] + 4, b"\x00\x00")


def test_host_entropy_path_on_corrupted_copies(cases):
    plain, restarts = cases["noise_33x31_420_q75"][0], cases["noise_33x31_420_q75_rb3"][0]
    seen = 0
    for what, stream in _corrupted(plain, restarts):
        buf, _, _, plan = _plan([plain, stream, restarts])
        p = plan()                                               # a stream that stops inside its scan is planned, not refused
        coefs, status, sentinel = native.op_jpeg_entropy_host(buf, p, sentinel_words=64)
        assert status[1] != 0, what
        assert status[0] == 0 and status[2] == 0, what           # the neighbours are untouched by it
        assert (sentinel == 0x5A5A).all(), what
        assert coefs.shape == (sum(p.blocks), 64)
        with pytest.raises(jpeg.JpegError):
            jpeg.entropy_decode_host(stream)
        seen += 1
    assert seen == 8


def test_decode_arguments_are_checked_on_the_host(cases):
    """what `l2s_jpeg_workspace_bytes` refuses needs no device: records outside their ranges"""
    p = _plan([cases["noise_8x8_420_q75"][0]])[3]()
    assert p.workspace_bytes() > 0
    for field, value, reason in (("H", 0, "outside [1, 4096]"), ("W", 5000, "outside [1, 4096]"), ("layout", 3, "layout"), ("table_set", 1, "table set"),
                                 ("restart", -1, "restart interval"), ("scan_bytes", -1, "scan bytes")):
        q = _plan([cases["noise_8x8_420_q75"][0]])[3]()
        setattr(q.images[0], field, value)
        with pytest.raises(RuntimeError) as e:
            q.workspace_bytes()
        assert "image 0" in str(e.value) and reason in str(e.value), str(e.value)


# ---- loader and collate routes -------------------------------------------------------------------------------------------------------------------------------

def test_packed_jpeg_frames_layout_equals_packed_frames():
    from lip2speech_amd.datasets import PackedFrames, PackedJpegFrames
    a = load_jpeg_strings(os.path.join(SAMPLE, "ABOUT_00001_mouth.npz"))
    b = load_jpeg_strings(os.path.join(SAMPLE, "ABOUT_00002_mouth.npz"))[:5]
    b = [np.frombuffer(s, dtype=np.uint8) for s in b[:3]] + [np.frombuffer(s, dtype=np.uint8).reshape(-1, 1) for s in b[3:]]      # arrays (n,) and (n, 1) too
    pj = PackedJpegFrames([a, b], pin=False)
    twin = PackedFrames([torch.zeros(29, 96, 96, 3, dtype=torch.uint8), torch.zeros(5, 96, 96, 3, dtype=torch.uint8)], pin=False)
    assert (pj.H, pj.W, pj.frames, pj.offsets) == (twin.H, twin.W, twin.frames, twin.offsets) and torch.equal(pj.lengths, twin.lengths)
    assert pj.packed_bytes == twin.data.numel() and pj.image_offsets == [t * 96 * 96 * 3 for t in range(34)]
    assert pj.data.numpy().tobytes() == b"".join(a) + b"".join(x.tobytes() for x in b)                  # the compressed bytes, exactly as they are
    assert pj.plan.n == 34 and pj.plan.n_sets == 1
    assert pj.data.numel() * 10 < twin.data.numel()                                                    # a fraction of the decoded bytes crosses to the device
    with pytest.raises(RuntimeError, match="image 1:"):
        PackedJpegFrames([[a[0], a[1][:100]]], pin=False)
    with pytest.raises(AssertionError, match="one crop size"):
        PackedJpegFrames([[a[0], _other_size()]], pin=False)


def _other_size() -> bytes:
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    return z["s_noise_16x16_420_q75"].tobytes()


def test_packed_faces_takes_jpeg_strings(cases):
    from lip2speech_amd.datasets import PackedFaces
    names = ["noise_33x31_420_q75", "ramp_24x40_420_q75", "noise_146x120_420_q75", "noise_17x9_444_q75", "noise_33x31_grey_q75"]
    strings = [cases[n][0] for n in names]
    pixels = [torch.from_numpy(cases[n][1].copy()) for n in names]                     # (H,W,3), what PackedFaces takes decoded
    lm = np.zeros((68, 2), dtype=np.int64)
    lm[36:42] = (10, 20)
    lm[42:48] = (30, 24)
    items_s = [(strings[:3], True, (0, 2)), (strings[3:], False, (1, 1), [lm, lm])]
    items_p = [(pixels[:3], True, (0, 2)), (pixels[3:], False, (1, 1), [lm, lm])]
    ps, pp = PackedFaces(items_s, pin=False), PackedFaces(items_p, pin=False)
    assert ps.images == pp.images and ps.frames == pp.frames and ps.flips == pp.flips and torch.equal(ps.lengths, pp.lengths)
    assert ps.face_jobs == pp.face_jobs and ps.mouth_jobs() == pp.mouth_jobs() and ps.mouth_jobs(7) == pp.mouth_jobs(7) and ps.align_jobs == pp.align_jobs
    assert ps.jpeg_offsets == [o for o, _, _ in pp.images] and ps.jpeg_plan.n == 5 and ps.data.numel() == pp.data.numel()
    assert ps.jpeg_data.numpy().tobytes() == b"".join(strings)
    assert pp.jpeg_plan is None and pp.jpeg_data is None                               # faces that come decoded keep their path
    mixed = PackedFaces([([strings[0], pixels[1], strings[2]], False, (0, 1))], pin=False)
    assert mixed.jpeg_offsets == [mixed.images[0][0], mixed.images[2][0]] and mixed.images == PackedFaces([(pixels[:3], False, (0, 1))], pin=False).images
    o, H, W = mixed.images[1]
    assert torch.equal(mixed.data[o:o + H * W * 3].view(H, W, 3), pixels[1]) and not mixed.data[:o].any()


def _lrw_tree(tmp_path, with_face):
    import bz2
    import pickle
    d = tmp_path / "LRW_Faces" / "ABOUT" / "test"
    a = tmp_path / "lipread_audio" / "ABOUT" / "test"
    d.mkdir(parents=True); a.mkdir(parents=True)
    for i in (1, 2):
        shutil.copy(os.path.join(SAMPLE, f"ABOUT_0000{i}_mouth.npz"), d / f"ABOUT_0000{i}_mouth.npz")
        shutil.copy(os.path.join(SAMPLE, f"ABOUT_0000{i}.npz"), a / f"ABOUT_0000{i}.npz")
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    face = [z["s_noise_146x120_420_q75"].reshape(-1, 1), z["s_ramp_146x120_420_q75"].reshape(-1, 1)]
    blobs = [face[t % 2] for t in range(29)]                                          # a face file in the corpus format: a bz2 pickle of (n, 1) JPEG byte arrays
    for i in with_face:
        with bz2.BZ2File(str(d / f"ABOUT_0000{i}_face.npz"), "w") as fh:
            pickle.dump(blobs, fh)
    return [b.tobytes() for b in face]


def test_lrw_raw_jpeg_items_and_rng_consumption(tmp_path):
    from lip2speech_amd.datasets import LRW
    face = _lrw_tree(tmp_path, with_face=(1,))
    raw, ref = LRW(str(tmp_path), mode="test", raw_jpeg=True, raw_audio=True), LRW(str(tmp_path), mode="test", raw_frames=True, raw_audio=True, raw_faces=True)
    for idx in (0, 1):
        torch.manual_seed(11)
        a = raw[idx]
        after_a = torch.rand(3)
        torch.manual_seed(11)
        b = ref[idx]
        after_b = torch.rand(3)
        assert torch.equal(after_a, after_b)                                           # the loader's RNG consumption is unchanged
        assert isinstance(a[0], list) and len(a[0]) == 29 and all(isinstance(s, bytes) and s[:2] == b"\xff\xd8" for s in a[0])
        assert a[0] == load_jpeg_strings(os.path.join(SAMPLE, f"ABOUT_0000{idx + 1}_mouth.npz"))
        assert torch.equal(a[1], b[1]) and a[2] is None and b[2] is None
    torch.manual_seed(11)
    want = (torch.rand(2) * 29).int().tolist()
    torch.manual_seed(11)
    faces = raw[0][3]
    assert isinstance(faces, list) and faces == [face[t % 2] for t in want]          # the two drawn faces' strings, undecoded
    assert torch.equal(raw[1][3], torch.zeros(2, 3, 160, 160))                        # no face file: the usual zeros


def test_device_collate_fn_pad_jpeg(tmp_path):
    from lip2speech_amd.datasets import LRW, PackedAudio, PackedFaces, PackedJpegFrames, device_collate_fn_pad_jpeg, device_collate_fn_pad_raw
    _lrw_tree(tmp_path, with_face=(1, 2))
    raw = LRW(str(tmp_path), mode="test", raw_jpeg=True, raw_audio=True, demo=True)
    twin = LRW(str(tmp_path), mode="test", raw_frames=True, raw_audio=True)
    torch.manual_seed(3)
    (frames, vlen), audio, audio2, faces, paths = device_collate_fn_pad_jpeg([raw[0], raw[1]])
    torch.manual_seed(3)
    (tframes, tvlen), taudio, _, _ = device_collate_fn_pad_raw([twin[0], twin[1]])
    assert isinstance(frames, PackedJpegFrames) and isinstance(audio, PackedAudio) and audio is audio2 and isinstance(faces, PackedFaces) and len(paths) == 2
    assert torch.equal(vlen, tvlen) and frames.frames == tframes.frames and frames.offsets == tframes.offsets and (frames.H, frames.W) == (tframes.H, tframes.W)
    assert torch.equal(audio.data, taudio.data) and audio.samples == taudio.samples
    assert faces.frames == [2, 2] and faces.face_jobs == [(o, 146, 120, 0, 0, 146, 120, 0, k) for k, (o, _, _) in enumerate(faces.images)]
    # a loader without face files: the stacked zeros, as before
    for f in (tmp_path / "LRW_Faces" / "ABOUT" / "test").glob("*_face.npz"):
        f.unlink()
    out = device_collate_fn_pad_jpeg([raw[0], raw[1]])
    assert torch.equal(out[3], torch.zeros(2, 2, 3, 160, 160))
