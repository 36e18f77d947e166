"""Face alignment on the GPU (`l2s_align_faces`, face_align.hip) against the HOST restatement `face_utils.warp_affine_u8` (itself held to a per-pixel
restatement and to closed forms by tests/test_face_align_host.py) and against closed forms - never against the kernel itself.  Every comparison is bit
for bit: the transform is integer arithmetic after four float64 roundings that the kernel makes one by one, so there is nothing to allow for.

Both routes of the kernel are reached: a band whose source rows fit 60 KiB of LDS stages them (the small images at every angle, the larger ones at the
small angles), the others read their taps from global memory (45 and 90 degrees on 250 x 233 and 700 x 900, and every rotation of 700 x 900)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = ((16, 16), (33, 16), (122, 117), (192, 203), (250, 233), (700, 900))      # 192 x 203: a row pitch of 609 bytes, every row starts unaligned
ANGLES = (0.0, 0.9, -0.9, 7.3, -12.0, 45.0, 90.0, 180.0)
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _image(h, w, seed=0):
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _pack(images, fill=0, gap=0, tail=0):
    """images (H,W,3) on 4-byte boundaries, `gap` (a multiple of 4) unnamed bytes after every third one and `tail` after the last; the pad bytes, the gaps
    and the tail hold `fill` -> (buffer, offsets)"""
    offs, total = [], 0
    for k, im in enumerate(images):
        offs.append(total)
        total = (total + im.size + 3) // 4 * 4 + (gap if k % 3 == 2 else 0)
    buf = np.full(total + tail, fill, dtype=np.uint8)
    for im, o in zip(images, offs):
        buf[o:o + im.size] = im.reshape(-1)
    return buf, offs


def _run(images, maps, fill=0, gap=0, tail=0, prefill=0xAB):
    """one `l2s_align_faces` call on the packed images -> (the output buffer on the CPU, offsets)"""
    from lip2speech_amd import native
    buf, offs = _pack(images, fill, gap, tail)
    jobs = [(o,) + im.shape[:2] + tuple(m) for o, im, m in zip(offs, images, maps)]
    out = torch.full((buf.size,), prefill, dtype=torch.uint8, device="cuda")
    got = native.align_faces(torch.from_numpy(buf).cuda(), jobs, out=out)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy(), offs


def _expect(images, wants, offs, size, prefill=0xAB):
    """what the call must leave: every image's result at its offset, zeros in its pad bytes, `prefill` everywhere else"""
    want = np.full(size, prefill, dtype=np.uint8)
    for im, w, o in zip(images, wants, offs):
        want[o:o + im.size] = w.reshape(-1)
        want[o + im.size:min((o + im.size + 3) // 4 * 4, size)] = 0
    return want


def _same(got, want, what=""):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {bad[:5].tolist()}: {got[bad[:5]].tolist()} for {want[bad[:5]].tolist()}"


@pytest.fixture(scope="module")
def grid():
    """every size at every angle: images, maps and the host restatement's results, made once"""
    from lip2speech_amd.datasets.face_utils import rotation_inverse_map, warp_affine_u8
    images = [_image(h, w, k) for h, w in SIZES for k in range(len(ANGLES))]
    maps = [rotation_inverse_map(a, h, w) for h, w in SIZES for a in ANGLES]
    return images, maps, [warp_affine_u8(im, m) for im, m in zip(images, maps)]


@pytest.fixture(scope="module")
def mixed_call(grid):
    """ONE call that holds all sizes at mixed angles, in an order that mixes the sizes inside a launch; gaps and tail of the input hold 0xFF"""
    images, maps, wants = grid
    order = [s * len(ANGLES) + a for a in range(len(ANGLES)) for s in range(len(SIZES))]
    images, maps, wants = [images[i] for i in order], [maps[i] for i in order], [wants[i] for i in order]
    got, offs = _run(images, maps, fill=0xFF, gap=8, tail=6)
    return images, wants, offs, got


@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{h}x{w}" for h, w in SIZES])
def test_one_call_of_all_sizes_at_mixed_angles(mixed_call, size):
    images, wants, offs, got = mixed_call
    for k in range(size, len(images), len(SIZES)):
        o, n = offs[k], images[k].size
        _same(got[o:o + n], wants[k].reshape(-1), f"{SIZES[size]} at {ANGLES[k // len(SIZES)]} degrees")


def test_pad_bytes_are_zero_and_unnamed_bytes_stay(mixed_call):
    images, wants, offs, got = mixed_call
    want = _expect(images, wants, offs, got.size)
    assert (want == 0xAB).sum() >= 8 * (len(images) // 3) + 6                       # the gaps and the tail are there
    _same(got, want, "the whole buffer")


def test_120_small_images_cross_the_launch_boundaries():
    from lip2speech_amd import native
    from lip2speech_amd.datasets.face_utils import rotation_inverse_map, warp_affine_u8
    assert 120 > 2 * native.ALIGN_JOBS_PER_LAUNCH
    images = [_image(16, 16, k) for k in range(120)]
    maps = [rotation_inverse_map(-15.0 + 0.25 * k, 16, 16) for k in range(120)]
    wants = [warp_affine_u8(im, m) for im, m in zip(images, maps)]
    got, offs = _run(images, maps)
    _same(got, _expect(images, wants, offs, got.size), "120 images of 16 x 16")
    got_ff, _ = _run(images, maps, fill=0xFF, gap=4, tail=5)                           # 0xFF in the gaps and after the last image: the same results
    for k, (im, o) in enumerate(zip(images, _pack(images, 0, 4, 5)[1])):
        _same(got_ff[o:o + im.size], wants[k].reshape(-1), f"image {k} with 0xFF around it")


def test_an_image_alone_and_as_the_last_after_a_boundary():
    from lip2speech_amd import native
    from lip2speech_amd.datasets.face_utils import rotation_inverse_map, warp_affine_u8
    n = native.ALIGN_JOBS_PER_LAUNCH
    for h, w, angle in ((33, 16, 7.3), (192, 203, -12.0), (250, 233, 45.0)):
        im, m = _image(h, w, 9), rotation_inverse_map(angle, h, w)
        want = warp_affine_u8(im, m).reshape(-1)
        alone, _ = _run([im], [m])
        others = [_image(16 + k % 5, 16 + k % 3, k) for k in range(n + 1)]           # the image is job n + 1: the second of the second launch
        last, offs = _run(others + [im], [rotation_inverse_map(3.0 * (k % 7) - 9.0, *o.shape[:2]) for k, o in enumerate(others)] + [m])
        _same(alone[:im.size], want, f"{h} x {w} alone")
        _same(last[offs[-1]:offs[-1] + im.size], want, f"{h} x {w} as the last job")
    # a buffer that ends with its last image, not on a 4-byte boundary: 5 x 7 x 3 = 105 bytes
    im, m = _image(5, 7), rotation_inverse_map(10.0, 5, 7)
    buf = torch.from_numpy(im.reshape(-1).copy()).cuda()
    _same(native.align_faces(buf, [(0, 5, 7) + tuple(m)]).cpu().numpy(), warp_affine_u8(im, m).reshape(-1), "a 105-byte buffer")


def test_closed_forms_hold_on_the_device():
    from lip2speech_amd.datasets.face_utils import rotation_inverse_map
    images, maps, wants = [], [], []
    for h, w in ((16, 16), (33, 16), (122, 117), (192, 203)):
        im = _image(h, w, 4)
        images += [im, im]                                                            # identity copies the image
        maps += [IDENT, rotation_inverse_map(0.0, h, w)]
        wants += [im, im]
        for dx, dy in ((3, 0), (0, -2), (-5, 4), (w, 0)):                             # integer shifts: zeros are shifted in
            want = np.zeros_like(im)
            ys, xs = np.arange(h) + dy, np.arange(w) + dx
            oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
            want[np.ix_(oky, okx)] = im[np.ix_(ys[oky], xs[okx])]
            images.append(im); maps.append((1.0, 0.0, float(dx), 0.0, 1.0, float(dy))); wants.append(want)
        wide = np.concatenate([im.astype(np.int64), np.zeros((h, 1, 3), np.int64)], axis=1)      # half a pixel: the tap past the last column is 0
        images.append(im); maps.append((1.0, 0.0, 0.5, 0.0, 1.0, 0.0)); wants.append(((wide[:, :-1] + wide[:, 1:] + 1) >> 1).astype(np.uint8))
    for h, w in ((33, 17), (121, 117), (251, 233)):                                   # 180 degrees on odd x odd reverses both axes
        im = _image(h, w, 5)
        images.append(im); maps.append(rotation_inverse_map(180.0, h, w)); wants.append(im[::-1, ::-1])
    for n in (17, 117, 233):                                                          # 90 degrees on an odd square
        im = _image(n, n, 6)
        images.append(im); maps.append(rotation_inverse_map(90.0, n, n)); wants.append(np.rot90(im, 1))
    got, offs = _run(images, maps)
    for k, (im, want, o) in enumerate(zip(images, wants, offs)):
        _same(got[o:o + im.size], np.ascontiguousarray(want).reshape(-1), f"closed form {k}: {im.shape[:2]} under {tuple(maps[k])}")


def _landmarks(eye1, eye2):
    lm = np.zeros((68, 2), dtype=np.int32)
    for sl, (mx, my) in ((slice(36, 42), eye1), (slice(42, 48), eye2)):
        lm[sl] = [(mx - 1, my - 1), (mx + 1, my - 1), (mx + 1, my + 1), (mx - 1, my + 1), (mx, my), (mx, my)]
    return lm.tolist()


def test_packed_faces_with_landmarks_equals_faces_aligned_on_the_host():
    """end to end: unrotated crops + landmarks through `PackedFaces.to_device()` (align, then the two resize calls) against the same crops rotated on the
    host by `align_and_crop_face` and handed over as today's 3-tuples"""
    from lip2speech_amd.datasets import PackedFaces, align_and_crop_face, face_box_crops
    sizes = [[(130, 121), (16, 16), (97, 140)], [(64, 48), (33, 16), (122, 117), (80, 80), (51, 67)], [(40, 35), (75, 91), (16, 19), (100, 100)]]
    flips, idx = [False, True, False], [(0, 2), (4, 1), (3, 3)]
    three, four = [], []
    for b, clip in enumerate(sizes):
        frames = torch.from_numpy(np.stack([_image(160, 200, 10 * b + t) for t in range(len(clip))])).permute(0, 3, 1, 2).contiguous()
        coords = [(7 + t, 3 + b, 7 + t + w, 3 + b + h) for t, (h, w) in enumerate(clip)]
        lms = [_landmarks((60, 50), (100, 50 + 4 * t - 7 * b)) for t in range(len(clip))]      # eye lines between -14 and +16 degrees or so
        crops, kept = face_box_crops(frames, coords, lms)
        assert [tuple(c.shape[1:]) for c in crops] == clip
        four.append((crops, flips[b], idx[b], kept))
        three.append(([align_and_crop_face(frames[t], coords[t], lms[t]) for t in range(len(clip))], flips[b], idx[b]))
    assert any(not torch.equal(a, c) for (al, _, _), (cr, _, _, _) in zip(three, four) for a, c in zip(al, cr))      # the rotation does something
    video4, crops4 = PackedFaces(four).to_device()
    video3, crops3 = PackedFaces(three).to_device()
    torch.cuda.synchronize()
    assert video4.shape == (3, 3, 5, 96, 96) and crops4.shape == (3, 2, 3, 160, 160)
    assert torch.equal(video4, video3) and torch.equal(crops4, crops3)
    # a batch that mixes both kinds of item: the images that came without landmarks are carried over as they are
    videom, cropsm = PackedFaces([three[0], four[1], three[2]]).to_device()
    torch.cuda.synchronize()
    assert torch.equal(videom, video3) and torch.equal(cropsm, crops3)
