"""Device-side face crops on the GPU (`l2s_resize_normalise`, frame_resize.hip) against the HOST path, `datasets.device.faces_item_host` and the
uint8 resize it is made of (`F.interpolate` + round on the CPU) - never the code under test.

What is compared is the uint8 the kernel chose, recovered from its float; since the epilogue is determined by that uint8, the floats must also be the
epilogue of it to the bit (`(u / 255 - mean) / std` for mouth crops, `(u - 127.5) / 128` for face crops).

Integer ratios (192 x 384 -> 96 x 96, 320 x 320 -> 160 x 160, identity): every weight and product is exact in fp32, a quarter of the pixels are exact
.5 ties: bit for bit, no allowance.  At identity size the mouth output also equals `native.normalise_pad_frames` to the bit.

Other sizes: |u8_dev - u8_host| <= 1 everywhere, and equal wherever the exact value (fp64 on rational weights, `_exact`) lies farther than delta from a
half-integer.  delta is computed by the `yard` fixture on the CPU, from the host path alone and for every input on its own: twice the largest
|host fp32 path - exact| over that input (one delta over all inputs would be the 700 x 900 rectangle's, 2e-2, for a 16 x 16 source whose own is 4e-4).
Measured on the CPU, before doubling: 2.2e-4 (16 x 16 -> 160, 17 x 16 -> 96), 6.2e-4 (61 x 117), 2.6e-3 (96 x 203), 3.0e-3 (250 x 233 -> 160),
1.0e-2 (700 x 900); the end-to-end faces 2.2e-4 .. 2.9e-3.  The zone then holds 0.25-1.7 % of an input's pixels, 4.1 % for the 700 x 900 one.  The condition
that keeps delta honest is asserted on the host path before the device is looked at: the zone may not hold more than 5 % of the pixels of any input.
Measured on the MI355X: the kernel's uint8 equals the host path's at every pixel of every input, the zone included."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MOUTH, FACE = 0, 1
MEAN = torch.tensor((0.485, 0.456, 0.406)).view(3, 1, 1)
STD = torch.tensor((0.229, 0.224, 0.225)).view(3, 1, 1)

# name: (mode, image H, image W).  Mouth cases take the lower half [H // 2, H) of the image, as the loaders do; face cases the whole image.
RATIO_CASES = {"192x384": (MOUTH, 384, 384), "320x320": (FACE, 320, 320), "id96": (MOUTH, 192, 96), "id160": (FACE, 160, 160)}
OTHER_CASES = {"17x16": (MOUTH, 33, 16),            # the reference's minimum face, 16 wide, and an odd height
               "61x117": (MOUTH, 122, 117),
               "96x203": (MOUTH, 192, 203),         # a row pitch of 609 bytes: every row starts unaligned
               "250x233": (FACE, 250, 233),
               "16x16": (FACE, 16, 16),
               "700x900": (MOUTH, 1400, 900)}       # ratios 7.3 and 9.4: the taps of neighbouring outputs are far apart


def _image(seed, H, W):
    return torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _rect(mode, H, W):
    return (H // 2, 0, H - H // 2, W) if mode == MOUTH else (0, 0, H, W)


def _crop(img_hwc, rect, flip=False):
    """the rectangle as uint8 (3,h,w), its columns mirrored if `flip`"""
    y0, x0, h, w = rect
    x = img_hwc.permute(2, 0, 1)[:, y0:y0 + h, x0:x0 + w]
    return (torch.flip(x, dims=(-1,)) if flip else x).contiguous()


def _pack(images, fill=0, tail=0):
    """images (H,W,3) back to back on 4-byte boundaries -> (buffer, offsets, end of the last image); gaps and `tail` extra bytes hold `fill`"""
    offs, total = [], 0
    for im in images:
        offs.append(total)
        end = total + im.numel()
        total = (end + 3) // 4 * 4
    buf = torch.full((total + tail,), fill, dtype=torch.uint8)
    for im, o in zip(images, offs):
        buf[o:o + im.numel()] = im.reshape(-1)
    return buf, offs, end


def _job(off, img, rect, flip, slot):
    return (off, img.shape[0], img.shape[1]) + tuple(rect) + (int(flip), slot)


def _size(mode, size=None):
    return size or (96 if mode == MOUTH else 160)


def _host_f32(crop, size):
    return torch.nn.functional.interpolate(crop[None].float(), size=(size, size), mode="bilinear", align_corners=False)[0]


def _host_u8(crop, size):
    from lip2speech_amd.datasets.device import _resize_u8
    return _resize_u8(crop, (size, size))


def _taps(n, o):
    """src = (n / o)(d + 0.5) - 0.5 = (n (2 d + 1) - o) / (2 o) in integers: lower tap, upper tap, weight of the upper tap (exact in fp64)"""
    d = torch.arange(o, dtype=torch.int64)
    num = (n * (2 * d + 1) - o).clamp(min=0)
    i0 = (num // (2 * o)).clamp(max=n - 1)
    return i0, (i0 + 1).clamp(max=n - 1), (num % (2 * o)).double() / (2 * o)


def _exact(crop, size):
    x = crop.double()
    ya, yb, ly = _taps(crop.shape[1], size)
    xa, xb, lx = _taps(crop.shape[2], size)
    top = x[:, ya][:, :, xa] * (1 - lx) + x[:, ya][:, :, xb] * lx
    bot = x[:, yb][:, :, xa] * (1 - lx) + x[:, yb][:, :, xb] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def _recover(out, mode):
    """the device's floats (..., 3, oh, ow) channel-first per image -> the uint8 behind them; the floats must be that uint8's epilogue to the bit.  An image of
    exact zeros is an unnamed slot (no uint8 has 0.0 for its epilogue): it is left to the caller's own zero checks and comes back as uint8 zeros"""
    out = out.cpu()
    live = (out.abs().amax(dim=(-3, -2, -1), keepdim=True) > 0).expand_as(out)
    if mode == MOUTH:
        u = ((out.double() * STD.double() + MEAN.double()) * 255.0).round()
        again = (u.float() / 255.0 - MEAN) / STD
    else:
        u = (out.double() * 128.0 + 127.5).round()
        again = (u.float() - 127.5) / 128.0
    assert float(u[live].min()) >= 0 and float(u[live].max()) <= 255
    assert torch.equal(again[live], out[live]), "the floats are not the epilogue of a uint8"
    return torch.where(live, u, torch.zeros_like(u)).to(torch.uint8)


def _run(images, jobs, mode, B, T=2, size=None, buf=None):
    """one call -> recovered uint8 (B,T,3,s,s) for mouth crops (slot order), (B,2,3,s,s) for face crops"""
    from lip2speech_amd import native
    if buf is None:
        buf = _pack(images)[0]
    out = native.resize_normalise(buf.cuda(), jobs, mode, B, T, size)
    torch.cuda.synchronize()
    s = _size(mode, size)
    assert out.shape == ((B, 3, T, s, s) if mode == MOUTH else (B, 2, 3, s, s))
    return _recover(out.permute(0, 2, 1, 3, 4) if mode == MOUTH else out, mode)


def _rules(u_dev, crop, size, delta, what):
    host, ex = _host_u8(crop, size), _exact(crop, size)
    d = (u_dev.int() - host.int()).abs()
    away = ((ex - ex.floor()) - 0.5).abs() > delta
    print(f"{what}: {int((d != 0).sum())} of {d.numel()} pixels differ from the host path, {int((d != 0)[away].sum())} of them away from ties; "
          f"max |d| {int(d.max())}; zone share {1 - float(away.double().mean()):.2e}")
    assert int(d.max()) <= 1, what
    assert torch.equal(u_dev[away], host[away]), what


def _e2e_items():
    g = torch.Generator().manual_seed(77)
    sizes = [(33, 16), (67, 59), (131, 127), (97, 111), (201, 181), (53, 47), (143, 149), (89, 101), (171, 163)]      # no simple ratios: few exact ties

    def face(i, chw):
        H, W = sizes[i % len(sizes)]
        x = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g)
        return x if chw else x.permute(1, 2, 0).contiguous()
    return [([face(i, True) for i in range(7)], True, (5, 2)), ([face(i + 3, False) for i in range(9)], False, (0, 8))]


@pytest.fixture(scope="module")
def yard():
    """CPU only, computed once, never modified: every case's image and crop, and delta = twice the host fp32 path's largest error against the exact value over
    each input of this file that is held to the tie rule (OTHER_CASES and the end-to-end items), every input with its own.  Asserts the zone condition on
    the host path alone."""
    from lip2speech_amd.datasets.device import _chw
    cases, rule_crops = {}, []
    for k, (name, (mode, H, W)) in enumerate({**RATIO_CASES, **OTHER_CASES}.items()):
        img = _image(100 + k, H, W)
        cases[name] = (mode, img, _rect(mode, H, W), _crop(img, _rect(mode, H, W)))
        if name in OTHER_CASES:
            rule_crops.append((name, cases[name][3], _size(mode)))
    for b, (faces, flip, idx) in enumerate(_e2e_items()):
        for t, f in enumerate(faces):
            f = _chw(f)
            f = torch.flip(f, dims=(-1,)) if flip else f
            rule_crops.append((f"item {b} face {t}", f[:, f.shape[1] // 2:], 96))
            if t in idx:
                rule_crops.append((f"item {b} face {t} whole", f, 160))
    delta = {}
    for name, crop, size in rule_crops:
        ex = _exact(crop, size)
        err = float((_host_f32(crop, size).double() - ex).abs().max())
        delta[name] = 2 * err
        share = float((((ex - ex.floor()) - 0.5).abs() <= delta[name]).double().mean())
        print(f"{name} -> {size}: |host fp32 - exact| <= {err:.3e}, delta {delta[name]:.3e}, {share:.4f} of the pixels within delta of a tie")
        assert err > 0 and share <= 0.05, f"{name}: {share:.3f} of the pixels lie within delta = {delta[name]:.2e} of a tie - the tie rule would check too little"
    return {"cases": cases, "delta": delta}


@pytest.fixture(scope="module")
def dev(yard):
    """every case through the device in ONE mouth call and ONE face call on one packed buffer -> name: recovered uint8 (3,s,s)"""
    names = list(yard["cases"])
    images = [yard["cases"][n][1] for n in names]
    buf, offs, _ = _pack(images)
    got = {}
    for mode in (MOUTH, FACE):
        mine = [n for n in names if yard["cases"][n][0] == mode]
        jobs = [_job(offs[names.index(n)], yard["cases"][n][1], yard["cases"][n][2], 0, s) for s, n in enumerate(mine)]
        if mode == MOUTH:
            u = _run(None, jobs, MOUTH, 1, len(mine), buf=buf)[0]
        else:
            assert len(mine) % 2 == 0
            u = _run(None, jobs, FACE, len(mine) // 2, buf=buf).reshape(len(mine), 3, 160, 160)
        got.update({n: u[s] for s, n in enumerate(mine)})
    return got


def test_zone_condition_on_the_host_path(yard):
    assert set(OTHER_CASES) <= set(yard["delta"]) and 0 < max(yard["delta"].values()) < 0.025        # a zone of width 2 delta: under 5 % of a unit


@pytest.mark.parametrize("name", list(RATIO_CASES))
def test_integer_ratios_bit_for_bit(yard, dev, name):
    mode, _, _, crop = yard["cases"][name]
    host, ex = _host_u8(crop, _size(mode)), _exact(crop, _size(mode))
    if not name.startswith("id"):
        ties = float(((ex - ex.floor()) == 0.5).double().mean())
        assert 0.15 < ties < 0.35, ties                       # about a quarter of the pixels test the rounding rule
        assert torch.equal(host.double(), ex.round())          # the host path IS the exact value rounded half to even
    else:
        assert torch.equal(host, crop)
    assert torch.equal(dev[name], host)


def test_identity_equals_normalise_pad_frames():
    from lip2speech_amd import native
    clips = [torch.stack([_image(300 + 10 * b + t, 96, 96) for t in range(n)]) for b, n in enumerate((3, 1))]
    images = [f for c in clips for f in c]
    buf, offs, _ = _pack(images)
    dev_buf = buf.cuda()
    T = 4
    jobs, k = [], 0
    for b, c in enumerate(clips):
        for t in range(len(c)):
            jobs.append(_job(offs[k], images[k], (0, 0, 96, 96), 0, b * T + t))
            k += 1
    got = native.resize_normalise(dev_buf, jobs, MOUTH, 2, T)
    want = native.normalise_pad_frames(dev_buf, [offs[0], offs[3]], [3, 1], 96, 96, T)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert float(got[0, :, 3:].abs().max()) == 0.0 and float(got[1, :, 1:].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(OTHER_CASES))
def test_other_sizes_within_one_lsb_equal_away_from_ties(yard, dev, name):
    mode, _, _, crop = yard["cases"][name]
    _rules(dev[name], crop, _size(mode), yard["delta"][name], name)


def test_flip_equals_flipped_source(yard):
    for name in ("61x117", "250x233", "700x900"):
        mode, img, rect, _ = yard["cases"][name]
        flipped = torch.flip(img, dims=(1,)).contiguous()
        T = 1 if mode == MOUTH else 2                           # every slot named: the image once per slot
        a = _run([img], [_job(0, img, rect, 1, s) for s in range(T)], mode, 1, T)
        b = _run([flipped], [_job(0, flipped, rect, 0, s) for s in range(T)], mode, 1, T)
        assert torch.equal(a, b), name
        assert not torch.equal(a, _run([img], [_job(0, img, rect, 0, s) for s in range(T)], mode, 1, T)), name


def test_offset_rectangle_and_flip_then_crop():
    """x0 != 0 and an odd y0, at an exact ratio: bit for bit against the host path on the crop.  The flip bit mirrors the columns inside the rectangle; the
    reference's order - flip the whole image, then crop - is the mirrored rectangle with the bit set."""
    img = _image(400, 210, 203)
    rect = (7, 5, 192, 192)
    for flip in (False, True):
        got = _run([img], [_job(0, img, rect, flip, 0)], MOUTH, 1, 1)[0, 0]
        assert torch.equal(got, _host_u8(_crop(img, rect, flip), 96)), flip
    flipped = torch.flip(img, dims=(1,)).contiguous()
    mirrored = (rect[0], img.shape[1] - rect[1] - rect[3], rect[2], rect[3])
    assert torch.equal(_run([img], [_job(0, img, mirrored, 1, 0)], MOUTH, 1, 1)[0, 0], _host_u8(_crop(flipped, rect), 96))


def test_wide_rectangle_walks_the_band_two_rows_at_a_time():
    """3 840 columns: the staged rows of one output row pair fill the block's LDS, so a band is walked in groups of two rows; ratios 2 and 40, bit for bit,
    next to a narrow image in the same launch (the launch's LDS is sized by its widest rectangle)"""
    wide, narrow = _image(800, 384, 3840), _image(801, 384, 384)
    buf, offs, _ = _pack([wide, narrow])
    rect = _rect(MOUTH, 384, 3840)
    u = _run(None, [_job(offs[0], wide, rect, 1, 0), _job(offs[1], narrow, _rect(MOUTH, 384, 384), 0, 1)], MOUTH, 1, 2, buf=buf)[0]
    assert torch.equal(u[0], _host_u8(_crop(wide, rect, flip=True), 96))
    assert torch.equal(u[1], _host_u8(_crop(narrow, _rect(MOUTH, 384, 384)), 96))


def test_short_clip_empty_clip_and_88():
    """three clips of 3, 0 and 1 frames at T = 4 and the 88-pixel output (176 x 176 faces: ratios 1 and 2, bit for bit); unnamed slots are exact zeros"""
    from lip2speech_amd import native
    frames = [3, 0, 1]
    images = [_image(500 + i, 176, 176) for i in range(4)]
    buf, offs, _ = _pack(images)
    T, jobs, k = 4, [], 0
    for b, n in enumerate(frames):
        for t in range(n):
            jobs.append(_job(offs[k], images[k], _rect(MOUTH, 176, 176), 0, b * T + t))
            k += 1
    out = native.resize_normalise(buf.cuda(), jobs[::-1], MOUTH, 3, T, 88)            # the table's order is free
    torch.cuda.synchronize()
    assert out.shape == (3, 3, T, 88, 88)
    u = _recover(out.permute(0, 2, 1, 3, 4), MOUTH)
    k = 0
    for b, n in enumerate(frames):
        for t in range(n):
            assert torch.equal(u[b, t], _host_u8(_crop(images[k], _rect(MOUTH, 176, 176)), 88)), (b, t)
            k += 1
        assert torch.equal(out[b, :, n:], torch.zeros_like(out[b, :, n:])), b
    # a call with no job at all writes zeros everywhere
    none = native.resize_normalise(buf.cuda(), [], MOUTH, 1, 2, 88)
    torch.cuda.synchronize()
    assert torch.equal(none, torch.zeros_like(none))


def test_chunk_boundary_and_independence(yard):
    """one job more than a launch's table holds; a frame's bits are the same alone and as the last job of the larger call"""
    from lip2speech_amd import native
    n = native.RESIZE_JOBS_PER_LAUNCH + 1
    images = [_image(600 + i, 32 + i % 5, 16 + i % 7) for i in range(n)]
    buf, offs, _ = _pack(images)
    jobs = [_job(offs[i], images[i], _rect(MOUTH, *images[i].shape[:2]), i & 1, i) for i in range(n)]
    big = _run(None, jobs, MOUTH, 1, n, buf=buf)[0]
    for i in (0, native.RESIZE_JOBS_PER_LAUNCH - 1, n - 1):
        alone = _run([images[i]], [_job(0, images[i], _rect(MOUTH, *images[i].shape[:2]), i & 1, 0)], MOUTH, 1, 1)[0, 0]
        assert torch.equal(big[i], alone), i
    for i in range(n):
        d = (big[i].int() - _host_u8(_crop(images[i], _rect(MOUTH, *images[i].shape[:2]), flip=bool(i & 1)), 96).int()).abs()
        assert int(d.max()) <= 1, i


def test_guard_bytes_are_never_seen(yard):
    """0xFF in the 4-byte rounding gaps between images and in 64 bytes after the last one, inside a larger allocation: the outputs do not change"""
    from lip2speech_amd import native
    images = [_image(700 + i, H, W) for i, (H, W) in enumerate(((33, 17), (35, 19), (21, 23), (41, 17)))]        # every image's bytes are 3 mod 4 or 1 mod 4
    outs = []
    for fill in (0, 255):
        buf, offs, end = _pack(images, fill=fill, tail=64)
        assert end % 4 != 0 and buf.numel() == (end + 3) // 4 * 4 + 64
        alloc = torch.full((buf.numel() + 4096,), fill, dtype=torch.uint8)
        alloc[:buf.numel()] = buf
        alloc = alloc.cuda()
        mouth = [_job(offs[i], images[i], _rect(MOUTH, *images[i].shape[:2]), i & 1, i) for i in range(4)]
        face = [_job(offs[i], images[i], _rect(FACE, *images[i].shape[:2]), i & 1, i) for i in range(4)]
        for view in (alloc[:end], alloc[:buf.numel()]):                 # the buffer ends with the last image's last byte | after the guard bytes
            outs.append((native.resize_normalise(view, mouth, MOUTH, 1, 4), native.resize_normalise(view, face, FACE, 2)))
    torch.cuda.synchronize()
    for m, f in outs[1:]:
        assert torch.equal(m, outs[0][0]) and torch.equal(f, outs[0][1])


def test_end_to_end_packed_faces(yard):
    from lip2speech_amd import synth
    from lip2speech_amd.datasets import PackedFaces, faces_item_host, train_collate_fn_pad
    from model.model import get_network
    items = _e2e_items()
    packed = PackedFaces(items)
    video, crops = packed.to_device()
    torch.cuda.synchronize()
    host = [faces_item_host(*it) for it in items]
    (want_video, lengths), _, _, want_crops = train_collate_fn_pad(
        [(lo, torch.zeros(1, 600), torch.zeros(80, 3), fc) for lo, fc in host])
    assert lengths.tolist() == [7, 9] == packed.lengths.tolist()
    assert video.shape == want_video.shape == (2, 3, 9, 96, 96) and crops.shape == want_crops.shape == (2, 2, 3, 160, 160)
    assert torch.equal(video[0, :, 7:], torch.zeros_like(video[0, :, 7:]))
    u_video, u_crops = _recover(video.permute(0, 2, 1, 3, 4), MOUTH), _recover(crops, FACE)
    h_video, h_crops = _recover(want_video.permute(0, 2, 1, 3, 4), MOUTH), _recover(want_crops, FACE)
    from lip2speech_amd.datasets.device import _chw
    for b, (faces, flip, idx) in enumerate(items):
        for t, f in enumerate(faces):
            f = torch.flip(_chw(f), dims=(-1,)) if flip else _chw(f)
            assert torch.equal(h_video[b, t], _host_u8(f[:, f.shape[1] // 2:], 96))            # the collate carries the host path's uint8 unchanged
            _rules(u_video[b, t], f[:, f.shape[1] // 2:], 96, yard["delta"][f"item {b} face {t}"], f"item {b} face {t}")
        for k, i in enumerate(idx):
            f = torch.flip(_chw(faces[i]), dims=(-1,)) if flip else _chw(faces[i])
            assert torch.equal(h_crops[b, k], _host_u8(f, 160))
            _rules(u_crops[b, k], f, 160, yard["delta"][f"item {b} face {i} whole"], f"item {b} face {i} whole")
    # the model takes both as they stand
    net = get_network("test")
    net.load_state_dict({**synth.synth_state_dict(), **synth.synth_face_state_dict()}, strict=True)
    net = net.cuda().eval()
    emb = net.vgg_face.inference(crops[:, 0])
    mel, out_len = net.inference(video, crops, video_lengths=packed.lengths.tolist())
    torch.cuda.synchronize()
    assert emb.shape == (2, 256) and bool(torch.isfinite(emb).all())
    assert mel.shape[:2] == (2, 80) and bool(torch.isfinite(mel).all()) and out_len.shape == (2,)
