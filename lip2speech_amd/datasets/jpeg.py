"""Baseline JPEG decoding restated on the host: the checker of `l2s_jpeg_decode` (csrc/jpeg_decode.hip).

LRW's `*_mouth.npz` / `*_face.npz` and the in-the-wild loader's `*_face.npz` hold JPEG byte strings as `cv2.imencode` writes them: baseline sequential
(SOF0), 8-bit, YCbCr 4:2:0, one interleaved scan.  libjpeg's default decoder is integer arithmetic throughout - the `jidctint` "islow" IDCT, triangle ("fancy")
chroma upsampling, fixed-point YCbCr -> RGB - so it can be restated exactly.  Pillow (libjpeg-turbo) is the authority for this restatement
(tests/test_jpeg_decode_host.py, tests/golden/make_jpeg_cases.py: equal bit for bit); this restatement is the authority for the kernel
(tests/test_jpeg_decode_gpu.py: equal bit for bit).  Parity with cv2.imdecode stays UNPINNED (OpenCV is absent from the build image; it links a libjpeg of its own
build).

`parse_jpeg` reads the headers and refuses, by name, what the device path does not decode; `l2s_jpeg_plan` refuses the same streams with the same reasons.
`decode_jpeg_host` is numpy except for the bit reader, whose loop is one Python iteration per Huffman symbol.

Where libjpeg's C path and its SIMD paths differ - IDCT outputs further than 512 from the centre wrap through the C path's range-limit table and saturate in the
SIMD paths - no encoder-made stream gets there; this restatement (and the kernel) saturate, and no fixture case tells the two apart.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

MAX_DIM = 4096
# natural (row-major) position of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36,
                   29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)
LAYOUT_GREY, LAYOUT_444, LAYOUT_420 = 0, 1, 2


class JpegError(ValueError):
    """a stream outside the supported subset; the message is the reason"""


@dataclass
class JpegComponent:
    id: int
    h: int
    v: int
    tq: int
    td: int = 0
    ta: int = 0


@dataclass
class JpegHeader:
    H: int
    W: int
    components: List[JpegComponent]
    qtables: Dict[int, np.ndarray]                              # id -> 64 uint16 in zigzag order, as the stream holds them
    htables: Dict[Tuple[int, int], Tuple[np.ndarray, np.ndarray]]      # (class 0 DC / 1 AC, id) -> (16 counts, values)
    restart_interval: int
    scan_offset: int                                            # the entropy-coded segment: first byte after the SOS header ..
    scan_length: int                                            # .. up to the marker that ends it
    eoi: bool                                                   # that marker is EOI (False: the stream stops short)
    layout: int = field(default=LAYOUT_420)

    @property
    def mcu(self) -> Tuple[int, int]:
        """(height, width) of an MCU in pixels"""
        s = 16 if self.layout == LAYOUT_420 else 8
        return s, s

    @property
    def mcus(self) -> Tuple[int, int]:
        mh, mw = self.mcu
        return (self.H + mh - 1) // mh, (self.W + mw - 1) // mw

    def plane_blocks(self, c: int) -> Tuple[int, int]:
        """(block rows, block columns) of component c's plane, whole MCUs"""
        my, mx = self.mcus
        k = 2 if (self.layout == LAYOUT_420 and c == 0) else 1
        return my * k, mx * k

    @property
    def n_blocks(self) -> int:
        return sum(int(np.prod(self.plane_blocks(c))) for c in range(len(self.components)))


_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding (SOF10)",
              0xCB: "arithmetic coding (SOF11)", 0xCD: "arithmetic coding (SOF13)", 0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}


def _bytes(data) -> bytes:
    return data if isinstance(data, (bytes, bytearray)) else np.asarray(data, dtype=np.uint8).tobytes()


def parse_jpeg(data) -> JpegHeader:
    """The headers of one JPEG stream (bytes or a 1-D uint8 array).  Raises `JpegError` with the reason for a stream outside the supported subset: SOF0 only,
    8-bit samples and quantisation tables, one interleaved scan of one component (grey) or three (YCbCr, sampling 2x2 / 1x1 / 1x1 or all 1x1), H and W in
    [1, 4096]."""
    d = _bytes(data)
    n = len(d)
    past = JpegError("a header runs past the stream")
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise JpegError("no SOI marker at the start of the stream")
    p = 2
    qtables, htables, comps = {}, {}, None
    H = W = restart = 0
    adobe = None
    while True:
        if p + 2 > n:
            raise past
        if d[p] != 0xFF:
            raise JpegError(f"no marker at byte {p}")
        m = d[p + 1]
        if m == 0xFF:                      # a fill byte
            p += 1
            continue
        p += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise JpegError("EOI before any scan")
        if p + 2 > n:
            raise past
        L = (d[p] << 8) | d[p + 1]
        if L < 2 or p + L > n:
            raise past
        seg = d[p + 2:p + L]
        if m in _SOF_NAMES:
            raise JpegError(_SOF_NAMES[m] + " is not supported: baseline sequential (SOF0) only")
        if m == 0xC0:
            if comps is not None:
                raise JpegError("more than one frame header")
            if len(seg) < 6:
                raise past
            if seg[0] != 8:
                raise JpegError(f"{seg[0]}-bit samples are not supported: 8-bit only")
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if H == 0:
                raise JpegError("the frame header leaves the height to a DNL marker: not supported")
            if nc == 4:
                raise JpegError("four components (CMYK / YCCK) are not supported")
            if nc not in (1, 3):
                raise JpegError(f"{nc} components are not supported: one (grey) or three (YCbCr)")
            if len(seg) < 6 + 3 * nc:
                raise past
            if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
                raise JpegError(f"image {H} x {W} is outside [1, 4096] x [1, 4096]")
            comps = [JpegComponent(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq != 0:
                    raise JpegError("16-bit quantisation tables are not supported: 8-bit only")
                if tq > 3:
                    raise JpegError(f"quantisation table id {tq} is outside [0, 3]")
                if q + 65 > len(seg):
                    raise past
                qtables[tq] = np.frombuffer(seg[q + 1:q + 65], dtype=np.uint8).astype(np.uint16)
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                tc, th = seg[q] >> 4, seg[q] & 15
                if tc > 1 or th > 1:
                    raise JpegError(f"Huffman table class {tc} id {th}: baseline has classes 0 / 1 and ids 0 / 1")
                if q + 17 > len(seg):
                    raise past
                counts = np.frombuffer(seg[q + 1:q + 17], dtype=np.uint8).astype(np.int64)
                nv = int(counts.sum())
                if nv > 256 or q + 17 + nv > len(seg):
                    raise past if nv <= 256 else JpegError("a Huffman table holds more than 256 codes")
                vals = np.frombuffer(seg[q + 17:q + 17 + nv], dtype=np.uint8).astype(np.int64)
                code = 0
                for l in range(16):
                    code += int(counts[l])
                    if code > (2 << l):
                        raise JpegError("a Huffman table assigns more codes than its lengths allow")
                    code <<= 1
                if tc == 0 and nv and int(vals.max()) > 15:
                    raise JpegError("a DC Huffman table names a category above 15")
                htables[(tc, th)] = (counts, vals)
                q += 17 + nv
        elif m == 0xDD:
            if len(seg) < 2:
                raise past
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xDC:
            raise JpegError("a DNL marker is not supported")
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDA:
            break
        p += L
    # p: the SOS segment's length field
    if comps is None:
        raise JpegError("a scan before the frame header")
    ns = seg[0] if len(seg) >= 1 else 0
    if len(seg) < 1 + 2 * ns + 3:
        raise past
    if ns != len(comps):
        raise JpegError(f"the scan holds {ns} of the frame's {len(comps)} components: more than one scan is not supported")
    for i, c in enumerate(comps):
        if seg[1 + 2 * i] != c.id:
            raise JpegError("the scan's components are not the frame's, in order")
        c.td, c.ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
    ss, se, ahal = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]
    if (ss, se, ahal) != (0, 63, 0):
        raise JpegError("the scan is not a whole sequential one (Ss, Se, Ah / Al = 0, 63, 0)")
    if len(comps) == 3:
        if adobe == 0 or [c.id for c in comps] == [ord("R"), ord("G"), ord("B")]:
            raise JpegError("RGB-coded components (Adobe transform 0, or component ids R, G, B) are not supported: YCbCr only")
        samp = [(c.h, c.v) for c in comps]
        if samp == [(2, 2), (1, 1), (1, 1)]:
            layout = LAYOUT_420
        elif samp == [(1, 1), (1, 1), (1, 1)]:
            layout = LAYOUT_444
        else:
            raise JpegError("sampling factors " + " / ".join(f"{h}x{v}" for h, v in samp) + " are not supported: 2x2 / 1x1 / 1x1 (4:2:0) or all 1x1 (4:4:4)")
    else:
        layout = LAYOUT_GREY                # a single component's sampling factors do not matter: its scan is not interleaved
    for c in comps:
        if c.tq not in qtables:
            raise JpegError(f"component {c.id} names quantisation table {c.tq}, which was never defined")
        if c.td > 1 or c.ta > 1 or (0, c.td) not in htables or (1, c.ta) not in htables:
            raise JpegError(f"the scan names Huffman table DC {c.td} / AC {c.ta} for component {c.id}, which was never defined")
    s0 = p + L
    q = s0
    eoi = False
    while True:                            # the entropy-coded segment ends at the first marker that is neither a stuffed FF 00 nor RSTn
        q = d.find(b"\xff", q)
        if q < 0 or q + 1 >= n:
            q = n if q < 0 else q
            break
        m = d[q + 1]
        if m == 0 or 0xD0 <= m <= 0xD7:
            q += 2
            continue
        if m == 0xD9:
            eoi = True
        elif m == 0xDC:
            raise JpegError("a DNL marker is not supported")
        elif m == 0xDA or m == 0xC4 or m == 0xDB or (0xC0 <= m <= 0xCF and m != 0xC8):
            raise JpegError("more than one scan is not supported")
        break
    return JpegHeader(H=H, W=W, components=comps, qtables=qtables, htables=htables, restart_interval=restart, scan_offset=s0, scan_length=q - s0, eoi=eoi,
                      layout=layout)


# ---- entropy decoding ---------------------------------------------------------------------------------------------------------------------------------------------

_lut_cache: Dict[bytes, Tuple[list, list]] = {}


def _huff_lut(counts: np.ndarray, vals: np.ndarray) -> Tuple[list, list]:
    """16-bit window -> (code length, 0 where no code starts the window; symbol)"""
    key = counts.tobytes() + vals.tobytes()
    if key not in _lut_cache:
        length, sym = np.zeros(65536, dtype=np.int64), np.zeros(65536, dtype=np.int64)
        code, k = 0, 0
        for l in range(1, 17):
            for _ in range(int(counts[l - 1])):
                length[code << (16 - l):(code + 1) << (16 - l)] = l
                sym[code << (16 - l):(code + 1) << (16 - l)] = vals[k]
                code, k = code + 1, k + 1
            code <<= 1
        _lut_cache[key] = (length.tolist(), sym.tolist())
    return _lut_cache[key]


def _windows(seg: bytes) -> Tuple[list, int]:
    """a restart interval's bytes, FF 00 unstuffed -> (the 16-bit window at every bit position, zeros past the end; its number of bits)"""
    a = np.frombuffer(seg, dtype=np.uint8)
    if a.size:
        keep = np.ones(a.size, dtype=bool)
        keep[1:] = ~((a[:-1] == 0xFF) & (a[1:] == 0))
        a = a[keep]
    bits = np.concatenate([np.unpackbits(a), np.zeros(64, dtype=np.uint8)]).astype(np.int64)
    nb = a.size * 8
    win = np.zeros(nb + 32, dtype=np.int64)
    for j in range(16):
        win += bits[j:j + nb + 32] << (15 - j)
    return win.tolist(), nb


def _block_order(h: JpegHeader):
    """per MCU, the (component, block row offset, block column offset) of its blocks in scan order"""
    if h.layout == LAYOUT_420:
        return [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)], 2
    return [(c, 0, 0) for c in range(len(h.components))], 1


def entropy_decode_host(data, header: JpegHeader = None) -> List[np.ndarray]:
    """-> per component the quantised coefficients `(block rows, block columns, 64)` int16 in natural order, planes of whole MCUs: what the entropy kernel
    writes to the workspace, component after component.  Raises `JpegError` on a stream that does not decode cleanly."""
    d = _bytes(data)
    h = header or parse_jpeg(d)
    if not h.eoi:
        raise JpegError("premature end of data: no EOI after the scan")
    scan = d[h.scan_offset:h.scan_offset + h.scan_length]
    planes = [np.zeros(h.plane_blocks(c) + (64,), dtype=np.int64) for c in range(len(h.components))]
    luts = [(_huff_lut(*h.htables[(0, c.td)]), _huff_lut(*h.htables[(1, c.ta)])) for c in h.components]
    order, ky = _block_order(h)
    my, mx = h.mcus
    n_mcu, ri = my * mx, h.restart_interval
    # the restart intervals: split at the RSTn markers, which must count up from 0 modulo 8
    segs, q, start, k = [], 0, 0, 0
    while True:
        q = scan.find(b"\xff", q)
        if q < 0 or q + 1 >= len(scan):
            break
        if 0xD0 <= scan[q + 1] <= 0xD7:
            if ri == 0 or scan[q + 1] != 0xD0 + (k & 7):
                raise JpegError("a wrong restart marker")
            segs.append(scan[start:q])
            q, start, k = q + 2, q + 2, k + 1
        else:
            q += 2
    segs.append(scan[start:])
    if len(segs) != ((n_mcu + ri - 1) // ri if ri else 1):
        raise JpegError("a missing restart marker")
    zz = ZIGZAG.tolist()
    mcu = 0
    for seg in segs:
        win, nb = _windows(seg)
        p = 0
        pred = [0, 0, 0]
        for _ in range(min(ri, n_mcu - mcu) if ri else n_mcu):
            y0, x0 = divmod(mcu, mx)
            for c, dy, dx in order:
                (dlen, dsym), (alen, asym) = luts[c]
                blk = planes[c][(y0 * ky + dy) if c == 0 else y0, (x0 * ky + dx) if c == 0 else x0]
                if p > nb:
                    raise JpegError("premature end of data")
                w = win[p]
                l = dlen[w]
                if l == 0:
                    raise JpegError("an invalid Huffman code")
                s = dsym[w]
                p += l
                if s:
                    v = win[p] >> (16 - s)
                    p += s
                    pred[c] += v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    if p > nb:
                        raise JpegError("premature end of data")
                    w = win[p]
                    l = alen[w]
                    if l == 0:
                        raise JpegError("an invalid Huffman code")
                    rs = asym[w]
                    p += l
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    if k > 63:
                        raise JpegError("a coefficient run past the end of its block")
                    v = win[p] >> (16 - s)
                    p += s
                    blk[zz[k]] = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                    k += 1
            mcu += 1
        if p > nb:
            raise JpegError("premature end of data")
        if p + 8 <= nb:
            raise JpegError("data left over after the last block")
    return [pl.astype(np.int16) for pl in planes]


# ---- reconstruction -----------------------------------------------------------------------------------------------------------------------------------------------

def _fix(x: float) -> int:
    return int(x * 8192 + 0.5)


def _idct_pass(v: List[np.ndarray], d: int) -> List[np.ndarray]:
    """one 1-D pass of libjpeg's jidctint (CONST_BITS 13) over v[0..7], descaled by d bits; int32 arithmetic, arithmetic shifts"""
    i32 = np.int32
    z1 = (v[2] + v[6]) * i32(_fix(0.541196100))
    t2 = z1 - v[6] * i32(_fix(1.847759065))
    t3 = z1 + v[2] * i32(_fix(0.765366865))
    t0 = (v[0] + v[4]) << 13
    t1 = (v[0] - v[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * i32(_fix(1.175875602))
    a0, a1, a2, a3 = a0 * i32(_fix(0.298631336)), a1 * i32(_fix(2.053119869)), a2 * i32(_fix(3.072711026)), a3 * i32(_fix(1.501321110))
    z1, z2 = z1 * i32(-_fix(0.899976223)), z2 * i32(-_fix(2.562915447))
    z3, z4 = z3 * i32(-_fix(1.961570560)) + z5, z4 * i32(-_fix(0.390180644)) + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    r = i32(1 << (d - 1))
    return [(x + r) >> d for x in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)]


def idct_plane(coefs: np.ndarray, qt_zigzag: np.ndarray) -> np.ndarray:
    """quantised coefficients `(bh, bw, 64)` (natural order) and the 64 quantisers in zigzag order -> the uint8 sample plane `(8 bh, 8 bw)`"""
    q = np.zeros(64, dtype=np.int32)
    q[ZIGZAG] = qt_zigzag.astype(np.int32)
    bh, bw = coefs.shape[:2]
    with np.errstate(over="ignore"):
        x = (coefs.astype(np.int32) * q).reshape(bh, bw, 8, 8)
        cols = _idct_pass([x[:, :, i, :] for i in range(8)], 11)             # columns first: v[i] = row i, all columns at once
        ws = np.stack(cols, axis=2)                                          # (bh, bw, 8 rows, 8 columns)
        rows = _idct_pass([ws[:, :, :, j] for j in range(8)], 18)           # then rows
        out = np.stack(rows, axis=3) + np.int32(128)
    return np.clip(out, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v2(p: np.ndarray, H: int, W: int) -> np.ndarray:
    """libjpeg's h2v2_fancy_upsample on the `ceil(H/2) x ceil(W/2)` real chroma samples of plane p, edge rows replicated -> `(H, W)` int32"""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    p = p[:ch, :cw].astype(np.int32)
    up, down = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    cs = np.empty((2 * ch, cw), dtype=np.int32)
    cs[0::2], cs[1::2] = 3 * p + up, 3 * p + down
    left, right = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1), np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int32)
    out[:, 0::2], out[:, 1::2] = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4      # at the edges 3 cs + cs = 4 cs: the first- and last-column rules
    return out[:H, :W]


def _fx(x: float) -> int:
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray) -> np.ndarray:
    """libjpeg's jdcolor on int32 planes -> uint8 `(H, W, 3)`"""
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((_fx(1.40200) * cr + 32768) >> 16)
    b = y + ((_fx(1.77200) * cb + 32768) >> 16)
    g = y + ((-_fx(0.34414) * cb + 32768 - _fx(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode_jpeg_host(data) -> np.ndarray:
    """One baseline JPEG stream -> uint8 `(H, W, 3)` RGB, the bits Pillow / libjpeg-turbo give (grey: R = G = B)."""
    d = _bytes(data)
    h = parse_jpeg(d)
    coefs = entropy_decode_host(d, h)
    planes = [idct_plane(coefs[c], h.qtables[comp.tq]) for c, comp in enumerate(h.components)]
    H, W = h.H, h.W
    if h.layout == LAYOUT_GREY:
        return np.repeat(planes[0][:H, :W, None], 3, axis=2)
    if h.layout == LAYOUT_420:
        cb, cr = upsample_h2v2(planes[1], H, W), upsample_h2v2(planes[2], H, W)
    else:
        cb, cr = planes[1][:H, :W], planes[2][:H, :W]
    return ycc_to_rgb(planes[0][:H, :W], cb, cr)
