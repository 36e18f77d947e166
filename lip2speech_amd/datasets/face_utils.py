"""Face alignment of the GRID / AVSpeech / in-the-wild loaders (reference: datasets/face_utils.py:12-103, called per frame at
datasets/grid/dataset.py:216, avspeech/dataset.py:241 and in the wild loader): the face box is cut out of the frame and the cut is rotated about its
centre by the angle of the eye line, with `cv2.getRotationMatrix2D` and `cv2.warpAffine`.

OpenCV is absent from the build image.  What is implemented is the algorithm as restated here - the fixed-point bilinear path of OpenCV 4.x's
generic `warpAffine` (INTER_LINEAR, constant border 0; not its IPP or OpenCL path) - PARITY UNPINNED against the package, like the resize
(`lrw.face_recog_resize`), the mel transform and the vocoder.  The device kernel (`l2s_align_faces`, csrc/face_align.hip) is tested bit for bit
against `warp_affine_u8`, and `warp_affine_u8` against a per-pixel restatement and closed forms (tests/test_face_align_host.py).

  eye angle    the integer bounding boxes of landmark slices [36:42] and [42:48] (x = min, w = max - min + 1), their mid points
               (x + w // 2, y + h // 2), angle = arctan(dy / dx) 180 / pi in float64, 0 where dx == 0
  forward map  getRotationMatrix2D((w // 2, h // 2), angle, 1): a = cos, b = sin of the angle in radians,
               M = [a, b, (1 - a) cx - b cy, -b, a, b cx + (1 - a) cy]
  inverse map  as warpAffine inverts it: D = 1 / (M0 M4 - M1 M3) (0 if the determinant is 0), m0 = M4 D, m1 = M1 (-D), m3 = M3 (-D), m4 = M0 D,
               m2 = -m0 M2 - m1 M5, m5 = -m3 M2 - m4 M5
  per pixel    ad = rn(m0 x 1024), bd = rn(m3 x 1024), X0 = rn((m1 y + m2) 1024) + 16, Y0 = rn((m4 y + m5) 1024) + 16 (rn: float64 to the nearest
               integer, ties to even); X = (X0 + ad) >> 5, Y = (Y0 + bd) >> 5; sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31; the four taps
               weighted 32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy (sum 32768), a tap outside the image counting 0,
               out = (sum + 16384) >> 15.  Everything after the four rn is integer arithmetic.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

EYE1, EYE2 = slice(36, 42), slice(42, 48)      # the two eyes of the 68-point landmark set
MIN_FACE = 16                                   # a face under 16 x 16 makes the reference's loaders draw another item (`reset_item`)


def _roi_mid_point(points: np.ndarray) -> Tuple[int, int]:
    """`cv2.boundingRect` of integer points (x = min, w = max - min + 1) and the mid point the reference takes of it"""
    x, y = int(points[:, 0].min()), int(points[:, 1].min())
    w, h = int(points[:, 0].max()) - x + 1, int(points[:, 1].max()) - y + 1
    return x + w // 2, y + h // 2


def eye_angle_degrees(landmarks) -> float:
    """The angle of the eye line in degrees (reference lines 23-42).  `landmarks`: the 68 integer points the preprocessing stores
    (`astype(np.int32).tolist()`); only differences enter, so their coordinate frame does not matter."""
    lm = np.asarray(landmarks)
    assert lm.ndim == 2 and lm.shape[0] >= 48 and lm.shape[1] == 2, "landmarks are (68, 2) points"
    assert np.issubdtype(lm.dtype, np.integer) or np.all(lm == np.rint(lm)), "landmarks are integer points"
    lm = lm.astype(np.int64)
    x1, y1 = _roi_mid_point(lm[EYE1])
    x2, y2 = _roi_mid_point(lm[EYE2])
    dx, dy = x2 - x1, y2 - y1
    if dx == 0:
        return 0.0
    return float((np.arctan(dy / dx) * 180) / np.pi)


def rotation_inverse_map(angle_deg: float, h: int, w: int) -> List[float]:
    """The six float64 of the destination-to-source map `warpAffine` applies for `getRotationMatrix2D((w // 2, h // 2), angle_deg, 1.0)` on an
    `h x w` image: source x = m0 x + m1 y + m2, source y = m3 x + m4 y + m5."""
    cx, cy = float(int(w) // 2), float(int(h) // 2)
    rad = float(angle_deg) * math.pi / 180.0
    a, b = math.cos(rad), math.sin(rad)
    M = [a, b, (1.0 - a) * cx - b * cy, -b, a, b * cx + (1.0 - a) * cy]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0.0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    m0, m1, m3, m4 = A11, M[1] * (-D), M[3] * (-D), A22
    m2 = -m0 * M[2] - m1 * M[5]
    m5 = -m3 * M[2] - m4 * M[5]
    return [m0, m1, m2, m3, m4, m5]


def warp_affine_u8(img_hwc, inverse_map) -> np.ndarray:
    """`cv2.warpAffine(img, M, (w, h))` as restated above, vectorised: uint8 `(H,W,C)` and the inverse map of M -> uint8 `(H,W,C)`."""
    img = np.ascontiguousarray(img_hwc)
    assert img.dtype == np.uint8 and img.ndim == 3, "an image is uint8 (H,W,C)"
    H, W = img.shape[:2]
    m = [float(v) for v in inverse_map]
    assert len(m) == 6 and all(math.isfinite(v) for v in m), "the inverse map is six finite numbers"
    if H == 0 or W == 0:
        return img.copy()
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    ad, bd = np.rint(m[0] * x * 1024.0).astype(np.int64), np.rint(m[3] * x * 1024.0).astype(np.int64)
    X0, Y0 = np.rint((m[1] * y + m[2]) * 1024.0).astype(np.int64) + 16, np.rint((m[4] * y + m[5]) * 1024.0).astype(np.int64) + 16
    X, Y = (X0[:, None] + ad[None, :]) >> 5, (Y0[:, None] + bd[None, :]) >> 5
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    src = img.astype(np.int64)

    def tap(yy, xx):           # constant border 0
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * inside[..., None]

    acc = ((32 * (32 - fx) * (32 - fy))[..., None] * tap(sy, sx) + (32 * fx * (32 - fy))[..., None] * tap(sy, sx + 1)
           + (32 * (32 - fx) * fy)[..., None] * tap(sy + 1, sx) + (32 * fx * fy)[..., None] * tap(sy + 1, sx + 1))
    return ((acc + 16384) >> 15).astype(np.uint8)


def align_and_crop_face(frame: torch.Tensor, face_coords, landmarks) -> torch.Tensor:
    """The reference's `align_and_crop_face` (datasets/face_utils.py:100-103): a uint8 `(3,H,W)` frame, the face box `(x1, y1, x2, y2)` and the frame's
    landmarks -> the box cut out and rotated about its centre by the eye angle, uint8 `(3,h,w)`."""
    frame = torch.as_tensor(frame)
    assert frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[0] == 3, "a frame is uint8 (3,H,W)"
    x1, y1, x2, y2 = (int(v) for v in face_coords)
    img = frame[:, y1:y2, x1:x2].permute(1, 2, 0).contiguous().numpy()
    h, w = img.shape[:2]
    rotated = warp_affine_u8(img, rotation_inverse_map(eye_angle_degrees(landmarks), h, w))
    return torch.from_numpy(rotated).permute(2, 0, 1)


def face_box_crops(frames: torch.Tensor, face_coords: Sequence, landmarks: Sequence) -> Optional[Tuple[List[torch.Tensor], List]]:
    """The loop of `GRID.__getitem__` (datasets/grid/dataset.py:206-220) without the rotation: uint8 frames `(N,3,H,W)` and, per frame, its face box
    `(x1, y1, x2, y2)` and its landmarks from the preprocessing JSON (`None` for a frame without an entry, which is skipped; negative
    coordinates are clamped to 0) -> `(crops, landmarks)`: the UNROTATED face-box crops, uint8 `(3,h_i,w_i)`, and the landmarks of the same frames
    - the first and last elements of a 4-tuple item of `PackedFaces`, which rotates them on the device (what `align_and_crop_face` does per frame on
    the host).  `None`: the item is unusable - a face under 16 x 16 or no face at all - where the reference's loaders call `reset_item`."""
    frames = torch.as_tensor(frames)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[1] == 3, "frames are uint8 (N,3,H,W)"
    assert len(face_coords) == frames.shape[0] and len(landmarks) == frames.shape[0], "one face box and one landmark set (or None) per frame"
    crops, kept = [], []
    for idx in range(frames.shape[0]):
        if face_coords[idx] is None or landmarks[idx] is None:
            continue
        x1, y1, x2, y2 = (max(int(v), 0) for v in face_coords[idx])
        face = frames[idx, :, y1:y2, x1:x2]
        if face.shape[1] < MIN_FACE or face.shape[2] < MIN_FACE:
            return None
        crops.append(face)
        kept.append(landmarks[idx])
    return (crops, kept) if crops else None
