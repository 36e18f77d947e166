"""Device-side half of the data boundary (reference: datasets/lrw/dataset.py:83-86,123-146 and
datasets/__init__.py:7-46).

The reference normalises every decoded frame to fp32 on the CPU and its collate zero-pads and permutes the clips into the
`(B,3,T,96,96)` batch - 102.6 MB per B=32 LRW batch assembled by the host and copied over PCIe.  Here the loader hands over the decoded
uint8 frames (`LRW(..., raw_frames=True)`), `device_collate_fn_pad` packs them back to back into ONE pinned buffer (25.7 MB) next to the
usual audio / mel / gate padding, and `PackedFrames.to_device()` runs `l2s_normalise_pad_frames`: the same three fp32 operations per value
(`/255`, `- mean`, `/ std`), the zero padding and the layout change in one kernel - bit-identical to `train_collate_fn_pad` on the
normalised clips (tests/test_data_boundary.py, tests/test_gpu_parity.py).

The audio half has the same shape: `LRW(..., raw_audio=True)` skips the CPU mel transform, `device_collate_fn_pad_raw` packs the waveforms
into one pinned fp32 buffer (`PackedAudio`) and `PackedAudio.to_device()` runs `l2s_mel_targets` - log-mel targets, gates, lengths and the
zero-padded audio from one launch chain.  The audio, the gates and the lengths are exactly the host collate's; the mels are another order of
the same fp32 sums than `torch.stft` + matmul, inside 8x the fp32 torch path's own error against fp64 (tests/test_mel_targets_gpu.py).

The face crops of the loaders whose faces have no common size (reference: datasets/grid/dataset.py:216-236 and its avspeech / wild twins):
an item is the list of a clip's aligned uint8 faces, the flip decision and the two drawn face indices; `PackedFaces` packs the images once
into one pinned buffer and `PackedFaces.to_device()` runs `l2s_resize_normalise` twice on the one upload - the lower half of every face to the
`(B,3,T,96,96)` video, the two drawn faces whole to the `(B,2,3,160,160)` face crops.  `faces_item_host` is the same tail in torch on the
CPU: what a loader without the device does, and what the kernel is tested against (tests/test_frame_resize_gpu.py).

The step before those crops, the rotation of every face-box crop by its eye-line angle (reference: datasets/face_utils.py:12-103): an item that comes as
`(crops, flip, face_indices, landmarks)` is rotated on the device, by one `l2s_align_faces` call on the same upload before the two resize calls -
bit-identical to rotating the crops on the host with `face_utils.align_and_crop_face` (tests/test_face_align_gpu.py).

The step before all of these for the loaders that store JPEG byte strings (reference: datasets/lrw/dataset.py:62-70 and the in-the-wild loader): with
`LRW(..., raw_jpeg=True)` nothing is decoded on the host; `device_collate_fn_pad_jpeg` packs the COMPRESSED strings into one pinned buffer (about 1.7 KB per
mouth frame instead of 27.6 KB), `PackedJpegFrames.to_device()` uploads it and runs `l2s_jpeg_decode` into a device buffer in `PackedFrames`' layout, then
`l2s_normalise_pad_frames` - bit-identical to `PackedFrames` on the frames `datasets.jpeg.decode_jpeg_host` (Pillow's bits) decodes
(tests/test_jpeg_decode_gpu.py).  `PackedFaces` takes faces that are JPEG strings the same way.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import native
from .face_utils import eye_angle_degrees, rotation_inverse_map


class PackedFrames:
    """B clips of uint8 RGB frames `(T_b,H,W,3)` packed back to back (4-byte aligned) in one host buffer."""

    def __init__(self, clips: Sequence[torch.Tensor], pin: bool = True):
        assert len(clips) > 0 and all(c.dtype == torch.uint8 and c.dim() == 4 and c.shape[3] == 3 for c in clips), "clips are uint8 (T,H,W,3)"
        self.H, self.W = int(clips[0].shape[1]), int(clips[0].shape[2])
        assert all(c.shape[1:3] == clips[0].shape[1:3] for c in clips), "one crop size per batch"
        self.frames: List[int] = [int(c.shape[0]) for c in clips]
        self.offsets: List[int] = []
        total = 0
        for c in clips:
            self.offsets.append(total)
            total += (c.numel() + 3) // 4 * 4
        buf = torch.empty(total, dtype=torch.uint8)
        if pin and torch.cuda.is_available():
            buf = buf.pin_memory()
        for c, o in zip(clips, self.offsets):
            buf[o:o + c.numel()] = c.reshape(-1)
        self.data = buf

    @property
    def lengths(self) -> torch.Tensor:
        return torch.tensor(self.frames)

    def to_device(self, device="cuda", T: int = None) -> torch.Tensor:
        """-> `(B,3,T,H,W)` fp32 on the device, normalised and zero-padded (T defaults to the longest clip)."""
        dev = self.data.to(device, non_blocking=True)
        return native.normalise_pad_frames(dev, self.offsets, self.frames, self.H, self.W, T)


def _jpeg_string(x):
    """a JPEG stream as a 1-D uint8 numpy array, or None if x is not one: bytes, bytearray, or a uint8 array / tensor of shape (n,) or - what cv2.imencode
    returns and the corpus files hold - (n, 1)"""
    if isinstance(x, (bytes, bytearray)):
        return np.frombuffer(x, dtype=np.uint8)
    if isinstance(x, torch.Tensor):
        x = x.numpy() if x.dtype == torch.uint8 and not x.is_cuda else None
    if isinstance(x, np.ndarray) and x.dtype == np.uint8 and (x.ndim == 1 or (x.ndim == 2 and x.shape[1] == 1)):
        return np.ascontiguousarray(x).reshape(-1)
    return None


def _pack_streams(strings, pin: bool):
    """JPEG streams -> (one host buffer that holds them back to back, exactly as they are; their offsets; their sizes)"""
    sizes = [int(s.size) for s in strings]
    offsets = [0] * len(sizes)
    for i in range(1, len(sizes)):
        offsets[i] = offsets[i - 1] + sizes[i - 1]
    buf = torch.empty(sum(sizes), dtype=torch.uint8)
    if pin and torch.cuda.is_available():
        buf = buf.pin_memory()
    view = buf.numpy()
    for s, o, n in zip(strings, offsets, sizes):
        view[o:o + n] = s
    return buf, offsets, sizes


class PackedJpegFrames:
    """B clips of JPEG byte strings (bytes or 1-D uint8 arrays; one frame size per batch, H W a multiple of 4 so that a clip's decoded frames follow one
    another on 4-byte boundaries) packed back to back, COMPRESSED, in one host buffer, and planned once (`native.jpeg_plan`: headers, table sets; a stream
    outside the supported subset raises here, with its index).  `offsets` / `frames` / `H` / `W` are those of `PackedFrames` on the decoded clips;
    `image_offsets`: every frame's offset in that layout."""

    def __init__(self, clips: Sequence, pin: bool = True):
        assert len(clips) > 0, "at least one clip"
        strings = [_jpeg_string(s) for c in clips for s in c]
        assert all(s is not None for s in strings), "a frame is a JPEG byte string: bytes or a 1-D uint8 array"
        assert len(strings) > 0, "at least one frame"
        self.frames: List[int] = [len(c) for c in clips]
        self.data, self.stream_offsets, self.stream_sizes = _pack_streams(strings, pin)
        self.plan = native.jpeg_plan(self.data, self.stream_offsets, self.stream_sizes)
        self.H, self.W = self.plan.sizes[0]
        assert all(hw == (self.H, self.W) for hw in self.plan.sizes), "one crop size per batch"
        assert (self.H * self.W) % 4 == 0, "H W must be a multiple of 4: a clip's frames follow one another without gaps, each on a 4-byte boundary"
        frame_bytes = self.H * self.W * 3
        self.offsets: List[int] = []
        self.image_offsets: List[int] = []
        total = 0
        for n in self.frames:
            self.offsets.append(total)
            self.image_offsets.extend(total + t * frame_bytes for t in range(n))
            total += n * frame_bytes
        self.packed_bytes = total

    @property
    def lengths(self) -> torch.Tensor:
        return torch.tensor(self.frames)

    def decode(self, device="cuda") -> torch.Tensor:
        """-> the decoded clips on the device, the bytes of `PackedFrames(decoded clips).data`: ONE upload of the compressed bytes, one `l2s_jpeg_decode`"""
        dev = self.data.to(device, non_blocking=True)
        return native.jpeg_decode(dev, self.plan, self.image_offsets, packed_bytes=self.packed_bytes)

    def to_device(self, device="cuda", T: int = None) -> torch.Tensor:
        """-> `(B,3,T,H,W)` fp32 on the device, normalised and zero-padded (T defaults to the longest clip): the bits of `PackedFrames.to_device`"""
        return native.normalise_pad_frames(self.decode(device), self.offsets, self.frames, self.H, self.W, T)


class PackedAudio:
    """B waveforms `(1,n_b)` / `(n_b,)` fp32 packed back to back (16-byte aligned) in one host buffer: the audio-side twin of `PackedFrames`.
    `.to_device()` runs `l2s_mel_targets`: log-mel targets, gates and the zero-padded audio come from one launch chain on the device instead of
    one CPU STFT per item in the loader workers plus the host collate's padding."""
    HOP, MIN_SAMPLES = 256, 513      # the transform's hop; torch.stft(center=True, pad_mode="reflect") at n_fft 1024 needs more than 512 samples

    def __init__(self, speeches: Sequence[torch.Tensor], pin: bool = True):
        assert len(speeches) > 0 and all(s.dtype == torch.float32 and s.numel() == s.shape[-1] for s in speeches), "waveforms are fp32 (1,n) or (n,)"
        self.samples: List[int] = [int(s.shape[-1]) for s in speeches]
        assert min(self.samples) >= self.MIN_SAMPLES, "a waveform needs at least 513 samples (reflect padding of 512)"
        self.offsets: List[int] = []                  # in floats
        total = 0
        for n in self.samples:
            self.offsets.append(total)
            total += (n + 3) // 4 * 4
        buf = torch.zeros(total, dtype=torch.float32)
        if pin and torch.cuda.is_available():
            buf = buf.pin_memory()
        for s, o, n in zip(speeches, self.offsets, self.samples):
            buf[o:o + n] = s.reshape(-1)
        self.data = buf

    @property
    def lengths(self) -> torch.Tensor:
        return torch.tensor(self.samples)

    @property
    def mel_lengths(self) -> torch.Tensor:
        """frames per clip, `n // 256 + 1` - known on the host without touching the device"""
        return torch.tensor([n // self.HOP + 1 for n in self.samples])

    def to_device(self, device="cuda", mel_pad: float = native.MEL_PAD, mel_transform=None):
        """-> `((audio (B,a_max), audio_lengths), (mels (B,80,m_max), mel_lengths, gate))` with the tensors on the device and the lengths as CPU int64
        tensors: the shapes, dtypes and values of `_pad_audio_mels` on the items' CPU mels.  `mel_pad` defaults to the collates' ln(1e-5);
        `mel_transform`: the `MelSpectrogram` whose filterbank defines the mel scale (default: the hparams one, built once)."""
        dev = self.data.to(device, non_blocking=True)
        mt = mel_transform or PackedAudio._default_transform(dev.device)
        assert (mt.n_fft, mt.win, mt.hop) == (1024, 1024, self.HOP) and mt.log, "the device transform is the n_fft = win = 1024, hop 256 log-mel"
        mels, gate, audio, _ = native.mel_targets(dev, self.offsets, self.samples, mt.fb.to(dev.device), mt.fb_nnz, mel_pad=mel_pad)
        return (audio, self.lengths), (mels, self.mel_lengths, gate)

    _transforms = {}

    @staticmethod
    def _default_transform(device):
        """the hparams log-mel transform with its filterbank on `device`, built once per device"""
        if device not in PackedAudio._transforms:
            from .spectrograms import MelSpectrogram
            PackedAudio._transforms[device] = MelSpectrogram().to(device)
        return PackedAudio._transforms[device]


def _resize_u8(x_u8: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """`transforms.Resize(size)` on a uint8 `(3,H,W)` tensor as `lrw.face_recog_resize` restates it (torchvision is absent here): bilinear,
    half-pixel centres, no antialias, rounded back to uint8"""
    x = torch.nn.functional.interpolate(x_u8[None].float(), size=size, mode="bilinear", align_corners=False)[0]
    return x.round().clamp(0, 255).to(torch.uint8)


def _chw(face) -> torch.Tensor:
    """an aligned face as uint8 `(3,H,W)`: the reference's layout as it stands, `(H,W,3)` permuted (a face is at least 16 rows high, so a
    first axis of 3 is the channels)"""
    face = torch.as_tensor(face)
    assert face.dtype == torch.uint8 and face.dim() == 3 and 3 in (face.shape[0], face.shape[2]), "a face is uint8 (3,H,W) or (H,W,3)"
    return face if face.shape[0] == 3 else face.permute(2, 0, 1)


def faces_item_host(faces, flip: bool, face_indices, size: int = 96):
    """The tail of `GRID.__getitem__` (datasets/grid/dataset.py:225-236; the avspeech / wild loaders do the same) in torch on the CPU: the
    aligned faces of one clip, uint8 `(3,H_i,W_i)` each with its own size -> `(lower_faces (T,3,size,size), face_crop (2,3,160,160))`.
    `flip`: `FaceAugmentation`'s decision for the item (all faces mirrored); `face_indices`: the two drawn faces."""
    from .lrw import IMAGENET_MEAN, IMAGENET_STD, face_recog_resize
    faces = [_chw(f) for f in faces]
    if flip:
        faces = [torch.flip(f, dims=(-1,)) for f in faces]
    face_crop = torch.stack([face_recog_resize(faces[int(i)]) for i in face_indices], dim=0)
    mean, std = torch.tensor(IMAGENET_MEAN).view(3, 1, 1), torch.tensor(IMAGENET_STD).view(3, 1, 1)
    lower = [(_resize_u8(f[:, f.shape[1] // 2:, :], (size, size)).float() / 255.0 - mean) / std for f in faces]
    return (torch.stack(lower, dim=0) if lower else torch.zeros(0, 3, size, size)), face_crop


class PackedFaces:
    """B items of aligned faces packed back to back in one host buffer, every image interleaved `(H_i,W_i,3)` on a 4-byte boundary.  An item is
    `(faces, flip, face_indices)`: the clip's faces (uint8 `(3,H_i,W_i)` as the reference holds them, or `(H_i,W_i,3)`), the item's flip decision
    and its two face indices.  `mouth_jobs` / `face_jobs` are the job tables of `l2s_resize_normalise` (rows `(offset, H, W, y0, x0, h, w, flip,
    slot)`): the lower half `[H // 2, H)` of face t of item b to mouth slot `(b, t)`, the whole of face `face_indices[k]` to face slot `(b, k)`.

    An item may also be `(crops, flip, face_indices, landmarks)`: the UNROTATED face-box crops and the landmarks of the same frames
    (`face_utils.face_box_crops`).  Its images get one row each in `align_jobs`, the table of `l2s_align_faces` (rows `(offset, H, W, m0, .., m5)` with
    the map `rotation_inverse_map(eye_angle_degrees(landmarks), H, W)`), and `to_device` rotates them on the device before the two resize calls - what
    `face_utils.align_and_crop_face` does per frame on the host, to the bit.

    A face may also be a JPEG byte string (bytes or a 1-D uint8 array): its size comes from its header, the strings travel compressed in a second buffer
    (`jpeg_data`, planned once: `jpeg_plan`; `jpeg_offsets` their images' offsets in the packed layout), and `to_device` decodes them into the packed buffer
    with one `l2s_jpeg_decode` before anything else runs; the job tables are those of the decoded faces."""

    def __init__(self, items: Sequence, pin: bool = True):
        assert len(items) > 0, "at least one item"
        strings = [s for s in (_jpeg_string(f) for item in items for f in item[0]) if s is not None]
        self.jpeg_data = self.jpeg_plan = None
        self.jpeg_offsets: List[int] = []
        if strings:
            self.jpeg_data, stream_offsets, stream_sizes = _pack_streams(strings, pin)
            self.jpeg_plan = native.jpeg_plan(self.jpeg_data, stream_offsets, stream_sizes)
        jpeg_sizes = iter(self.jpeg_plan.sizes if strings else ())
        self.frames: List[int] = []
        self.images: List[Tuple[int, int, int]] = []       # (offset, H, W) of every image, in item order
        self.flips: List[int] = []
        self.face_jobs: List[Tuple[int, ...]] = []
        self.align_jobs: List[Tuple] = []
        self._slots: List[Tuple[int, int]] = []            # (b, t) of every image
        chw, total = [], 0
        for b, item in enumerate(items):
            assert len(item) in (3, 4), "an item is (faces, flip, face_indices) or (crops, flip, face_indices, landmarks)"
            faces, flip, face_indices = item[:3]
            landmarks = item[3] if len(item) == 4 else None
            assert landmarks is None or len(landmarks) == len(faces), "one landmark set per crop"
            first = len(self.images)
            self.frames.append(len(faces))
            self.flips.append(int(bool(flip)))
            for t, f in enumerate(faces):
                if _jpeg_string(f) is not None:
                    f, (H, W) = None, next(jpeg_sizes)
                    self.jpeg_offsets.append(total)
                else:
                    f = _chw(f)
                    H, W = int(f.shape[1]), int(f.shape[2])
                assert 1 <= H <= 4096 and 1 <= W <= 4096, "a face is at most 4096 x 4096"
                chw.append(f)
                self.images.append((total, H, W))
                self._slots.append((b, t))
                if landmarks is not None:
                    self.align_jobs.append((total, H, W) + tuple(rotation_inverse_map(eye_angle_degrees(landmarks[t]), H, W)))
                total += (H * W * 3 + 3) // 4 * 4
            assert len(face_indices) == 2 and all(0 <= int(i) < len(faces) for i in face_indices), "two face indices inside the clip"
            for k, i in enumerate(face_indices):
                o, H, W = self.images[first + int(i)]
                self.face_jobs.append((o, H, W, 0, 0, H, W, self.flips[b], 2 * b + k))
        buf = torch.zeros(total, dtype=torch.uint8)        # the alignment gaps are zeros
        if pin and torch.cuda.is_available():
            buf = buf.pin_memory()
        for f, (o, H, W) in zip(chw, self.images):
            if f is not None:
                buf[o:o + H * W * 3] = f.permute(1, 2, 0).reshape(-1)
        self.data = buf

    @property
    def lengths(self) -> torch.Tensor:
        return torch.tensor(self.frames)

    def mouth_jobs(self, T: int = None) -> List[Tuple[int, ...]]:
        """the lower half of every face -> slot `b * T + t` (T defaults to the longest clip)"""
        T = max(max(self.frames), 1) if T is None else int(T)
        return [(o, H, W, H // 2, 0, H - H // 2, W, self.flips[b], b * T + t) for (o, H, W), (b, t) in zip(self.images, self._slots)]

    def to_device(self, device="cuda", T: int = None, size: int = 96):
        """-> `(video (B,3,T,size,size), face_crops (B,2,3,160,160))` fp32 on the device from ONE host-to-device copy and two calls; clips shorter
        than T (default: the longest clip) are zero-padded.  Items that came with landmarks are rotated first, by one `l2s_align_faces` call on the
        upload; the images of the other items of such a batch are carried over as they are."""
        if self.jpeg_plan is None:
            dev = self.data.to(device, non_blocking=True)
        else:                                              # the compressed faces: decoded into the packed buffer, next to the faces that came decoded (if any)
            some = len(self.jpeg_offsets) < len(self.images)
            dev = native.jpeg_decode(self.jpeg_data.to(device, non_blocking=True), self.jpeg_plan, self.jpeg_offsets,
                                     out=self.data.to(device, non_blocking=True) if some else None, packed_bytes=self.data.numel())
        if self.align_jobs:
            dev = native.align_faces(dev, self.align_jobs, out=dev.clone() if len(self.align_jobs) < len(self.images) else None)
        B = len(self.frames)
        T = max(max(self.frames), 1) if T is None else int(T)
        video = native.resize_normalise(dev, self.mouth_jobs(T), native.RESIZE_MOUTH, B, T, size)
        return video, native.resize_normalise(dev, self.face_jobs, native.RESIZE_FACE, B)


def device_collate_fn_pad_faces(batch):
    """`device_collate_fn_pad_raw` for loaders whose items carry aligned faces of their own sizes: an item is
    `((faces, flip, face_indices), speech, melspec, _[, path])` - or `((crops, flip, face_indices, landmarks), ...)` with unrotated face-box crops,
    which `PackedFaces` has the device rotate - and the tuple is `((packed_faces, lengths), packed_audio, packed_audio,
    packed_faces[, paths])` - ONE `PackedFaces` in the video and face positions; `packed_faces.to_device()` returns both,
    `(video, face_crops)`."""
    with_paths = len(batch[0]) == 5
    faces = PackedFaces([b[0] for b in batch])
    audio = PackedAudio([b[1] for b in batch])
    out = ((faces, faces.lengths), audio, audio, faces)
    return out + (tuple(b[4] for b in batch),) if with_paths else out


def device_collate_fn_pad_jpeg(batch):
    """`device_collate_fn_pad_raw` for `LRW(raw_jpeg=True, raw_audio=True)`, whose items carry JPEG byte strings: the tuple is
    `((PackedJpegFrames, lengths), packed_audio, packed_audio, faces[, paths])`.  `faces`: ONE `PackedFaces` of the items' two drawn face strings
    (`faces.to_device()[1]` is the `(B,2,3,160,160)` face crops), or, for a loader without face files, the stacked zeros as before."""
    with_paths = len(batch[0]) == 5
    frames = PackedJpegFrames([b[0] for b in batch])
    audio = PackedAudio([b[1] for b in batch])
    have = [not isinstance(b[3], torch.Tensor) for b in batch]
    assert all(have) or not any(have), "either every item of a batch has a face file or none has"
    faces = PackedFaces([(b[3], False, (0, 1)) for b in batch]) if all(have) else torch.stack([b[3] for b in batch], dim=0)
    out = ((frames, frames.lengths), audio, audio, faces)
    return out + (tuple(b[4] for b in batch),) if with_paths else out


def device_collate_fn_pad_raw(batch):
    """`device_collate_fn_pad` for loaders that also leave the mel transform to the device (`LRW(raw_frames=True, raw_audio=True)`): the same
    tuple with ONE `PackedAudio` in the audio and mel positions - `((PackedFrames, lengths), packed_audio, packed_audio, faces[, paths])`; the
    items' melspec slot is ignored (it is `None` with `raw_audio=True`).  `packed_audio.to_device()` returns both halves,
    `((audio, audio_lengths), (mels, mel_lengths, gate))`, so that `(packed_frames.to_device(), vlen), *packed_audio.to_device(), faces` is the
    reference's 4-tuple."""
    with_paths = len(batch[0]) == 5
    frames = PackedFrames([b[0] for b in batch])
    audio = PackedAudio([b[1] for b in batch])
    out = ((frames, frames.lengths), audio, audio, torch.stack([b[3] for b in batch], dim=0))
    return out + (tuple(b[4] for b in batch),) if with_paths else out


def device_collate_fn_pad(batch):
    """`train_collate_fn_pad` for items whose first element is the RAW clip (uint8 `(T,H,W,3)`, `LRW(raw_frames=True)`): the same
    4-tuple, with `PackedFrames` in place of the padded fp32 video - call `.to_device()` on it where the reference's loop calls
    `videos.to(device)` (train.py:163)."""
    from . import _pad_audio_mels
    with_paths = len(batch[0]) == 5
    packed = PackedFrames([b[0] for b in batch])
    out = ((packed, packed.lengths),) + _pad_audio_mels([b[1] for b in batch], [b[2] for b in batch]) + (torch.stack([b[3] for b in batch], dim=0),)
    return out + (tuple(b[4] for b in batch),) if with_paths else out
