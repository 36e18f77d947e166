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
"""
from __future__ import annotations

from typing import List, Sequence

import torch

from .. import native


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
