"""Device-side mel targets, host side (no GPU): the three C-ABI symbols are declared, exported and bound; `l2s_mel_frames` counts frames as
`torch.stft(center=True)` does; `l2s_mel_targets` refuses shapes outside what it is built for, naming the argument, before anything reaches the
device; `PackedAudio` lays the waveforms out verbatim; `MelSpectrogram` keeps its bits on CPU tensors; `LRW(raw_audio=True)` only drops the mel."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_lrw")
SYMBOLS = ("l2s_mel_frames", "l2s_mel_targets_workspace_bytes", "l2s_mel_targets")


@pytest.fixture(scope="module")
def L():
    from lip2speech_amd import native
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lip2speech_amd", "csrc"), "-j", "8"], check=True)
    return native.lib()


def test_symbols_declared_exported_bound(L):
    from lip2speech_amd import datasets, native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l2s.h")).read(), flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} not declared in include/l2s.h"
        assert sym in native.ABI_SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None, f"{sym} has no ctypes signature"
    assert L.l2s_mel_targets_workspace_bytes.restype is ctypes.c_int64 and L.l2s_mel_targets_workspace_bytes(32, 80) > 0
    assert L.l2s_abi_version() == 2                      # the change only adds symbols
    assert native.MEL_PAD == datasets.MEL_PAD            # one padding value on both sides of the binding


def test_mel_frames(L):
    from lip2speech_amd import native
    for n in (513, 768, 1000, 18560, 48000):
        assert L.l2s_mel_frames(n) == n // 256 + 1 == native.mel_frames(n)
    assert [native.mel_frames(n) for n in (513, 768, 1000, 18560, 48000)] == [3, 4, 4, 73, 188]
    assert L.l2s_mel_frames(512) == 0 and b"n_samples = 512" in L.l2s_last_error()
    with pytest.raises(RuntimeError, match="n_samples = 512"):
        native.mel_frames(512)


def _call(L, n_samples, B=None, n_fft=1024, hop=256, n_mels=80, M_pad=80, A_pad=20000, fb_nnz=1100):
    """l2s_mel_targets with dummy (never dereferenced) device pointers: every case below must be refused before any device call"""
    B = len(n_samples) if B is None else B
    off, o = [], 0
    for n in n_samples:
        off.append(o); o += n
    dummy = 4096
    return L.l2s_mel_targets(dummy, (ctypes.c_int64 * len(off))(*off), (ctypes.c_int64 * len(off))(*n_samples), B, dummy, fb_nnz, n_mels, n_fft, hop, 1,
                             -11.5129, M_pad, A_pad, dummy, dummy, dummy, dummy, dummy, 1 << 20, None)


def test_refused_before_any_launch(L):
    for kw, names in ((dict(n_samples=[18560], B=0), b"B must be positive"),
                      (dict(n_samples=[18560, 400]), b"n_samples[1] = 400"),
                      (dict(n_samples=[18560], n_fft=512), b"n_fft"),
                      (dict(n_samples=[18560], hop=128), b"hop"),
                      (dict(n_samples=[18560], n_mels=129), b"n_mels"),
                      (dict(n_samples=[18560], n_mels=0), b"n_mels"),
                      (dict(n_samples=[513, 18560], M_pad=72), b"M_pad = 72 is below the 73 frames of n_samples[1]"),
                      (dict(n_samples=[18560], A_pad=18559), b"A_pad = 18559"),
                      (dict(n_samples=[18560], fb_nnz=2049), b"fb_nnz")):
        assert _call(L, **kw) != 0, kw
        assert names in L.l2s_last_error(), (kw, L.l2s_last_error())


def test_packed_audio_layout():
    from lip2speech_amd.datasets import PackedAudio
    g = torch.Generator().manual_seed(0)
    waves = [torch.randn(1, 513, generator=g), torch.randn(4096, generator=g), torch.randn(1, 1791, generator=g)]
    p = PackedAudio(waves, pin=False)
    assert p.samples == [513, 4096, 1791] and p.offsets == [0, 516, 516 + 4096]           # float offsets, 16-byte aligned
    assert p.lengths.tolist() == [513, 4096, 1791] and p.lengths.dtype == torch.int64
    assert p.mel_lengths.tolist() == [3, 17, 7] and p.mel_lengths.dtype == torch.int64
    assert p.data.dtype == torch.float32 and p.data.numel() == 516 + 4096 + 1792
    for w, o, n in zip(waves, p.offsets, p.samples):
        assert torch.equal(p.data[o:o + n], w.reshape(-1))                                 # the samples verbatim
    assert float(p.data[513:516].abs().max()) == 0.0                                       # the alignment gaps are zeros, not stale memory
    with pytest.raises(AssertionError, match="513"):
        PackedAudio([torch.zeros(1, 512)], pin=False)


def test_mel_spectrogram_cpu_bits_unchanged():
    from lip2speech_amd.datasets import MelSpectrogram
    x = 0.1 * torch.randn(2, 1, 18560, generator=torch.Generator().manual_seed(0))
    want = MelSpectrogram(backend="torch")(x)
    assert torch.equal(MelSpectrogram()(x), want) and torch.equal(MelSpectrogram(backend="auto")(x), want)
    assert MelSpectrogram().backend == "auto" and want.shape == (2, 1, 80, 73)
    with pytest.raises(RuntimeError, match="backend='hip'"):
        MelSpectrogram(backend="hip")(x)                                                   # a CPU tensor: no quiet fall-back when the kernel is asked for


def test_lrw_raw_audio_drops_only_the_mel(tmp_path):
    from lip2speech_amd.datasets import LRW, PackedAudio, PackedFrames, device_collate_fn_pad, device_collate_fn_pad_raw
    d = tmp_path / "LRW_Faces" / "ABOUT" / "test"
    a = tmp_path / "lipread_audio" / "ABOUT" / "test"
    d.mkdir(parents=True); a.mkdir(parents=True)
    for i in (1, 2):
        shutil.copy(os.path.join(SAMPLE, f"ABOUT_0000{i}_mouth.npz"), d / f"ABOUT_0000{i}_mouth.npz")
        shutil.copy(os.path.join(SAMPLE, f"ABOUT_0000{i}.npz"), a / f"ABOUT_0000{i}.npz")
    raw, ref = LRW(str(tmp_path), mode="test", raw_audio=True), LRW(str(tmp_path), mode="test")
    for i in range(2):
        torch.manual_seed(i)
        got = raw[i]
        torch.manual_seed(i)
        want = ref[i]
        assert len(got) == len(want) == 4 and got[2] is None and want[2].shape == (80, 77)
        assert all(torch.equal(got[k], want[k]) for k in (0, 1, 3))
    # the collate of raw items: packed frames and ONE packed audio in the audio and mel positions; everything the host knows is the host collate's
    both = LRW(str(tmp_path), mode="test", raw_frames=True, raw_audio=True)
    frames_ref = LRW(str(tmp_path), mode="test", raw_frames=True)
    (pf, vlen), pa, pa2, faces = device_collate_fn_pad_raw([both[0], both[1]])
    (pf_ref, vlen_ref), (audio, alen), (mels, mlen, gate), _ = device_collate_fn_pad([frames_ref[0], frames_ref[1]])
    assert isinstance(pf, PackedFrames) and isinstance(pa, PackedAudio) and pa2 is pa and faces.shape == (2, 2, 3, 160, 160)
    assert torch.equal(pf.data, pf_ref.data) and torch.equal(vlen, vlen_ref)
    assert torch.equal(pa.lengths, alen) and torch.equal(pa.mel_lengths, mlen)
    assert all(torch.equal(pa.data[o:o + n], audio[i, :n]) for i, (o, n) in enumerate(zip(pa.offsets, pa.samples)))
