"""The long forms of the device vocoder and metric (vocoder.hip): Griffin-Lim past 121 mel frames (one launch per iteration over tiles of
frames) and ESTOI past 16 512 samples at 10 kHz (signals in the workspace).  Same comparisons and tolerances as tests/test_vocoder_metrics.py
makes for the short forms, at the shapes GRID (188 frames) and `net.inference` (up to 300 frames) hand over."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from lip2speech_amd import metrics, native
from lip2speech_amd.datasets.spectrograms import MelSpec2Audio, MelSpectrogram

from test_vocoder_metrics import speechlike

pytestmark = pytest.mark.gpu

F = native.GRIFFIN_LIM_TILE_FRAMES
K = 121 // F + 1                                  # the first multiple of the tile past the short kernel


def _restatement(power, ang, iters):
    """`MelSpec2Audio.griffin_lim` on torch.stft / istft with explicit start angles (test_griffin_lim_kernel_matches_the_torch_restatement)."""
    L = power.shape[-1]
    win = torch.hann_window(1024, periodic=True, device=power.device)
    mag = power.sqrt()
    a = torch.view_as_complex(ang.clone())
    prev = torch.zeros_like(a)
    length = 256 * (L - 1)
    stft = lambda x: torch.stft(x, 1024, 256, 1024, win, center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)   # noqa: E731
    istft = lambda z: torch.istft(z, 1024, 256, 1024, win, length=length)          # noqa: E731
    for _ in range(iters):
        rebuilt = stft(istft(mag * a))
        a = rebuilt - prev * (0.99 / 1.99)
        a = a / (a.abs() + 1e-16)
        prev = rebuilt
    return istft(mag * a)


def _spectrum(N, L):
    g = torch.Generator(device="cuda")
    power = torch.rand(N, 513, L, device="cuda", generator=g.manual_seed(2)) ** 4 * 3.0
    ang = torch.rand(N, 513, L, 2, device="cuda", generator=g.manual_seed(3))
    ang[:, 0, :, 1] = 0                          # a C2R transform ignores the imaginary parts of DC and Nyquist: make them real
    ang[:, 512, :, 1] = 0
    return power, ang


@pytest.mark.parametrize("N,L,iters,tol", [(2, 122, 0, 2e-5), (2, 122, 1, 5e-5), (1, K * F + 1, 4, 1e-4), (1, K * F + 4, 4, 1e-4), (2, 188, 8, 2e-4),
                                           (1, 300, 2, 1e-4)])
def test_griffin_lim_long_form_matches_the_torch_restatement(N, L, iters, tol):
    """The tiled launch chain against the restatement, same start angles: the first length past the short kernel, a last tile of one frame
    (it reads the mirrored sample below its own range), a last tile shorter than the halo, GRID's 188 frames, inference's 300."""
    assert L > native.GRIFFIN_LIM_SHORT_FRAMES
    power, ang = _spectrum(N, L)
    want = _restatement(power, ang, iters)
    got = native.griffin_lim(power, ang, iters)
    assert got.shape == want.shape == (N, 256 * (L - 1))
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"griffin_lim long N={N} L={L} iters={iters}: max|d| {err:.3e} scale {scale:.3e}")
    assert err < tol * max(1.0, scale), (err, scale)


def test_griffin_lim_long_form_row_does_not_depend_on_its_neighbours():
    power, ang = _spectrum(3, 130)
    three = native.griffin_lim(power, ang, 4)
    alone = native.griffin_lim(power[1:2].contiguous(), ang[1:2].contiguous(), 4)
    assert torch.equal(three[1:2], alone)


def test_griffin_lim_long_form_full_run_converges_like_the_restatement():
    """256 iterations at GRID's 188 frames, judged as the short kernel's full-length run is: through the spectral inconsistency."""
    g = torch.Generator(device="cuda")
    x = torch.from_numpy(np.stack([speechlike(256 * 187, seed=s) for s in range(2)])).float().cuda()
    win = torch.hann_window(1024, periodic=True, device="cuda")
    stft = lambda v: torch.stft(v, 1024, 256, 1024, win, center=True, pad_mode="reflect", return_complex=True)       # noqa: E731
    power = stft(x).abs() ** 2
    ang = torch.rand(2, 513, 188, 2, device="cuda", generator=g.manual_seed(3))
    voc = MelSpec2Audio(max_iters=256, backend="torch").cuda()
    got = native.griffin_lim(power, ang, 256)
    want = voc.griffin_lim(power, g.manual_seed(3))
    mag = power.sqrt()
    inc = lambda y: float(((stft(y).abs() - mag).norm() / mag.norm()))      # noqa: E731
    print(f"griffin_lim long 256 iterations: inconsistency hip {inc(got):.4f} torch {inc(want):.4f}")
    assert torch.isfinite(got).all()
    assert inc(got) < 1.15 * inc(want) + 1e-3, (inc(got), inc(want))
    assert inc(got) < 0.35


@functools.lru_cache(maxsize=None)
def _clean(n):
    return np.stack([speechlike(n, seed=s) for s in range(3)]).astype(np.float32)


@pytest.mark.parametrize("n", [26624, 30976, 47872, 76544])
def test_estoi_long_form_matches_the_numpy_restatement(n):
    """130, 150, 232 and 372 frames at 10 kHz (26 624 is the first mel-aligned size past the short kernel): three clips at five noise levels."""
    clean = _clean(n)
    assert -(-n * 10000 // 16000) > native.ESTOI_SHORT_SAMPLES
    rng = np.random.default_rng(0)
    for level in (0.0, 0.1, 0.5, 2.0, 8.0):
        pred = (clean + level * clean.std(axis=1, keepdims=True) * rng.standard_normal(clean.shape)).astype(np.float32)
        want = np.array([metrics.stoi(clean[i], pred[i], 16000, extended=True) for i in range(3)])
        got = metrics.estoi_device(torch.from_numpy(clean).cuda(), torch.from_numpy(pred).cuda(), 16000).cpu().numpy()
        print(f"estoi long n={n} level={level}: max|d| {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() < 1e-4, (level, got, want)


def test_estoi_long_form_without_the_resampler():
    x10 = torch.from_numpy(_clean(30976)).cuda()                       # already at 10 kHz: 30 976 > 16 512 samples, no resampler
    y10 = x10 + 0.3 * x10.std() * torch.randn(x10.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    want = np.array([metrics.stoi(x10[i].cpu().numpy(), y10[i].cpu().numpy(), 10000, extended=True) for i in range(3)])
    got = metrics.estoi_device(x10, y10, 10000).cpu().numpy()
    assert np.abs(got - want).max() < 1e-4, (got, want)


def test_estoi_long_form_silent_tail_and_neighbours():
    """A clip zero-padded to a longer batch is scored as the reference scores the padded pair (silent-frame removal drops the tail); too
    little signal for one segment gives pystoi's 1e-5; and a row's bits do not depend on the other rows."""
    n = 47872
    clean = _clean(n)[0].copy()
    clean[30000:] = 0
    pred = (clean + 0.5 * clean[:30000].std() * np.random.default_rng(3).standard_normal(n)).astype(np.float32)
    want = metrics.stoi(clean, pred, 16000, extended=True)
    c, p = torch.from_numpy(clean).cuda()[None], torch.from_numpy(pred).cuda()[None]
    got = metrics.estoi_device(c, p, 16000)
    assert abs(float(got[0]) - want) < 1e-4, (float(got[0]), want)
    short = clean.copy()
    short[4000:] = 0
    s = torch.from_numpy(short).cuda()[None]
    assert float(metrics.estoi_device(s, p, 16000)[0]) == float(np.float32(1e-5))
    assert metrics.stoi(short, pred, 16000, extended=True) == 1e-5
    others = torch.from_numpy(_clean(n)[1:]).cuda()
    three = metrics.estoi_device(torch.cat([others, c]), torch.cat([others.flip(0), p]), 16000)
    assert torch.equal(three[2:3], got)


def test_melspec2audio_routes_long_clips_to_the_device(monkeypatch):
    """A GRID-length log-mel: backend="hip" accepts it, backend="auto" launches the device kernels (and no torch STFT), and both backends
    return (2, 47 872) from the same generator state."""
    g = torch.Generator(device="cuda")
    mel = torch.randn(2, 80, 188, device="cuda", generator=g.manual_seed(5)) * 2.0 - 5.0
    hip = MelSpec2Audio(max_iters=4, backend="hip").cuda()(mel, generator=g.manual_seed(9))
    tor = MelSpec2Audio(max_iters=4, backend="torch").cuda()(mel, generator=g.manual_seed(9))
    assert hip.shape == tor.shape == (2, 47872) and torch.isfinite(hip).all()
    auto = MelSpec2Audio(max_iters=4, backend="auto").cuda()

    def no_stft(*a, **k):
        raise AssertionError("the torch restatement ran")
    monkeypatch.setattr(torch, "stft", no_stft)
    native.profile_enable(True)
    try:
        native.profile_reset()
        out = auto(mel, generator=g.manual_seed(9))
        torch.cuda.synchronize()
        names = {name for name, _, _ in native.profile_read()}
    finally:
        native.profile_enable(False)
    assert "vocoder_griffin_lim" in names and "vocoder_inverse_mel" in names, names
    assert torch.equal(out, hip)


def test_evaluate_net_grid_shape_runs_its_tail_on_the_device():
    """evaluate.py:22-51 at GRID's shape (75 video frames, 188 mel frames): device tail against host tail, hip vocoder against torch
    vocoder, and two batches of different audio width in one group both scored on the device."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from model.model import get_network
    from lip2speech_amd import callers, synth
    B, T, S = 2, 75, 188
    net = get_network("test").cuda()
    audio = torch.from_numpy(np.stack([speechlike(256 * (S - 1), seed=s) for s in range(B)])).float()
    mel_t = MelSpectrogram()
    mels = mel_t(audio)[:, :, :S]
    batches = [((synth.synth_video(B, T, tag=f"evl{i}"), torch.full((B,), T)), (audio, torch.full((B,), audio.shape[1])),
                (mels, torch.full((B,), S), torch.zeros(B, S)), None) for i in range(2)]

    class Spk:
        def inference(self, a):
            return synth.synth_speaker_embedding(a.shape[0], tag="ev").to(a.device)
    scores = {}
    for vb, me in (("hip", "hip"), ("hip", "host"), ("torch", "host")):
        torch.manual_seed(0)
        scores[vb, me] = callers.evaluate_net(net, batches, speaker_encoder=Spk(), max_iters=32, vocoder_backend=vb, metric=me)
    print("evaluate_net GRID shape:", scores)
    assert abs(scores["hip", "hip"] - scores["hip", "host"]) < 1e-4, scores
    assert abs(scores["hip", "host"] - scores["torch", "host"]) < 5e-3, scores
    # the second batch's audio was padded further by its loader batch: same mels, another audio width, one group
    wide = torch.nn.functional.pad(audio, (0, 1024))
    mixed = [batches[0], (batches[1][0], (wide, torch.full((B,), wide.shape[1])), batches[1][2], None)]
    torch.manual_seed(0)
    dev = callers.evaluate_net(net, mixed, speaker_encoder=Spk(), max_iters=32, vocoder_backend="hip", metric="hip")
    torch.manual_seed(0)
    host = callers.evaluate_net(net, mixed, speaker_encoder=Spk(), max_iters=32, vocoder_backend="hip", metric="host")
    assert abs(dev - host) < 1e-4, (dev, host)


def test_time_vocoder_long_tool_runs():
    """tools/vocoder_long/time_vocoder_long.py end to end at one small long-form shape (two iterations, one round)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SHAPES="2x122", ROUNDS="1", REPS="1", ITERS="2")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "vocoder_long", "time_vocoder_long.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "N = 2 x 122 mel frames" in r.stdout and "whole span of (b) below the whole span of (a)" in r.stdout and "l2s_griffin_lim alone" in r.stdout
