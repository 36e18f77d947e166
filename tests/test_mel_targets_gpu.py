"""Device-side mel targets on the GPU (`l2s_mel_targets`, mel_targets.hip) against the project's own restatement of the transform in fp64,
`MelSpectrogram(log=False).double()` on the CPU - never the code under test.

Accuracy bound.  No constant can be derived for it, so the yardstick is the existing fp32 torch path (`MelSpectrogram(log=False)` in float32 on the CPU)
on the same inputs: the worst value of each metric over all signal x length cases, times 8 - the margin for another factorisation (radix-8 Stockham
against the library FFT), fp32 twiddles from `sincospif`, a window table that is torch's own fp32 one only to the rounding of its cosine, and another
summation order in the bands, all O(eps log N) effects like the yardstick's own.  Metric (a): max |log got - log ref| over the bins with ref >= 1e-5 and
ref >= 1e-3 x the frame's largest band; metric (b): max |got - ref| / the frame's largest band, over all bins.  The test prints both sides."""
import ctypes
import math
import os
import shutil

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_lrw")
LENGTHS = (513, 768, 1000, 18560)          # 3 frames, all reflecting | a multiple of the hop | no multiple of hop or load pattern | LRW's own, 73 frames
SIGNALS = ("noise", "tone", "imp", "dc", "silence")
MARGIN = 8.0


def _signal(kind, n):
    g = torch.Generator().manual_seed(0)
    if kind == "noise":
        return 0.1 * torch.randn(n, generator=g)
    if kind == "tone":
        return 0.5 * torch.sin(2 * math.pi * 440.0 * torch.arange(n, dtype=torch.float64) / 16000.0).float() + 1e-4 * torch.randn(n, generator=g)
    if kind == "imp":
        x = torch.zeros(n)
        x[0], x[-1] = -0.5, 1.0                # both reflections
        return x
    if kind == "dc":
        return torch.full((n,), 0.25)
    return torch.zeros(n)


def _metrics(got, ref):
    """got, ref (..., n_mels, frames) power-mels -> (metric a, metric b, share of the bins (a) covers); frames whose reference is all zero must be exact zeros"""
    got, ref = got.double(), ref.double()
    peak = ref.amax(dim=-2, keepdim=True)
    live = (peak > 0).expand_as(ref)
    assert torch.equal(got[~live], torch.zeros_like(got[~live])), "an all-zero reference frame is not all zero"
    sel = (ref >= 1e-5) & (ref >= 1e-3 * peak) & live
    a = float((got[sel].log() - ref[sel].log()).abs().max()) if sel.any() else 0.0
    b = float(((got - ref).abs() / peak.clamp(min=1e-300))[live].max()) if live.any() else 0.0
    return a, b, float(sel.double().mean())


@pytest.fixture(scope="module")
def cases():
    """every signal x length: the waveform, the fp64 reference and the fp32 torch yardstick (power-mels, CPU); computed once, never modified"""
    from lip2speech_amd.datasets import MelSpectrogram
    ref_t, yard_t = MelSpectrogram(log=False, backend="torch").double(), MelSpectrogram(log=False, backend="torch")
    out = {}
    for n in LENGTHS:
        for kind in SIGNALS:
            x = _signal(kind, n)
            out[kind, n] = (x, ref_t(x.double()[None])[0], yard_t(x[None])[0])
    return out


@pytest.fixture(scope="module")
def bound(cases):
    """8 x the yardstick's worst (a) and (b) over all cases; the noise cases must be covered bin for bin by (a)"""
    worst_a = worst_b = 0.0
    for (kind, n), (_, ref, yard) in cases.items():
        a, b, cover = _metrics(yard, ref)
        if kind == "noise":
            assert cover == 1.0, f"metric (a) covers {cover:.3f} of the noise case n = {n}"
        worst_a, worst_b = max(worst_a, a), max(worst_b, b)
    print(f"yardstick (fp32 torch path vs fp64): worst (a) {worst_a:.3e}  worst (b) {worst_b:.3e}")
    assert 0 < worst_a < 1e-5 and 0 < worst_b < 1e-5          # orientation: 6.2e-7 and 3.2e-7
    return MARGIN * worst_a, MARGIN * worst_b


@pytest.fixture(scope="module")
def mt():
    from lip2speech_amd.datasets import MelSpectrogram
    return MelSpectrogram().cuda()


def _pack(waves, lead=0):
    """the PackedAudio layout on the device, `lead` floats in (lead = 1: every clip starts on an odd float)"""
    from lip2speech_amd.datasets import PackedAudio
    p = PackedAudio(waves, pin=False)
    buf = torch.cat([torch.full((lead,), float("nan")), p.data]).cuda()
    return buf, [o + lead for o in p.offsets], p.samples


def _run(mt, waves, lead=0, **kw):
    from lip2speech_amd import native
    buf, off, ns = _pack(waves, lead)
    return native.mel_targets(buf, off, ns, mt.fb, mt.fb_nnz, **kw)


def test_accuracy_against_fp64(cases, bound, mt):
    worst_a = worst_b = 0.0
    for n in LENGTHS:                                       # one call per length: the five signals as a batch
        power = _run(mt, [cases[k, n][0] for k in SIGNALS], log=False, want_audio=False)[0].cpu()
        assert power.shape == (5, 80, n // 256 + 1)
        for i, kind in enumerate(SIGNALS):
            a, b, cover = _metrics(power[i], cases[kind, n][1])
            print(f"{kind:8s} n = {n:6d}: (a) {a:.3e} over {cover:.3f} of the bins   (b) {b:.3e}")
            worst_a, worst_b = max(worst_a, a), max(worst_b, b)
    print(f"kernel vs fp64: worst (a) {worst_a:.3e} (bound {bound[0]:.3e})  worst (b) {worst_b:.3e} (bound {bound[1]:.3e})")
    assert worst_a <= bound[0] and worst_b <= bound[1]


def test_filterbank_with_zeros_inside_its_bands(cases, bound):
    """bands whose two non-zero bins lie 512 - 2 m apart: the contiguous [first, last] ranges sum to more than the compact table holds, so the kernel reads
    the weights from the dense filterbank - the same sums"""
    from lip2speech_amd import native
    from lip2speech_amd.datasets import MelSpectrogram
    g = torch.Generator().manual_seed(1)
    fb = torch.zeros(513, 8)
    for m in range(8):
        fb[m, m], fb[512 - m, m] = torch.rand(2, generator=g) + 0.5
    x = cases["noise", 1000][0]
    t = MelSpectrogram(log=False, backend="torch").double()
    t.fb = fb.double()
    buf, off, ns = _pack([x])
    got = native.mel_targets(buf, off, ns, fb.cuda(), 16, log=False, want_audio=False)[0].cpu()
    a, b, _ = _metrics(got[0], t(x.double()[None])[0])
    print(f"zeros inside the bands: (a) {a:.3e}  (b) {b:.3e}")
    assert a <= bound[0] and b <= bound[1]


def _raw_call(mt, waves, M, A, mel_pad, log=True):
    """the C entry point on NaN-filled outputs of the caller's own"""
    from lip2speech_amd import native
    buf, off, ns = _pack(waves)
    B, L = len(ns), native.lib()
    mels = torch.full((B, 80, M), float("nan"), device="cuda")
    gate = torch.full((B, M), float("nan"), device="cuda")
    audio = torch.full((B, A), float("nan"), device="cuda")
    lengths = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(L.l2s_mel_targets_workspace_bytes(B, 80)), dtype=torch.uint8, device="cuda")
    native.check(L.l2s_mel_targets(buf.data_ptr(), (ctypes.c_int64 * B)(*off), (ctypes.c_int64 * B)(*ns), B, mt.fb.data_ptr(), mt.fb_nnz, 80, 1024, 256,
                                   int(log), mel_pad, M, A, mels.data_ptr(), gate.data_ptr(), audio.data_ptr(), lengths.data_ptr(), ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream))
    return mels, gate, audio, lengths


def test_exact_properties(cases, mt):
    from lip2speech_amd.datasets import MEL_PAD, MelSpectrogram, _pad_audio_mels
    waves = [cases["noise", 513][0][None], cases["silence", 1000][0][None], cases["tone", 18560][0][None], cases["imp", 768][0][None]]
    cpu_mels = [MelSpectrogram(backend="torch")(w)[0] for w in waves]
    for mel_pad in (MEL_PAD, 0.0):                          # the LRW / top-level collates' value and the per-corpus collates'
        mels, gate, audio, lengths = _raw_call(mt, waves, 75, 18563, mel_pad)
        assert not torch.isnan(mels).any() and not torch.isnan(gate).any() and not torch.isnan(audio).any()      # every element written
        assert lengths.tolist() == [3, 4, 73, 4]
        for b, m_b in enumerate((3, 4, 73, 4)):
            assert torch.equal(mels[b, :, m_b:], torch.full((80, 75 - m_b), mel_pad, device="cuda")), f"pad frames of clip {b}"
        assert float((mels[1, :, :4].double() - math.log(1e-5)).abs().max()) <= 1e-6                           # silence: the floor, logf(1e-5f), in every real frame
        # the same batch through the host collate: gate, lengths and padded audio are its values exactly
        (audio_ref, alen), (mels_ref, mlen, gate_ref) = _pad_audio_mels(waves, cpu_mels, mel_pad)
        assert torch.equal(gate[:, :73].cpu(), gate_ref) and torch.equal(gate[:, 73:].cpu(), torch.ones(4, 2))
        assert torch.equal(audio[:, :18560].cpu(), audio_ref) and torch.equal(audio[:, 18560:].cpu(), torch.zeros(4, 3))
        assert torch.equal(lengths.cpu(), mlen) and lengths.dtype == mlen.dtype
    # the power-mel of log_output = 0, clamped and logged, is the log_output = 1 result bit for bit (the kernel's log is the fp64 one rounded to nearest:
    # what every library's fp64 log gives, where the fp32 logs of two libraries may differ in the last bit)
    power = _raw_call(mt, waves, 75, 18563, 0.0, log=False)[0]
    for b, m_b in enumerate((3, 4, 73, 4)):
        assert torch.equal(torch.log(torch.clamp(power[b, :, :m_b], min=1e-5).double()).float(), mels[b, :, :m_b]), f"clip {b}"
        assert torch.equal(power[b, :, m_b:], torch.zeros(80, 75 - m_b, device="cuda"))


def test_packed_audio_to_device_is_the_host_collate(cases, mt):
    from lip2speech_amd.datasets import MEL_PAD, MelSpectrogram, PackedAudio, _pad_audio_mels
    waves = [cases["noise", 513][0][None], cases["tone", 18560][0][None], cases["dc", 1000][0][None]]
    want = _pad_audio_mels(waves, [MelSpectrogram(backend="torch")(w)[0] for w in waves])
    (audio, alen), (mels, mlen, gate) = PackedAudio(waves).to_device()
    assert audio.is_cuda and mels.is_cuda and gate.is_cuda and not alen.is_cuda and not mlen.is_cuda
    assert torch.equal(audio.cpu(), want[0][0]) and torch.equal(alen, want[0][1]) and alen.dtype == want[0][1].dtype
    assert torch.equal(mlen, want[1][1]) and mlen.dtype == want[1][1].dtype and torch.equal(gate.cpu(), want[1][2])
    assert mels.shape == want[1][0].shape and mels.dtype == want[1][0].dtype
    assert torch.equal(mels[0, :, 3:].cpu(), want[1][0][0, :, 3:]) and float(mels[0, 0, 3]) == float(torch.tensor(MEL_PAD))


def test_batch_invariance_in_bits(mt):
    g = torch.Generator().manual_seed(2)
    a, b, c = (0.1 * torch.randn(n, generator=g) for n in (513, 4096, 1791))
    alone = _run(mt, [c])[0]
    assert alone.shape == (1, 80, 7)
    last = _run(mt, [a, b, c], M=17)[0]
    first = _run(mt, [c, a], M=40)[0]
    odd = _run(mt, [c, a], lead=1, M=40)[0]                 # clips on odd float offsets: the 4-byte load path, the same values
    assert torch.equal(last[2, :, :7], alone[0]) and torch.equal(first[0, :, :7], alone[0]) and torch.equal(odd, first)


def test_collate_equivalence(tmp_path, cases, bound):
    from lip2speech_amd.datasets import LRW, MelSpectrogram, device_collate_fn_pad, device_collate_fn_pad_raw
    d = tmp_path / "LRW_Faces" / "ABOUT" / "test"
    au = tmp_path / "lipread_audio" / "ABOUT" / "test"
    d.mkdir(parents=True); au.mkdir(parents=True)
    for i in (1, 2, 3):
        shutil.copy(os.path.join(SAMPLE, f"ABOUT_0000{i}_mouth.npz"), d / f"ABOUT_0000{i}_mouth.npz")
        shutil.copy(os.path.join(SAMPLE, f"ABOUT_0000{i}.npz"), au / f"ABOUT_0000{i}.npz")
    raw, host = LRW(str(tmp_path), mode="test", raw_frames=True, raw_audio=True), LRW(str(tmp_path), mode="test", raw_frames=True)
    (pf, vlen), pa, _, faces = device_collate_fn_pad_raw([raw[i] for i in range(3)])
    (pf_h, vlen_h), (audio_h, alen_h), (mels_h, mlen_h, gate_h), faces_h = device_collate_fn_pad([host[i] for i in range(3)])
    (audio, alen), (mels, mlen, gate) = pa.to_device()
    assert torch.equal(pf.to_device(), pf_h.to_device()) and torch.equal(vlen, vlen_h) and faces.shape == faces_h.shape
    assert torch.equal(audio.cpu(), audio_h) and torch.equal(alen, alen_h) and torch.equal(mlen, mlen_h) and torch.equal(gate.cpu(), gate_h)
    assert mels.shape == mels_h.shape
    ref_t = MelSpectrogram(log=False, backend="torch").double()
    for i in range(3):
        m_i = int(mlen[i])
        ref = ref_t(host[i][1].double())[0]                 # fp64 power-mel of the item's waveform
        sel = (ref >= 1e-5) & (ref >= 1e-3 * ref.amax(dim=0, keepdim=True))
        a = float((mels[i, :, :m_i].cpu().double()[sel] - ref[sel].log()).abs().max())
        print(f"clip {i}: log-mel against fp64 (a) {a:.3e} (bound {bound[0]:.3e}), fp32 torch path {float((mels_h[i, :, :m_i].double()[sel] - ref[sel].log()).abs().max()):.3e}")
        assert a <= bound[0]
        assert torch.equal(mels[i, :, m_i:].cpu(), mels_h[i, :, m_i:])


def test_mel_spectrogram_hip_backend(mt):
    from lip2speech_amd import native
    from lip2speech_amd.datasets import MelSpectrogram
    x = (0.1 * torch.randn(2, 1, 18560, generator=torch.Generator().manual_seed(3))).cuda()
    hip, auto = MelSpectrogram(backend="hip").cuda(), MelSpectrogram().cuda()
    want = native.mel_targets(x.reshape(-1), [0, 18560], [18560, 18560], mt.fb, mt.fb_nnz, want_audio=False)[0]
    got = hip(x)
    assert got.shape == (2, 1, 80, 73) and torch.equal(got.reshape(2, 80, 73), want) and torch.equal(auto(x), got)
    torch_path = MelSpectrogram(backend="torch").cuda()(x)
    assert not torch.equal(torch_path, got) and float((torch_path - got).abs().max()) < 1e-3      # another order of the same sums: the kernel did run
    with pytest.raises(RuntimeError, match="backend='hip'"):
        hip(torch.zeros(1, 400, device="cuda"))
