"""The ragged forms of the device vocoder and metric (include/l2s.h `l2s_inverse_mel_ragged`, `l2s_griffin_lim_ragged`, `l2s_estoi_ragged`; vocoder.hip):
clips of unequal length in one launch chain, every clip BIT FOR BIT what the solo entry point computes for it alone at its own length - whatever shares the
call, in whatever order, and whatever lies behind the clip in its row.  Few iterations: the iteration count changes nothing about indexing.
Parity with torchaudio / pystoi stays unpinned, as in tests/test_vocoder_metrics.py; the solo kernels are held to the torch / numpy restatements there."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from lip2speech_amd import callers, metrics, native, synth
from lip2speech_amd.datasets.spectrograms import MelSpec2Audio, MelSpectrogram

from test_vocoder_metrics import speechlike

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------------ inverse mel
IM_LENGTHS = [5, 8, 9, 77, 130]      # one row; a full block of 8 rows; a clip that straddles a block; the long clips
IM_ITERS = 6


@functools.lru_cache(maxsize=None)
def _inverse_mel_case(early: bool):
    """Per clip: power mel (80, L_b), start spectrum (L_b, 513) and the solo call's (spec, loss, iterations run).  `early`: the 9-frame clip's mel is exactly
    its start spectrum through the filterbank, so its first loss is below 1e-5 and it stops after one iteration; its neighbours run all of them."""
    voc = MelSpec2Audio(max_iters=IM_ITERS).cuda()
    clips = []
    for b, L in enumerate(IM_LENGTHS):
        mel = torch.exp(torch.randn(80, L, device="cuda", generator=_gen(10 + b)) * 2.0 - 5.0)
        init = torch.rand(L, 513, device="cuda", generator=_gen(20 + b))
        if early and L == 9:
            mel = (init.double() @ voc.fb.double()).float().t().contiguous()
        spec, loss, ran = native.inverse_mel(mel[None].contiguous(), voc.fb, voc.fb_nnz, init, IM_ITERS, rows_per_call=1, want_loss=True)
        clips.append((mel, init, spec[0].clone(), loss[0].clone(), int(ran[0])))
    return voc, clips


def _check_inverse_mel(voc, clips, mel_buf, offsets, pitches, what):
    spec, loss, ran = native.inverse_mel_ragged(mel_buf, IM_LENGTHS, voc.fb, voc.fb_nnz, torch.cat([c[1] for c in clips]), IM_ITERS, offsets, pitches, want_loss=True)
    torch.cuda.synchronize()
    o = 0
    for b, (L, (_, _, want, want_loss, want_ran)) in enumerate(zip(IM_LENGTHS, clips)):
        got = spec[o: o + 513 * L].view(513, L)
        o += 513 * L
        assert torch.equal(got, want), (what, b, float((got - want).abs().max()))
        assert int(ran[b]) == want_ran, (what, b, int(ran[b]), want_ran)
        assert torch.equal(loss[b, :want_ran], want_loss[:want_ran]), (what, b)
    return [int(v) for v in ran]


@pytest.mark.parametrize("early", [False, True])
def test_inverse_mel_ragged_is_the_solo_call_per_clip(early):
    voc, clips = _inverse_mel_case(early)
    # (1) a padded tensor whose pad frames hold NaN
    padded = torch.full((len(clips), 80, max(IM_LENGTHS) + 3), NAN, device="cuda")
    for b, (mel, *_) in enumerate(clips):
        padded[b, :, :mel.shape[1]] = mel
    ran = _check_inverse_mel(voc, clips, padded, None, None, "padded")
    # (2) packed blocks of different pitch, NaN between the rows and between the blocks, in a scrambled block order
    pitches = [L + 1 + b for b, L in enumerate(IM_LENGTHS)]
    offsets, floats = [0] * len(clips), 3
    for b in (3, 0, 4, 2, 1):
        offsets[b] = floats
        floats += 80 * pitches[b] + 5
    buf = torch.full((floats,), NAN, device="cuda")
    for b, (mel, *_) in enumerate(clips):
        buf[offsets[b]: offsets[b] + 80 * pitches[b]].view(80, pitches[b])[:, :mel.shape[1]] = mel
    assert _check_inverse_mel(voc, clips, buf, offsets, pitches, "packed") == ran
    if early:
        assert ran == [IM_ITERS, IM_ITERS, 1, IM_ITERS, IM_ITERS], ran
    else:
        assert ran == [IM_ITERS] * 5, ran


def test_inverse_mel_ragged_refuses_a_read_past_the_buffer():
    voc, clips = _inverse_mel_case(False)
    padded = torch.zeros(len(clips), 80, max(IM_LENGTHS), device="cuda")
    off, pitch = native.padded_mel_layout(len(clips), 80, max(IM_LENGTHS))
    with pytest.raises(RuntimeError, match="clip 4:.*past the buffer"):
        native.inverse_mel_ragged(padded, IM_LENGTHS, voc.fb, voc.fb_nnz, torch.cat([c[1] for c in clips]), 2, off[:4] + [off[4] + 1], pitch)


# ------------------------------------------------------------------------------------------------------------------------ Griffin-Lim
GL_LENGTHS = [5, 77, 78, 121, 122, 145]      # both short forms at their boundaries; the tile form with a one-frame (145 = 6 x 24 + 1) and a two-frame last tile


@functools.lru_cache(maxsize=None)
def _griffin_case(iters: int):
    clips = []
    for b, L in enumerate(GL_LENGTHS):
        power = torch.rand(513, L, device="cuda", generator=_gen(30 + b)) ** 4 * 3.0
        ang = torch.rand(513, L, 2, device="cuda", generator=_gen(40 + b))
        clips.append((power, ang, native.griffin_lim(power[None], ang[None], iters)[0].clone()))
    return clips


def _check_griffin(clips, order, iters, pitch):
    lengths = [GL_LENGTHS[i] for i in order]
    out = torch.full((len(order), pitch), NAN, device="cuda")
    native.griffin_lim_ragged(torch.cat([clips[i][0].reshape(-1) for i in order]), torch.cat([clips[i][1].reshape(-1) for i in order]), lengths, iters, out=out)
    torch.cuda.synchronize()
    for row, i in enumerate(order):
        n = 256 * (GL_LENGTHS[i] - 1)
        assert torch.equal(out[row, :n], clips[i][2]), (order, i, float((out[row, :n] - clips[i][2]).abs().max()))
        assert torch.equal(out[row, n:], torch.zeros(pitch - n, device="cuda")), (order, i)      # exact zeros over the NaN pre-fill: every element is written


@pytest.mark.parametrize("iters", [0, 1, 4])
def test_griffin_lim_ragged_is_the_solo_call_per_clip(iters):
    clips = _griffin_case(iters)
    assert GL_LENGTHS[3] == native.GRIFFIN_LIM_SHORT_FRAMES and 256 * (77 - 1) == 19456
    _check_griffin(clips, list(range(6)), iters, 256 * 144 + 7)
    _check_griffin(clips, list(range(6))[::-1], iters, 256 * 144)
    _check_griffin(clips, [4], iters, 256 * 121)                   # the 122-frame clip alone: the tile chain with no short launch


def test_griffin_lim_ragged_launches():
    """Two short launches (the 12-wave and the 8-wave form) plus one tile launch per iteration over the long clips' tiles only."""
    clips = _griffin_case(4)
    native.profile_enable(True)
    try:
        native.profile_reset()
        _check_griffin(clips, list(range(6)), 4, 256 * 144)
        names = {name: n for name, n, _ in native.profile_read()}
    finally:
        native.profile_enable(False)
    assert names.get("vocoder_griffin_lim_ragged") == 1 and "vocoder_griffin_lim" not in names, names


# ------------------------------------------------------------------------------------------------------------------------ ESTOI
ES_COUNTS = [6400, 12800, 26400, 26624, 30976]      # at 16 kHz: 4 000 (too short for one segment), 8 000, 16 500 (short form), 16 640 and 19 360 (long form)


@functools.lru_cache(maxsize=None)
def _estoi_case():
    rng = np.random.default_rng(5)
    pairs = []
    for b, n in enumerate(ES_COUNTS):
        t = np.arange(n) / 16000
        clean = (np.sin(2 * np.pi * (180 + 40 * b) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.3 * t)) + 0.5 * rng.standard_normal(n)).astype(np.float32)
        pred = (clean + 0.7 * clean.std() * rng.standard_normal(n)).astype(np.float32)
        pairs.append((clean, pred))
    return pairs


def test_estoi_ragged_is_the_solo_call_per_clip():
    pairs = _estoi_case()
    host = [metrics.stoi(c, p, 16000, extended=True) for c, p in pairs]
    assert host[0] == 1e-5 and all(h != 1e-5 for h in host[1:]), host
    res = [-(-n * 10000 // 16000) for n in ES_COUNTS]
    assert res[2] <= native.ESTOI_SHORT_SAMPLES < res[3]
    solo = [metrics.estoi_device(torch.from_numpy(c).cuda()[None], torch.from_numpy(p).cuda()[None], 16000) for c, p in pairs]
    for order in (list(range(5)), [4, 3, 2, 1, 0], [3], [2, 0]):
        counts = [ES_COUNTS[i] for i in order]
        pitch = max(counts) + 5
        clean = torch.full((len(order), pitch), NAN, device="cuda")
        pred = torch.full((len(order), pitch), NAN, device="cuda")
        for row, i in enumerate(order):
            clean[row, :counts[row]] = torch.from_numpy(pairs[i][0]).cuda()
            pred[row, :counts[row]] = torch.from_numpy(pairs[i][1]).cuda()
        got = metrics.estoi_device(clean, pred, 16000, lengths=counts)
        zeros = metrics.estoi_device(torch.nan_to_num(clean), torch.nan_to_num(pred), 16000, lengths=counts)
        torch.cuda.synchronize()
        for row, i in enumerate(order):
            assert torch.equal(got[row], solo[i][0]), (order, i, float(got[row]), float(solo[i][0]))
        assert torch.equal(got, zeros)                           # NaN or zeros past n_samples[b]: the same bits
        if 0 in order:
            assert float(got[order.index(0)]) == float(np.float32(1e-5))
    full = metrics.estoi_device(*[torch.stack([torch.nn.functional.pad(torch.from_numpy(x[k]), (0, 30976 - len(x[k]))) for x in pairs]).cuda() for k in (0, 1)],
                                16000, lengths=ES_COUNTS).cpu().numpy()
    assert np.abs(full[1:] - np.array(host[1:])).max() < 1e-4, (full, host)      # the bound tests/test_vocoder_long_gpu.py holds the solo kernel to


def test_estoi_ragged_without_the_resampler():
    x = torch.from_numpy(np.stack([speechlike(30976, seed=s) for s in range(2)]).astype(np.float32)).cuda()
    y = x + 0.3 * x.std() * torch.randn(x.shape, device="cuda", generator=_gen(1))
    counts = [30976, 9000]                                        # already at 10 kHz: the long and the short form, no filter table
    got = metrics.estoi_device(x, y, 10000, lengths=counts)
    for b, n in enumerate(counts):
        assert torch.equal(got[b], metrics.estoi_device(x[b:b + 1, :n].contiguous(), y[b:b + 1, :n].contiguous(), 10000)[0]), b


# ------------------------------------------------------------------------------------------------------------------------ end to end
def test_melspec2audio_lengths_on_the_device_is_the_loop_of_solo_calls(monkeypatch):
    lengths = [33, 5, 130, 78]
    mel = torch.randn(4, 80, 131, device="cuda", generator=_gen(5)) * 2.0 - 5.0
    junk = mel.clone()
    for b, n in enumerate(lengths):
        junk[b, :, n:] = NAN
    g = _gen(9)
    want = [MelSpec2Audio(max_iters=4, backend="hip").cuda()(mel[b:b + 1, :, :n].contiguous(), generator=g)[0] for b, n in enumerate(lengths)]

    def no_stft(*a, **k):
        raise AssertionError("the torch restatement ran")
    monkeypatch.setattr(torch, "stft", no_stft)
    got = MelSpec2Audio(max_iters=4, backend="auto").cuda()(junk, generator=_gen(9), lengths=lengths)
    assert got.shape == (4, 256 * 129)
    for b, n in enumerate(lengths):
        assert torch.equal(got[b, :256 * (n - 1)], want[b]), b
        assert not got[b, 256 * (n - 1):].any(), b


def _eval_loader():
    """Three loader batches of unequal B, T and mel length (train collate layout), clips of 32-60 mel frames with audio a little longer or shorter than
    hop (L_b - 1); the tower stub is keyed by the audio's last sample."""
    shapes = [([7, 13, 22, 16], [60, 45, 33, 52]), ([13, 9], [32, 41]), ([15], [57])]
    embs = [synth.synth_speaker_embedding(len(v), tag=f"vr{i}") for i, (v, _) in enumerate(shapes)]
    mel_t = MelSpectrogram()
    loader = []
    for i, (vl, ml) in enumerate(shapes):
        B, S = len(vl), max(ml)
        al = [256 * (L - 1) + (300 if b % 2 else -200) for b, L in enumerate(ml)]
        audio = torch.zeros(B, max(al) + 1)
        for b in range(B):
            audio[b, :al[b]] = torch.from_numpy(speechlike(al[b], seed=7 * i + b)).float()
        audio[:, -1] = float(i)
        mels = torch.zeros(B, 80, S)
        for b in range(B):
            m = mel_t(audio[b:b + 1, :al[b]])[0, :, :ml[b]]
            mels[b, :, :m.shape[1]] = m
        loader.append(((synth.synth_padded_video(B, vl, tag=f"vr{i}"), torch.tensor(vl)), (audio, torch.tensor(al)), (mels, torch.tensor(ml), torch.zeros(B, S)), None))

    class Tower:
        def inference(self, audios, audio_lengths=None):
            return embs[int(audios[0, -1])].cuda()
    return loader, Tower()


def test_evaluate_net_vocode_lengths(synth_sd):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from model.model import get_network
    net = get_network("test").cuda()
    net.load_state_dict(synth_sd, strict=True)
    loader, tower = _eval_loader()
    runs = {}
    for name, kw in (("dev3", dict(metric="hip", group=3)), ("host3", dict(metric="host", group=3)), ("dev1", dict(metric="hip", group=1))):
        torch.manual_seed(0)
        t = {}
        mean = callers.evaluate_net(net, loader, speaker_encoder=tower, max_iters=4, vocoder_backend="hip", honour_lengths=True, group_lengths=True,
                                    vocode_lengths=True, n_inflight=2, timings=t, vocoder_generator=_gen(3), **kw)
        runs[name] = (mean, t["scores"])
        assert t["clips"] == 7 and len(t["scores"]) == 7
    print("evaluate_net vocode_lengths:", runs)
    assert abs(runs["dev3"][0] - runs["host3"][0]) < 1e-4, runs
    assert max(abs(a - b) for a, b in zip(runs["dev3"][1], runs["host3"][1])) < 1e-4, runs
    assert any(s != float(np.float32(1e-5)) for s in runs["dev3"][1])
    assert runs["dev1"][1] == runs["dev3"][1] and runs["dev1"][0] == runs["dev3"][0], runs      # regrouped: the same bits per clip
    with pytest.raises(ValueError, match="honour_lengths"):
        callers.evaluate_net(net, loader, speaker_encoder=tower, vocode_lengths=True)


def test_vocode_clips_is_the_loop_of_solo_calls(synth_sd):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from model.model import get_network
    net = get_network("test").cuda()
    # the synthetic weights stop every clip at its first frame: a stop bias far below zero lets the clips run to the decoder's 300 frames instead, and the
    # unequal lengths a trained model's stop tokens give are then cut the way demo_clips cuts them (views `mel[:1, :, :n]` of the yielded tensors)
    sd = dict(synth_sd)
    sd["decoder.stop_token_layer.linear_layer.bias"] = torch.full((1,), -1e4)
    net.load_state_dict(sd, strict=True)
    batches = [((synth.synth_video(1, T, tag=f"vc{i}"), torch.tensor([T])), (torch.zeros(1, 600), torch.tensor([600])), None, None, None)
               for i, T in enumerate((15, 9, 22))]
    torch.manual_seed(1)
    mels = [mel for mel, _, _ in callers.demo_clips(net, batches, speaker_embedding=synth.synth_speaker_embedding(1, tag="vc").cuda())]
    assert [tuple(m.shape) for m in mels] == [(1, 80, 300)] * 3
    mels = [m[:1, :, :n] for m, n in zip(mels, (300, 64, 131))]
    assert not mels[1].is_contiguous()
    g = _gen(11)
    voc = MelSpec2Audio(max_iters=4).cuda()
    want = [voc(m.contiguous(), generator=g)[0] for m in mels]
    got = callers.vocode_clips(mels, max_iters=4, generator=_gen(11))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------ tool
def test_time_vocoder_ragged_tool_runs():
    """tools/vocoder_ragged/time_vocoder_ragged.py end to end in a smoke configuration (short clips, two iterations, one round)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CLIPS="4", BATCHES="2", FRAMES="40-125", ROUNDS="1", REPS="1", ITERS="2", DEFAULT_SHAPE="2x122")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "vocoder_ragged", "time_vocoder_ragged.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "(a) solo calls back to back" in r.stdout and "(c) one ragged call" in r.stdout and "waveforms of (c) bit-identical to (a): True" in r.stdout, r.stdout
    assert "l2s_griffin_lim at 2 x 122" in r.stdout
