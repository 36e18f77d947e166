"""The ragged forms of the vocoder and the metric (include/l2s.h `l2s_inverse_mel_ragged`, `l2s_griffin_lim_ragged`, `l2s_estoi_ragged`), the parts that need
no GPU: the pure host checks and workspace sizers, the `lengths=` keyword of `MelSpec2Audio` on the torch backend, the property of `resample_poly_plan` the
one-FIR-per-call contract rests on, and the `vocode_lengths` route of `evaluate_net` with the host metric."""
import numpy as np
import pytest
import torch

from lip2speech_amd import callers, metrics, native
from lip2speech_amd.datasets.spectrograms import MelSpec2Audio

from test_vocoder_metrics import speechlike


def _refused(fn, *a, **k):
    with pytest.raises(RuntimeError) as e:
        fn(*a, **k)
    return str(e.value)


def test_inverse_mel_check_names_the_clip():
    L = [9, 5, 130]
    off, pitch = native.padded_mel_layout(3, 80, 130)
    native.inverse_mel_ragged_check(L, off, pitch, 3 * 80 * 130, 80, 513, 1000, 4)
    assert "clip 1: 4 frames" in _refused(native.inverse_mel_ragged_check, [9, 4, 130], off, pitch, 3 * 80 * 130, 80, 513, 1000, 4)
    # the last clip's last band ends one float past the stated buffer
    msg = _refused(native.inverse_mel_ragged_check, L, off, pitch, 3 * 80 * 130 - 1, 80, 513, 1000, 4)
    assert "clip 2:" in msg and "past the buffer" in msg
    # a pitch that walks out of the buffer, and one below the clip's frames
    native.inverse_mel_ragged_check(L, off, [130, 131, 130], 3 * 80 * 130, 80, 513, 1000, 4)      # clip 1 strays into clip 2's floats, not out of the buffer
    msg = _refused(native.inverse_mel_ragged_check, L, off, [130, 130, 131], 3 * 80 * 130, 80, 513, 1000, 4)
    assert "clip 2:" in msg and "pitch 131" in msg and "past the buffer" in msg
    msg = _refused(native.inverse_mel_ragged_check, [9, 5, 130, 5], off + [31196], pitch + [130], 3 * 80 * 130, 80, 513, 1000, 4)
    assert "clip 3:" in msg and "offset 31196" in msg
    assert "clip 0: mel pitch 8" in _refused(native.inverse_mel_ragged_check, L, off, [8, 130, 130], 3 * 80 * 130, 80, 513, 1000, 4)
    assert "clip 2: mel offset -1" in _refused(native.inverse_mel_ragged_check, L, [0, 10400, -1], pitch, 3 * 80 * 130, 80, 513, 1000, 4)
    assert "N = 0" in _refused(native.inverse_mel_ragged_check, [], [], [], 0, 80, 513, 1000, 4)
    assert "N = 65536" in _refused(native.inverse_mel_ragged_check, L, off, pitch, 3 * 80 * 130, 80, 513, 1000, 4, N=65536)
    assert "null table" in _refused(native.inverse_mel_ragged_check, None, off, pitch, 3 * 80 * 130, 80, 513, 1000, 4, N=3)
    assert "null table" in _refused(native.inverse_mel_ragged_check, L, None, pitch, 3 * 80 * 130, 80, 513, 1000, 4)
    assert "128 mel bands" in _refused(native.inverse_mel_ragged_check, L, off, pitch, 3 * 80 * 130, 129, 513, 1000, 4)


def test_griffin_lim_check_names_the_clip():
    native.griffin_lim_ragged_check([5, 122, 77], 4, 256 * 121)
    assert "clip 2: 3 frames" in _refused(native.griffin_lim_ragged_check, [5, 122, 3], 4, 256 * 121)
    msg = _refused(native.griffin_lim_ragged_check, [5, 122, 77], 4, 256 * 121 - 1)
    assert "clip 1:" in msg and "overlap" in msg
    assert "N = 0" in _refused(native.griffin_lim_ragged_check, [], 4, 1024)
    assert "null table" in _refused(native.griffin_lim_ragged_check, None, 4, 1024, N=2)
    assert "n_fft" in _refused(native.griffin_lim_ragged_check, [5, 6], 4, 4096, n_fft=512)
    assert "clip 0:" in _refused(native.griffin_lim_ragged_check, [(1 << 20) + 1], 4, 1 << 40)


def test_estoi_check_names_the_clip():
    ok = dict(pitch=30976, has_fir=True, n_fir_max=700, up=5, down=8, n_pre_remove=40)
    native.estoi_ragged_check([6400, 30976], [650, 700], [4000, 19360], **ok)
    assert "clip 1: 48257 samples at 10 kHz" in _refused(native.estoi_ragged_check, [6400, 30976], [650, 700], [4000, 48257], **ok)
    assert "clip 0:" in _refused(native.estoi_ragged_check, [0, 30976], [650, 700], [4000, 19360], **ok)
    msg = _refused(native.estoi_ragged_check, [6400, 30977], [650, 700], [4000, 19360], **ok)
    assert "clip 1:" in msg and "overlap" in msg
    assert "clip 0: its filter of 701 taps" in _refused(native.estoi_ragged_check, [6400, 30976], [701, 700], [4000, 19360], **ok)
    assert "N = 0" in _refused(native.estoi_ragged_check, [], [], [], **ok)
    assert "null table" in _refused(native.estoi_ragged_check, None, [650, 700], [4000, 19360], N=2, **ok)
    assert "null table" in _refused(native.estoi_ragged_check, [6400, 30976], None, [4000, 19360], **ok)
    no_fir = dict(pitch=30976, has_fir=False, n_fir_max=0, up=1, down=1, n_pre_remove=0)
    native.estoi_ragged_check([6400, 30976], None, [6400, 30976], **no_fir)
    assert "clip 1: without a resampling filter" in _refused(native.estoi_ragged_check, [6400, 30976], None, [6400, 30000], **no_fir)


def test_workspace_sizers_grow_with_the_frames_and_cover_the_solo_calls():
    L = native.lib()
    tables = [[5], [5, 8], [5, 8, 9, 77, 130], [5, 8, 9, 78, 130], [5, 8, 9, 121, 131], [122, 145, 188, 300]]
    for iters in (0, 4, 256):
        sizes = [native.inverse_mel_ragged_workspace_bytes(t, 80, 513, iters) for t in tables]
        for t, s in zip(tables, sizes):
            assert s >= sum(L.l2s_inverse_mel_workspace_bytes(1, n, 80, 513, 1, iters) for n in t), (t, iters)
        assert sizes[2] <= sizes[3] <= sizes[4] and sizes[0] < sizes[1] < sizes[2]
    sizes = [native.griffin_lim_ragged_workspace_bytes(t) for t in tables]
    for t, s in zip(tables, sizes):
        assert s >= sum(L.l2s_griffin_lim_workspace_bytes(1, n) for n in t), t
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3] < sizes[4]
    res = [[4000], [4000, 16512], [4000, 16512, 16513], [4000, 16512, 48256]]
    sizes = [native.estoi_ragged_workspace_bytes(t) for t in res]
    for t, s in zip(res, sizes):
        assert s >= sum(L.l2s_estoi_workspace_bytes_long(1, n) for n in t), t
    assert sizes[0] < sizes[1] < sizes[2] == sizes[3]
    assert L.l2s_griffin_lim_ragged_workspace_bytes(None, 2) == -1 and b"null table" in L.l2s_last_error()
    assert native.inverse_mel_ragged_workspace_bytes([5, 4], 80, 513, 4) == -1


def test_melspec2audio_lengths_is_the_loop_of_solo_calls_on_the_torch_backend():
    g = torch.Generator()
    lengths = [9, 5, 12, 7]
    mel = torch.randn(4, 80, 12, generator=g.manual_seed(5)) * 2.0 - 5.0
    junk = mel.clone()
    for b, n in enumerate(lengths):
        junk[b, :, n:] = float("nan")                        # what pads a clip is never read
    voc = MelSpec2Audio(max_iters=6, backend="torch")
    got = voc(junk, generator=g.manual_seed(9), lengths=lengths)
    assert got.shape == (4, 256 * 11)
    g.manual_seed(9)
    for b, n in enumerate(lengths):
        want = voc(mel[b:b + 1, :, :n], generator=g)
        assert torch.equal(got[b, :256 * (n - 1)], want[0]), b
        assert torch.equal(got[b, 256 * (n - 1):], torch.zeros(256 * (12 - n))), b
    # the stages on their own draw clip by clip too
    spec = voc.inverse_mel(torch.exp(junk), generator=g.manual_seed(3), lengths=lengths)
    g.manual_seed(3)
    for b, n in enumerate(lengths):
        assert torch.equal(spec[b, :, :n], voc.inverse_mel(torch.exp(mel[b:b + 1, :, :n]), generator=g)[0]), b
        assert float(spec[b, :, n:].abs().sum()) == 0.0
    wave = voc.griffin_lim(spec, generator=g.manual_seed(4), lengths=lengths)
    g.manual_seed(4)
    for b, n in enumerate(lengths):
        assert torch.equal(wave[b, :256 * (n - 1)], voc.griffin_lim(spec[b:b + 1, :, :n], generator=g)[0]), b
    # lengths=None: today's call, unchanged by the keyword
    assert torch.equal(voc(mel, generator=g.manual_seed(9), lengths=None), voc(mel, generator=g.manual_seed(9)))
    assert torch.equal(voc(mel, generator=g.manual_seed(9), rows_per_call=2, lengths=None), voc(mel, generator=g.manual_seed(9), rows_per_call=2))
    with pytest.raises(ValueError):
        voc(mel, lengths=[9, 5, 13, 7])
    with pytest.raises(ValueError):
        voc(mel, lengths=[9, 5, 12])


@pytest.mark.parametrize("fs", [16000, 22050, 8000])
def test_resample_plans_of_shorter_clips_are_prefixes_of_the_longest(fs):
    """What lets one FIR table serve a ragged ESTOI call: for a fixed up / down the plans differ only in the trailing zero pad."""
    lengths = [6400, 12800, 26400, 26624, 30976, 5, 30975]
    plans = {n: metrics.resample_poly_plan(n, metrics.FS, fs) for n in lengths}
    h_max, up, down, pre, _ = plans[max(lengths)]
    for n, (h, u, d, p, n_out) in plans.items():
        assert (u, d, p) == (up, down, pre)
        assert len(h) <= len(h_max) and np.array_equal(h, h_max[:len(h)]), n
        assert n_out == -(-n * up // down)
        assert np.allclose(metrics.resample_oct(np.ones(n), metrics.FS, fs).shape, n_out)


class _FakeNet(torch.nn.Module):
    """`net(...)[1]` = a fixed log-mel per batch: the model half of evaluate_net without a GPU."""

    def __init__(self, mels):
        super().__init__()
        self.mels, self.calls, self.honour_video_lengths = mels, 0, False

    def forward(self, videos, face_crops, audios, melspecs, vlen, alen, mlen, tf_ratio, speaker_embedding=None):
        assert self.honour_video_lengths
        self.calls += 1
        return [None, self.mels[self.calls - 1]]


def _host_batches():
    g = torch.Generator()
    shapes = [([40, 34], [9984, 9000]), ([36], [8700]), ([33, 38, 45], [8192, 12000, 10000])]      # (mel lengths, audio lengths) per batch
    batches, mels = [], []
    for i, (ml, al) in enumerate(shapes):
        B, S, A = len(ml), max(ml), max(al)
        audio = torch.stack([torch.from_numpy(speechlike(A, seed=10 * i + b)).float() for b in range(B)])
        for b in range(B):
            audio[b, al[b]:] = 0
        mels.append(torch.randn(B, 80, S, generator=g.manual_seed(i)) * 2.0 - 5.0)
        batches.append(((torch.zeros(B, 3, 4, 8, 8), torch.full((B,), 4)), (audio, torch.tensor(al)), (mels[-1], torch.tensor(ml), torch.zeros(B, S)), None))
    return batches, mels, shapes


def test_evaluate_net_vocode_lengths_requires_honour_lengths():
    batches, mels, _ = _host_batches()
    with pytest.raises(ValueError, match="honour_lengths"):
        callers.evaluate_net(_FakeNet(mels), batches, device="cpu", vocode_lengths=True)
    with pytest.raises(ValueError, match="honour_lengths"):
        callers.evaluate_net(_FakeNet(mels), batches, device="cpu", vocode_lengths=True, group_lengths=True)


@pytest.mark.parametrize("group", [1, 2, 8])
def test_evaluate_net_vocode_lengths_host_metric_scores_the_per_clip_slices(group):
    batches, mels, shapes = _host_batches()
    g = torch.Generator()
    t = {}
    got = callers.evaluate_net(_FakeNet(mels), batches, device="cpu", max_iters=3, vocoder_backend="torch", metric="host", encoding="face",
                               honour_lengths=True, vocode_lengths=True, group=group, timings=t, vocoder_generator=g.manual_seed(7))
    voc = MelSpec2Audio(max_iters=3, backend="torch")
    g.manual_seed(7)
    want = []
    for (_, (audio, _), _, _), mel, (ml, al) in zip(batches, mels, shapes):
        for b, (L, a) in enumerate(zip(ml, al)):
            pred = voc(mel[b:b + 1, :, :L], generator=g)[0].numpy()
            n = min(a, 256 * (L - 1))
            want.append(metrics.stoi(audio[b, :n].numpy(), pred[:n], 16000, extended=True))
    assert t["scores"] == want and t["clips"] == 6
    assert all(w != 1e-5 for w in want), want                # every clip is long enough for a segment: the scores are real ones
    assert got == sum(want) / len(want)
