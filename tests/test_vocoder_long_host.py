"""Host side of the long vocoder / metric forms (no GPU): workspace sizes, the exported symbol, the routing predicate and `evaluate_net`'s
flush rule."""
import ctypes

import numpy as np
import pytest
import torch

from lip2speech_amd import callers, native
from lip2speech_amd.datasets.spectrograms import MelSpec2Audio


@pytest.fixture(scope="module")
def L():
    return native.lib()


def test_griffin_lim_workspace_keeps_its_short_size_and_grows_past_121_frames(L):
    for N in (1, 3, 32):
        assert L.l2s_griffin_lim_workspace_bytes(N, 121) == N * 121 * 520 * 4 + N * 2 * 121 * 520 * 8 + 512
        assert L.l2s_griffin_lim_workspace_bytes(N, 77) == N * 77 * 520 * 4 + N * 2 * 77 * 520 * 8 + 512
        per_frame_short = (L.l2s_griffin_lim_workspace_bytes(N, 121) - 512) / (N * 121)
        per_frame_long = (L.l2s_griffin_lim_workspace_bytes(N, 122) - 512) / (N * 122)
        assert per_frame_long > per_frame_short
        assert L.l2s_griffin_lim_workspace_bytes(N, 300) == N * 300 * 520 * 4 + N * 3 * 300 * 520 * 8 + 512      # three rotating slots: 14 560 B per frame
    assert native.GRIFFIN_LIM_SHORT_FRAMES == 121 and 2 <= native.GRIFFIN_LIM_TILE_FRAMES <= 121


def test_estoi_long_workspace_query_is_exported_and_continues_the_short_one(L):
    assert "l2s_estoi_workspace_bytes_long" in native.ABI_SYMBOLS and hasattr(ctypes.CDLL(native.LIB_PATH), "l2s_estoi_workspace_bytes_long")
    assert L.l2s_abi_version() == 2
    for N in (1, 4, 32):
        assert L.l2s_estoi_workspace_bytes_long(N, 16512) == L.l2s_estoi_workspace_bytes(N)
        assert L.l2s_estoi_workspace_bytes_long(N, 100) == L.l2s_estoi_workspace_bytes(N)
        assert L.l2s_estoi_workspace_bytes_long(N, 16513) > L.l2s_estoi_workspace_bytes(N)
        assert L.l2s_estoi_workspace_bytes_long(N, 48000) >= N * 2 * 2 * 48000 * 4      # both signals twice: resampled, and without the silent frames
    assert native.ESTOI_SHORT_SAMPLES == 16512 and native.ESTOI_MAX_SAMPLES >= 48000


def test_estoi_past_the_built_maximum_names_it(L):
    """Argument checks come before any launch: a call past the long form's maximum fails with that maximum in the message."""
    bands = (ctypes.c_int * 30)(*([0] * 30))
    one = ctypes.c_void_p(256)                   # never dereferenced: the size check comes first
    rc = L.l2s_estoi(one, one, 1, native.ESTOI_MAX_SAMPLES + 1, None, 0, 1, 1, 0, native.ESTOI_MAX_SAMPLES + 1, bands, one, one, 1 << 40, None)
    assert rc != 0 and b"48 256" in L.l2s_last_error()


class _Dev:
    """What `_use_hip` reads of a tensor."""
    is_cuda = True


def test_melspec2audio_takes_the_device_path_at_any_length():
    voc = MelSpec2Audio(max_iters=1, backend="auto")
    assert voc._use_hip(_Dev(), 300) and voc._use_hip(_Dev(), 122) and voc._use_hip(_Dev(), 121) and voc._use_hip(_Dev(), 5)
    assert not voc._use_hip(_Dev(), 4) and not voc._use_hip(torch.zeros(1), 300)
    assert MelSpec2Audio(max_iters=1, backend="hip")._use_hip(_Dev(), 300)
    with pytest.raises(RuntimeError, match="at least 5 frames"):
        MelSpec2Audio(max_iters=1, backend="hip")._use_hip(_Dev(), 4)
    assert not MelSpec2Audio(max_iters=1, backend="torch")._use_hip(_Dev(), 300)


def test_evaluate_net_flushes_a_group_when_the_audio_width_changes(monkeypatch):
    """Batches of one mel shape but different audio widths are vocoded and scored per equal-width run: the widths inside a pass are equal,
    and the mean is the mean of the batches scored on their own."""
    S, B = 40, 2
    rng = np.random.default_rng(0)
    widths = [256 * (S - 1), 256 * (S - 1), 256 * (S - 1) + 512, 256 * (S - 1)]
    batches = [(None, (torch.from_numpy(rng.standard_normal((B, w))).float(), torch.full((B,), w)), None, None) for w in widths]
    mels = [torch.from_numpy(rng.standard_normal((B, 80, S))).float() - 5.0 for _ in widths]

    def outputs(net, bs, *a, **k):
        for b, m in zip(bs, mels):
            yield b, (None, m)
    monkeypatch.setattr(callers, "_evaluate_outputs", outputs)
    passes = []
    real = MelSpec2Audio.forward

    def forward(self, melspec, generator=None, rows_per_call=None):
        passes.append(melspec.shape[0] // B)
        return real(self, melspec, generator, rows_per_call)
    monkeypatch.setattr(MelSpec2Audio, "forward", forward)
    net = torch.nn.Linear(1, 1)
    torch.manual_seed(0)
    grouped = callers.evaluate_net(net, batches, device="cpu", max_iters=2, vocoder_backend="torch", metric="host", group=8)
    assert passes == [2, 1, 1]
    del passes[:]
    torch.manual_seed(0)
    single = callers.evaluate_net(net, batches, device="cpu", max_iters=2, vocoder_backend="torch", metric="host", group=1)
    assert passes == [1, 1, 1, 1]
    assert np.isfinite(grouped) and np.isfinite(single)
