"""The voice tower over clips of unequal length, host side (no GPU): the three C-ABI symbols are declared, exported and bound;
`l2s_speaker_packed_plan` gives the time-major compact layout the header describes; lengths and offsets outside the limits are refused by row before
anything else is looked at; the Python layers take and forward the audio lengths."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED = ("l2s_speaker_packed_plan", "l2s_speaker_workspace_bytes_packed", "l2s_speaker_encoder_packed")


@pytest.fixture(scope="module")
def L():
    from lip2speech_amd import native
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lip2speech_amd", "csrc"), "-j", "8"], check=True)
    return native.lib()


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def test_symbols_declared_exported_bound(L):
    from lip2speech_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l2s.h")).read(), flags=re.S)
    for sym in PACKED:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} not declared in include/l2s.h"
        assert sym in native.ABI_SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None, f"{sym} has no ctypes signature"
    assert L.l2s_speaker_workspace_bytes_packed.restype is ctypes.c_int64
    assert L.l2s_abi_version() == 2                      # the change only adds symbols
    diag_header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l2s_diag.h")).read(), flags=re.S)
    assert re.search(r"\bl2s_op_speaker_taps_packed\s*\(", diag_header) and "l2s_op_speaker_taps_packed" in native.DIAG_SYMBOLS
    assert not hasattr(L, "l2s_op_speaker_taps_packed")  # the product library exports the product ABI only
    assert hasattr(native.NativeModel, "speaker_encoder_packed")


def _numpy_plan(ns):
    L = np.asarray(ns) // 160 + 1
    order = np.argsort(-L, kind="stable")
    rows = np.array([(L > t).sum() for t in range(L.max())])
    return list(order), list(rows), [0] + list(np.cumsum(rows)), int(L.max()), int(L.sum())


@pytest.mark.parametrize("ns", [[201, 360, 16000, 360], [1761] * 5, [16079], [3200, 3359, 480, 3200, 639, 3210]],
                         ids=["mixed", "all-equal", "B=1", "ties-keep-call-order"])
def test_plan_against_numpy(L, ns):
    """L_b = n_b // 160 + 1; clips by L_b descending, ties in call order (3200, 3359 and 3210 samples all have 21 frames; 480 and 639 both 4);
    step_rows[t] = #{L_b > t} never rises; step_row0 its prefix sum over L_max + 1 entries; R = sum L_b"""
    from lip2speech_amd import native
    order, rows, row0, L_max, R = native.speaker_packed_plan(ns)
    assert (order, rows, row0, L_max, R) == _numpy_plan(ns)
    assert R == sum(n // 160 + 1 for n in ns) == row0[-1] and L_max == max(ns) // 160 + 1 and len(row0) == L_max + 1
    assert all(a >= b for a, b in zip(rows, rows[1:])) and rows[0] == len(ns) and rows[-1] >= 1
    if ns == [3200, 3359, 480, 3200, 639, 3210]:
        assert order == [0, 1, 3, 5, 2, 4]
    # every (rank, frame) has a row of its own
    seen = sorted(row0[l] + r for r, b in enumerate(order) for l in range(ns[b] // 160 + 1))
    assert seen == list(range(R))


def test_errors_name_the_row(L):
    """n_b = 200 and a negative offset: refused by row - by the plan, the workspace query (-1) and the entry point itself, which looks at the rows
    before it looks at the model (a model without weights, pointers that are never followed)"""
    from lip2speech_amd import native
    with pytest.raises(RuntimeError, match=r"n_samples\[2\] = 200 is outside \[201, 2\^30\]"):
        native.speaker_packed_plan([201, 360, 200, 16000])
    with pytest.raises(RuntimeError, match=r"n_samples\[0\] = -5 "):
        native.speaker_packed_plan([-5, 360])
    assert native.speaker_packed_plan([201])[3:] == (2, 2)           # the limit itself is legal
    assert L.l2s_speaker_workspace_bytes_packed(_i64([201, 200]), 2) == -1 and b"n_samples[1] = 200" in L.l2s_last_error()
    assert L.l2s_speaker_workspace_bytes_packed(_i64([201]), 0) == -1 and b"B = 0" in L.l2s_last_error()
    assert L.l2s_speaker_workspace_bytes_packed(_i64([2 ** 30 + 1]), 1) == -1 and b"n_samples[0]" in L.l2s_last_error()
    # R = sum L_b beyond L2S_SPK_MAX_ROWS: 1 clip of 2^30 samples has 6 710 887 frames
    assert L.l2s_speaker_workspace_bytes_packed(_i64([2 ** 30]), 1) == -1 and b"L2S_SPK_MAX_ROWS" in L.l2s_last_error()
    nm = native.NativeModel()
    fake = ctypes.c_void_p(4096)                                     # non-null, never dereferenced: every call below is refused first
    for off, ns, msg in (([0, 1000], [1000, 200], "n_samples[1] = 200"), ([0, -4], [1000, 1000], "offsets[1] = -4 is negative")):
        rc = L.l2s_speaker_encoder_packed(nm._h, fake, _i64(off), _i64(ns), 2, fake, fake, ctypes.c_int64(1 << 30), None)
        assert rc != 0 and msg in L.l2s_last_error().decode()
    rc = L.l2s_speaker_encoder_packed(nm._h, fake, _i64([0, 1000]), _i64([1000, 1000]), 2, fake, fake, ctypes.c_int64(1 << 30), None)
    assert rc != 0 and "not finalized" in L.l2s_last_error().decode()   # legal rows: now the model is looked at


def test_workspace_is_sized_from_the_compact_rows(L):
    """R rows, not B x L_max: 16 clips of 1 s plus one of 3 s need well under the padded call's workspace, and the query grows with every clip"""
    ns = [16000] * 16 + [48000]
    packed = L.l2s_speaker_workspace_bytes_packed(_i64(ns), len(ns))
    padded = L.l2s_speaker_workspace_bytes(len(ns), 48000)
    R, BL = sum(n // 160 + 1 for n in ns), len(ns) * 301
    assert 0 < packed < padded and packed / padded < 1.1 * R / BL
    assert L.l2s_speaker_workspace_bytes_packed(_i64(ns + [201]), len(ns) + 1) > packed
    assert L.l2s_speaker_workspace_bytes_packed(_i64([48000] * 4), 4) >= L.l2s_speaker_workspace_bytes(4, 48000)      # all equal: at least the padded call's


def test_python_layers_take_and_forward_lengths():
    from lip2speech_amd import callers
    from model.modules import SpeakerEncoder
    sig = inspect.signature(SpeakerEncoder.inference)
    assert list(sig.parameters)[1:] == ["x", "audio_lengths"] and sig.parameters["audio_lengths"].default is None
    assert hasattr(SpeakerEncoder, "inference_packed")

    class Stub:
        def __init__(self):
            self.seen = []

        def inference(self, x, **kw):
            self.seen.append(kw)
            return torch.zeros(x.shape[0], 256)

    class Net:
        honour_video_lengths = False

        def inference(self, videos, faces, **kw):
            self.kw = kw
            B = videos.shape[0]
            return torch.zeros(B, 80, 4), torch.full((B,), 4), torch.zeros(B, 4, videos.shape[2])

        def __call__(self, *a, **kw):
            return [None, torch.zeros(2, 80, 4)]

        def native_model(self):
            raise AssertionError("no option is set in this test")

    audios, alen, vlen = torch.zeros(2, 1000), torch.tensor([640, 1000]), torch.tensor([7, 9])
    batch = ((torch.zeros(2, 3, 9, 8, 8), vlen), (audios, alen), None, None, None)
    spk, net = Stub(), Net()
    real = callers.native.check_persist_timeouts
    callers.native.check_persist_timeouts = lambda: None
    try:
        callers.demo_clip(net, batch, speaker_encoder=spk, device="cpu")
        assert spk.seen == [{}] and net.kw["video_lengths"] is None           # the default: today's call, no keyword at all
        callers.demo_clip(net, batch, speaker_encoder=spk, device="cpu", honour_lengths=True)
        assert spk.seen[1]["audio_lengths"] is alen and net.kw["video_lengths"] is vlen
        list(callers.demo_clips(net, [batch], speaker_encoder=spk, device="cpu", honour_lengths=True))
        assert spk.seen[2]["audio_lengths"] is alen
    finally:
        callers.native.check_persist_timeouts = real
    # evaluate.py's loop (train collate layout): lengths only under honour_lengths
    ebatch = ((torch.zeros(2, 3, 9, 8, 8), vlen), (audios, alen), (torch.zeros(2, 80, 4), torch.tensor([4, 4]), None), None)
    spk = Stub()
    list(callers._evaluate_outputs(net, [ebatch], spk, "cpu", 8, 3, honour_lengths=True))
    assert spk.seen == [{"audio_lengths": alen}] and spk.seen[0]["audio_lengths"] is alen
    # _voice_embedding itself: the face route and a supplied embedding never reach the tower
    spk = Stub()
    assert callers._voice_embedding("face", spk, None, audios, "cpu", alen) is None
    given = torch.ones(2, 256)
    assert callers._voice_embedding("voice", spk, given, audios, "cpu", alen) is given and spk.seen == []
    callers._voice_embedding("voice", spk, None, audios, "cpu")
    callers._voice_embedding("voice", spk, None, audios, "cpu", alen)
    assert spk.seen == [{}, {"audio_lengths": alen}]


def test_python_validation_comes_first():
    """lengths are checked on the host before a tensor is touched; CPU tensors then meet the no-fallback error"""
    from lip2speech_amd import native
    nm = native.NativeModel()
    x = torch.zeros(2, 1000)
    with pytest.raises(TypeError):
        native._host_ints([640.0, 1000.0], "samples")
    with pytest.raises(TypeError):
        native._host_ints(torch.tensor([640.0, 1000.0]), "samples")
    assert native._host_ints(torch.tensor([640, 1000]), "samples") == [640, 1000] == native._host_ints(np.array([640, 1000]), "samples")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nm.speaker_encoder_packed(x, [0, 1000], [640, 1000])
