"""Per-clip video lengths, host side (no GPU): the new C-ABI symbols are declared, exported and bound; the library's BiLSTM launch planner gives
the plan the header describes; the Python plumbing validates `video_lengths` before any native call; the switches default to off."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKED = ("l2s_workspace_bytes_masked", "l2s_masked_bilstm_plan", "l2s_inference_masked", "l2s_forward_eval_masked", "l2s_decoder_prologue_masked",
          "l2s_decode_steps_masked")


@pytest.fixture(scope="module")
def L():
    from lip2speech_amd import native
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lip2speech_amd", "csrc"), "-j", "8"], check=True)
    return native.lib()


def test_symbols_declared_exported_bound(L):
    from lip2speech_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l2s.h")).read(), flags=re.S)
    for sym in MASKED:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} not declared in include/l2s.h"
        assert sym in native.ABI_SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None, f"{sym} has no ctypes signature"
    # one extra argument, the host length array, after the unmasked signature
    for sym in ("l2s_inference", "l2s_forward_eval", "l2s_decoder_prologue", "l2s_decode_steps"):
        base, masked = getattr(L, sym).argtypes, getattr(L, sym + "_masked").argtypes
        assert list(masked[:-1]) == list(base) and masked[-1] == ctypes.POINTER(ctypes.c_int32)
    assert L.l2s_abi_version() == 2
    # out of scope, and absent rather than silently unmasked: grouped and training forms
    for sym in ("l2s_inference_multi_masked", "l2s_forward_eval_multi_masked", "l2s_train_prologue_fwd_masked", "l2s_train_steps_fwd_masked"):
        assert not hasattr(L, sym)
    # the length table fits the masked workspace query; the unmasked query is what it was
    for B in (1, 4, 64, 256):
        assert L.l2s_workspace_bytes_masked(B, 29, 96, 96, 300) >= L.l2s_workspace_bytes(B, 29, 96, 96, 300) + 2 * 4 * B


def test_bilstm_launch_plan(L):
    """include/l2s.h: capture AFTER step len_b - 1 (forward finals of the clips that ended there), reset BEFORE step T - len_b for len_b < T (the
    backward direction reads frame T-1-step); ascending, no repeats."""
    from lip2speech_amd import native
    assert native.masked_bilstm_plan([7, 13, 22, 16], 22) == ([6, 12, 15, 21], [6, 9, 15])
    assert native.masked_bilstm_plan([14, 14], 14) == ([13], [])                                  # all full length: one capture, no reset
    assert native.masked_bilstm_plan([13, 9, 13, 9, 7], 13) == ([6, 8, 12], [4, 6])               # repeats collapse: at most 2 x (distinct lengths) launches
    lens = [7, 13, 22, 16]
    cap, rst = native.masked_bilstm_plan(lens, 22)
    assert cap == sorted({n - 1 for n in lens}) and rst == sorted({22 - n for n in lens if n < 22})
    for bad in ([6, 13], [7, 23]):
        with pytest.raises(RuntimeError, match=r"outside \[7, T = 22\]"):
            native.masked_bilstm_plan(bad, 22)
    assert [native.min_T(n) for n in lens] == [n // 7 for n in lens] == [1, 1, 3, 2]               # m_b of the test batch


def test_video_lengths_validated_before_the_call():
    from lip2speech_amd import native
    arr = native.video_lengths_array([7, 13, 22, 16], 4, 22)
    assert list(arr) == [7, 13, 22, 16] and isinstance(arr, ctypes.Array) and arr._type_ is ctypes.c_int32
    assert list(native.video_lengths_array(torch.tensor([9, 8], dtype=torch.int64), 2, 9)) == [9, 8]
    with pytest.raises(ValueError, match="shape"):
        native.video_lengths_array([7, 13, 22], 4, 22)
    with pytest.raises(ValueError, match="shape"):
        native.video_lengths_array(torch.tensor([[7, 13]]), 2, 22)
    with pytest.raises(TypeError):
        native.video_lengths_array(torch.tensor([7.0, 13.0]), 2, 22)
    with pytest.raises(TypeError):
        native.video_lengths_array([7.5, 13], 2, 22)
    for bad in (6, 23, -1):
        with pytest.raises(ValueError, match=r"outside \[7, T = 22\]"):
            native.video_lengths_array([7, bad], 2, 22)
    # NativeModel.inference checks shapes, dtype and range before anything reaches the device: CPU tensors still raise the no-fallback error first
    nm = native.NativeModel()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nm.inference(torch.zeros(1, 3, 8, 96, 96), torch.zeros(1, 256), torch.zeros(1, 501), S=4, video_lengths=[8])
    with pytest.raises(NotImplementedError):
        nm.inference_multi([], S=4, video_lengths=[8])


def test_switches_default_off_and_train_mode_raises():
    import hparams
    from model.model import Lip2Speech, get_network
    import inspect
    assert hparams.create_hparams().mask_padding is True           # the reference's dead flag stays what it was - and switches nothing on:
    net = get_network("test")
    assert net.honour_video_lengths is False
    sig = inspect.signature(Lip2Speech.inference).parameters
    assert sig["video_lengths"].default is None and any(p.kind is p.VAR_KEYWORD for p in sig.values())
    tr = get_network("train")
    tr.honour_video_lengths = True
    with pytest.raises(NotImplementedError, match="length-masked"):
        tr(torch.zeros(1, 3, 8, 96, 96), None, None, torch.zeros(1, 80, 4), torch.tensor([8]), None, None, 1.0, speaker_embedding=torch.zeros(1, 256))
    net.honour_video_lengths = True
    with pytest.raises(NotImplementedError):
        list(net.forward_many([]))
