"""Training with per-clip mel lengths (include/l2s.h "training with per-clip mel lengths"), the parts that need no GPU: the entry points are declared,
exported and bound; the pure checks refuse each bad table and name the clip; the Python switches default off and refuse what the library refuses."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["l2s_loss_lengths_check", "l2s_train_scratch_bytes_lengths", "l2s_loss_lengths", "l2s_train_postnet_tape_floats_masked",
           "l2s_train_postnet_ws_bytes_masked", "l2s_train_postnet_masked_fwd", "l2s_train_postnet_masked_bwd"]


@pytest.fixture(scope="module")
def L():
    from lip2speech_amd import native
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lip2speech_amd", "csrc"), "-j", "8"], check=True)
    return native.lib()


def test_symbols_declared_exported_bound(L):
    from lip2speech_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l2s.h")).read(), flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} not declared in include/l2s.h"
        assert sym in native.ABI_SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None, f"{sym} has no ctypes signature"
    # ABI_SYMBOLS is exactly what the header declares
    declared = set(re.findall(r"\b(l2s_[A-Za-z0-9_]+)\s*\(", header))
    assert declared == set(native.ABI_SYMBOLS), declared ^ set(native.ABI_SYMBOLS)
    lens = ctypes.POINTER(ctypes.c_int32)
    for d in ("fwd", "bwd"):      # the unmasked signature plus the host length array
        base, masked = getattr(L, f"l2s_train_postnet_{d}").argtypes, getattr(L, f"l2s_train_postnet_masked_{d}").argtypes
        assert list(masked[:-1]) == list(base) and masked[-1] == lens
    assert list(L.l2s_loss_lengths.argtypes[:len(L.l2s_loss.argtypes)]) == list(L.l2s_loss.argtypes)
    assert L.l2s_abi_version() == 2
    # the names whose absence tests/test_masked_lengths_host.py pins stay absent
    assert not hasattr(L, "l2s_train_postnet_fwd_masked") and not hasattr(L, "l2s_train_postnet_bwd_masked")


def test_sizers(L):
    """The post-net's device table (S_b, m_b: 2 x B int32) lives behind the unmasked tape; the loss scratch covers l2s_loss's (equal lengths run its launches)
    plus four fp64 partials per clip and block and the table."""
    for B, S in ((1, 6), (4, 8), (17, 3), (16, 188), (96, 300)):
        assert L.l2s_train_postnet_tape_floats_masked(B, S) >= L.l2s_train_postnet_tape_floats(B, S) + 2 * B
        assert L.l2s_train_postnet_ws_bytes_masked(B, S) >= L.l2s_train_postnet_ws_bytes(B, S)
        assert L.l2s_train_scratch_bytes_lengths(B) >= L.l2s_train_scratch_bytes() + B * 4 * 8 + 2 * B * 4
    assert L.l2s_train_scratch_bytes_lengths(0) == -1 and L.l2s_train_scratch_bytes_lengths(97) == -1


def test_pure_checks_refuse_each_bad_table_by_clip(L):
    from lip2speech_amd import native
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    S, T = 8, 22

    def refused(match, *args):
        assert L.l2s_loss_lengths_check(*args) != 0
        with pytest.raises(RuntimeError, match=match):
            native.check(1, L)
    assert L.l2s_loss_lengths_check(i32(8, 1, 5, 7), None, 4, S, T) == 0
    assert L.l2s_loss_lengths_check(i32(8, 1, 5, 7), i32(7, 13, 22, 16), 4, S, T) == 0
    refused(r"mel_lengths\[1\] = 0 is outside \[1, S = 8\]", i32(8, 0, 5, 7), None, 4, S, T)
    refused(r"mel_lengths\[3\] = 9 is outside \[1, S = 8\]", i32(8, 1, 5, 9), None, 4, S, T)
    refused(r"mel_lengths is null", None, None, 4, S, T)
    refused(r"B = 0 is outside \[1, 96\]", i32(8), None, 0, S, T)
    refused(r"B = 97 is outside \[1, 96\]", i32(*([8] * 97)), None, 97, S, T)
    refused(r"video_lengths\[2\] = 23 is outside \[7, T = 22\]", i32(8, 1, 5, 7), i32(7, 13, 23, 16), 4, S, T)
    # the entry points run the same checks before they look at anything that needs a device: null model, null buffers
    assert L.l2s_train_postnet_masked_fwd(None, None, 4, S, None, None, None, None, i32(8, 1, 5, 7)) != 0
    assert L.l2s_loss_lengths(*([None] * 6), 4, S, 12, *([None] * 5), None, None, i32(8, 0, 5, 7), None, T, None) != 0
    with pytest.raises(RuntimeError, match=r"mel_lengths\[1\] = 0"):
        native.check(1, L)
    # the wrapper's own host check: ValueError naming the clip, TypeError for a non-integer table
    with pytest.raises(ValueError, match=r"outside \[1, S = 8\]: clip 1: 0, clip 3: 9"):
        native.mel_lengths_array([8, 0, 5, 9], 4, S)
    with pytest.raises(ValueError, match="shape"):
        native.mel_lengths_array([8, 1, 5], 4, S)
    with pytest.raises(TypeError):
        native.mel_lengths_array([8.0, 1.0, 5.0, 7.0], 4, S)
    with pytest.raises(ValueError, match="None"):
        native.mel_lengths_array(None, 4, S)
    nm = native.NativeModel()
    for call in (lambda ml: nm.train_postnet_fwd(torch.zeros(2, S, 80), None, mel_lengths=ml),
                 lambda ml: nm.train_postnet_bwd(torch.zeros(2, S, 80), torch.zeros(2, 80, S), torch.zeros(8), None, mel_lengths=ml)):
        with pytest.raises(ValueError, match=r"clip 1: 9"):
            call([3, 9])


def test_loss_and_loop_reject_mel_lengths_without_video_lengths():
    from lip2speech_amd import callers
    from lip2speech_amd.losses import Loss
    sig = inspect.signature(callers.train_iterations).parameters
    assert sig["honour_mel_lengths"].default is False and sig["honour_lengths"].default is False
    with pytest.raises(NotImplementedError, match="honour_mel_lengths needs honour_lengths"):
        callers.train_iterations(None, [], 0, honour_mel_lengths=True)
    with pytest.raises(NotImplementedError, match="train_bf16"):
        callers.train_iterations(None, [], 0, honour_lengths=True, honour_mel_lengths=True, bf16=True)
    assert inspect.signature(Loss.forward).parameters["melspec_lengths"].default is None
    B, S = 2, 4
    out = [torch.zeros(B, 80, S), torch.zeros(B, 80, S), torch.zeros(B, S, 1), None, None, torch.zeros(2 * B, 501), torch.tensor([14, 9])]
    targets = (torch.zeros(B, 80, S), torch.zeros(B, S))
    with pytest.raises(ValueError, match="no honoured video lengths"):      # lengths the model ignored: refused before anything else
        Loss()(out, targets, melspec_lengths=torch.tensor([4, 2]))
    out[-1].l2s_honoured = True
    with pytest.raises(RuntimeError, match="runs on the GPU"):              # honoured ones: on to the no-fallback error; nothing was launched either way
        Loss()(out, targets, melspec_lengths=torch.tensor([4, 2]))
    from lip2speech_amd import training
    with pytest.raises(ValueError, match="give mel_lengths"):
        training.loss_terms(out[0], out[1], out[2], out[5], *targets, video_lengths=[14, 9])


def test_model_flag_defaults_off_and_raises_by_name():
    from model.model import get_network
    net = get_network("train")
    assert net.train_mel_lengths is False
    args = (torch.zeros(1, 3, 8, 96, 96), None, None, torch.zeros(1, 80, 4), torch.tensor([8]), None, torch.tensor([3]), 1.0)
    net.train_mel_lengths = True      # alone: it needs the two video-length switches
    with pytest.raises(NotImplementedError, match="train_mel_lengths: needs `honour_video_lengths` and `train_video_lengths`"):
        net(*args, speaker_embedding=torch.zeros(1, 256))
    net.honour_video_lengths = True
    with pytest.raises(NotImplementedError, match="train_mel_lengths: needs"):
        net(*args, speaker_embedding=torch.zeros(1, 256))
    net.train_video_lengths = True    # all three, train() mode: batch statistics are refused by name before anything reaches the device
    with pytest.raises(NotImplementedError, match="train_mel_lengths: train\\(\\) mode normalises with batch statistics"):
        net(*args, speaker_embedding=torch.zeros(1, 256))
