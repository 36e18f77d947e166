"""Training with per-clip video lengths (include/l2s.h "training with per-clip video lengths"), the parts that need no GPU: the entry points are declared,
exported and bound; the switches default off and the old raise is intact; arguments are checked before anything reaches the device; the masked sizers
cover the unmasked ones plus what a masked call keeps."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ("encoder", "prologue", "steps")
ENTRY = [f"l2s_train_{st}_masked_{d}" for st in STAGES for d in ("fwd", "bwd")]
SIZERS = ["l2s_train_encoder_tape_floats_masked", "l2s_train_encoder_ws_bytes_masked", "l2s_train_prologue_tape_floats_masked",
          "l2s_train_prologue_ws_bytes_masked", "l2s_train_steps_tape_floats_masked"]


@pytest.fixture(scope="module")
def L():
    from lip2speech_amd import native
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lip2speech_amd", "csrc"), "-j", "8"], check=True)
    return native.lib()


def test_symbols_declared_exported_bound(L):
    from lip2speech_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l2s.h")).read(), flags=re.S)
    for sym in ENTRY + SIZERS:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} not declared in include/l2s.h"
        assert sym in native.ABI_SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None, f"{sym} has no ctypes signature"
    # each is its unmasked signature plus the host length array
    for st in STAGES:
        for d in ("fwd", "bwd"):
            base, masked = getattr(L, f"l2s_train_{st}_{d}").argtypes, getattr(L, f"l2s_train_{st}_masked_{d}").argtypes
            assert list(masked[:-1]) == list(base) and masked[-1] == ctypes.POINTER(ctypes.c_int32)
    assert L.l2s_abi_version() == 2


def test_sizers(L):
    """The device length table is 3 x B int32 (len_b, m_b, first compact frame) and lives in the tape; the masked encoder tape also keeps the padded
    pooled front-end map (T x 24 x 24 x 24 floats per clip at 96 x 96) and the compact features; the masked backward workspaces add their row buffers."""
    for B, T in ((1, 14), (4, 22), (17, 14), (8, 75)):
        S = 6
        assert L.l2s_train_steps_tape_floats_masked(B, S) >= L.l2s_train_steps_tape_floats(B, S) + 3 * B
        assert L.l2s_train_prologue_tape_floats_masked(B, T) >= L.l2s_train_prologue_tape_floats(B, T) + 3 * B
        assert L.l2s_train_encoder_tape_floats_masked(B, T, 96) >= L.l2s_train_encoder_tape_floats(B, T, 96) + B * T * (24 * 24 * 24 + 768) + 3 * B
        Bp = (B + 15) // 16 * 16
        assert L.l2s_train_prologue_ws_bytes_masked(B, T) >= L.l2s_train_prologue_ws_bytes(B, T) + 4 * (Bp * 2048 + B * 1024)      # reset rows' gate gradients, dh rows
        assert L.l2s_train_encoder_ws_bytes_masked(B, T, 96) >= L.l2s_train_encoder_ws_bytes(B, T, 96) + 4 * B * T * 768


def test_switches_default_off_and_the_old_raise_is_intact():
    from model.model import Lip2Speech, get_network
    net = get_network("train")
    assert net.honour_video_lengths is False and net.train_video_lengths is False
    args = (torch.zeros(1, 3, 8, 96, 96), None, None, torch.zeros(1, 80, 4), torch.tensor([8]), None, None, 1.0)
    # neither switch: lengths ignored as in the reference (nothing to raise about them; the call itself needs the GPU)
    # honour_video_lengths alone: the raise of the forward-only masked family, in train() and in eval() with gradients
    net.honour_video_lengths = True
    with pytest.raises(NotImplementedError, match="length-masked"):
        net(*args, speaker_embedding=torch.zeros(1, 256))
    net.eval()
    with pytest.raises(NotImplementedError, match="length-masked"):
        net(*args, speaker_embedding=torch.zeros(1, 256))
    # train_video_lengths alone switches nothing on
    net.honour_video_lengths, net.train_video_lengths = False, True
    assert "honour_lengths" in inspect.signature(Lip2Speech._forward_train).parameters
    # both, train() mode: batch statistics with lengths are refused by name, before anything reaches the device
    net.honour_video_lengths = True
    net.train()
    with pytest.raises(NotImplementedError, match="batch statistics"):
        net(*args, speaker_embedding=torch.zeros(1, 256))


def test_arguments_checked_before_the_device():
    from lip2speech_amd import callers, native
    nm = native.NativeModel()
    video, emb = torch.zeros(2, 3, 14, 96, 96), torch.zeros(2, 256)
    # a bad length raises from the host check (ValueError naming the clip), a good one reaches the no-fallback error: nothing was launched either way
    for call in (lambda vl: nm.train_encoder_fwd(video, emb, video_lengths=vl),
                 lambda vl: nm.train_prologue_fwd(torch.zeros(2, 14, 1024), emb, torch.zeros(4, 501), video_lengths=vl),
                 lambda vl: nm.train_steps_fwd(torch.zeros(8), 2, 14, 3, video_lengths=vl)):
        with pytest.raises(ValueError, match=r"outside \[7, T = 14\]: clip 1: 15"):
            call([9, 15])
        with pytest.raises(ValueError, match="shape"):
            call([9])
        with pytest.raises(TypeError):
            call([9.5, 14])
    sig = inspect.signature(callers.train_iterations).parameters
    assert sig["honour_lengths"].default is False
    with pytest.raises(NotImplementedError, match="train_bf16"):
        callers.train_iterations(None, [], 0, honour_lengths=True, bf16=True)


def test_library_refuses_bad_lengths_by_row(L):
    """The C entry points check the lengths before they look at anything else of the call that needs a device: no model is needed to see the refusal of a
    null model, and l2s_masked_bilstm_plan (the plan both prologue directions walk) names the row."""
    from lip2speech_amd import native
    with pytest.raises(RuntimeError, match=r"video_lengths\[1\] = 23 is outside \[7, T = 22\]"):
        native.masked_bilstm_plan([7, 23], 22)
    lens = (ctypes.c_int32 * 2)(9, 14)
    assert L.l2s_train_steps_masked_fwd(None, None, 2, 14, 3, None, None, None, None, None, None, None, None, None, None, None, 0, None, lens) != 0      # null model: refused
