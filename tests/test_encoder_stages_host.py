"""The bound of the per-unit trunk tests (tests/test_encoder_stages_gpu.py), examined on the host: for every ShuffleNet unit the fp32 oracle passes it,
four wrong restatements of the unit (tests/video_trunk_torch.py) fail it, and it stays below 1e-5 of a frame's largest value.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

import video_trunk_torch as vt
from lip2speech_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hw", [96, 88])
def test_unit_bound_passes_fp32_and_catches_wrong_units(synth_sd, hw):
    """synth_video(2, 3, hw, hw): unit u gets the fp64 oracle's output of unit u - 1 rounded to fp32 (what a device tap would hand it).  Judged as the
    GPU tests judge a tap - frame_check per frame against the fp64 unit, e32 from the fp32 unit on the same input:
      - the fp32 unit passes;
      - a depthwise conv that pads pw1's input, the two largest channels swapped, pointwise weights without their lowest bf16 plane and one value of the
        last frame times 1 + 1e-4 (each computed in fp64, so the deviation is the damage alone) all fail, at every unit;
      - the bound 8 * max(e32, eps32) is below 1e-5 at every unit.
    Not claimed: a lost low plane of the unit's INPUT activations (it stays inside the bound at the stride-2 units 4 and 12)."""
    video = synth.synth_video(2, 3, hw, hw)
    x = vt.frontend(synth_sd, video).float()
    missed = []
    for u in range(vt.N_UNITS):
        ref64, ref32 = vt.unit(synth_sd, u, x), vt.unit(synth_sd, u, x, torch.float32)
        ok, rel, e32 = vt.map_check(vt.rows(ref32), ref64, ref32)
        bound = vt.MARGIN * max(e32, vt.EPS32)
        line = f"hw={hw} unit {u:2d}: e32 {e32:.2e}, bound {bound:.2e};"
        assert ok, (u, rel, e32)
        assert bound < 1e-5, (u, bound)
        for wrong in vt.WRONG:
            ok_w, rel_w, _ = vt.map_check(vt.rows(vt.unit(synth_sd, u, x, wrong=wrong)), ref64, ref32)
            line += f" {wrong} {rel_w:.2e}"
            if ok_w or rel_w <= bound:
                missed.append((u, wrong, rel_w, bound))
        print(line)
        x = ref64.float()
    assert not missed, missed


def test_header_declares_the_encoder_taps_and_the_product_lacks_them():
    diag = open(os.path.join(ROOT, "include", "l2s_diag.h")).read()
    assert re.search(r"int\s+l2s_op_encoder_taps\s*\(\s*l2s_model\* m,\s*const float\* video,\s*int B,\s*int T,\s*int H,\s*int W,\s*float\* const\* taps", diag)
    assert "l2s_op_encoder_taps" not in open(os.path.join(ROOT, "include", "l2s.h")).read()
    from lip2speech_amd import native
    assert "l2s_op_encoder_taps" in native.DIAG_SYMBOLS and "l2s_op_encoder_taps" not in native.ABI_SYMBOLS
    if not (os.path.exists(native.LIB_PATH) and os.path.exists(native.DIAG_LIB_PATH)):
        pytest.fail("native libraries not built: run __graft_entry__.build() first")
    assert not hasattr(ctypes.CDLL(native.LIB_PATH), "l2s_op_encoder_taps"), "a diagnostic entry point in the product library"
    assert hasattr(ctypes.CDLL(native.DIAG_LIB_PATH), "l2s_op_encoder_taps")
    assert vt.N_TAPS == 18 and len(native.encoder_tap_shapes(6, 96)) == 18
    assert native.encoder_tap_shapes(3, 88) == [(3, 22, 22, 24)] + [(3, 11, 11, 116)] * 4 + [(3, 6, 6, 232)] * 8 + [(3, 3, 3, 464)] * 4 + [(27, 768)]
