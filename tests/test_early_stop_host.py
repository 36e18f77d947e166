"""Option "early_stop" without a GPU: the product library knows the option, the Python surface takes the keyword, and the masked-reference helper
of the GPU tests agrees with the goldens' own lengths and shapes."""
import ctypes
import inspect
import os

import pytest
import torch

import early_stop_common as es
import parity_common as pc
from lip2speech_amd import callers, native
from lip2speech_amd.model.model import Lip2Speech

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_product_library_accepts_early_stop():
    L = native.lib()
    assert "early_stop" not in native.DIAG_OPTIONS
    h = ctypes.c_void_p()
    assert L.l2s_model_create(ctypes.byref(h)) == 0
    try:
        for v in (1, 0):
            assert L.l2s_model_set_option(h, b"early_stop", v) == 0
        assert L.l2s_model_set_option(h, b"early_stopp", 1) != 0
    finally:
        L.l2s_model_destroy(h)
    try:
        assert L.l2s_set_option(b"early_stop", 1) == 0
    finally:
        assert L.l2s_set_option(b"early_stop", 0) == 0
    assert L.l2s_abi_version() == 2


def test_header_documents_early_stop():
    text = open(os.path.join(ROOT, "include", "l2s.h")).read()
    assert '"early_stop"' in text and "use_graph" in text
    block = text[text.index('"early_stop"'):]
    assert "output_lengths" in block or "lengths" in block


@pytest.mark.parametrize("fn", [Lip2Speech.inference, Lip2Speech.inference_many])
def test_model_keyword_defaults_to_leaving_the_option_alone(fn):
    p = inspect.signature(fn).parameters
    assert "early_stop" in p and p["early_stop"].default is None


@pytest.mark.parametrize("fn", [callers.demo_clip, callers.demo_clips])
def test_callers_keyword_defaults_off(fn):
    p = inspect.signature(fn).parameters
    assert "early_stop" in p and p["early_stop"].default is False


def test_masked_reference_helper_against_goldens():
    g = pc.golden("stop_lrw_b32.npz")
    mel = pc.golden("inference_lrw_b32_full_mel.npz")["mel_post"]
    lens = g["output_lengths"]
    assert mel.shape == (32, 80, 300) and lens.dtype == torch.int64
    assert es.MARGIN == 10
    for max_len, n_clips, E in es.SUB_BATCHES:
        idx = es.rows_upto(lens, max_len)
        assert len(idx) == n_clips and es.end_step(lens[idx], 300) == E
        assert es.gumbel_rows(g["gumbel"], idx).shape == (4 * n_clips, 501)
    m = es.masked_mel(mel, lens)
    for b in range(32):
        n = int(lens[b])
        assert torch.equal(m[b, :, :n], mel[b, :, :n]) and not m[b, :, n:].any()
    assert torch.equal(m[lens == 300], mel[lens == 300])
    g2 = pc.golden("stop_lrw_b2.npz")
    assert g2["output_lengths"].tolist() == [183, 300] or sorted(g2["output_lengths"].tolist()) == [183, 300]
    a = es.masked_attn(g2["attn"], g2["output_lengths"])
    assert a.shape == (2, 300, 29)
    for b in range(2):
        n = int(g2["output_lengths"][b])
        assert torch.equal(a[b, :n], g2["attn"][b, :n]) and not a[b, n:].any()
