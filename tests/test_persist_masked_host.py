"""Option "persist_masked" without a GPU: the product library knows the option (per model and process-wide), the header documents it between
"persist_frames" and "use_graph" and no longer says that masked calls never take the persistent loop, and the caller functions take the keyword."""
import ctypes
import inspect
import os

import pytest

from lip2speech_amd import callers, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_product_library_accepts_persist_masked():
    L = native.lib()
    assert "persist_masked" not in native.DIAG_OPTIONS
    h = ctypes.c_void_p()
    assert L.l2s_model_create(ctypes.byref(h)) == 0
    try:
        for v in (1, 0, 4):
            assert L.l2s_model_set_option(h, b"persist_masked", v) == 0
        assert L.l2s_model_set_option(h, b"persist_mask", 1) != 0
        assert L.l2s_model_set_option(h, b"persist_masked_", 1) != 0
    finally:
        L.l2s_model_destroy(h)
    try:
        assert L.l2s_set_option(b"persist_masked", 1) == 0
    finally:
        assert L.l2s_set_option(b"persist_masked", 0) == 0
    assert L.l2s_set_option(b"persist_mask", 1) != 0
    assert L.l2s_abi_version() == 2


def test_header_documents_persist_masked():
    text = open(os.path.join(ROOT, "include", "l2s.h")).read()
    assert text.index('"persist_frames"    (32)') < text.index('"persist_masked"    (0)') < text.index('"use_graph"         (0)')
    assert "masked calls always take the launch-per-phase route" not in text
    assert 'unless "persist_masked"' in text


@pytest.mark.parametrize("fn", [callers.demo_clip, callers.demo_clips])
def test_callers_keyword_defaults_to_leaving_the_option_alone(fn):
    p = inspect.signature(fn).parameters
    assert "persist_masked" in p and p["persist_masked"].default == 0
