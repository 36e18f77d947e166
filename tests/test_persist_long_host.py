"""Option "persist_frames" without a GPU: the product library knows the option, the header documents it next to "persist_decode", and the caller
functions take the keyword."""
import ctypes
import inspect
import os

import pytest

from lip2speech_amd import callers, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_product_library_accepts_persist_frames():
    L = native.lib()
    assert "persist_frames" not in native.DIAG_OPTIONS
    h = ctypes.c_void_p()
    assert L.l2s_model_create(ctypes.byref(h)) == 0
    try:
        for v in (75, 32, 0, 300):
            assert L.l2s_model_set_option(h, b"persist_frames", v) == 0
        assert L.l2s_model_set_option(h, b"persist_frame", 75) != 0
    finally:
        L.l2s_model_destroy(h)
    try:
        assert L.l2s_set_option(b"persist_frames", 75) == 0
    finally:
        assert L.l2s_set_option(b"persist_frames", 32) == 0
    assert L.l2s_abi_version() == 2


def test_header_documents_persist_frames():
    text = open(os.path.join(ROOT, "include", "l2s.h")).read()
    assert text.index('"persist_decode"    (4)') < text.index('"persist_frames"    (32)') < text.index('"use_graph"         (0)')


@pytest.mark.parametrize("fn", [callers.demo_clip, callers.demo_clips])
def test_callers_keyword_defaults_to_leaving_the_option_alone(fn):
    p = inspect.signature(fn).parameters
    assert "persist_frames" in p and p["persist_frames"].default == 0
