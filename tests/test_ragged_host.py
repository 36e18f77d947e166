"""Ragged groups, host side (no GPU): the three C-ABI symbols are declared, exported and bound; `l2s_ragged_plan` gives the compact layout the header
describes and refuses shapes outside the limits by batch and row; the workspace query grows with every argument; the pool's grouping rule ignores B
and T; the Python layer validates before anything reaches the device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ("l2s_ragged_plan", "l2s_workspace_bytes_ragged", "l2s_inference_ragged")


@pytest.fixture(scope="module")
def L():
    from lip2speech_amd import native
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lip2speech_amd", "csrc"), "-j", "8"], check=True)
    return native.lib()


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def test_symbols_declared_exported_bound(L):
    from lip2speech_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l2s.h")).read(), flags=re.S)
    for sym in RAGGED:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} not declared in include/l2s.h"
        assert sym in native.ABI_SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None, f"{sym} has no ctypes signature"
    assert re.search(r"#define\s+L2S_MAX_RAGGED_CLIPS\s+256\b", header) and native.MAX_RAGGED_CLIPS == 256
    assert L.l2s_workspace_bytes_ragged.restype is ctypes.c_int64
    assert L.l2s_abi_version() == 2                      # the change only adds symbols
    for sym in ("l2s_inference_multi_masked", "l2s_forward_eval_multi_masked"):      # the ragged entry takes new names: these stay absent
        assert not hasattr(L, sym)


def test_plan():
    """B = [4, 2], T = [22, 15], lengths [7,13,22,16 | 13,9]: prefix sums of len and of ceil(len / 2)"""
    from lip2speech_amd import native
    want = ([0, 7, 20, 42, 58, 71, 80], [0, 4, 11, 22, 30, 37, 42], 6, 22)
    assert native.ragged_plan([4, 2], [22, 15], [[7, 13, 22, 16], [13, 9]]) == want
    assert native.ragged_plan([4, 2], [22, 15], [7, 13, 22, 16, 13, 9]) == want                   # the flat form of the same lengths
    assert native.ragged_plan([2, 4], [15, 22], [[13, 9], [7, 13, 22, 16]]) == ([0, 13, 22, 29, 42, 64, 80], [0, 7, 12, 16, 23, 34, 42], 6, 22)
    assert native.ragged_plan([1], [300], [[300]]) == ([0, 300], [0, 150], 1, 300)


def test_plan_errors(L):
    from lip2speech_amd import native
    with pytest.raises(RuntimeError, match=r"video_lengths\[1\] = 6 \(batch 0, row 1\) is outside \[7, T = 22\]"):
        native.ragged_plan([4, 2], [22, 15], [[7, 6, 22, 16], [13, 9]])
    with pytest.raises(RuntimeError, match=r"video_lengths\[4\] = 16 \(batch 1, row 0\) is outside \[7, T = 15\]"):      # legal in batch 0, longer than ITS batch's T
        native.ragged_plan([4, 2], [22, 15], [[7, 13, 22, 16], [16, 9]])
    with pytest.raises(RuntimeError, match=r"G = 9 is outside \[1, L2S_MAX_GROUP = 8\]"):
        native.ragged_plan([1] * 9, [7] * 9, [[7]] * 9)
    with pytest.raises(RuntimeError, match=r"N = 257 clips exceed L2S_MAX_RAGGED_CLIPS = 256"):
        native.ragged_plan([32] * 7 + [33], [7] * 8, [[7] * 32] * 7 + [[7] * 33])
    assert native.ragged_plan([32] * 8, [7] * 8, [[7] * 32] * 8)[2] == 256                        # the limit itself is legal
    with pytest.raises(RuntimeError, match=r"batch 1 has T = 301"):
        native.ragged_plan([1, 1], [7, 301], [[7], [7]])
    with pytest.raises(RuntimeError, match=r"batch 0 has B = 0"):
        native.ragged_plan([0, 1], [7, 7], [[], [7]])
    # the workspace query refuses the same shapes with -1 and the same message
    assert L.l2s_workspace_bytes_ragged(9, _i32([1] * 9), _i32([7] * 9), 96, 96, 40) == -1 and b"G = 9" in L.l2s_last_error()
    assert L.l2s_workspace_bytes_ragged(8, _i32([32] * 7 + [33]), _i32([7] * 8), 96, 96, 40) == -1 and b"N = 257" in L.l2s_last_error()


def test_workspace_query_is_monotone(L):
    from lip2speech_amd import native
    base = dict(batch_B=[4, 2], batch_T=[22, 15], H=88, W=88, S=40)
    w0 = native.workspace_bytes_ragged(**base)
    grown = [dict(base, batch_B=[4, 2, 1], batch_T=[22, 15, 7]),       # G
             dict(base, batch_B=[5, 2]), dict(base, batch_B=[4, 3]),   # B_g
             dict(base, batch_T=[23, 15]), dict(base, batch_T=[22, 16]),      # T_g (the second does not move Tmax: the encoder's frames alone)
             dict(base, H=96, W=96), dict(base, S=41)]
    for g in grown:
        assert native.workspace_bytes_ragged(**g) > w0, g
    # one batch: at least the masked call's workspace (the group's decoder stages are those of one masked call)
    for B, T in ((1, 7), (4, 22), (16, 75), (32, 50)):
        for H in (88, 96):
            assert native.workspace_bytes_ragged([B], [T], H, H, 300) >= L.l2s_workspace_bytes_masked(B, T, H, H, 300)
    # the largest group of the benchmarked shapes has a size (no overflow of the query)
    assert native.workspace_bytes_ragged([32] * 8, [50] * 8, 96, 96, 300) > native.workspace_bytes_ragged([16] * 8, [50] * 8, 96, 96, 300)


def _job(B, T, S=300, want_attn=False, entry="inference_ragged", H=96):
    return {"entry": entry, "video": torch.empty(B, 3, T, H, H, device="meta"), "S": S, "want_attn": want_attn}


def test_pool_grouping_rule():
    from lip2speech_amd.parallel import InflightPool as P
    jobs = [_job(4, 22), _job(2, 15), _job(16, 75)]
    assert P._job_key(jobs[0]) == P._job_key(jobs[1]) == P._job_key(jobs[2]) == ("inference_ragged", 96, 96, 300, False)
    assert P.job_groups(jobs, 8) == [[0, 1, 2]]                                                   # B and T differ: one group
    assert P.job_groups(jobs, 2) == [[0, 1], [2]]                                                 # `group` batches close it
    assert P.job_groups([_job(100, 9), _job(100, 30), _job(56, 7), _job(1, 7), _job(255, 8)], 8) == [[0, 1, 2], [3, 4]]      # 256 clips fit, 257 do not
    assert P.job_groups([_job(4, 22), _job(2, 15, S=200), _job(2, 15, S=200), _job(2, 15, S=200, want_attn=True)], 8) == [[0], [1, 2], [3]]
    assert P.job_groups([_job(4, 22), _job(4, 22, H=88)], 8) == [[0], [1]]
    # the unmasked entry keeps its rule: a shape change closes a group
    assert P.job_groups([_job(4, 22, entry="inference"), _job(4, 22, entry="inference"), _job(2, 15, entry="inference")], 8) == [[0, 1], [2]]
    assert P.job_groups([_job(4, 22, entry="inference"), _job(4, 22)], 8) == [[0], [1]]


def test_python_validation_comes_first():
    """lengths, shapes and group limits are checked before a tensor is touched; CPU tensors then meet the no-fallback error; the grouped entry points
    still refuse lengths"""
    from lip2speech_amd import native
    nm = native.NativeModel()
    a = (torch.zeros(4, 3, 22, 96, 96), torch.zeros(4, 256), torch.zeros(4 * 3, 501))
    b = (torch.zeros(2, 3, 15, 96, 96), torch.zeros(2, 256), torch.zeros(2 * 2, 501))
    for bad, match in (([[7, 13, 22, 16], [13, 6]], r"outside \[7, T = 15\]"), ([[7, 13, 22, 16], [16, 9]], r"outside \[7, T = 15\]"),
                       ([[7, 13, 22], [13, 9]], "shape"), ([[7, 13, 22, 16]], "one sequence of lengths per batch")):
        with pytest.raises(ValueError, match=match):
            nm.inference_ragged([a, b], bad, S=4)
    with pytest.raises(TypeError):
        nm.inference_ragged([a, b], [[7, 13, 22, 16], [13.0, 9.0]], S=4)
    with pytest.raises(ValueError, match="1..8 batches"):
        nm.inference_ragged([b] * 9, [[13, 9]] * 9, S=4)
    with pytest.raises(ValueError, match="gumbel"):
        nm.inference_ragged([a, (b[0], b[1], torch.zeros(2 * 3, 501))], [[7, 13, 22, 16], [13, 9]], S=4)      # batch b's noise has min_T(15) = 2 rows per clip
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nm.inference_ragged([a, b], [[7, 13, 22, 16], [13, 9]], S=4)
    assert nm.calls["l2s_inference_ragged"] == 0
    with pytest.raises(NotImplementedError):
        nm.inference_multi([a], S=4, video_lengths=[7, 13, 22, 16])
    from model.model import get_network
    net = get_network("test")
    net.honour_video_lengths = True
    with pytest.raises(NotImplementedError):
        next(iter(net.forward_many([])))
    with pytest.raises(ValueError, match="video_lengths"):
        net._inference_job(a[0], None, speaker_embedding=a[1], gumbel_noise=a[2], video_lengths=[7, 13, 22, 23])
