"""The evaluate-shaped ragged group, host side (no GPU): the three C-ABI symbols are declared, exported and bound; `l2s_forward_eval_ragged_plan` gives
the packed layout the header describes and refuses shapes outside the limits by batch and value; the workspace query refuses the same shapes and grows
with its arguments; the pool's grouping rule for "forward_ragged" ignores B, T and S; the Python layer validates before anything reaches the device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("l2s_forward_eval_ragged_plan", "l2s_workspace_bytes_eval_ragged", "l2s_forward_eval_ragged")


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
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} not declared in include/l2s.h"
        assert sym in native.ABI_SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None, f"{sym} has no ctypes signature"
    assert header.index("l2s_inference_ragged") < header.index("l2s_forward_eval_ragged_plan")      # placed after the "ragged groups" block
    assert L.l2s_workspace_bytes_eval_ragged.restype is ctypes.c_int64
    assert L.l2s_abi_version() == 2                      # the change only adds symbols
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert f" T {sym}\n" in exported


def test_plan():
    """B = [4, 2, 1], T = [22, 15, 7], S = [40, 23, 3]: every block has the layout of its batch's own masked call, back to back in batch order"""
    from lip2speech_amd import native
    mel, stop, attn, dis, N, Tmax, Smax = native.forward_eval_ragged_plan([4, 2, 1], [22, 15, 7], [40, 23, 3])
    assert mel == [0, 12800, 16480, 16720]               # B_g * 80 * S_g floats per batch
    assert stop == [0, 160, 206, 209]                    # B_g * S_g
    assert attn == [0, 3520, 4210, 4231]                 # B_g * S_g * T_g
    assert dis == [501 * r for r in (0, 12, 16, 17)]     # B_g * min_T(T_g) rows of 501
    assert (N, Tmax, Smax) == (7, 22, 40)
    # another order of the same batches: the same block sizes in that order
    mel, stop, attn, dis, N, Tmax, Smax = native.forward_eval_ragged_plan([1, 2, 4], [7, 15, 22], [3, 23, 40])
    assert mel == [0, 240, 3920, 16720] and stop == [0, 3, 49, 209] and attn == [0, 21, 711, 4231] and dis == [501 * r for r in (0, 1, 5, 17)]
    assert (N, Tmax, Smax) == (7, 22, 40)
    assert native.forward_eval_ragged_plan([1], [300], [300])[:3] == ([0, 24000], [0, 300], [0, 90000])


def test_plan_errors(L):
    from lip2speech_amd import native
    with pytest.raises(RuntimeError, match=r"batch 1 has S = 0, outside \[1, 300\]"):
        native.forward_eval_ragged_plan([4, 2, 1], [22, 15, 7], [40, 0, 3])
    with pytest.raises(RuntimeError, match=r"batch 1 has S = 301, outside \[1, 300\]"):
        native.forward_eval_ragged_plan([4, 2, 1], [22, 15, 7], [40, 301, 3])
    assert native.forward_eval_ragged_plan([4, 2, 1], [22, 15, 7], [300, 1, 3])[6] == 300        # both limits are legal
    with pytest.raises(RuntimeError, match=r"G = 9 is outside \[1, L2S_MAX_GROUP = 8\]"):
        native.forward_eval_ragged_plan([1] * 9, [7] * 9, [3] * 9)
    with pytest.raises(RuntimeError, match=r"N = 257 clips exceed L2S_MAX_RAGGED_CLIPS = 256"):
        native.forward_eval_ragged_plan([32] * 7 + [33], [7] * 8, [3] * 8)
    assert native.forward_eval_ragged_plan([32] * 8, [7] * 8, [3] * 8)[4] == 256
    with pytest.raises(RuntimeError, match=r"batch 1 has T = 301"):
        native.forward_eval_ragged_plan([1, 1], [7, 301], [3, 3])
    with pytest.raises(ValueError, match="one entry per batch"):
        native.forward_eval_ragged_plan([1, 1], [7, 7], [3])
    # the workspace query refuses the same shapes with -1 and the same message
    for B, T, S, msg in (([4, 2, 1], [22, 15, 7], [40, 0, 3], b"batch 1 has S = 0, outside [1, 300]"),
                         ([4, 2, 1], [22, 15, 7], [40, 301, 3], b"batch 1 has S = 301, outside [1, 300]"),
                         ([1] * 9, [7] * 9, [3] * 9, b"G = 9"), ([32] * 7 + [33], [7] * 8, [3] * 8, b"N = 257"), ([1, 1], [7, 301], [3, 3], b"batch 1 has T = 301")):
        assert L.l2s_workspace_bytes_eval_ragged(len(B), _i32(B), _i32(T), _i32(S), 96, 96) == -1 and msg in L.l2s_last_error(), msg
    with pytest.raises(RuntimeError, match=r"batch 1 has S = 301"):
        native.workspace_bytes_eval_ragged([4, 2, 1], [22, 15, 7], [40, 301, 3])


def test_workspace_query_grows(L):
    from lip2speech_amd import native
    base = dict(batch_B=[4, 2], batch_T=[22, 15], batch_S=[40, 23], H=88, W=88)
    w0 = native.workspace_bytes_eval_ragged(**base)
    grown = [dict(base, batch_B=[4, 2, 1], batch_T=[22, 15, 7], batch_S=[40, 23, 3]),      # G
             dict(base, batch_B=[5, 2]), dict(base, batch_B=[4, 3]),                       # B_g
             dict(base, batch_T=[23, 15]), dict(base, batch_T=[22, 16]),                   # T_g (the second does not move Tmax: the encoder's frames alone)
             dict(base, batch_S=[41, 23]), dict(base, H=96, W=96)]                         # the chain runs Smax steps: S grows through the longest batch
    for g in grown:
        assert native.workspace_bytes_eval_ragged(**g) > w0, g
    assert native.workspace_bytes_eval_ragged(**dict(base, batch_S=[40, 24])) == w0        # a shorter batch's S moves no buffer: all are sized by Smax
    # the ragged group's own workspace at Smax plus the staging buffers (mel twice, stop, attention and content_dis at the staging pitches)
    N, Tmax, Smax, mT = 6, 22, 40, 3
    assert w0 >= native.workspace_bytes_ragged([4, 2], [22, 15], 88, 88, Smax) + 4 * (2 * N * Smax * 80 + N * Smax + N * Smax * Tmax + N * mT * 501)
    # the benchmarked shapes have a size (no overflow of the query)
    assert native.workspace_bytes_eval_ragged([32] * 8, [50] * 8, [125] * 8) > native.workspace_bytes_eval_ragged([16] * 8, [50] * 8, [125] * 8)


def _job(B, T, S, entry="forward_ragged", H=96):
    return {"entry": entry, "video": torch.empty(B, 3, T, H, H, device="meta"), "S": S, "mask": None}


def test_pool_grouping_rule():
    from lip2speech_amd.parallel import InflightPool as P
    jobs = [_job(4, 22, 40), _job(2, 15, 23), _job(1, 7, 3)]
    assert P._job_key(jobs[0]) == P._job_key(jobs[1]) == P._job_key(jobs[2]) == ("forward_ragged", 96, 96)
    assert P.job_groups(jobs, 8) == [[0, 1, 2]]                                                   # B, T and S differ: one group
    assert P.job_groups(jobs, 2) == [[0, 1], [2]]                                                 # `group` batches close it
    assert P.job_groups([_job(100, 9, 20), _job(100, 30, 75), _job(56, 7, 18), _job(1, 7, 3), _job(255, 8, 20)], 8) == [[0, 1, 2], [3, 4]]      # 256 clips fit, 257 do not
    assert P.job_groups([_job(4, 22, 40), _job(4, 22, 40, H=88)], 8) == [[0], [1]]
    # the other entries keep their rules, and never share a group with this one
    assert P.job_groups([_job(4, 22, 40, entry="forward"), _job(4, 22, 40, entry="forward"), _job(4, 22, 41, entry="forward")], 8) == [[0, 1], [2]]
    assert P.job_groups([_job(4, 22, 40, entry="forward"), _job(4, 22, 40)], 8) == [[0], [1]]
    ragged = dict(_job(4, 22, 40, entry="inference_ragged"), want_attn=False)
    assert P.job_groups([ragged, _job(4, 22, 40)], 8) == [[0], [1]]


def test_python_validation_comes_first():
    """step counts, lengths, shapes and group limits are checked before a tensor is touched; CPU tensors then meet the no-fallback error"""
    from lip2speech_amd import native
    nm = native.NativeModel()
    a = (torch.zeros(4, 3, 22, 96, 96), torch.zeros(4, 256), torch.zeros(4 * 3, 501))
    b = (torch.zeros(2, 3, 15, 96, 96), torch.zeros(2, 256), torch.zeros(2 * 2, 501))
    lens = [[7, 13, 22, 16], [13, 9]]
    for S, match in (([40], "one step count per batch"), ([40, 23, 3], "one step count per batch"), (40, "one step count per batch"),
                     ([40, 0], r"S outside \[1, 300\]: batch 1: 0"), ([301, 23], r"S outside \[1, 300\]: batch 0: 301")):
        with pytest.raises(ValueError, match=match):
            nm.forward_eval_ragged([a, b], lens, S)
    with pytest.raises(TypeError, match="S must hold integers"):
        nm.forward_eval_ragged([a, b], lens, [40.0, 23.0])
    for bad, match in (([[7, 13, 22, 16], [13, 6]], r"outside \[7, T = 15\]"), ([[7, 13, 22], [13, 9]], "shape"), ([[7, 13, 22, 16]], "one sequence of lengths per batch")):
        with pytest.raises(ValueError, match=match):
            nm.forward_eval_ragged([a, b], bad, [40, 23])
    with pytest.raises(TypeError):
        nm.forward_eval_ragged([a, b], [[7, 13, 22, 16], [13.0, 9.0]], [40, 23])                  # float lengths
    with pytest.raises(ValueError, match="1..8 batches"):
        nm.forward_eval_ragged([b] * 9, [[13, 9]] * 9, [23] * 9)
    with pytest.raises(ValueError, match="gumbel"):
        nm.forward_eval_ragged([a, (b[0], b[1], torch.zeros(2 * 3, 501))], lens, [40, 23])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nm.forward_eval_ragged([a, b], lens, [40, 23])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nm.forward_eval_ragged([a, b], lens, torch.tensor([40, 23]))                              # an integer tensor of step counts is accepted
    assert nm.calls["l2s_forward_eval_ragged"] == 0


def test_forward_many_lengths_refuses():
    from model.model import get_network
    net = get_network("train")
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        net.forward_many_lengths([])
    net = get_network("test")
    v, e, g = torch.zeros(2, 3, 15, 96, 96), torch.zeros(2, 256), torch.zeros(2 * 2, 501)
    mels = torch.zeros(2, 80, 23)
    with pytest.raises(ValueError, match="video_lengths"):
        net._forward_ragged_job(v, None, mels, None, 1, speaker_embedding=e, gumbel_noise=g)
    with pytest.raises(ValueError, match=r"outside \[7, T = 15\]"):
        net._forward_ragged_job(v, None, mels, torch.tensor([13, 16]), 1, speaker_embedding=e, gumbel_noise=g)
    torch.manual_seed(0)
    with pytest.raises(ValueError, match="teacher-forces a step"):                                # tf_ratio = 0.5: rand > 0.5 within the first steps, 11 may be forced
        net._forward_ragged_job(v, None, mels, torch.tensor([13, 9]), 0.5, speaker_embedding=e, gumbel_noise=g)
    # tf_ratio = 1 forces no step (rand is never > 1) and consumes one host draw per step, as forward does
    torch.manual_seed(0)
    job = net._forward_ragged_job(v, None, mels, torch.tensor([13, 9]), 1, speaker_embedding=e, gumbel_noise=g)
    after = torch.rand(1)
    torch.manual_seed(0)
    for _ in range(23):
        torch.rand(1)
    assert torch.equal(after, torch.rand(1))
    assert job["entry"] == "forward_ragged" and job["video_lengths"] == [13, 9] and job["S"] == 23 and job["mask"] is None
    # forward_many keeps refusing honour_video_lengths, and now names the method that groups such calls
    net.honour_video_lengths = True
    with pytest.raises(NotImplementedError, match="forward_many_lengths"):
        next(iter(net.forward_many([])))
