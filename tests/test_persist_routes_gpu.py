"""Which calls take the persistent forms (pdecode.hip), stated as a table and read from the library's own launch profile: `decode_persistent` /
`bilstm_persistent` are the persistent decode loop and BiLSTM, `step_lstm_cell` / `bilstm_step` the launch-per-phase forms of the same stages.  The
envelope rule is persist_envelope (l2s_api.hip) plus each stage's own terms; where the device cannot hold the persistent forms
(native.persist_available() false) every call takes the launch names.  `-m gpu`."""
import pytest
import torch

from lip2speech_amd import native, synth
import parity_common as pc

pytestmark = pytest.mark.gpu

S, HW = 4, 88
ON = dict(persist_decode=8, persist_frames=80, persist_masked=1)
DEFAULT = dict(persist_decode=4)                      # the library's defaults: persist_frames 32, persist_masked 0 (the suite pins persist_decode 0)
OFF = dict(persist_decode=0, persist_frames=80, persist_masked=1)
BOTH, DECODE, BILSTM, NEITHER = (True, True), (False, True), (True, False), (False, False)      # (persistent BiLSTM, persistent decode loop)

_models = {}


def model(sd, options):
    """A NativeModel per option set, shared by the cases of this module."""
    key = tuple(sorted(options.items()))
    if key not in _models:
        _models[key] = pc.fresh_native_model(sd, **options)
    return _models[key]


def inputs(B, T, lens=None):
    tag = f"route{B}_{T}"
    video = synth.synth_video(B, T, H=HW, W=HW, tag=tag)
    for b, n in enumerate(lens or []):
        video[b, :, n:] = 0
    return video.cuda(), synth.synth_speaker_embedding(B, tag=tag).cuda(), synth.synth_gumbel(B * native.min_T(T), tag=tag).cuda()


def launched(call):
    """the names of the kernels that `call` launched"""
    native.profile_enable(True)
    try:
        native.profile_reset()
        call()
        torch.cuda.synchronize()
        return {name for name, launches, _ in native.profile_read() if launches > 0}
    finally:
        native.profile_enable(False)


def check_route(names, expected):
    bilstm, decode = expected if native.persist_available() else NEITHER
    print(f"expected persistent (BiLSTM, decode) = {(bilstm, decode)}; launched: {sorted(n for n in names if 'persistent' in n or n in ('bilstm_step', 'step_lstm_cell'))}")
    assert native.persist_timeouts() == 0
    assert ("bilstm_persistent" in names) == bilstm and ("bilstm_step" in names) != bilstm
    assert ("decode_persistent" in names) == decode and ("step_lstm_cell" in names) != decode


@pytest.mark.parametrize("B,T,lens,expected", [
    (1, 29, None, BOTH), (2, 80, None, BOTH), (3, 33, None, DECODE), (5, 29, None, NEITHER), (1, 81, None, NEITHER),
    (2, 32, [7, 32], BOTH), (2, 75, [20, 26], BOTH), (3, 62, [27, 50, 62], DECODE), (2, 81, [13, 29], NEITHER)])
def test_inference_routes(synth_sd, B, T, lens, expected):
    nm, args = model(synth_sd, ON), inputs(B, T, lens)
    check_route(launched(lambda: nm.inference(*args, S=S, video_lengths=lens)), expected)


@pytest.mark.parametrize("lens,expected", [(None, BILSTM), ([13, 29], NEITHER)])
def test_teacher_forced_routes(synth_sd, lens, expected):
    """One forced step: the decode loop keeps the launch route; an unmasked call keeps its persistent BiLSTM, a masked one does not."""
    nm, args = model(synth_sd, ON), inputs(2, 29, lens)
    teacher = synth.synth_mels(2, S, tag="route-tf").permute(0, 2, 1).contiguous().cuda()
    vlen = None if lens is None else torch.tensor(lens)
    check_route(launched(lambda: nm.forward_eval(*args, S, teacher=teacher, teacher_mask=[0, 1, 0, 0], video_lengths=vlen)), expected)


@pytest.mark.parametrize("B,T,lens", [(1, 33, None), (2, 29, [13, 29])])
def test_default_options_routes(synth_sd, B, T, lens):
    """persist_frames 32: a 33-frame clip is outside the envelope; persist_masked 0: so is every masked call."""
    nm, args = model(synth_sd, DEFAULT), inputs(B, T, lens)
    check_route(launched(lambda: nm.inference(*args, S=S, video_lengths=lens)), NEITHER)


@pytest.mark.parametrize("B,T,lens", [(1, 29, None), (2, 32, [7, 32])])
def test_persist_decode_off_routes(synth_sd, B, T, lens):
    nm, args = model(synth_sd, OFF), inputs(B, T, lens)
    check_route(launched(lambda: nm.inference(*args, S=S, video_lengths=lens)), NEITHER)


def test_grouped_entry_routes(synth_sd):
    """The grouped entry points never take the persistent forms, whatever G."""
    nm, args = model(synth_sd, ON), inputs(1, 29)
    check_route(launched(lambda: nm.inference_multi([args], S=S)), NEITHER)
