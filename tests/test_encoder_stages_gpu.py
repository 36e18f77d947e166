"""The video trunk unit by unit (`-m gpu`): every kernel form of the 16 ShuffleNet units, conv_last and the pooling, each held to the fp64 oracle of THAT
stage applied to the device's own tap of the stage before (l2s_op_encoder_taps: copies of the trunk's ping-pong buffers, no other launch).  Bound per
stage, from tests/speaker_tower_torch.py through tests/video_trunk_torch.py: per frame |got - ref64| <= 8 * max(e32, eps32) * S_frame, e32 = what the
fp32 oracle loses on the same input (1.8e-6 - 6.1e-6 of a frame's largest value; tests/test_encoder_stages_host.py shows what that catches)."""
import pytest
import torch

import parity_common as pc
import video_trunk_torch as vt
from lip2speech_amd import native, synth

pytestmark = pytest.mark.gpu

ALL = tuple(range(vt.N_TAPS))
UNITS = tuple(range(vt.N_UNITS))
SHAPES = [(96, 1, 1), (96, 2, 3), (88, 1, 3), (88, 3, 3)]
# what a model with the stage chain on can hand out: the front-end, the stride-2 units, the last unit of each chained stage, conv_last
DEFAULT_TAPS = (0,) + tuple(vt.tap(u) for u in (0, 3, 4, 11, 12, 13, 14, 15)) + (vt.TAP_LAST,)
CHAIN2_TAPS = (0,) + tuple(vt.tap(u) for u in (0, 3, 4, 11, 12, 15)) + (vt.TAP_LAST,)

_nms, _runs = {}, {}


def _nm(sd, **options):
    """NativeModels of the synthetic checkpoint, one per option set (options are per model, set before the weights are packed)."""
    key = tuple(sorted(options.items()))
    if key not in _nms:
        _nms[key] = pc.fresh_native_model(sd, **options)
    return _nms[key]


def _video(hw, B, T):
    return synth.synth_video(B, T, hw, hw, tag=f"stages{hw}_{B}_{T}")


def _run(nm, video, which):
    feat, taps = nm.encoder_fwd(video.cuda(), taps=which)
    torch.cuda.synchronize()
    return feat.cpu(), {i: t.cpu() for i, t in taps.items()}


def _small(sd, shape, which=ALL, **options):
    """(feat, taps) of one of the small shapes on the model with these options: run once, shared between the tests, never modified."""
    key = (shape, which, tuple(sorted(options.items())))
    if key not in _runs:
        _runs[key] = _run(_nm(sd, **options), _video(*shape), which)
    return _runs[key]


def _check(sd, feat, taps, label, units=UNITS, video=None):
    """Every stage whose tap and whose predecessor's tap are in `taps`: the units in `units`, conv_last, feat, and with `video` the front-end map.  Prints
    the deviation of every stage (of the frame's largest value, next to the fp32 oracle's), then asserts them all."""
    res = {}
    if video is not None:
        res["frontend"] = vt.map_check(taps[0], vt.frontend(sd, video), vt.frontend(sd, video, torch.float32))
    for u in units:
        res[f"unit{u}"] = vt.unit_check(sd, u, taps[vt.tap(u) - 1], taps[vt.tap(u)])
    if vt.TAP_LAST in taps:
        res["last"] = vt.last_check(sd, taps[vt.tap(15)], taps[vt.TAP_LAST])
    for k, (ok, dev, e32) in res.items():
        print(f"trunk stage {label} {k:8s}: device {dev:.2e} (of the frame's largest, fp32 torch {e32:.2e}) {'ok' if ok else 'EXCEEDS its bound'}")
    if vt.TAP_LAST in taps:
        ok, dev, bound = res["feat"] = vt.feat_check(taps[vt.TAP_LAST], feat)
        print(f"trunk stage {label} feat    : device {dev:.2e} (abs, bound {bound:.2e}) {'ok' if ok else 'EXCEEDS its bound'}")
        assert ((feat.norm(dim=2) - 1).abs() < 1e-5).all()
    bad = [k for k, r in res.items() if not r[0]]
    assert not bad, f"{label}: stages beyond 8 x max(e32, eps32) of the frame's largest: {bad}"
    return res


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ every unit, default arithmetic
@pytest.mark.parametrize("hw,B,T", SHAPES)
def test_every_unit_split_bf16(synth_sd, hw, B, T):
    """"trunk_chain" = 0: shuffle_s1x per unit, shuffle_s2x at units 0 and 4, the f32 shuffle_s2 at unit 12.  (96,1,1): one frame - every two-frame block half
    filled, every temporal tap of the front-end but the centre is padding; (96,2,3): six frames; (88,1,3): 22 -> 11 -> 6 -> 3, the stride-2 unit on an odd
    map (the last output row and column lose their far taps), NF odd; (88,3,3): NF = 9, two-frame blocks straddle clip boundaries."""
    feat, taps = _small(synth_sd, (hw, B, T), trunk_chain=0)
    assert [tuple(taps[i].shape) for i in ALL] == native.encoder_tap_shapes(B * T, hw)
    _check(synth_sd, feat, taps, f"per-unit hw={hw} B={B} T={T}", video=_video(hw, B, T))


# ------------------------------------------------------------------------------------------------ the chain is the per-unit arithmetic, map by map
@pytest.mark.parametrize("hw,B,T", SHAPES)
def test_stage_chain_taps_have_the_per_unit_bits(synth_sd, hw, B, T):
    """shuffle_s1xc (default: stages 2 and 3; "trunk_chain" = 2: stage 4 too): every map that reaches memory - the front-end, units 0, 3, 4, 11, 12 and
    13 - 15 (15 alone with stage 4 chained), conv_last - and feat have the bits of the per-unit launches."""
    feat0, taps0 = _small(synth_sd, (hw, B, T), trunk_chain=0)
    for which, options in ((DEFAULT_TAPS, {}), (CHAIN2_TAPS, {"trunk_chain": 2})):
        feat, taps = _small(synth_sd, (hw, B, T), which, **options)
        assert sorted(taps) == sorted(which)
        assert torch.isfinite(feat).all() and _same_bits(feat, feat0), options
        for i in which:
            assert _same_bits(taps[i], taps0[i]), (options, f"tap {i}")


def test_interior_unit_of_a_chain_is_refused(synth_sd):
    """units 1 - 2 and 5 - 10 (and 13 - 14 under "trunk_chain" = 2) never reach memory: asking for one fails the call before anything is launched"""
    v = _video(96, 2, 3).cuda()
    for options, unit in (({}, 1), ({}, 10), ({"trunk_chain": 2}, 13)):
        with pytest.raises(RuntimeError, match=rf"encoder tap of unit {unit} asked for, but the unit is interior to a stage-chain launch"):
            _nm(synth_sd, **options).encoder_fwd(v, taps=[vt.tap(unit)])
    _, taps = _run(_nm(synth_sd), _video(96, 2, 3), [vt.tap(13)])      # stage 4 is not chained by default
    assert torch.isfinite(taps[vt.tap(13)]).all()


# ------------------------------------------------------------------------------------------------ the other kernels
@pytest.mark.parametrize("hw,B,T", [(96, 2, 3), (88, 1, 3)])
@pytest.mark.parametrize("option", ["trunk_x3", "fuse_trunk", "fuse_s2"])
def test_every_unit_other_kernels(synth_sd, option, hw, B, T):
    """"trunk_x3" = 0: shuffle_s1 / shuffle_s2 on f32 MFMA; "fuse_trunk" = 0: dwconv3x3_kernel + GEMM for every unit; "fuse_s2" = 0: the unfused stride-2
    units only (with "trunk_chain" = 0, since the chain stays on beside them and would keep ten units on chip).  The f32 units' taps differ from the
    default's: another kernel really ran - unit 0 shows it on the SAME input (the front-end tap has the default's bits); from unit 1 on the inputs
    differ already, so those comparisons only say that the difference is carried along."""
    options = {option: 0, "trunk_chain": 0} if option == "fuse_s2" else {option: 0}
    feat, taps = _small(synth_sd, (hw, B, T), **options)
    _check(synth_sd, feat, taps, f"{option}=0 hw={hw} B={B} T={T}")
    if option == "trunk_x3":
        _, taps0 = _small(synth_sd, (hw, B, T), trunk_chain=0)
        assert _same_bits(taps[0], taps0[0])
        assert all(not torch.equal(taps[vt.tap(u)], taps0[vt.tap(u)]) for u in UNITS)


# ------------------------------------------------------------------------------------------------ the five-frames-per-block instances
BIG_TAPS = tuple(vt.tap(u) for u in (11, 12, 13, 14, 15)) + (vt.TAP_LAST,)


def _big_video(B, T):
    """as test_encoder_stage_chain_same_bits builds it: two synthetic clips repeated, plus seeded noise"""
    v = synth.synth_video(2, T, 96, 96, tag=f"stages_big_{T}").repeat((B + 1) // 2, 1, 1, 1, 1)[:B].clone()
    return v + 0.01 * torch.randn(v.shape, generator=torch.Generator().manual_seed(B))


@pytest.fixture(scope="module")
def big_default(synth_sd):
    """B = 64, T = 32: NF = 2048, the first launch size of the five-frames-per-block instances of the 3x3 stage (2048 mod 5 = 3: the last block is part
    filled), on the default model: shuffle_s1x<3,232,5>, and conv_last takes the split-bf16 kernel by its own rule"""
    return _run(_nm(synth_sd), _big_video(64, 32), BIG_TAPS)


def test_five_frame_blocks_default(synth_sd, big_default):
    feat, taps = big_default
    _check(synth_sd, feat, taps, "NF=2048 default", units=(12, 13, 14, 15))


def test_five_frame_blocks_f32_units(synth_sd, big_default):
    """"trunk_x3" = 0: shuffle_s1<3,232,5>"""
    feat, taps = _run(_nm(synth_sd, trunk_x3=0), _big_video(64, 32), BIG_TAPS)
    _check(synth_sd, feat, taps, "NF=2048 trunk_x3=0", units=(12, 13, 14, 15))
    assert all(not torch.equal(taps[vt.tap(u)], big_default[1][vt.tap(u)]) for u in (13, 14, 15))


def test_five_frame_blocks_chain(synth_sd, big_default):
    """"trunk_chain" = 2: shuffle_s1xc<3,232,5>; units 13 and 14 stay on chip, unit 15 and everything after it has the default's bits"""
    which = (vt.tap(11), vt.tap(12), vt.tap(15), vt.TAP_LAST)
    feat, taps = _run(_nm(synth_sd, trunk_chain=2), _big_video(64, 32), which)
    assert torch.isfinite(feat).all() and _same_bits(feat, big_default[0])
    for i in which:
        assert _same_bits(taps[i], big_default[1][i]), f"tap {i}"


def test_two_frame_blocks_one_frame_below_the_switch(synth_sd):
    """B = 89, T = 23: NF = 2047, the two-frame instance at its largest launch (the last block half filled)"""
    feat, taps = _run(_nm(synth_sd), _big_video(89, 23), BIG_TAPS)
    _check(synth_sd, feat, taps, "NF=2047 default", units=(12, 13, 14, 15))


# ------------------------------------------------------------------------------------------------ conv_last and the pooling
@pytest.mark.parametrize("options", [{"gemm_x3": 0}, {"gemm_x3": 3}, {"gemm_x3": 7}, {"gemm_x3_dma": 0}], ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_conv_last_and_pooling_kernel_forms(synth_sd, options):
    """conv_last (54 x 768 x 464; K = 14.5 steps of 32: the half-step tail of the 16x16x32 form) on the f32 kernel, forced onto the split-bf16 kernel with
    the wide and with the narrow tile, and with the weights split in the staging waves instead of fetched as planes; then mean + L2 norm of the device's tap"""
    which = (vt.tap(15), vt.TAP_LAST)
    feat, taps = _small(synth_sd, (96, 2, 3), which, **options)
    _check(synth_sd, feat, taps, "-".join(f"{k}={v}" for k, v in options.items()), units=())


# ------------------------------------------------------------------------------------------------ frames do not leak into each other
@pytest.mark.parametrize("options", [{}, {"trunk_chain": 0}], ids=["chain", "per-unit"])
@pytest.mark.parametrize("hw", [96, 88])
def test_neighbours_of_a_nan_clip_keep_their_bits(synth_sd, hw, options):
    """(hw, 3, 3) with clip 1 all NaN: every tap row and feat row of clips 0 and 2 has the bits of the all-finite call.  Frame 2 of clip 0 shares a two-frame
    block with frame 0 of the NaN clip."""
    B, T = 3, 3
    which = ALL if options else DEFAULT_TAPS
    feat0, taps0 = _small(synth_sd, (hw, B, T), which, **options)
    poisoned = _video(hw, B, T).clone()
    poisoned[1] = float("nan")
    feat1, taps1 = _run(_nm(synth_sd, **options), poisoned, which)
    keep = torch.tensor([0, 2])
    assert torch.isfinite(feat0).all() and _same_bits(feat0[keep], feat1[keep])
    for i in which:
        a, b = taps0[i].reshape(B, -1), taps1[i].reshape(B, -1)
        assert torch.isfinite(a).all() and _same_bits(a[keep], b[keep]), f"tap {i}"
    assert not torch.isfinite(taps1[0].reshape(B, -1)[1]).any()          # and the poison did arrive (the pool's fmaxf turns an all-NaN window into -inf)

# ------------------------------------------------------------------------------------------------ error paths
def test_short_workspace_is_refused_and_nothing_is_written(synth_sd):
    """a workspace one byte short of l2s_workspace_bytes(B, T, H, W, 1): the library's message, feat and every tap untouched"""
    nm, (hw, B, T) = _nm(synth_sd, trunk_chain=0), (96, 2, 3)
    D = native.diag()
    video = _video(hw, B, T).cuda()
    feat = torch.full((B, T, 768), 7.0, device="cuda")
    outs = [torch.full(s, 7.0, device="cuda") for s in native.encoder_tap_shapes(B * T, hw)]
    arr = (native._vp * len(outs))(*[t.data_ptr() for t in outs])
    need = int(D.l2s_workspace_bytes(B, T, hw, hw, 1))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert D.l2s_op_encoder_taps(nm._h, video.data_ptr(), B, T, hw, hw, arr, feat.data_ptr(), ws.data_ptr(), need - 1, stream) != 0
    assert "encoder workspace too small" in D.l2s_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [feat])
    assert D.l2s_op_encoder_taps(nm._h, video.data_ptr(), B, T, hw, hw, arr, feat.data_ptr(), ws.data_ptr(), need, stream) == 0
    torch.cuda.synchronize()
    ref_feat, ref_taps = _small(synth_sd, (hw, B, T), trunk_chain=0)
    assert _same_bits(feat.cpu(), ref_feat) and all(_same_bits(outs[i].cpu(), ref_taps[i]) for i in ALL)
