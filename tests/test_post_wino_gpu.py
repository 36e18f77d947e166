"""The Winograd F(4,5) route of post-net layers 1-3 on the GPU (csrc/post_wino.h; diagnostic option "post_wino": 0 = direct, 1 = from 4 096 rows per
batch on, 2 = at any row count).  Synthetic weights.  The small shapes run with "post_wino" = 2: a whole tile (S = 4), partial tiles with S mod 4 in
{1, 3}, S < 8 (every tile touches both paddings) and several clips.  Accuracy is measured against the fp64 oracle NEXT TO the direct route's own error
on the same input; everything else is bit for bit."""
import ctypes

import pytest
import torch

import parity_common as pc
from lip2speech_amd import native
from oracle import l2s_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4), (2, 5), (3, 7), (2, 77), (1, 123)]
_models = {}


def model(sd, **options):
    key = tuple(sorted(options.items()))
    if key not in _models:
        _models[key] = pc.fresh_native_model(sd, **options)
    return _models[key]


def mel_in(B, S, seed=11):
    g = torch.Generator().manual_seed(seed + 1000 * B + S)
    return torch.randn(B, S, 80, generator=g)


def post(nm, mel):
    out, _ = nm.postnet(mel.cuda())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.fixture(scope="module")
def sd64(synth_sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in synth_sd.items()}


@pytest.mark.parametrize("B,S", SHAPES)
def test_error_against_fp64_is_within_four_times_the_direct_routes(synth_sd, sd64, B, S):
    mel = mel_in(B, S)
    with torch.no_grad():
        cf = mel.double().transpose(1, 2).contiguous()
        ref = orc.postnet(sd64, cf) + cf
    wino, direct = post(model(synth_sd, post_wino=2), mel), post(model(synth_sd, post_wino=0), mel)
    assert torch.isfinite(wino).all() and not torch.equal(wino, direct), "the Winograd route did not run"
    e_w, e_d = pc.maxdiff(wino, ref), pc.maxdiff(direct, ref)
    print(f"post-net (B, S) = ({B}, {S}): max |d| against fp64: Winograd {e_w:.3e}, direct {e_d:.3e}, ratio {e_w / e_d:.2f}; max |post| {float(ref.abs().max()):.2f}")
    assert e_w <= 4 * e_d


def test_a_clip_in_a_batch_has_the_bits_it_has_alone(synth_sd):
    nm = model(synth_sd, post_wino=2)
    for S in (7, 77):
        mel = mel_in(3, S)
        batch = post(nm, mel)
        for b in range(3):
            assert torch.equal(batch[b], post(nm, mel[b:b + 1])[0]), f"S = {S}, clip {b}"


def test_weight_planes_by_dma_same_bits(synth_sd):
    mel = mel_in(3, 7)
    a, b = post(model(synth_sd, post_wino=2, gemm_x3_dma=1), mel), post(model(synth_sd, post_wino=2, gemm_x3_dma=0), mel)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, post(model(synth_sd, post_wino=0), mel))


def test_ragged_evaluate_group_has_the_bits_of_each_batch_alone(synth_sd):
    from test_forward_ragged_gpu import _batch, _dev, _same_bits
    nm = model(synth_sd, post_wino=2)
    X, Y = _batch([7, 8], 8, 6, "wino-x"), _batch([7], 7, 9, "wino-y")
    out = nm.forward_eval_ragged([_dev(X), _dev(Y)], [X["lens"], Y["lens"]], [6, 9])
    torch.cuda.synchronize()
    for name, bt, got in zip("XY", (X, Y), out):
        want = nm.forward_eval(*_dev(bt), bt["S"], video_lengths=bt["lens"])
        torch.cuda.synchronize()
        _same_bits(got, want, f"ragged [X, Y] with post_wino = 2 against the masked call on {name}")
    direct = model(synth_sd, post_wino=0).forward_eval(*_dev(Y), 9, video_lengths=Y["lens"])
    assert not torch.equal(direct[1], out[1][1]), "the Winograd route did not run"


def launches(nm, call):
    """{kernel name: launches} of `call`, read from the launch profile of the library that owns `nm`"""
    L = nm._L
    native.check(L.l2s_profile_enable(1), L)
    try:
        native.check(L.l2s_profile_reset(), L)
        call()
        torch.cuda.synchronize()
        out = {}
        for i in range(L.l2s_profile_count()):
            name, n, ms = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_double()
            native.check(L.l2s_profile_get(i, ctypes.byref(name), ctypes.byref(n), ctypes.byref(ms)), L)
            out[name.value.decode()] = int(n.value)
        return out
    finally:
        native.check(L.l2s_profile_enable(0), L)


def wino_launches(nm, B, S):
    mel = torch.zeros(B, S, 80, device="cuda")
    prof = launches(nm, lambda: nm.postnet(mel))
    return prof.get("postnet_wino_in", 0), prof.get("postnet_wino_out", 0), prof.get("postnet_conv_gemm", 0)


def test_route(synth_sd):
    nm = pc.native_model(synth_sd)                                  # the product library's compiled-in rule
    assert wino_launches(nm, 32, 300) == (3, 3, 5)                  # 9 600 rows: layers 1-3 through the new kernels, five product launches in all
    assert wino_launches(nm, 34, 100)[:2] == (0, 0)                 # 3 400 rows: below the edge
    assert wino_launches(nm, 2, 300)[:2] == (0, 0)                  # tap-split
    assert wino_launches(model(synth_sd, overlap_postnet=1), 32, 300)[:2] == (0, 0)
    assert wino_launches(model(synth_sd, infer_bf16=1), 32, 300)[:2] == (0, 0)
    assert wino_launches(model(synth_sd, post_wino=0), 32, 300)[:2] == (0, 0)
    assert wino_launches(model(synth_sd, post_wino=2), 2, 5)[:2] == (3, 3)
