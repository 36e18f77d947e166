"""Ragged groups on the GPU (include/l2s.h "ragged groups"): batches of unequal B and T as rows of ONE launch chain, every clip decoded as it would be
alone, the encoder on the real frames only.  Synthetic weights, S = 40, 96 x 96.
  batch A: clips of 7, 13, 22, 16 frames padded to 22 - the batch of test_masked_lengths_gpu.py: odd and even lengths, a clip at full T, the shortest legal one
  batch B: clips of 13 and 9 frames padded to T = 15: a pitch that differs from every length, another B, frames past the batch's longest clip
The reference per clip is the CPU oracle on the clip alone, computed once per module.  At these sizes no GEMM of any call reaches the split-bf16 tile
threshold and every post-net has at most 640 rows, so every kernel choice falls as it does for 1, 2 and 4 clips: rows are compared bit for bit."""
import ctypes

import pytest
import torch

import parity_common as pc
from lip2speech_amd import native, synth
from oracle import l2s_oracle as orc

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-3          # the project's parity gate
MARGIN = 1e-4           # attention argmax is compared where the oracle's top-2 margin exceeds this
S = 40
LENS_A, T_A = [7, 13, 22, 16], 22
LENS_B, T_B = [13, 9], 15
PAIRS = sum((n + 1) // 2 for n in LENS_A + LENS_B)      # 42 front-end pair blocks, not 4 * 11 + 2 * 8


def _batch(lens, T, tag):
    B, m = len(lens), native.min_T(T)
    video = synth.synth_padded_video(B, lens, tag=tag)
    if video.shape[2] < T:
        video = torch.cat([video, torch.zeros(B, 3, T - video.shape[2], 96, 96)], dim=2)
    return {"lens": lens, "T": T, "m": m, "video": video.contiguous(), "emb": synth.synth_speaker_embedding(B, tag=tag), "gumbel": synth.synth_gumbel(B * m, tag=tag)}


def _solo(bt, b):
    """clip b alone: (video (1,3,len,H,W), emb (1,256), its first len // 7 Gumbel rows)"""
    n, m = bt["lens"][b], bt["m"]
    return bt["video"][b:b + 1, :, :n].contiguous(), bt["emb"][b:b + 1], bt["gumbel"][b * m:b * m + n // 7]


def _dev(bt):
    return bt["video"].cuda(), bt["emb"].cuda(), bt["gumbel"].cuda()


@pytest.fixture(scope="module")
def case(synth_sd):
    c = {"sd": synth_sd, "A": _batch(LENS_A, T_A, "masked"), "B": _batch(LENS_B, T_B, "ragged-b")}
    assert c["A"]["video"].shape[2] == T_A and c["B"]["video"].shape[2] == T_B and not c["B"]["video"][0, :, 13:].any()
    with torch.no_grad():
        for bt in (c["A"], c["B"]):
            bt["ref"], stops = [], []
            for b in range(len(bt["lens"])):
                taps = {}
                bt["ref"].append(orc.inference(synth_sd, *_solo(bt, b), S=S, taps=taps))
                stops.append(taps["stop"])
            bt["ref_stop"] = torch.cat(stops)      # (B,S): the solo stop logits
    return c


def _ragged(nm, bts, **kw):
    out = nm.inference_ragged([_dev(bt) for bt in bts], [bt["lens"] for bt in bts], S=S, want_attn=True, **kw)
    torch.cuda.synchronize()
    return [tuple(t.clone() for t in o) for o in out]


@pytest.fixture(scope="module")
def ragged_ab(case):
    """the group [A, B] through l2s_inference_ragged, once"""
    nm = pc.native_model(case["sd"])
    out = _ragged(nm, [case["A"], case["B"]])
    assert nm.calls["l2s_inference_ragged"] >= 1
    return out


def _same_rows(got, want, lens, tag):
    """mel_post, lengths and attention at t < len of every row, bit for bit (attention columns past len: zeros on both sides, checked apart)"""
    assert torch.equal(got[1], want[1]), tag
    for b, n in enumerate(lens):
        d = pc.maxdiff(got[0][b], want[0][b])
        print(f"{tag}: row {b} ({n} frames) max |d mel_post| = {d:.3e}")
        assert torch.equal(got[0][b], want[0][b]), f"{tag}: row {b}"
        assert torch.equal(got[2][b, :, :n], want[2][b, :, :n]), f"{tag}: row {b} attention"


def test_each_clip_matches_the_oracle_alone(case, ragged_ab):
    for name, out in zip("AB", ragged_ab):
        bt = case[name]
        mel, lengths, attn = (t.cpu() for t in out)
        assert mel.shape == (len(bt["lens"]), 80, S) and attn.shape == (len(bt["lens"]), S, bt["T"])
        for b, n in enumerate(bt["lens"]):
            r_mel, r_len, r_attn = bt["ref"][b]
            d = pc.maxdiff(mel[b], r_mel[0])
            arg, margin = pc.top2(r_attn[0])
            sure = margin > MARGIN
            print(f"ragged [A, B]: batch {name} clip {b} ({n} frames) max |mel_post - solo oracle| = {d:.3e}, output length {int(lengths[b])}, "
                  f"mean |mel| {float(r_mel.abs().mean()):.3f}, argmax compared at {float(sure.float().mean()):.1%} of the positions")
            assert d < MEL_TOL
            assert int(lengths[b]) == int(r_len[0])
            assert not attn[b, :, n:].any(), "attention columns past the clip's length must be exactly 0"
            assert pc.maxdiff(attn[b, :, :n].sum(dim=-1), torch.ones(S)) < 1e-5
            assert float(sure.float().mean()) >= 0.9
            assert torch.equal(attn[b, :, :n].argmax(dim=-1).to(torch.int32)[sure], arg[sure])


def test_bits_of_todays_route(case, ragged_ab):
    """rows of the ragged call = l2s_inference_masked on A and on B separately"""
    nm = pc.native_model(case["sd"])
    for name, out in zip("AB", ragged_ab):
        bt = case[name]
        want = nm.inference(*_dev(bt), S=S, want_attn=True, video_lengths=bt["lens"])
        torch.cuda.synchronize()
        _same_rows(out, want, bt["lens"], f"ragged against the masked call on {name}")
        assert not out[2][:, :, max(bt["lens"]):].any()


def test_pad_frames_are_never_read(case, ragged_ab):
    """every frame t >= len_b of both videos NaN: the same bits"""
    nm = pc.native_model(case["sd"])
    bts = []
    for name in "AB":
        bt = dict(case[name])
        bt["video"] = bt["video"].clone()
        for b, n in enumerate(bt["lens"]):
            bt["video"][b, :, n:] = float("nan")
        assert bt["video"].isnan().any() or max(bt["lens"]) == bt["T"]
        bts.append(bt)
    assert bts[0]["video"].isnan().any() and bts[1]["video"][:, :, 13:].isnan().all()
    out = _ragged(nm, bts)
    for name, got, want in zip("AB", out, ragged_ab):
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all()
        _same_rows(got, want, case[name]["lens"], f"NaN pad frames, batch {name}")


def test_composition_does_not_matter(case, ragged_ab):
    nm = pc.native_model(case["sd"])
    ba = _ragged(nm, [case["B"], case["A"]])
    a = _ragged(nm, [case["A"]])
    _same_rows(ba[1], ragged_ab[0], LENS_A, "A in [B, A] against A in [A, B]")
    _same_rows(ba[0], ragged_ab[1], LENS_B, "B in [B, A] against B in [A, B]")
    _same_rows(a[0], ragged_ab[0], LENS_A, "A alone against A in [A, B]")


def test_early_stop_composes(case):
    """A stop bias under which every clip stops inside S: with "early_stop" on, the ragged call's lengths and kept frames are the option-off call's,
    the dropped frames exact zeros."""
    ref_stop = torch.cat([case["A"]["ref_stop"], case["B"]["ref_stop"]])
    shift = -float(ref_stop[:, :25].max(dim=1).values.min()) + 1e-2      # the stop logits do not feed back: every clip now crosses within 25 steps
    sd = dict(case["sd"])
    sd["decoder.stop_token_layer.linear_layer.bias"] = sd["decoder.stop_token_layer.linear_layer.bias"] + shift
    nm = pc.fresh_native_model(sd, persist_decode=0)
    off = _ragged(nm, [case["A"], case["B"]])
    nm.set_option("early_stop", 1)
    on = _ragged(nm, [case["A"], case["B"]])
    for name, f, o in zip("AB", off, on):
        lens = f[1].cpu()
        print(f"early stop: batch {name} output lengths", lens.tolist())
        assert int(lens.max()) < S and torch.equal(o[1].cpu(), lens)
        for b, n in enumerate(lens.tolist()):
            assert torch.equal(o[0][b, :, :n], f[0][b, :, :n]) and torch.equal(o[2][b, :n], f[2][b, :n])
            assert not o[0][b, :, n:].any() and not o[2][b, n:].any()


def _c_call(L, nm, bts, lens_flat, mel, lengths, attn):
    G = len(bts)
    dev = [_dev(bt) for bt in bts]
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    bB, bT = (i32 * G)(*[len(bt["lens"]) for bt in bts]), (i32 * G)(*[bt["T"] for bt in bts])
    ws = torch.empty(native.workspace_bytes_ragged(list(bB), list(bT), 96, 96, S), dtype=torch.uint8, device="cuda")
    arr = lambda k: (vp * G)(*[d[k].data_ptr() for d in dev])      # noqa: E731
    rc = L.l2s_inference_ragged(nm._h, G, arr(0), arr(1), arr(2), bB, bT, (i32 * len(lens_flat))(*lens_flat), 96, 96, S, mel.data_ptr(), lengths.data_ptr(),
                                attn.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return rc, L.l2s_last_error().decode()


def test_errors_leave_the_outputs_untouched(case):
    bts = [case["A"], case["B"]]
    N = len(LENS_A) + len(LENS_B)
    mel = torch.full((N, 80, S), 7.0, device="cuda")
    lengths = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    attn = torch.full((N, S, T_A), 7.0, device="cuda")

    def untouched():
        return bool((mel == 7.0).all()) and bool((lengths == -1).all()) and bool((attn == 7.0).all())

    nm = pc.native_model(case["sd"])
    for flat, msg in (([7, 13, 22, 16, 13, 6], "video_lengths[5] = 6 (batch 1, row 1) is outside [7, T = 15]"),
                      ([7, 13, 22, 16, 16, 9], "video_lengths[4] = 16 (batch 1, row 0) is outside [7, T = 15]"),
                      ([7, 23, 22, 16, 13, 9], "video_lengths[1] = 23 (batch 0, row 1) is outside [7, T = 22]")):
        rc, err = _c_call(native.lib(), nm, bts, flat, mel, lengths, attn)
        assert rc != 0 and msg in err, err
        assert untouched()
    with pytest.raises(ValueError, match=r"outside \[7, T = 15\]"):
        nm.inference_ragged([_dev(bt) for bt in bts], [LENS_A, [13, 6]], S=S)
    # the ragged front-end exists in the default form only: the bf16 leg and the other block forms are refused by the option's name
    flat = LENS_A + LENS_B
    for lib, opts, name in ((native.lib(), {"infer_bf16": 1}, "infer_bf16"), (native.diag(), {"frontend_x3": 2}, "frontend_x3")):
        other = pc.fresh_native_model(case["sd"], diag=lib is not native.lib(), persist_decode=0, **opts)
        rc, err = _c_call(lib, other, bts, flat, mel, lengths, attn)
        assert rc != 0 and f'"{name}"' in err, err
        assert untouched()
        with pytest.raises(RuntimeError, match=name):
            other.inference_ragged([_dev(bt) for bt in bts], [LENS_A, LENS_B], S=S)
    rc, err = _c_call(native.lib(), nm, bts, flat, mel, lengths, attn)      # the same buffers through a call that is legal: now they are written
    assert rc == 0 and not untouched() and int(lengths.min()) >= 1


def _launches(call):
    native.profile_enable(True)
    try:
        native.profile_reset()
        call()
        torch.cuda.synchronize()
        return {name: n for name, n, _ in native.profile_read() if n > 0}
    finally:
        native.profile_enable(False)


def test_route(case):
    """One front-end launch over 42 pair blocks and one launch per trunk stage for the whole group; no persistent kernel, even with the persistent
    options set."""
    nm = pc.fresh_native_model(case["sd"], persist_decode=4, persist_masked=1)
    solo = _launches(lambda: nm.inference(*_dev(case["B"]), S=S, video_lengths=LENS_B))      # one masked call: what ONE launch chain issues
    group = _launches(lambda: nm.inference_ragged([_dev(case["A"]), _dev(case["B"])], [LENS_A, LENS_B], S=S))
    print("ragged group:", {k: v for k, v in group.items() if not k.startswith("step_")})
    assert group["frontend3d_conv_bn_prelu_pool_ragged"] == 1 and "frontend3d_conv_bn_prelu_pool" not in group
    assert group["frontend3d_ragged_pair_blocks"] == PAIRS == 42
    assert group["avgpool_l2norm_cat_ragged"] == 1 and "avgpool_l2norm_cat" not in group
    trunk = [k for k in solo if k.startswith("shuffle_") or k == "conv_last_gemm"]
    assert len(trunk) >= 4 and solo["conv_last_gemm"] == 1
    for k in trunk:
        assert group[k] == solo[k], k      # the trunk of the whole group: the launches of one call
    assert not [k for k in group if "persistent" in k]
    assert group["bilstm_step"] == T_A and group["step_lstm_cell"] == 2 * S


def test_python_layer(case):
    """Lip2Speech.inference_many_lengths over [A, B, A]: one ragged group, each result what net.inference(video_lengths=) gives;
    callers.demo_clips(honour_lengths=True, group_lengths=True) yields what honour_lengths=True alone yields."""
    from lip2speech_amd import callers
    from model.model import get_network
    net = get_network("test").cuda()
    net.load_state_dict(case["sd"], strict=True)
    was = net.decoder.hparams.max_decoder_steps
    net.decoder.hparams.max_decoder_steps = S      # 10 x 40 post-net rows: every call of this test takes the post-net form of one or two clips
    try:
        bts = [case["A"], case["B"], case["A"]]
        calls = [(bt["video"], None, bt["emb"], True, {"gumbel_noise": bt["gumbel"], "video_lengths": torch.tensor(bt["lens"])}) for bt in bts]
        outs = list(net.inference_many_lengths(calls, group=8, n_inflight=3))
        torch.cuda.synchronize()
        pool = net.pool(8, 3)
        assert pool.stats["inference_ragged_groups"] == 1 and pool.stats["inference_ragged_batches"] == 3 and pool.stats["max_group"] == 3
        assert net.native_model().calls["l2s_inference_ragged"] == 1
        for bt, got in zip(bts, outs):
            v, e, g = _dev(bt)
            want = net.inference(v, None, speaker_embedding=e, return_attention_map=True, gumbel_noise=g, video_lengths=bt["lens"])
            torch.cuda.synchronize()
            assert got[2].shape == (len(bt["lens"]), S, bt["T"])
            _same_rows(got, want, bt["lens"], "inference_many_lengths")
        with pytest.raises(ValueError, match="video_lengths"):
            list(net.inference_many_lengths([(bts[0]["video"], None, bts[0]["emb"])]))
        # the demo loop: batch_size 1, every clip at its own length; the Gumbel noise is drawn per batch, in loader order on both routes
        clips = [_solo(case["A"], 1), _solo(case["B"], 1), _solo(case["A"], 3)]
        loader = [((v, torch.tensor([v.shape[2]])), (None, None), None, None, None) for v, _, _ in clips]
        emb = case["A"]["emb"][:1].cuda()
        torch.manual_seed(7)
        want = list(callers.demo_clips(net, loader, speaker_embedding=emb, honour_lengths=True))
        n_ragged = net.native_model().calls["l2s_inference_ragged"]
        torch.manual_seed(7)
        got = list(callers.demo_clips(net, loader, speaker_embedding=emb, honour_lengths=True, group_lengths=True, group=2, n_inflight=2))
        torch.cuda.synchronize()
        assert net.native_model().calls["l2s_inference_ragged"] == n_ragged + 2      # groups of two clips: [13, 9] and [16]
        assert len(got) == len(want) == 3
        for g, w in zip(got, want):
            assert all(torch.equal(a, b) for a, b in zip(g, w))
        with pytest.raises(ValueError, match="honour_lengths"):
            list(callers.demo_clips(net, loader, speaker_embedding=emb, group_lengths=True))
    finally:
        net.decoder.hparams.max_decoder_steps = was
