"""The evaluate-shaped ragged group on the GPU (include/l2s.h "ragged groups", l2s_forward_eval_ragged): batches of unequal B, T AND step count S as rows
of ONE launch chain; batch g's packed blocks are what l2s_forward_eval_masked gives that batch alone at S = S_g.  Synthetic weights, 96 x 96.
  batch A: clips of 7, 13, 22, 16 frames padded to 22, S = 40 - the batch of test_masked_lengths_gpu.py
  batch B: clips of 13 and 9 frames padded to T = 15, S = 23: odd, and shorter than the group's - in [A, B, C] its rows hold 17 decoded frames past its S
  batch C: one clip of 7 frames, S = 3: shorter than one Conv1d's five taps, so every post-net layer overhangs at every row; 37 frames past its S
The group [A, B, C] has 7 x 40 = 280 post-net rows and every batch alone has fewer: all take the one-slice-per-tap post-net form, and no GEMM of any call
reaches a split-bf16 tile threshold, so rows are compared bit for bit.  The other two post-net forms are reached by the long-S batches D, E, F further down,
checked for bits against the masked call only.  The reference per clip is the CPU oracle on the clip alone, computed once per module."""
import ctypes

import pytest
import torch

import parity_common as pc
from lip2speech_amd import native, synth
from oracle import l2s_oracle as orc

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-3          # the project's parity gate
MARGIN = 1e-4           # attention argmax is compared where the oracle's top-2 margin exceeds this
NAMES = ("mel", "mel_post", "stop", "logits", "content_dis")


def _batch(lens, T, S, tag):
    B, m = len(lens), native.min_T(T)
    video = synth.synth_padded_video(B, lens, tag=tag)
    if video.shape[2] < T:
        video = torch.cat([video, torch.zeros(B, 3, T - video.shape[2], 96, 96)], dim=2)
    return {"lens": lens, "T": T, "S": S, "m": m, "video": video.contiguous(), "emb": synth.synth_speaker_embedding(B, tag=tag),
            "gumbel": synth.synth_gumbel(B * m, tag=tag)}


def _solo(bt, b):
    """clip b alone: (video (1,3,len,H,W), emb (1,256), its first len // 7 Gumbel rows)"""
    n, m = bt["lens"][b], bt["m"]
    return bt["video"][b:b + 1, :, :n].contiguous(), bt["emb"][b:b + 1], bt["gumbel"][b * m:b * m + n // 7]


def _dev(bt):
    return bt["video"].cuda(), bt["emb"].cuda(), bt["gumbel"].cuda()


@pytest.fixture(scope="module")
def case(synth_sd):
    c = {"sd": synth_sd, "A": _batch([7, 13, 22, 16], 22, 40, "masked"), "B": _batch([13, 9], 15, 23, "ragged-b"), "C": _batch([7], 7, 3, "ragged-c")}
    assert c["A"]["video"].shape[2] == 22 and c["B"]["video"].shape[2] == 15 and not c["B"]["video"][0, :, 13:].any()
    with torch.no_grad():
        for name in "ABC":
            bt = c[name]
            bt["ref"] = [orc.forward_eval(synth_sd, *_solo(bt, b)[:2], torch.zeros(1, 80, bt["S"]), _solo(bt, b)[2]) for b in range(len(bt["lens"]))]
    return c


def _ragged(nm, bts):
    out = nm.forward_eval_ragged([_dev(bt) for bt in bts], [bt["lens"] for bt in bts], [bt["S"] for bt in bts])
    torch.cuda.synchronize()
    return [tuple(t.clone() for t in o) for o in out]


def _masked(nm, bt, S=None):
    out = nm.forward_eval(*_dev(bt), bt["S"] if S is None else S, video_lengths=bt["lens"])
    torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


@pytest.fixture(scope="module")
def ragged_abc(case):
    """the group [A, B, C] through l2s_forward_eval_ragged, once"""
    nm = pc.native_model(case["sd"])
    out = _ragged(nm, [case["A"], case["B"], case["C"]])
    assert nm.calls["l2s_forward_eval_ragged"] >= 1
    return out


def _same_bits(got, want, tag):
    """the five outputs of one batch, bit for bit (-inf logits compare equal)"""
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, f"{tag}: {name} {tuple(g.shape)} against {tuple(w.shape)}"
        if not torch.equal(g, w):
            fin = torch.isfinite(w) & torch.isfinite(g)
            print(f"{tag}: {name} max |d| = {float((g - w)[fin].abs().max()):.3e}")
        assert torch.equal(g, w), f"{tag}: {name}"


def test_each_clip_matches_the_oracle_alone(case, ragged_abc):
    for name, out in zip("ABC", ragged_abc):
        bt = case[name]
        B, T, S, m = len(bt["lens"]), bt["T"], bt["S"], bt["m"]
        mel_cf, mel_post, stop, logits, dis = (t.cpu() for t in out)
        assert mel_cf.shape == mel_post.shape == (B, 80, S) and stop.shape == (B, S) and logits.shape == (B, S, T) and dis.shape == (B * m, 501)
        assert all(t.is_contiguous() for t in out)
        for b, n in enumerate(bt["lens"]):
            r = bt["ref"][b]
            d = [pc.maxdiff(mel_cf[b], r[0][0]), pc.maxdiff(mel_post[b], r[1][0]), pc.maxdiff(stop[b], r[2][0, :, 0]), pc.maxdiff(dis[b * m:b * m + n // 7], r[5])]
            arg, margin = pc.top2(torch.softmax(r[4][0], dim=-1))
            sure = margin > MARGIN
            print(f"forward_eval_ragged [A, B, C]: batch {name} clip {b} ({n} frames, S = {S}) max |d| mel {d[0]:.3e} mel_post {d[1]:.3e} stop {d[2]:.3e} "
                  f"content_dis {d[3]:.3e}; mean |mel_post| {float(r[1].abs().mean()):.3f}; argmax compared at {float(sure.float().mean()):.1%} of the steps")
            assert max(d) < MEL_TOL
            assert not dis[b * m + n // 7:(b + 1) * m].any(), "content_dis rows past the clip's slots must be exactly 0"
            assert torch.isneginf(logits[b, :, n:]).all() and torch.isfinite(logits[b, :, :n]).all()
            assert torch.equal(logits[b, :, :n].argmax(dim=-1).to(torch.int32)[sure], arg[sure])


def test_bits_of_todays_route(case, ragged_abc):
    """every batch's five outputs = l2s_forward_eval_masked on that batch alone at its own S"""
    nm = pc.native_model(case["sd"])
    for name, out in zip("ABC", ragged_abc):
        _same_bits(out, _masked(nm, case[name]), f"ragged [A, B, C] against the masked call on {name}")


def test_composition_does_not_matter(case, ragged_abc):
    nm = pc.native_model(case["sd"])
    cba = _ragged(nm, [case["C"], case["B"], case["A"]])
    for i, name in enumerate("CBA"):
        _same_bits(cba[i], ragged_abc["ABC".index(name)], f"{name} in [C, B, A] against {name} in [A, B, C]")
    _same_bits(_ragged(nm, [case["B"]])[0], ragged_abc[1], "B alone against B in [A, B, C]")
    _same_bits(_ragged(nm, [case["A"]])[0], ragged_abc[0], "A alone against A in [A, B, C]")


def test_inputs_discriminate(case):
    """Batch B decoded for S = 40 and cut to 23 frames against the S = 23 call: the decode loop is causal (same pre-post-net mel), the post-net is not - its
    five same-padded Conv1d layers carry the frames past 23 up to ten frames back (for clip 0 the CPU oracle gives 2.2e-2 at frame 13 rising to 5.7 at
    frame 21).  So a ragged call that forgot a row's own S would fail the bit checks above: they are not vacuous."""
    nm = pc.native_model(case["sd"])
    bt = case["B"]
    long, short = _masked(nm, bt, S=40), _masked(nm, bt)
    d_cf = pc.maxdiff(long[0][:, :, :23], short[0])
    d_post = (long[1][:, :, :23] - short[1]).abs().amax(dim=1).cpu()      # (B, 23): per clip and frame
    print(f"B at S = 40 cut to 23 against S = 23: max |d mel| = {d_cf:.3e}; max |d mel_post| per frame, clip 0: " + " ".join(f"{float(v):.1e}" for v in d_post[0]))
    print("clip 1: " + " ".join(f"{float(v):.1e}" for v in d_post[1]))
    assert d_cf < 1e-5
    assert bool((d_post[0, 13:] > 1e-3).all()), "every one of the last ten frames must see the frames past S"      # the clip the oracle figures are for
    assert float(d_post[1, 13:].max()) > 1e-3


def test_pad_frames_are_never_read(case, ragged_abc):
    """every frame t >= len_c of the videos NaN: the same bits"""
    nm = pc.native_model(case["sd"])
    bts = []
    for name in "ABC":
        bt = dict(case[name])
        bt["video"] = bt["video"].clone()
        for b, n in enumerate(bt["lens"]):
            bt["video"][b, :, n:] = float("nan")
        bts.append(bt)
    assert bts[0]["video"].isnan().any() and bts[1]["video"][:, :, 13:].isnan().all()
    for name, got, want in zip("ABC", _ragged(nm, bts), ragged_abc):
        assert torch.isfinite(got[1]).all() and torch.isfinite(got[0]).all()
        _same_bits(got, want, f"NaN pad frames, batch {name}")


def _c_call(L, nm, bts, lens_flat, steps, outs):
    G = len(bts)
    dev = [_dev(bt) for bt in bts]
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    bB, bT, bS = (i32 * G)(*[len(bt["lens"]) for bt in bts]), (i32 * G)(*[bt["T"] for bt in bts]), (i32 * G)(*steps)
    legal = [min(max(s, 1), 300) for s in steps]      # the workspace of the legal shapes: an illegal call never gets as far as using it
    ws = torch.empty(native.workspace_bytes_eval_ragged(list(bB), list(bT), legal), dtype=torch.uint8, device="cuda")
    arr = lambda k: (vp * G)(*[d[k].data_ptr() for d in dev])      # noqa: E731
    rc = L.l2s_forward_eval_ragged(nm._h, G, arr(0), arr(1), arr(2), bB, bT, bS, (i32 * len(lens_flat))(*lens_flat), 96, 96, *[t.data_ptr() for t in outs],
                                   ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return rc, L.l2s_last_error().decode()


def test_errors_leave_the_outputs_untouched(case):
    bts = [case["A"], case["B"], case["C"]]
    flat, steps = [v for bt in bts for v in bt["lens"]], [bt["S"] for bt in bts]
    mel_off, stop_off, attn_off, dis_off = native.forward_eval_ragged_plan([4, 2, 1], [22, 15, 7], steps)[:4]
    outs = [torch.full((n,), 7.0, device="cuda") for n in (mel_off[3], mel_off[3], stop_off[3], attn_off[3], dis_off[3])]

    def untouched():
        return all(bool((t == 7.0).all()) for t in outs)

    nm = pc.native_model(case["sd"])
    for f, s, msg in ((flat, [40, 301, 3], "batch 1 has S = 301, outside [1, 300]"), (flat, [40, 23, 0], "batch 2 has S = 0, outside [1, 300]"),
                      ([7, 13, 22, 16, 13, 6, 7], steps, "video_lengths[5] = 6 (batch 1, row 1) is outside [7, T = 15]"),
                      ([7, 13, 22, 16, 16, 9, 7], steps, "video_lengths[4] = 16 (batch 1, row 0) is outside [7, T = 15]")):
        rc, err = _c_call(native.lib(), nm, bts, f, s, outs)
        assert rc != 0 and msg in err, err
        assert untouched()
    with pytest.raises(ValueError, match=r"S outside \[1, 300\]"):
        nm.forward_eval_ragged([_dev(bt) for bt in bts], [bt["lens"] for bt in bts], [40, 301, 3])
    other = pc.fresh_native_model(case["sd"], persist_decode=0, infer_bf16=1)      # the ragged front-end exists in the default form only
    rc, err = _c_call(native.lib(), other, bts, flat, steps, outs)
    assert rc != 0 and '"infer_bf16"' in err and "l2s_forward_eval_ragged" in err, err
    assert untouched()
    with pytest.raises(RuntimeError, match="infer_bf16"):
        other.forward_eval_ragged([_dev(bt) for bt in bts], [bt["lens"] for bt in bts], steps)
    rc, err = _c_call(native.lib(), nm, bts, flat, steps, outs)      # the same buffers through a call that is legal: now every element is written
    assert rc == 0, err
    assert all(not bool((t == 7.0).any()) for t in outs[:3]) and not untouched()


def _launches(call):
    native.profile_enable(True)
    try:
        native.profile_reset()
        call()
        torch.cuda.synchronize()
        return {name: n for name, n, _ in native.profile_read() if n > 0}
    finally:
        native.profile_enable(False)


def test_plain_conv_postnet_form(case):
    """Every batch and the call above 640 post-net rows: the Conv1d layers run as plain K = 5 x Cin GEMMs.  D: 4 clips of 7 frames, S = 170 (680 rows); E:
    lengths [7, 8, 7, 9] padded to 9, S = 163 (652 rows; its rows hold 7 decoded frames past its S in [D, E]).  Bits against the masked call only."""
    nm = pc.native_model(case["sd"])
    D, E = _batch([7, 7, 7, 7], 7, 170, "ragged-d"), _batch([7, 8, 7, 9], 9, 163, "ragged-e")
    prof = _launches(lambda: nm.forward_eval_ragged([_dev(D), _dev(E)], [D["lens"], E["lens"]], [170, 163]))
    print("[D, E] launch profile (the post-net forms share one entry: the form follows from the rows, 8 x 170 = 1360 > 640):",
          {k: v for k, v in prof.items() if "postnet" in k or k.startswith("eval_")})
    de = _ragged(nm, [D, E])
    _same_bits(de[0], _masked(nm, D), "D in [D, E] against the masked call on D")
    _same_bits(de[1], _masked(nm, E), "E in [D, E] against the masked call on E")
    _same_bits(_ragged(nm, [E])[0], de[1], "E alone against E in [D, E]")


def test_split_bf16_postnet_form(case, ragged_abc):
    """F: 16 clips of 7 frames, S = 200: 3 200 post-net rows, where layers 1-3 take the split-bf16 GEMM; with C, 17 x 200 = 3 400 rows, the same bracket.
    F's rows are the masked call's bits; C's one row then takes another post-net form than it does alone (one slice per tap): held to the gate only."""
    nm = pc.native_model(case["sd"])
    F = _batch([7] * 16, 7, 200, "ragged-f")
    prof = _launches(lambda: nm.forward_eval_ragged([_dev(F), _dev(case["C"])], [F["lens"], case["C"]["lens"]], [200, 3]))
    print("[F, C] launch profile (the post-net forms share one entry: the form follows from the rows, 3 400):",
          {k: v for k, v in prof.items() if "postnet" in k or k.startswith("eval_")})
    fc = _ragged(nm, [F, case["C"]])
    _same_bits(fc[0], _masked(nm, F), "F in [F, C] against the masked call on F")
    for name, g, w in zip(NAMES, fc[1], ragged_abc[2]):
        fin = torch.isfinite(w)
        d = float((g - w)[fin].abs().max())
        print(f"C in [F, C] against C in [A, B, C]: {name} max |d| = {d:.3e}")
        assert g.shape == w.shape and torch.equal(torch.isfinite(g), fin) and d < MEL_TOL


def test_clip_table_crosses_a_chunk_of_the_carrier(synth_sd):
    """The per-clip table travels in kernel arguments, native.TABLE_CHUNK words per launch (csrc/host_table.h), and a clip's record is 8 words: one clip more
    than a launch carries, so the last clip's record is written by the second launch.  121 clips of 7 frames at 88 x 88 in eight batches of 16 and 15, S = 3
    and 4 by turns.  Row by row against the masked call on every batch alone; the group's 121 rows take other GEMM and post-net forms than a batch's 16 (the
    choices follow the rows of the call), so the rows are held to the gate, as C is in test_split_bf16_postnet_form."""
    N = native.TABLE_CHUNK // 8 + 1
    assert N <= native.MAX_RAGGED_CLIPS
    sizes = [N // 8 + (g < N % 8) for g in range(8)]
    nm = pc.native_model(synth_sd)
    bts = []
    for g, B in enumerate(sizes):
        bts.append({"lens": [7] * B, "T": 7, "S": 3 + g % 2, "m": 1, "video": synth.synth_video(B, 7, 88, 88, tag=f"chunk-{g}"),
                    "emb": synth.synth_speaker_embedding(B, tag=f"chunk-{g}"), "gumbel": synth.synth_gumbel(B, tag=f"chunk-{g}")})
    group = _ragged(nm, bts)
    for g, (bt, got) in enumerate(zip(bts, group)):
        want = _masked(nm, bt)
        for name, a, w in zip(NAMES, got, want):
            fin = torch.isfinite(w)
            d = float((a - w)[fin].abs().max())
            print(f"batch {g} ({len(bt['lens'])} clips, S = {bt['S']}) in the group of {N} against the masked call: {name} max |d| = {d:.3e}")
            assert a.shape == w.shape and torch.equal(torch.isfinite(a), fin) and d < MEL_TOL


def test_route(case):
    """One ragged front-end launch for the group, Smax decode steps, the five zero-fill launches exactly when the step counts differ, and no persistent
    kernel even with the persistent options set."""
    nm = pc.fresh_native_model(case["sd"], persist_decode=4, persist_masked=1)
    bts = [case["A"], case["B"], case["C"]]
    group = _launches(lambda: nm.forward_eval_ragged([_dev(bt) for bt in bts], [bt["lens"] for bt in bts], [40, 23, 3]))
    print("ragged evaluate group:", {k: v for k, v in group.items() if not k.startswith("step_")})
    assert group["frontend3d_conv_bn_prelu_pool_ragged"] == 1 and "frontend3d_conv_bn_prelu_pool" not in group
    assert group["step_lstm_cell"] == 2 * 40 and group["bilstm_step"] == 22
    assert group["eval_zero_rows_past_s"] == 5             # the decoded mel and the outputs of post-net layers 0..3
    assert group["eval_scatter_blocks"] == 4 and group["eval_scatter_mel_cf"] == 1
    assert not [k for k in group if "persistent" in k]
    same = _launches(lambda: nm.forward_eval_ragged([_dev(case["A"]), _dev(case["B"])], [case["A"]["lens"], case["B"]["lens"]], [40, 40]))
    assert "eval_zero_rows_past_s" not in same and same["eval_scatter_blocks"] == 4 and same["step_lstm_cell"] == 2 * 40
    assert not [k for k in same if "persistent" in k]


def test_python_layer(case):
    """Lip2Speech.forward_many_lengths over [A, B, A]: one ragged group, each result what net(...) gives with honour_video_lengths on;
    callers.evaluate_mels(honour_lengths=True, group_lengths=True) returns what honour_lengths=True alone returns."""
    from lip2speech_amd import callers
    from model.model import get_network
    net = get_network("test").cuda()
    net.load_state_dict(case["sd"], strict=True)
    bts = [case["A"], case["B"], case["A"]]
    mels = [torch.zeros(len(bt["lens"]), 80, bt["S"]) for bt in bts]
    calls = [(bt["video"], None, None, ml, torch.tensor(bt["lens"]), None, None, 1, {"speaker_embedding": bt["emb"], "gumbel_noise": bt["gumbel"]})
             for bt, ml in zip(bts, mels)]
    outs = list(net.forward_many_lengths(calls, group=8, n_inflight=3))
    torch.cuda.synchronize()
    pool = net.pool(8, 3)
    assert pool.stats["forward_ragged_groups"] == 1 and pool.stats["forward_ragged_batches"] == 3 and pool.stats["max_group"] == 3
    assert net.native_model().calls["l2s_forward_eval_ragged"] == 1
    assert not net.honour_video_lengths                    # the method does not depend on the attribute
    net.honour_video_lengths = True
    try:
        for bt, ml, got in zip(bts, mels, outs):
            v, e, g = _dev(bt)
            with torch.no_grad():
                want = net(v, None, None, ml, torch.tensor(bt["lens"]), None, None, 1, speaker_embedding=e, gumbel_noise=g)
            torch.cuda.synchronize()
            assert len(got) == len(want) == 7 and torch.equal(got[6], want[6]) and got[2].shape == (len(bt["lens"]), bt["S"], 1)
            _same_bits((got[0], got[1], got[2], got[4], got[5]), (want[0], want[1], want[2], want[4], want[5]), "forward_many_lengths")
            assert torch.equal(got[3], want[3])
    finally:
        net.honour_video_lengths = False
    with pytest.raises(ValueError, match="video_lengths"):
        list(net.forward_many_lengths([(bts[0]["video"], None, None, mels[0], None, None, None, 1, {"speaker_embedding": bts[0]["emb"]})]))

    # evaluate.py's loop (train collate layout): the embedding of a batch comes from a stub tower keyed by the audio's first sample; the Gumbel noise is
    # drawn per batch, in loader order on both routes
    class Tower:
        def inference(self, audios, audio_lengths=None):
            return bts[int(audios[0, 0])]["emb"].cuda()

    loader = [((bt["video"], torch.tensor(bt["lens"])), (torch.full((len(bt["lens"]), 600), float(i)), torch.full((len(bt["lens"]),), 600)),
               (ml, torch.full((len(bt["lens"]),), bt["S"]), None), None) for i, (bt, ml) in enumerate(zip(bts, mels))]
    nm = net.native_model()
    torch.manual_seed(7)
    want = callers.evaluate_mels(net, loader, speaker_encoder=Tower(), honour_lengths=True)
    n_masked, n_ragged = nm.calls["l2s_forward_eval_masked"], nm.calls["l2s_forward_eval_ragged"]
    torch.manual_seed(7)
    got = callers.evaluate_mels(net, loader, speaker_encoder=Tower(), honour_lengths=True, group_lengths=True, group=2, n_inflight=2)
    torch.cuda.synchronize()
    assert nm.calls["l2s_forward_eval_ragged"] == n_ragged + 2 and nm.calls["l2s_forward_eval_masked"] == n_masked      # groups of two batches: [A, B] and [A]
    assert len(got) == len(want) == 3 and [tuple(t.shape) for t in got] == [(4, 80, 40), (2, 80, 23), (4, 80, 40)]
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert not net.honour_video_lengths and not net.training
    with pytest.raises(ValueError, match="honour_lengths"):
        callers.evaluate_mels(net, loader, speaker_encoder=Tower(), group_lengths=True)
