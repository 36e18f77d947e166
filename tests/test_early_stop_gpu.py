"""Option "early_stop" on the GPU (include/l2s.h): the decode loop ends on the device once every clip of the call has stopped, and what comes back is
the reference's output masked by the reference's own lengths.  Cases are sub-batches of the committed reference goldens (rows of a batch are
independent; the reference's own batch-of-1 against batch-of-4 spread is 6.8e-5, far inside MEL_TOL)."""
import pytest
import torch

import early_stop_common as es
from lip2speech_amd import native, synth

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-3          # the project's gate against the reference goldens (tests/test_gpu_parity.py)
ROUTE_TOL = 5e-4        # persistent against launch-per-phase loop: another order of the same fp32 sums (test_persistent_decode_*)
S = 300


def _stop_sd(synth_sd, g):
    sd = dict(synth_sd)
    sd["decoder.stop_token_layer.linear_layer.weight"] = g["stop_weight"]
    sd["decoder.stop_token_layer.linear_layer.bias"] = g["stop_bias"]
    return sd


@pytest.fixture(scope="module")
def b32(synth_sd):
    import parity_common as pc
    g = pc.golden("stop_lrw_b32.npz")
    return {"g": g, "mel": pc.golden("inference_lrw_b32_full_mel.npz")["mel_post"], "sd": _stop_sd(synth_sd, g),
            "video": synth.synth_video(32, 29, tag="bench"), "emb": synth.synth_speaker_embedding(32, tag="bench")}


@pytest.fixture(scope="module")
def b2(synth_sd):
    import parity_common as pc
    g = pc.golden("stop_lrw_b2.npz")
    return {"g": g, "mel": pc.golden("inference_lrw_b2.npz")["mel_post"], "sd": _stop_sd(synth_sd, g),
            "video": synth.synth_video(2, 29, tag="video-lrw2"), "emb": synth.synth_speaker_embedding(2, tag="spk-lrw2")}


@pytest.fixture(scope="module")
def launch32(b32):
    import parity_common as pc
    return pc.fresh_native_model(b32["sd"], persist_decode=0)


@pytest.fixture(scope="module")
def persist32(b32):
    import parity_common as pc
    return pc.fresh_native_model(b32["sd"], persist_decode=8)


def _args(case, idx):
    return (case["video"][idx].cuda(), case["emb"][idx].cuda(), es.gumbel_rows(case["g"]["gumbel"], idx).cuda())


def _both(model, fn):
    """fn() with the option off, then on; the option is left off."""
    model.set_option("early_stop", 0)
    off = [t.clone() if t is not None else None for t in fn()]
    model.set_option("early_stop", 1)
    try:
        on = [t.clone() if t is not None else None for t in fn()]
    finally:
        model.set_option("early_stop", 0)
    torch.cuda.synchronize()
    return off, on


def _check_masked(on, off, lens, ref_mel=None, ref_attn=None, same_route_bits=True):
    mel_on, len_on, attn_on = on
    assert len_on.dtype == torch.int64 and torch.equal(len_on.cpu(), lens) and torch.equal(off[1].cpu(), lens)
    assert mel_on.shape == off[0].shape and attn_on.shape == off[2].shape
    want_mel, want_attn = es.masked_mel(off[0], lens), es.masked_attn(off[2], lens)
    keep = torch.arange(mel_on.shape[2])[None, :] < lens[:, None]
    assert not mel_on.cpu()[~keep[:, None, :].expand_as(mel_on)].any() and not attn_on.cpu()[~keep].any()      # dropped frames: exactly 0
    if same_route_bits:
        assert torch.equal(mel_on.cpu(), want_mel) and torch.equal(attn_on.cpu(), want_attn)                     # kept frames: the off call's bits
    if ref_mel is not None:
        d = (mel_on.cpu().double() - es.masked_mel(ref_mel, lens).double()).abs().max().item()
        print("early stop: max |mel - masked golden| =", d)
        assert d < MEL_TOL
    if ref_attn is not None:
        assert (attn_on.cpu().double() - es.masked_attn(ref_attn, lens).double()).abs().max().item() < MEL_TOL


@pytest.mark.parametrize("max_len,n_clips,E", es.SUB_BATCHES)
def test_launch_route_every_element(b32, launch32, max_len, n_clips, E):
    """Sub-batches of the B = 32 golden through l2s_inference and, as members 0 and 2 of a group, l2s_inference_multi: lengths equal the
    golden's, every kept frame is the golden's within MEL_TOL and BIT-identical to the option-off call on the same inputs (the post-net keeps
    its tiling: it still runs over all S frames), every dropped frame is exactly 0."""
    lens_all = b32["g"]["output_lengths"]
    idx = es.rows_upto(lens_all, max_len)
    assert len(idx) == n_clips and es.end_step(lens_all[idx], S) == E
    lens = lens_all[idx]
    args = _args(b32, idx)
    off, on = _both(launch32, lambda: launch32.inference(*args, S=S, want_attn=True))
    _check_masked(on, off, lens, ref_mel=b32["mel"][idx])
    other = (synth.synth_video(n_clips, 29, tag="grp1").cuda(), synth.synth_speaker_embedding(n_clips, tag="grp1").cuda(),
             synth.synth_gumbel(n_clips * 4, tag="grp1").cuda())
    goff, gon = _both(launch32, lambda: [t for member in launch32.inference_multi([args, other, args], S=S, want_attn=True) for t in member])
    for k in (0, 2):
        _check_masked(gon[3 * k:3 * k + 3], goff[3 * k:3 * k + 3], lens, ref_mel=b32["mel"][idx])
        assert torch.equal(gon[3 * k], on[0])
    _check_masked(gon[3:6], goff[3:6], goff[4].cpu())


@pytest.mark.parametrize("fold", [1, 0])
def test_loop_really_stopped(b32, fold):
    """The staged l2s_decode_steps on the 22-clip sub-batch (lengths 13 .. 27, E = 37), folded and literal step: steps < len_b + 10 carry the off
    call's bits, steps >= 37 are exactly 0 - the loop did stop - and the steps [27, 37) were computed."""
    import parity_common as pc
    lens_all = b32["g"]["output_lengths"]
    idx = es.rows_upto(lens_all, 27)
    lens = lens_all[idx]
    E = es.end_step(lens, S)
    assert E == 37
    m = pc.fresh_native_model(b32["sd"], persist_decode=0, fold_step_weights=fold)
    video, emb, gum = _args(b32, idx)
    state, _ = m.decoder_prologue(native.build_visual(m.encoder_fwd(video), emb), emb, gum)
    off, on = _both(m, lambda: m.decode_steps(state, len(idx), 29, S, want_attn=True))
    for b in range(len(idx)):
        n = int(lens[b]) + es.MARGIN
        for t_on, t_off in zip(on, off):
            assert torch.equal(t_on[b, :n], t_off[b, :n])
    for t_on, t_off in zip(on, off):
        assert not t_on[:, E:].any() and t_off[:, E:].any()
    assert on[0][:, 27:E].any() and on[1][:, 27:E].any()
    assert torch.equal(on[1][:, :E], off[1][:, :E])          # launch route: the batch runs until its last clip ends


def _need_persist():
    if not native.persist_available():
        pytest.skip("l2s_persist_available() is 0 on this device: the persistent decode loop cannot be taken")


def _persist_case(model, launch_model, args, lens, ref_mel=None, ref_attn=None, steps=S):
    assert native.persist_available()
    fn = lambda: model.inference(*args, S=steps, want_attn=True)      # noqa: E731
    off, on = _both(model, fn)
    _check_masked(on, off, lens, ref_mel=ref_mel, ref_attn=ref_attn)
    launch_model.set_option("early_stop", 0)
    ref = launch_model.inference(*args, S=steps, want_attn=True)
    assert not torch.equal(off[0], ref[0])                           # it did take the persistent route
    assert (on[0].cpu() - es.masked_mel(ref[0], lens)).abs().max().item() < ROUTE_TOL
    assert (on[2].cpu() - es.masked_attn(ref[2], lens)).abs().max().item() < ROUTE_TOL
    # staged: each clip leaves on its own - steps >= E_b exactly 0 per clip, steps < E_b the off call's bits; a second call gives the same bits
    B = args[0].shape[0]
    state, _ = model.decoder_prologue(native.build_visual(model.encoder_fwd(args[0]), args[1]), args[1], args[2])
    soff, son = _both(model, lambda: model.decode_steps(state, B, args[0].shape[2], steps, want_attn=True))
    model.set_option("early_stop", 1)
    try:
        again = [t.clone() for t in model.decode_steps(state, B, args[0].shape[2], steps, want_attn=True)]
    finally:
        model.set_option("early_stop", 0)
    for b in range(B):
        Eb = min(steps, int(lens[b]) + es.MARGIN)
        for t_on, t_off, t_again in zip(son, soff, again):
            assert torch.equal(t_on[b, :Eb], t_off[b, :Eb]) and not t_on[b, Eb:].any() and torch.equal(t_on[b], t_again[b])
    torch.cuda.synchronize()
    assert native.persist_timeouts() == 0


def test_persistent_one_clip_183(b2, synth_sd):
    import parity_common as pc
    _need_persist()
    g = b2["g"]
    b = g["output_lengths"].tolist().index(183)
    own = pc.fresh_native_model(b2["sd"], persist_decode=8)
    ref = pc.fresh_native_model(b2["sd"], persist_decode=0)
    _persist_case(own, ref, _args(b2, [b]), g["output_lengths"][[b]], ref_mel=b2["mel"][[b]], ref_attn=g["attn"][[b]])


def test_persistent_never_stops_pair(b2):
    """The B = 2 golden pair (183, 300): the clip that never stops runs to S untouched, the other leaves at 193."""
    import parity_common as pc
    _need_persist()
    g = b2["g"]
    own = pc.fresh_native_model(b2["sd"], persist_decode=8)
    ref = pc.fresh_native_model(b2["sd"], persist_decode=0)
    _persist_case(own, ref, _args(b2, [0, 1]), g["output_lengths"], ref_mel=b2["mel"], ref_attn=g["attn"])


@pytest.mark.parametrize("pick,steps", [((13, 220), S), ((13, 220, 14), S), ((13, 220, 14, 300), S), ((13, 220), 100)])
def test_persistent_clips_of_the_b32_golden(b32, launch32, persist32, pick, steps):
    """Two clips of lengths 13 and 220 in ONE persistent launch (they end independently), three and four clips (two launches), and S = 100 with one
    crossing inside S and one outside."""
    _need_persist()
    lens_all = b32["g"]["output_lengths"].tolist()
    idx = [lens_all.index(n) for n in pick]
    lens = torch.tensor([min(n, steps) for n in pick], dtype=torch.int64)
    ref_mel = b32["mel"][idx] if steps == S else None
    _persist_case(persist32, launch32, _args(b32, idx), lens, ref_mel=ref_mel, steps=steps)


def test_persistent_32_frames(b32, launch32, persist32):
    """T = 32, the longest clip a persistent workgroup holds: synthetic clips, against the option-off call on both routes."""
    _need_persist()
    args = (synth.synth_video(2, 32, H=88, W=88, tag="es32").cuda(), synth.synth_speaker_embedding(2, tag="es32").cuda(),
            synth.synth_gumbel(2 * native.min_T(32), tag="es32").cuda())
    launch32.set_option("early_stop", 0)
    lens = launch32.inference(*args, S=S)[1].cpu()
    _persist_case(persist32, launch32, args, lens)


def test_never_stops_on_the_launch_route(b2):
    """The B = 2 golden pair (183, 300) on the launch route: the loop runs to S, the result is the option-off result masked, and no frame of the
    300-length clip is touched."""
    import parity_common as pc
    m = pc.fresh_native_model(b2["sd"], persist_decode=0)
    g = b2["g"]
    off, on = _both(m, lambda: m.inference(*_args(b2, [0, 1]), S=S, want_attn=True))
    _check_masked(on, off, g["output_lengths"], ref_mel=b2["mel"], ref_attn=g["attn"])
    b = g["output_lengths"].tolist().index(300)
    assert torch.equal(on[0][b], off[0][b]) and torch.equal(on[2][b], off[2][b])


def test_ignored_where_it_does_not_apply(b32, launch32):
    """l2s_forward_eval and teacher-forced l2s_decode_steps take their S from the target: bit-identical with the option on."""
    idx = es.rows_upto(b32["g"]["output_lengths"], 27)[:4]
    video, emb, gum = _args(b32, idx)
    off, on = _both(launch32, lambda: [t for t in launch32.forward_eval(video, emb, gum, 60) if torch.is_tensor(t)])
    assert len(on) >= 3 and all(torch.equal(a, b) for a, b in zip(on, off))
    state, _ = launch32.decoder_prologue(native.build_visual(launch32.encoder_fwd(video), emb), emb, gum)
    teacher = torch.randn(4, 60, 80, generator=torch.Generator().manual_seed(5)).cuda()
    mask = [1 if i % 3 == 1 else 0 for i in range(60)]
    off, on = _both(launch32, lambda: launch32.decode_steps(state, 4, 29, 60, teacher=teacher, teacher_mask=mask, want_attn=True))
    assert all(torch.equal(a, b) for a, b in zip(on, off)) and on[0][:, 40:].any()


def test_option_off_is_untouched_by_a_toggle(b32, launch32):
    idx = es.rows_upto(b32["g"]["output_lengths"], 27)
    args = _args(b32, idx)
    launch32.set_option("early_stop", 0)
    before = [t.clone() for t in launch32.inference(*args, S=S, want_attn=True)]
    off, on = _both(launch32, lambda: launch32.inference(*args, S=S, want_attn=True))
    assert all(torch.equal(a, b) for a, b in zip(before, off))
    assert before[0][:, :, 40:].any() and not on[0][:, :, 40:].any()
