"""Option "persist_masked": the *_masked entry points on the persistent forms (pdecode.hip: the length-masked instantiations of pdecode_kernel and
pbilstm_kernel) against the masked launch route, the CPU oracle on each clip alone, the fp64 oracle at soft attention weights, and - where the code is
the same by construction - bit for bit.  `-m gpu`.

Bounds: ROUTE_TOL = 5e-4 on mel / attention is the project's persistent-versus-launch bound (test_persist_long_gpu.py), MEL_TOL =
1e-3 its parity gate, ATTN_TOL and the margins those of test_soft_attention.py / test_masked_lengths_gpu.py."""
import pytest
import torch

from lip2speech_amd import callers, native, synth
from oracle import l2s_oracle as orc
import early_stop_common as es
import parity_common as pc

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-3
ATTN_TOL = 1e-5
ROUTE_TOL = 5e-4            # persistent form against the launch path
SOFT = 1e-3                 # factor on both attention temperatures (test_soft_attention.py)
STOP_MARGIN = 1e-4
MARGIN = 1e-4               # attention argmax is compared where the oracle's top-2 margin exceeds this
ON = dict(persist_decode=8, persist_frames=80, persist_masked=1)

_models = {}


def model(sd, tag, **options):
    """A NativeModel per (checkpoint tag, options), shared by the tests of this module."""
    key = (tag, tuple(sorted(options.items())))
    if key not in _models:
        _models[key] = pc.fresh_native_model(sd, **options)
    return _models[key]


def masked_and_launch(sd, tag):
    return model(sd, tag, **ON), model(sd, tag, persist_decode=0)


def _mb(n):
    return n // 7       # l2s_min_T(len)


def padded(lens, T, tag, HW=96):
    """lens zero-padded to T (>= max(lens)): video, emb, gumbel on the host"""
    B = len(lens)
    tag = f"pm{B}_{T}_{tag}"
    video = synth.synth_video(B, T, H=HW, W=HW, tag=tag)
    for b, n in enumerate(lens):
        video[b, :, n:] = 0
    return video, synth.synth_speaker_embedding(B, tag=tag), synth.synth_gumbel(B * native.min_T(T), tag=tag)


def dev(args):
    return tuple(a.cuda() for a in args)


def check_routes(a, b, took_persistent, clear=None):
    """a: the persistent-eligible call, b: the launch path (check_routes of test_persist_long_gpu.py; lengths where the control's stop logits are clear)."""
    torch.cuda.synchronize()
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[2]).all()
    assert native.persist_timeouts() == 0
    d_mel, d_attn = pc.maxdiff(a[0], b[0]), pc.maxdiff(a[2], b[2])
    print(f"masked persistent vs masked launch: max |d mel_post| {d_mel:.3e}  max |d attn| {d_attn:.3e}")
    if took_persistent:
        assert torch.equal(a[0], b[0]) != native.persist_available()      # it did take the other route wherever the device allows it
        assert d_mel < ROUTE_TOL and d_attn < ROUTE_TOL
        la, lb = a[1].cpu(), b[1].cpu()
        if clear is None:
            assert torch.equal(la, lb)
        else:
            assert torch.equal(la[clear], lb[clear])
    else:
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])


def stop_clear(nm, args, lens, S):
    """rows of the control (launch route) whose staged stop logits all clear zero by more than STOP_MARGIN"""
    video, emb, gum = args
    B, T = video.shape[0], video.shape[2]
    vis = native.build_visual(nm.encoder_fwd(video), emb)
    state, _ = nm.decoder_prologue(vis, emb, gum, video_lengths=lens)
    _, stop, _ = nm.decode_steps(state, B, T, S, want_attn=False, video_lengths=lens)
    return (stop.abs().min(dim=1).values > STOP_MARGIN).cpu()


# ---------------------------------------------------------------------------------------------------------------- against the masked launch route
# short form with both BiLSTM directions ending mid-batch; the minimum length and the last register frame; either side of the two-frames-per-lane and
# LDS-tail boundaries and the built maximum; two launches with a short clip inside a long-padded batch; short clips under long padding (short form)
@pytest.mark.parametrize("lens,T,HW,S", [([13, 29], 29, 96, 12), ([7, 32], 32, 96, 12), ([33, 64], 64, 88, 12), ([65, 80], 80, 88, 12),
                                         ([27, 50, 62, 75], 75, 88, 12), ([20, 26], 75, 88, 12), ([40, 75], 75, 88, 300)])
def test_masked_shapes_against_launch_route(synth_sd, lens, T, HW, S):
    own, ref = masked_and_launch(synth_sd, "synth")
    args = dev(padded(lens, T, "shape", HW))
    a = own.inference(*args, S=S, want_attn=True, video_lengths=lens)
    b = ref.inference(*args, S=S, want_attn=True, video_lengths=lens)
    for row, n in enumerate(lens):
        assert not a[2][row, :, n:].any(), "attention columns past the clip's length must be exactly 0"
    check_routes(a, b, True, stop_clear(ref, args, lens, S))


# ---------------------------------------------------------------------------------------------------------------- the CPU oracle on each clip alone
ORACLE_CASES = {"short": ([7, 13, 22, 16], 22), "long": ([40, 75], 75)}
ORACLE_S = 40


@pytest.fixture(scope="module")
def oracle_cases(synth_sd):
    out = {}
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for name, (lens, T) in ORACLE_CASES.items():
        video, emb, gum = padded(lens, T, "oracle")
        m = native.min_T(T)
        ref = []
        with torch.no_grad():
            for b, n in enumerate(lens):
                ref.append(orc.inference(synth_sd, video[b:b + 1, :, :n].contiguous(), emb[b:b + 1], gum[b * m:b * m + _mb(n)], S=ORACLE_S))
        out[name] = dict(lens=lens, T=T, args=(video, emb, gum), ref=ref)
    return out


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_each_clip_matches_the_oracle_alone(synth_sd, oracle_cases, name):
    c = oracle_cases[name]
    own, _ = masked_and_launch(synth_sd, "synth")
    mel, lengths, attn = (t.cpu() for t in own.inference(*dev(c["args"]), S=ORACLE_S, want_attn=True, video_lengths=c["lens"]))
    assert native.persist_timeouts() == 0
    for b, n in enumerate(c["lens"]):
        r_mel, r_len, r_attn = c["ref"][b]
        d = pc.maxdiff(mel[b], r_mel[0])
        print(f"{name}: clip {b} ({n} frames) max |mel_post - solo oracle| = {d:.3e}")
        assert d < MEL_TOL
        assert int(lengths[b]) == int(r_len[0])
        assert not attn[b, :, n:].any(), "attention columns past the clip's length must be exactly 0"
        assert pc.maxdiff(attn[b, :, :n].sum(dim=-1), torch.ones(ORACLE_S)) < 1e-5
        arg, margin = pc.top2(r_attn[0])
        sure = margin > MARGIN
        assert torch.equal(attn[b, :, :n].argmax(dim=-1).to(torch.int32)[sure], arg[sure])


# ---------------------------------------------------------------------------------------------------------------- soft weights, fp64 oracle per clip
def soft_state_dict(sd):
    out = dict(sd)
    out["decoder.temperature"] = sd["decoder.temperature"] * SOFT
    out["decoder.content.temperature"] = sd["decoder.content.temperature"] * SOFT
    return out


def decoder_oracle(sd, feat, emb, gum, S):
    """fp64 oracle of prologue -> S-step loop -> post-net from the given encoder features (the method of test_soft_attention.py)."""
    sd64 = orc.to_dtype(sd, torch.float64)
    emb64 = emb.double()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        st = orc.decoder_prologue(sd64, orc.build_visual(feat.double(), emb64), emb64, gum.double())
        al = []
        mel, stop, logits = orc.decode_loop(sd64, st, S, return_logits=True, alphas=al)
        mel_cf = mel.permute(0, 2, 1)
        post = orc.postnet(sd64, mel_cf) + mel_cf
    return dict(post=post, stop=stop, attn=torch.softmax(logits, dim=-1), alpha=torch.stack(al, dim=1))


_soft_refs = {}


def soft_ref(sd, own, n, tag):
    """the n-frame clip `tag` alone: its video, embedding, Gumbel rows, and the fp64 oracle from the GPU encoder's features of the clip alone"""
    if (n, tag) not in _soft_refs:
        S = 40
        v = synth.synth_video(1, n, H=88, W=88, tag=f"pmsoft{n}_{tag}")
        e = synth.synth_speaker_embedding(1, tag=f"pmsoft{n}_{tag}")
        g = synth.synth_gumbel(_mb(n), tag=f"pmsoft{n}_{tag}")
        feat = own.encoder_fwd(v.cuda())
        _soft_refs[(n, tag)] = (v, e, g, decoder_oracle(sd, feat.cpu(), e, g, S))
    return _soft_refs[(n, tag)]


@pytest.mark.parametrize("lens,T", [([32, 33], 33), ([64, 65], 65), ([64, 65], 80)])
def test_soft_weights_match_the_oracle_per_clip(synth_sd, lens, T):
    """One-hot attention would hide a dropped or misplaced frame at a length boundary: at soft weights every frame's and every slot's weight is compared."""
    S = 40
    sd = soft_state_dict(synth_sd)
    own, _ = masked_and_launch(sd, "soft")
    clips = [soft_ref(sd, own, n, "a") for n in lens]
    B, m = len(lens), native.min_T(T)
    video = torch.zeros(B, 3, T, 88, 88)
    gum = synth.synth_gumbel(B * m, tag="pmsoft-fill")          # the rows past a clip's slots are never used
    for b, (n, (v, e, g, _)) in enumerate(zip(lens, clips)):
        video[b, :, :n] = v[0]
        gum[b * m:b * m + _mb(n)] = g
    emb = torch.cat([c[1] for c in clips])
    mel_post, lengths, attn = own.inference(video.cuda(), emb.cuda(), gum.cuda(), S=S, want_attn=True, video_lengths=lens)
    torch.cuda.synchronize()
    assert native.persist_timeouts() == 0
    for b, n in enumerate(lens):
        ref = clips[b][3]
        assert ref["attn"].max().item() < 0.5, f"attention is not soft: max weight {ref['attn'].max().item():.3f}"
        if ref["alpha"].shape[-1] > 1:
            assert ref["alpha"].max().item() < 0.5
        d_mel, d_attn = pc.maxdiff(mel_post[b], ref["post"][0]), pc.maxdiff(attn[b, :, :n], ref["attn"][0])
        print(f"soft {lens} padded to {T}: clip {b} max |d mel_post| {d_mel:.3e}  max |d attn| {d_attn:.3e}")
        assert d_mel < MEL_TOL
        assert d_attn < ATTN_TOL
        assert not attn[b, :, n:].any()
        if bool((ref["stop"][0].abs().min() > STOP_MARGIN)):
            assert int(lengths[b]) == int(orc.output_lengths_from_stop(ref["stop"], S)[0])


# ---------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("T", [14, 40])
def test_all_lengths_equal_T_is_the_unmasked_persistent_call(synth_sd, T):
    own, _ = masked_and_launch(synth_sd, "synth")
    args = dev(padded([T, T], T, "full", 88))
    plain = own.inference(*args, S=20, want_attn=True)
    masked = own.inference(*args, S=20, want_attn=True, video_lengths=[T, T])
    torch.cuda.synchronize()
    assert native.persist_timeouts() == 0
    assert all(torch.equal(a, b) for a, b in zip(plain, masked))


def test_row_bits_do_not_depend_on_partner_or_padding(synth_sd):
    """The 13-frame clip as row 0 of [13, 9] padded to 13 and as row 0 of [13, 29] padded to 29: two clips, the short form both times.  Against the solo
    persistent call only the route bound is required (the BiLSTM's one-clip instantiation splits the gate columns differently): printed."""
    S = 40
    own, _ = masked_and_launch(synth_sd, "synth")
    v13, e13, g13 = padded([13], 13, "inv")
    (v9, e9, g9), (v29, e29, g29) = padded([9], 9, "inv"), padded([29], 29, "inv")
    m29 = native.min_T(29)
    pa_v = torch.cat([v13, torch.cat([v9, torch.zeros(1, 3, 4, 96, 96)], dim=2)])
    pa_g = torch.cat([g13, g9])                                                  # min_T(13) = 1 row per clip
    pb_v = torch.cat([torch.cat([v13, torch.zeros(1, 3, 16, 96, 96)], dim=2), v29])
    pb_g = torch.cat([g13, synth.synth_gumbel(m29 - 1, tag="pm-inv-fill"), g29])
    a = own.inference(pa_v.cuda(), torch.cat([e13, e9]).cuda(), pa_g.cuda(), S=S, want_attn=True, video_lengths=[13, 9])
    b = own.inference(pb_v.cuda(), torch.cat([e13, e29]).cuda(), pb_g.cuda(), S=S, want_attn=True, video_lengths=[13, 29])
    solo = own.inference(v13.cuda(), e13.cuda(), g13.cuda(), S=S, want_attn=True)
    torch.cuda.synchronize()
    assert native.persist_timeouts() == 0
    d_solo = pc.maxdiff(a[0][0], solo[0][0])
    print(f"row 0 of [13, 9] against [13, 29]: max |d mel_post| {pc.maxdiff(a[0][0], b[0][0]):.3e}; against the solo persistent call: {d_solo:.3e}")
    assert torch.equal(a[0][0], b[0][0]) and int(a[1][0]) == int(b[1][0])
    assert torch.equal(a[2][0, :, :13], b[2][0, :, :13])
    assert d_solo < ROUTE_TOL and pc.maxdiff(a[2][0, :, :13], solo[2][0]) < ROUTE_TOL


# ---------------------------------------------------------------------------------------------------------------- the staged route
def test_staged_route_gives_the_bits_of_inference(synth_sd):
    lens, T, S = [13, 29], 29, 40
    own, ref = masked_and_launch(synth_sd, "synth")
    video, emb, gum = dev(padded(lens, T, "staged"))
    one = own.inference(video, emb, gum, S=S, want_attn=True, video_lengths=lens)
    vis = native.build_visual(own.encoder_fwd(video), emb)
    state, _ = own.decoder_prologue(vis, emb, gum, video_lengths=lens)
    mel, stop, attn = own.decode_steps(state, len(lens), T, S, want_attn=True, video_lengths=lens)
    mel_post, _ = own.postnet(mel)
    lengths = native.output_lengths(stop)
    torch.cuda.synchronize()
    assert native.persist_timeouts() == 0
    assert torch.equal(mel_post, one[0]) and torch.equal(lengths, one[1]) and torch.equal(attn, one[2])
    launch = ref.inference(video, emb, gum, S=S, want_attn=True, video_lengths=lens)
    assert torch.equal(one[0], launch[0]) != native.persist_available()


# ---------------------------------------------------------------------------------------------------------------- the prologue's persistent BiLSTM
@pytest.mark.parametrize("lens,T", [([13, 29], 29), ([40, 75], 75)])
def test_persistent_masked_bilstm(synth_sd, lens, T):
    """The state against the masked launch-route prologue, within the bounds of test_persist_long_gpu.py::test_persistent_bilstm_on_long_clips; enc rows
    past a clip exactly 0; other bits than the launch route wherever the persistent forms are available."""
    B = len(lens)
    own, ref = masked_and_launch(synth_sd, "synth")
    v, e, g = dev(padded(lens, T, "pro", 88))
    m = native.min_T(T)
    vis = native.build_visual(ref.encoder_fwd(v), e)
    sa, _ = own.decoder_prologue(vis, e, g, video_lengths=lens)
    sb, _ = ref.decoder_prologue(vis, e, g, video_lengths=lens)
    torch.cuda.synchronize()
    assert native.persist_timeouts() == 0
    fa = lambda f, shape: native.state_field(sa, B, T, f, shape)      # noqa: E731
    fb = lambda f, shape: native.state_field(sb, B, T, f, shape)      # noqa: E731
    enc_a, enc_b = fa(native.ST_ENC, (B, T, 512)), fb(native.ST_ENC, (B, T, 512))
    assert torch.equal(enc_a, enc_b) != native.persist_available()
    assert pc.maxdiff(enc_a, enc_b) < 2e-5
    ka, kb, va, vb = fa(native.ST_K, (B, T, 512)), fb(native.ST_K, (B, T, 512)), fa(native.ST_V, (B, T, 512)), fb(native.ST_V, (B, T, 512))
    cka, ckb, cva, cvb = fa(native.ST_CKEY, (B, m, 256)), fb(native.ST_CKEY, (B, m, 256)), fa(native.ST_CVAL, (B, m, 256)), fb(native.ST_CVAL, (B, m, 256))
    for b, n in enumerate(lens):
        assert not enc_a[b, n:].any(), "enc rows past the clip must be exactly 0"
        assert pc.maxdiff(ka[b, :n], kb[b, :n]) < 5e-5 and pc.maxdiff(va[b, :n], vb[b, :n]) < 5e-5
        assert pc.maxdiff(cka[b, :_mb(n)], ckb[b, :_mb(n)]) < 2e-5
        assert pc.maxdiff(cva[b], cvb[b]) < 1e-4 and not cva[b, _mb(n):].any()
    assert pc.maxdiff(fa(native.ST_ECELL, (B, 512)), fb(native.ST_ECELL, (B, 512))) < 2e-5
    ha, hb = fa(native.ST_H, (2, 16 * 512)), fb(native.ST_H, (2, 16 * 512))
    for layer in range(2):
        assert pc.maxdiff(pc.unfrag(ha[layer], B, 512), pc.unfrag(hb[layer], B, 512)) < 2e-5


# ---------------------------------------------------------------------------------------------------------------- early_stop composes
def test_early_stop_composes(synth_sd):
    """A stop bias under which every clip stops inside S (the shift of test_masked_lengths_gpu.py::test_early_stop_composes, from the control's stop
    logits - they do not feed back): "early_stop" on against off, both masked persistent - the same lengths, kept frames within ROUTE_TOL (the ES forms
    are another instantiation), dropped frames and attention rows exact zeros."""
    lens, T, S = [27, 50, 62, 75], 75, 60
    _, ref = masked_and_launch(synth_sd, "synth")
    args = dev(padded(lens, T, "es", 88))
    video, emb, gum = args
    vis = native.build_visual(ref.encoder_fwd(video), emb)
    state, _ = ref.decoder_prologue(vis, emb, gum, video_lengths=lens)
    _, stop, _ = ref.decode_steps(state, len(lens), T, S, want_attn=False, video_lengths=lens)
    shift = -float(stop.cpu()[:, :25].max(dim=1).values.min()) + 1e-2      # every clip now crosses within 25 steps
    sd = dict(synth_sd)
    sd["decoder.stop_token_layer.linear_layer.bias"] = sd["decoder.stop_token_layer.linear_layer.bias"] + shift
    own = pc.fresh_native_model(sd, **ON)
    off = [t.clone() for t in own.inference(*args, S=S, want_attn=True, video_lengths=lens)]
    own.set_option("early_stop", 1)
    on = [t.clone() for t in own.inference(*args, S=S, want_attn=True, video_lengths=lens)]
    torch.cuda.synchronize()
    assert native.persist_timeouts() == 0
    out = off[1].cpu()
    print("early stop on the masked persistent route: output lengths", out.tolist())
    assert int(out.max()) < S and torch.equal(on[1].cpu(), out)
    keep = torch.arange(S)[None, :] < out[:, None]
    assert not on[0].cpu()[~keep[:, None, :].expand_as(on[0])].any() and not on[2].cpu()[~keep].any()
    assert pc.maxdiff(on[0].cpu(), es.masked_mel(off[0], out)) < ROUTE_TOL
    assert pc.maxdiff(on[2].cpu(), es.masked_attn(off[2], out)) < ROUTE_TOL
    for b, n in enumerate(lens):
        assert not on[2][b, :, n:].any()


# ---------------------------------------------------------------------------------------------------------------- outside the envelope
def test_outside_the_envelope_is_the_launch_route(synth_sd):
    S = 9
    _, ref = masked_and_launch(synth_sd, "synth")
    # the option set to 0 explicitly
    off = model(synth_sd, "synth", persist_decode=8, persist_frames=80, persist_masked=0)
    lens = [13, 29]
    args = dev(padded(lens, 29, "out", 88))
    check_routes(off.inference(*args, S=S, want_attn=True, video_lengths=lens), ref.inference(*args, S=S, want_attn=True, video_lengths=lens), False)
    own = model(synth_sd, "synth", persist_decode=8, persist_frames=300, persist_masked=1)
    # padded T past the built maximum, although both clips are short
    lens = [13, 29]
    args = dev(padded(lens, 81, "out", 88))
    check_routes(own.inference(*args, S=S, want_attn=True, video_lengths=lens), ref.inference(*args, S=S, want_attn=True, video_lengths=lens), False)
    # five clips
    lens = [13, 29, 7, 22, 16]
    args = dev(padded(lens, 29, "out5", 88))
    check_routes(own.inference(*args, S=S, want_attn=True, video_lengths=lens), ref.inference(*args, S=S, want_attn=True, video_lengths=lens), False)


def test_teacher_forced_masked_calls_keep_the_launch_route(synth_sd):
    lens, T, S = [13, 29], 29, 12
    own, ref = masked_and_launch(synth_sd, "synth")
    video, emb, gum = dev(padded(lens, T, "tf", 88))
    mels = synth.synth_mels(2, S, tag="pm-tf")
    bos = synth_sd["decoder.BOS"].view(1, 1, -1).expand(2, -1, -1)
    teacher = torch.cat([bos, mels.permute(0, 2, 1)], dim=1)[:, :S].contiguous().cuda()
    tmask = [i % 2 for i in range(S)]
    a = own.forward_eval(video, emb, gum, S, teacher=teacher, teacher_mask=tmask, video_lengths=torch.tensor(lens))
    b = ref.forward_eval(video, emb, gum, S, teacher=teacher, teacher_mask=tmask, video_lengths=torch.tensor(lens))
    torch.cuda.synchronize()
    assert native.persist_timeouts() == 0
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the staged loop with teacher frames, from one (launch-route) state
    vis = native.build_visual(ref.encoder_fwd(video), emb)
    state, _ = ref.decoder_prologue(vis, emb, gum, video_lengths=lens)
    sa = own.decode_steps(state.clone(), 2, T, S, teacher=teacher, teacher_mask=tmask, want_attn=True, video_lengths=lens)
    sb = ref.decode_steps(state.clone(), 2, T, S, teacher=teacher, teacher_mask=tmask, want_attn=True, video_lengths=lens)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(sa, sb))


# ---------------------------------------------------------------------------------------------------------------- callers
def test_demo_clip_keyword(synth_sd):
    """demo_clip(..., honour_lengths=True, persist_masked=1) returns what net.inference(video_lengths=) returns with the option set, and leaves the
    option alone when the keyword is 0."""
    from model.model import get_network
    lens, T = [13, 29], 29
    video, emb, _ = padded(lens, T, "demo")
    vlen = torch.tensor(lens)
    batch = ((video, vlen), (None, None), None, None, None)
    net = get_network("test").cuda()
    net.load_state_dict(synth_sd, strict=True)
    nm = net.native_model()
    nm.set_option("persist_decode", 8)       # the suite pins 0 (tests/conftest.py); a run-time switch, read per call
    calls = []
    real = nm.set_option
    nm.set_option = lambda name, value: (calls.append((name, value)), real(name, value))[1]
    try:
        torch.manual_seed(7)
        m0, l0, a0 = callers.demo_clip(net, batch, speaker_embedding=emb.cuda(), honour_lengths=True)
        assert not [c for c in calls if c[0] == "persist_masked"], "keyword 0 must leave the option alone"
        torch.manual_seed(7)
        m1, l1, a1 = callers.demo_clip(net, batch, speaker_embedding=emb.cuda(), honour_lengths=True, persist_masked=1)
        assert ("persist_masked", 1) in calls
        torch.manual_seed(7)
        with torch.no_grad():
            mel, lengths, attn = net.inference(video.cuda(), None, speaker_embedding=emb.cuda(), return_attention_map=True, video_lengths=vlen)
    finally:
        nm.set_option = real
    torch.cuda.synchronize()
    assert native.persist_timeouts() == 0
    n = int(lengths[0])
    assert torch.equal(l1, lengths) and torch.equal(m1, mel[:1, :, :n]) and torch.equal(a1, attn[:, :n])
    assert torch.equal(m0, m1) != native.persist_available()      # the keyword moved the call onto the persistent route
