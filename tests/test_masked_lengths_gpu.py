"""Per-clip video lengths on the GPU (include/l2s.h "per-clip video lengths"): row b of a zero-padded batch through the *_masked entry points is what
clip b gives ALONE at T = len_b.  Synthetic weights; clips of 7, 13, 22 and 16 frames padded to 22 (content slots m_b = 1, 1, 3, 2 of m = 3): the minimum
length, a full-length row, and rows that start and end mid-batch in both BiLSTM directions.  The reference per clip is the CPU oracle on the clip alone,
computed once per module."""
import ctypes

import pytest
import torch

import parity_common as pc
from lip2speech_amd import native, synth
from oracle import l2s_oracle as orc

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-3          # the project's parity gate
MARGIN = 1e-4           # attention argmax is compared where the oracle's top-2 margin exceeds this
LENS = [7, 13, 22, 16]
T = 22
S = 40


def _mb(n):
    return n // 7       # l2s_min_T(len): the stride-7 branch of Content.agg (checked against the library in the host test)


def _solo(case, b):
    """clip b alone: (video (1,3,len,H,W), emb (1,256), its first m_b Gumbel rows)"""
    n, m = case["lens"][b], case["m"]
    return case["video"][b:b + 1, :, :n].contiguous(), case["emb"][b:b + 1], case["gumbel"][b * m:b * m + _mb(n)]


@pytest.fixture(scope="module")
def case(synth_sd):
    B, m = len(LENS), native.min_T(T)
    c = {"lens": LENS, "m": m, "sd": synth_sd,
         "video": synth.synth_padded_video(B, LENS, tag="masked"), "emb": synth.synth_speaker_embedding(B, tag="masked"),
         "gumbel": synth.synth_gumbel(B * m, tag="masked"), "mels": synth.synth_mels(B, S, tag="masked")}
    assert c["video"].shape[2] == T and not c["video"][0, :, 7:].any()
    c["tmask"] = [i % 2 for i in range(S)]
    ref_inf, ref_fwd, ref_stop = [], [], []
    with torch.no_grad():
        for b in range(B):
            v, e, g = _solo(c, b)
            taps = {}
            ref_inf.append(orc.inference(synth_sd, v, e, g, S=S, taps=taps))
            ref_stop.append(taps["stop"])
            ref_fwd.append(orc.forward_eval(synth_sd, v, e, c["mels"][b:b + 1], g, teacher_mask=torch.tensor(c["tmask"], dtype=torch.bool)))
    c["ref_inf"], c["ref_fwd"], c["ref_stop"] = ref_inf, ref_fwd, torch.cat(ref_stop)      # ref_stop (B,S): the solo stop logits
    return c


def _teacher(sd, mels):
    """cat(BOS, mels)[:, :S] channel-last: what the native entry points take as teacher frames"""
    B, _, s = mels.shape
    bos = sd["decoder.BOS"].view(1, 1, -1).expand(B, -1, -1)
    return torch.cat([bos, mels.permute(0, 2, 1)], dim=1)[:, :s].contiguous()


def _dev(case):
    return case["video"].cuda(), case["emb"].cuda(), case["gumbel"].cuda()


def _check_inference(case, out, tag):
    """row b of a masked inference against the oracle on clip b alone"""
    mel, lengths, attn = (t.cpu() for t in out)
    for b, n in enumerate(case["lens"]):
        r_mel, r_len, r_attn = case["ref_inf"][b]
        d = pc.maxdiff(mel[b], r_mel[0])
        print(f"{tag}: clip {b} ({n} frames) max |mel_post - solo oracle| = {d:.3e}")
        assert d < MEL_TOL
        assert int(lengths[b]) == int(r_len[0])
        assert not attn[b, :, n:].any(), "attention columns past the clip's length must be exactly 0"
        arg, margin = pc.top2(r_attn[0])
        sure = margin > MARGIN
        assert torch.equal(attn[b, :, :n].argmax(dim=-1).to(torch.int32)[sure], arg[sure])
        assert pc.maxdiff(attn[b, :, :n].sum(dim=-1), torch.ones(S)) < 1e-5


def test_inference_masked_matches_each_clip_alone(case):
    nm = pc.native_model(case["sd"])
    out = nm.inference(*_dev(case), S=S, want_attn=True, video_lengths=case["lens"])
    torch.cuda.synchronize()
    assert nm.calls["l2s_inference_masked"] >= 1
    _check_inference(case, out, "inference_masked")


def test_forward_eval_masked_matches_each_clip_alone(case):
    """teacher frames on an alternating mask: pre- and post-net mel, stop logits, attention logits (-inf past the clip), content_dis rows < m_b
    (the others exactly 0)"""
    nm = pc.native_model(case["sd"])
    teacher = _teacher(case["sd"], case["mels"]).cuda()
    mel_cf, mel_post, stop, logits, dis = (t.cpu() for t in nm.forward_eval(*_dev(case), S, teacher=teacher, teacher_mask=case["tmask"],
                                                                            video_lengths=torch.tensor(case["lens"])))
    m = case["m"]
    for b, n in enumerate(case["lens"]):
        r = case["ref_fwd"][b]
        d = [pc.maxdiff(mel_cf[b], r[0][0]), pc.maxdiff(mel_post[b], r[1][0]), pc.maxdiff(stop[b], r[2][0, :, 0]),
             pc.maxdiff(dis[b * m:b * m + _mb(n)], r[5])]
        print(f"forward_eval_masked: clip {b} ({n} frames) max |d| mel {d[0]:.3e} mel_post {d[1]:.3e} stop {d[2]:.3e} content_dis {d[3]:.3e}")
        assert max(d) < MEL_TOL
        assert not dis[b * m + _mb(n):(b + 1) * m].any(), "content_dis rows past the clip's slots must be exactly 0"
        assert torch.isneginf(logits[b, :, n:]).all() and torch.isfinite(logits[b, :, :n]).all()
        ref_a = torch.softmax(r[4][0], dim=-1)
        arg, margin = pc.top2(ref_a)
        sure = margin > MARGIN
        a = torch.softmax(logits[b], dim=-1)
        assert not a[:, n:].any()
        assert torch.equal(a[:, :n].argmax(dim=-1).to(torch.int32)[sure], arg[sure])


def test_inputs_discriminate(case):
    """The same padded batch through the UNMASKED l2s_inference: the three short clips come out as other utterances (far outside the gate), the
    full-length one as itself - padding disturbs these inputs, so the masked checks above are not vacuous."""
    nm = pc.native_model(case["sd"])
    mel = nm.inference(*_dev(case), S=S)[0].cpu()
    for b, n in enumerate(case["lens"]):
        d = pc.maxdiff(mel[b], case["ref_inf"][b][0][0])
        print(f"unmasked padded batch: clip {b} ({n} frames) max |mel_post - solo oracle| = {d:.3e}")
        assert (d < MEL_TOL) if n == T else (d > MEL_TOL)


def test_batch_invariance_bits(case):
    """The 13-frame clip as row 1 of [7, 13, 22, 16] padded to 22, as row 0 of [13, 9] padded to 13, and alone through the library's own unmasked call
    (launch-per-phase route): the same bits of mel_post, output_lengths and attention - the masked kernels run the solo call's sums in the solo call's
    order, and at these sizes every GEMM of the path takes the same kernel whatever the row count."""
    nm = pc.native_model(case["sd"])                                         # "persist_decode" = 0 (tests/conftest.py): the solo call takes the launch route too
    m = case["m"]
    big = nm.inference(*_dev(case), S=S, want_attn=True, video_lengths=case["lens"])
    v13, e13, g13 = _solo(case, 1)
    v9 = synth.synth_padded_video(1, [9], tag="masked-9")
    v9 = torch.cat([v9, torch.zeros(1, 3, 4, 96, 96)], dim=2)
    pair_v = torch.cat([v13, v9]).cuda()
    pair_e = torch.cat([e13, case["emb"][3:4]]).cuda()
    pair_g = torch.cat([g13, case["gumbel"][3 * m:3 * m + 1]]).cuda()      # min_T(13) = 1 row per clip
    pair = nm.inference(pair_v, pair_e, pair_g, S=S, want_attn=True, video_lengths=[13, 9])
    solo = nm.inference(v13.cuda(), e13.cuda(), g13.cuda(), S=S, want_attn=True)
    torch.cuda.synchronize()
    for name, other, row in (("pair", pair, 0), ("solo", solo, 0)):
        d = pc.maxdiff(big[0][1], other[0][row])
        print(f"batch invariance: row 1 of the batch of 4 against the {name} call: max |d mel_post| = {d:.3e}")
        assert torch.equal(big[0][1], other[0][row]), name
        assert int(big[1][1]) == int(other[1][row])
        assert torch.equal(big[2][1, :, :13], other[2][row, :, :13]), name


@pytest.mark.parametrize("fold", [1, 0])
def test_staged_route_and_both_step_forms(case, fold):
    """l2s_decoder_prologue_masked + l2s_decode_steps_masked give the bits of l2s_inference_masked, with the phase-merged step and with the literal
    6-phase step, each within the gate of the solo oracle."""
    nm = pc.native_model(case["sd"]) if fold else pc.fresh_native_model(case["sd"], persist_decode=0, fold_step_weights=0)
    video, emb, gum = _dev(case)
    one = nm.inference(video, emb, gum, S=S, want_attn=True, video_lengths=case["lens"])
    vis = native.build_visual(nm.encoder_fwd(video), emb)
    state, _ = nm.decoder_prologue(vis, emb, gum, video_lengths=case["lens"])
    mel, stop, attn = nm.decode_steps(state, len(LENS), T, S, want_attn=True, video_lengths=case["lens"])
    mel_post, _ = nm.postnet(mel)
    lengths = native.output_lengths(stop)
    torch.cuda.synchronize()
    assert torch.equal(mel_post, one[0]) and torch.equal(lengths, one[1]) and torch.equal(attn, one[2])
    _check_inference(case, one, f"fold_step_weights={fold}")


def test_all_lengths_equal_T_is_the_unmasked_call():
    B, t = 2, 14
    nm = pc.native_model()
    video, emb = synth.synth_video(B, t, tag="masked-full").cuda(), synth.synth_speaker_embedding(B, tag="masked-full").cuda()
    gum = synth.synth_gumbel(B * native.min_T(t), tag="masked-full").cuda()
    plain = nm.inference(video, emb, gum, S=S, want_attn=True)
    masked = nm.inference(video, emb, gum, S=S, want_attn=True, video_lengths=[t, t])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain, masked))


def test_early_stop_composes(case):
    """A stop bias under which every clip stops inside S: with "early_stop" on, the masked call's lengths and kept frames are the option-off masked
    call's, the dropped frames exact zeros."""
    shift = -float(case["ref_stop"][:, :25].max(dim=1).values.min()) + 1e-2      # the stop logits do not feed back: every clip now crosses within 25 steps
    sd = dict(case["sd"])
    sd["decoder.stop_token_layer.linear_layer.bias"] = sd["decoder.stop_token_layer.linear_layer.bias"] + shift
    nm = pc.fresh_native_model(sd, persist_decode=0)
    args = _dev(case)
    off = [t.clone() for t in nm.inference(*args, S=S, want_attn=True, video_lengths=case["lens"])]
    nm.set_option("early_stop", 1)
    on = [t.clone() for t in nm.inference(*args, S=S, want_attn=True, video_lengths=case["lens"])]
    torch.cuda.synchronize()
    lens = off[1].cpu()
    print("early stop: output lengths", lens.tolist())
    assert int(lens.max()) < S and torch.equal(on[1].cpu(), lens)
    for b, n in enumerate(lens.tolist()):
        assert torch.equal(on[0][b, :, :n], off[0][b, :, :n]) and torch.equal(on[2][b, :n], off[2][b, :n])
        assert not on[0][b, :, n:].any() and not on[2][b, n:].any()


def test_default_persist_option_takes_the_launch_route(case):
    """"persist_decode" at the library's default (4), B = 2: a masked call does not take the persistent loop - it still matches each clip alone."""
    nm = pc.shipped_model(case["sd"])
    idx = [1, 3]
    m = case["m"]
    video = case["video"][idx][:, :, :16].contiguous().cuda()                       # [13, 16] padded to 16
    gum = torch.cat([case["gumbel"][b * m:b * m + native.min_T(16)] for b in idx]).cuda()
    mel, lengths, attn = nm.inference(video, case["emb"][idx].cuda(), gum, S=S, want_attn=True, video_lengths=[13, 16])
    launch = pc.native_model(case["sd"]).inference(video, case["emb"][idx].cuda(), gum, S=S, want_attn=True, video_lengths=[13, 16])
    torch.cuda.synchronize()
    native.check_persist_timeouts()
    assert torch.equal(mel, launch[0]) and torch.equal(attn, launch[2])
    for row, b in enumerate(idx):
        d = pc.maxdiff(mel[row], case["ref_inf"][b][0][0])
        print(f"persist_decode default: clip {b} max |mel_post - solo oracle| = {d:.3e}")
        assert d < MEL_TOL and int(lengths[row]) == int(case["ref_inf"][b][1][0])
        assert not attn[row, :, case["lens"][b]:].any()


def test_errors(case):
    nm = pc.native_model(case["sd"])
    L = native.lib()
    video, emb, gum = _dev(case)
    B = len(LENS)
    mel = torch.empty(B, 80, S, device="cuda")
    lengths = torch.empty(B, dtype=torch.int64, device="cuda")
    ws = nm.workspace(B, T, 96, 96, S, video.device, masked=True)
    for bad in (6, T + 1):
        lens = (ctypes.c_int32 * B)(7, bad, 22, 16)
        rc = L.l2s_inference_masked(nm._h, video.data_ptr(), emb.data_ptr(), gum.data_ptr(), B, T, 96, 96, S, mel.data_ptr(), lengths.data_ptr(), None,
                                    ws.data_ptr(), ws.numel(), None, lens)
        assert rc != 0 and f"video_lengths[1] = {bad}" in L.l2s_last_error().decode()
        with pytest.raises(ValueError, match="outside"):
            nm.inference(video, emb, gum, S=S, video_lengths=[7, bad, 22, 16])
    assert not hasattr(L, "l2s_inference_multi_masked") and not hasattr(L, "l2s_forward_eval_multi_masked")
    with pytest.raises(NotImplementedError):
        nm.inference_multi([(video, emb, gum)], S=S, video_lengths=case["lens"])
    from model.model import get_network
    net = get_network("train").cuda()
    net.honour_video_lengths = True
    with pytest.raises(NotImplementedError):
        net(video, None, None, case["mels"].cuda(), torch.tensor(case["lens"]), None, None, 1.0, speaker_embedding=emb)


def test_model_keyword_and_attribute(case):
    """Lip2Speech.inference(video_lengths=...) and eval-mode forward with `honour_video_lengths` on take the masked entry points."""
    from model.model import get_network
    net = get_network("test").cuda()
    net.load_state_dict(case["sd"], strict=True)
    video, emb, gum = _dev(case)
    mel, lengths = net.inference(video, None, speaker_embedding=emb, gumbel_noise=gum, video_lengths=torch.tensor(case["lens"]))
    S_full = net.decoder.hparams.max_decoder_steps
    assert mel.shape == (len(LENS), 80, S_full) and net.native_model().calls["l2s_inference_masked"] == 1
    for b in range(len(LENS)):      # 300 steps here, 40 in the reference: the post-net's receptive field (10 frames) ends inside the first 30
        assert pc.maxdiff(mel[b, :, :S - 10], case["ref_inf"][b][0][0][:, :S - 10]) < MEL_TOL
    vl = torch.tensor(case["lens"])
    with torch.no_grad():                                                           # evaluate.py's setting; with gradients enabled forward is the training route
        net(video, None, None, case["mels"].cuda(), vl, None, None, 1.0, speaker_embedding=emb, gumbel_noise=gum)
        assert net.native_model().calls["l2s_forward_eval_masked"] == 0             # attribute off (the default): lengths ignored as before
        net.honour_video_lengths = True
        out = net(video, None, None, case["mels"].cuda(), vl, None, None, 1.0, speaker_embedding=emb, gumbel_noise=gum)
    assert net.native_model().calls["l2s_forward_eval_masked"] == 1 and out[6] is vl
    assert torch.isneginf(out[4][0, :, 7:]).all()
