"""The voice tower over clips of unequal length on the GPU (l2s_speaker_encoder_packed, SpeakerEncoder.inference(audio_lengths=) / inference_packed,
callers with honour_lengths): every clip's embedding is what the tower gives for that clip ALONE.  Synthetic weights; the longest clip is 16 000 samples
(101 frames, 303 step launches).  The fp64 restatement is tests/speaker_tower_torch.py (st), the bounds are those of tests/test_speaker_encoder.py.

Forms ("the voice tower at per-clip lengths"): every test here has R = sum L_b < 3 969 compact rows (every GEMM on the f32 MFMA
kernel, as in the solo call) and B <= 96 clips (every step launch in the 1x1 sixteen-row blocks, as in the solo call), so wherever a test compares
the packed call with a solo call or with another packed call it asserts BITS."""
import ctypes

import numpy as np
import pytest
import torch

import parity_common as pc
import speaker_tower_torch as st
from lip2speech_amd import native, statespec, synth
from oracle import l2s_oracle as orc

pytestmark = pytest.mark.gpu

EMB_TOL, NORM_TOL = 2e-4, 1e-5       # test_speaker_encoder_hip_matches_oracle's bounds
MEL_TOL = 1e-3                       # the masked tests' gate (test_masked_lengths_gpu.py)
STAGES = ("spec", "power", "mel", "h0", "h1", "h2", "linear", "emb")
LENS = [201, 360, 3200, 16000]       # L = 2 (the minimum), 3, 21, 101; n % 160 = 41, 40, 0, 0
N = 16000


def _spk_sd():
    return synth.synth_state_dict(statespec.speaker_encoder_spec("speaker_encoder."), seed=99)


def _audio(B, n=N, seed=5, amp=0.2):
    """test_speaker_encoder.py's clips: a sine per clip plus noise a quarter of its amplitude"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / 16000.0
    base = amp * torch.sin(2 * np.pi * (180.0 + 40 * torch.arange(B).view(B, 1)) * t)
    return (base + 0.25 * amp * torch.randn(B, n, generator=g)).float()


def _padded(audio, lens, fill=0.0):
    out = audio.clone()
    for b, n in enumerate(lens):
        out[b, n:] = fill
    return out


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_form(lens):
    """the packed call takes the solo call's kernel forms: the DFT product below its move to the split-bf16 kernel, the recurrence in 1x1 blocks"""
    return sum(n // 160 + 1 for n in lens) < 3969 and len(lens) <= 96


@pytest.fixture(scope="module")
def sd():
    return _spk_sd()


@pytest.fixture(scope="module")
def nm(sd):
    return pc.fresh_native_model(sd)


@pytest.fixture(scope="module")
def enc(sd):
    from model.modules import SpeakerEncoder
    return SpeakerEncoder(state_dict={k[len("speaker_encoder."):]: v for k, v in sd.items()}).cuda()


@pytest.fixture(scope="module")
def base(nm):
    """the four clips of LENS as a zero-padded (4, 16000) tensor through the packed entry point with taps, and each clip through the solo call: computed
    once, shared, never changed"""
    audio = _padded(_audio(4), LENS)
    emb, taps = nm.speaker_encoder_packed(audio.cuda(), [b * N for b in range(4)], LENS, taps=True)
    solo = [nm.speaker_encoder_fwd(audio[b:b + 1, :n].contiguous().cuda()) for b, n in enumerate(LENS)]
    torch.cuda.synchronize()
    return {"audio": audio, "emb": emb.cpu(), "taps": [t.cpu() for t in taps], "solo": torch.cat(solo).cpu()}


def test_oracle_and_every_stage(sd, base):
    """every row within 2e-4 (unit norm 1e-5) of the oracle on the clip alone; through the taps, every stage of every clip - its compact rows mapped back
    through l2s_speaker_packed_plan - against the fp64 restatement of that stage on the device's own output of the stage before, as
    test_speaker_encoder.py's _check_stages judges the padded call (bound 8 x max(e32, eps32 x S))"""
    audio, emb, taps = base["audio"], base["emb"], base["taps"]
    order, rows, row0, L_max, R = native.speaker_packed_plan(LENS)
    assert (L_max, R) == (101, 2 + 3 + 21 + 101) and order == [3, 2, 1, 0]
    spec, power, mel, h0, h1, h2, lin = taps
    assert spec.shape == (R, 402) and power.shape == (R, 204) and mel.shape == (R, 40) and h2.shape == (R, 256) and lin.shape == (4, 256)
    assert torch.equal(power[:, 201:], torch.zeros(R, 3)), "power columns 201-203 must be exactly 0"
    assert emb.shape == (4, 256) and (emb >= 0).all() and ((emb.norm(dim=1) - 1).abs() < NORM_TOL).all()
    bad = []
    for b, n in enumerate(LENS):
        clip = audio[b:b + 1, :n]
        with torch.no_grad():
            want = orc.speaker_encoder_inference(sd, clip)
        d = (emb[b] - want[0]).abs().max().item()
        print(f"packed clip {b} (n = {n}): max |emb - oracle on the clip alone| = {d:.2e}")
        assert d < EMB_TOL
        L, r = st.n_frames(n), order.index(b)
        idx = torch.tensor([row0[l] + r for l in range(L)])
        s_b, p_b, m_b = spec[idx], power[idx], mel[idx]
        res = {"spec": st.frame_check(s_b, st.spec(clip), st.spec(clip, torch.float32)),
               "power": st.frame_check(p_b, st.power(s_b.double()), st.power(s_b)),
               "mel": st.frame_check(m_b, st.mel(p_b.double()), st.mel(p_b))}
        x = m_b.view(1, L, 40)
        for layer, h in enumerate((h0, h1, h2)):
            h_b = h[idx].view(1, L, 256)
            res[f"h{layer}"] = st.global_check(h_b, st.lstm_layer(sd, layer, x.double()), st.lstm_layer(sd, layer, x))
            x = h_b
        res["linear"] = st.global_check(lin[b:b + 1], st.linear_relu(sd, x[:, -1].double()), st.linear_relu(sd, x[:, -1]))
        res["emb"] = st.global_check(emb[b:b + 1], st.normalise(lin[b:b + 1].double()), st.normalise(lin[b:b + 1]))
        for k in STAGES:
            ok, dev, ref = res[k]
            print(f"packed clip {b} (n = {n}) stage {k:6s}: device {dev:.2e} (reference scale {ref:.2e}) {'ok' if ok else 'EXCEEDS its bound'}")
            if not ok:
                bad.append((b, k))
    assert not bad, f"(clip, stage) beyond 8 x max(e32, eps32 x S): {bad}"


def test_each_row_is_the_solo_call(base):
    """row b against l2s_speaker_encoder_fwd on audio[b:b+1, :n_b].  R = 127 rows and 4 clips: inside the solo call's forms, so bit for bit"""
    same = _same_form(LENS)
    print(f"packed [201, 360, 3200, 16000] against the solo calls: {'same kernel forms: bits asserted' if same else 'other forms: oracle bound asserted'}")
    for b, n in enumerate(LENS):
        d = (base["emb"][b] - base["solo"][b]).abs().max().item()
        print(f"packed clip {b} (n = {n}): max |emb - solo call| = {d:.2e}")
        assert _bits(base["emb"][b], base["solo"][b]) if same else d < EMB_TOL


def test_independent_of_company(nm, enc, base):
    """Clip A (3 200 samples) and clip B (16 000): [A, B] and [B, A]; A beside a longer partner (B) and beside a shorter one (360 samples); the padded
    tensor with audio_lengths against the same clips packed at odd float offsets, and as a datasets.PackedAudio.  Every call here has at most 4 clips
    and R <= 127 rows - one form - so every comparison is of bits.  All lengths equal to N: the unmasked call's bits too (B = 3, R = 36)."""
    audio = base["audio"]
    A, Bc, C = audio[2, :3200], audio[3, :16000], audio[1, :360]

    def run(clips, lead=0, gap=0):
        """clips packed back to back after `lead` floats with `gap` floats between them (NaN, as are 7 guard floats at the end)"""
        off, pos = [], lead
        for c in clips:
            off.append(pos)
            pos += c.numel() + gap
        buf = torch.full((pos + 7,), float("nan"))
        for c, o in zip(clips, off):
            buf[o:o + c.numel()] = c
        return enc.inference_packed(buf.cuda(), off, [c.numel() for c in clips]).cpu()

    ab, ba = run([A, Bc]), run([Bc, A])
    assert _bits(ab[0], ba[1]) and _bits(ab[1], ba[0]), "[A, B] against [B, A]"
    ac = run([A, C])
    assert _bits(ab[0], ac[0]) and _bits(ab[0], base["emb"][2]) and _bits(ac[1], base["emb"][1]), "A beside a longer and beside a shorter partner"
    odd = run([audio[b, :n] for b, n in enumerate(LENS)], lead=3, gap=5)      # offsets 3, 209, 574, 3779: none a multiple of 4
    assert _bits(odd, base["emb"]), "padded tensor + lengths against the packed buffer at odd offsets"
    via_lengths = enc.inference(audio.cuda(), audio_lengths=torch.tensor(LENS)).cpu()
    assert _bits(via_lengths, base["emb"]), "SpeakerEncoder.inference(audio_lengths=)"
    from lip2speech_amd.datasets.device import PackedAudio
    pa = PackedAudio([audio[2:3, :3200], audio[3, :16000], audio[0:1, :1000]], pin=False)      # a PackedAudio needs 513 samples per clip
    got = enc.inference_packed(pa).cpu()
    assert _bits(got[:2], base["emb"][2:]) and _bits(got[2], run([audio[0, :1000]])[0])
    full = _audio(3, 1761)
    eq = enc.inference(full.cuda(), audio_lengths=[1761] * 3).cpu()
    unmasked = enc.inference(full.cuda()).cpu()
    assert (eq - unmasked).abs().max() < EMB_TOL and _bits(eq, unmasked), "all lengths equal to N"
    assert torch.isfinite(ab).all() and torch.isfinite(odd).all() and torch.isfinite(got).all()


def test_never_reads_outside_a_clip(enc, base):
    """NaN in the padding of the (B, N) tensor - a reflection at the padded end, or a recurrence running on over it, would spread it; NaN in the lead,
    the gaps and the guard floats of a packed buffer - a read into the neighbour would.  Same bits as with zeros, all finite."""
    poisoned = _padded(base["audio"], LENS, fill=float("nan"))
    assert torch.isnan(poisoned[0, 201:]).all()
    got = enc.inference(poisoned.cuda(), audio_lengths=LENS).cpu()
    assert torch.isfinite(got).all() and _bits(got, base["emb"])
    off, pos = [], 9
    for n in LENS:
        off.append(pos)
        pos += n + 11
    buf = torch.full((pos + 64,), float("nan"))
    for b, (o, n) in enumerate(zip(off, LENS)):
        buf[o:o + n] = base["audio"][b, :n]
    got = enc.inference_packed(buf.cuda(), off, LENS).cpu()
    assert torch.isfinite(got).all() and _bits(got, base["emb"])


def test_the_gap_is_real(enc, nm):
    """lengths [3 200, 16 000] zero-padded to 16 000: the UNMASKED call's row 0 - the top LSTM's state after 80 frames of padding, its last real frames
    reflected against zeros - is another embedding than the clip's own: at least 100 x the oracle bound away (the fp32 oracle on the host gives 9.1e-2
    for these weights and clips, 450 x).  With audio_lengths row 0 is the solo embedding; row 1, the full-length clip, is itself either way."""
    lens = [3200, 16000]
    audio = _padded(_audio(2), lens)
    unmasked = enc.inference(audio.cuda()).cpu()
    masked = enc.inference(audio.cuda(), audio_lengths=lens).cpu()
    solo = nm.speaker_encoder_fwd(audio[:1, :3200].contiguous().cuda()).cpu()
    gap, left = (unmasked[0] - solo[0]).abs().max().item(), (masked[0] - solo[0]).abs().max().item()
    print(f"padded 3 200-sample clip beside a 16 000-sample one: max |emb - solo| = {gap:.3e} unmasked, {left:.3e} with audio_lengths")
    assert gap >= 100 * EMB_TOL
    assert left == 0.0 and _bits(masked[0], solo[0])
    assert (unmasked[1] - masked[1]).abs().max() < EMB_TOL


def test_callers_honour_lengths(enc, synth_sd, monkeypatch):
    """demo_clip on a batch of two clips of unequal audio AND video length (13 and 22 frames, 3 200 and 16 000 samples), the shorter first: with
    honour_lengths its mel is the mel of that clip run alone through demo_clip, inside the masked tests' gate (1e-3; test_masked_lengths_gpu.py asserts
    bits for a 13-frame clip in batches of 4 and 2 at S = 40 - this batch and S = 300 are other sizes, so the gate is what is asserted and the bit
    comparison is printed).  Without honour_lengths: today's output - net.inference with the unmasked embedding, bit for bit."""
    from lip2speech_amd import callers
    from lip2speech_amd.model.modules.decoder import Decoder
    from model.model import get_network
    noise = synth.synth_gumbel(8, tag="spk-packed")
    monkeypatch.setattr(Decoder, "draw_gumbel", staticmethod(lambda rows, device, dtype=torch.float32: noise[:rows].to(device)))
    vlens, alens = [13, 22], [3200, 16000]
    video = synth.synth_padded_video(2, vlens, tag="spk-packed")
    audio = _padded(_audio(2), alens)
    net = get_network("test").cuda()
    net.load_state_dict(synth_sd, strict=True)
    batch = ((video, torch.tensor(vlens)), (audio, torch.tensor(alens)), None, None, None)
    alone = ((video[:1, :, :13].contiguous(), torch.tensor([13])), (audio[:1, :3200].contiguous(), torch.tensor([3200])), None, None, None)
    m_h, l_h, a_h = callers.demo_clip(net, batch, speaker_encoder=enc, honour_lengths=True)
    m_1, l_1, a_1 = callers.demo_clip(net, alone, speaker_encoder=enc)
    n = int(l_1[0])
    assert int(l_h[0]) == n and m_h.shape == m_1.shape == (1, 80, n)
    d = pc.maxdiff(m_h, m_1)
    print(f"demo_clip(honour_lengths=True), the short clip against itself alone: max |d mel| = {d:.3e}, {'same bits' if torch.equal(m_h, m_1) else 'other bits'}")
    assert d < MEL_TOL
    # the default: lengths ignored on both sides, as before
    m_0, l_0, a_0 = callers.demo_clip(net, batch, speaker_encoder=enc)
    with torch.no_grad():
        mel, lengths, attn = net.inference(video.cuda(), None, speaker_embedding=enc.inference(audio.cuda()), return_attention_map=True)
    n0 = int(lengths[0])
    assert torch.equal(l_0, lengths) and torch.equal(m_0, mel[:1, :, :n0]) and torch.equal(a_0, attn[:, :n0])


def test_errors_launch_nothing(nm, synth_sd):
    """a clip of 200 samples, a workspace one byte short, a model without speaker_encoder.* weights: the library's message, `emb` untouched"""
    L = nm._L
    audio = _audio(2, 1761).cuda()
    off = (ctypes.c_int64 * 2)(0, 1761)
    other = pc.native_model(synth_sd)                # the Lip2Speech checkpoint: no speaker tower in it
    for h, ns, short, msg in ((nm._h, [1761, 200], 0, "n_samples[1] = 200"), (nm._h, [1761, 1000], 1, "speaker-encoder workspace too small"),
                              (other._h, [1761, 1000], 0, "no speaker_encoder.* weights")):
        c_ns = (ctypes.c_int64 * 2)(*ns)
        need = int(L.l2s_speaker_workspace_bytes_packed((ctypes.c_int64 * 2)(1761, 1000), 2))
        emb = torch.full((2, 256), 7.0, device="cuda")
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        rc = L.l2s_speaker_encoder_packed(h, audio.data_ptr(), off, c_ns, 2, emb.data_ptr(), ws.data_ptr(), ctypes.c_int64(need - short), None)
        torch.cuda.synchronize()
        assert rc != 0 and msg in L.l2s_last_error().decode()
        assert (emb == 7.0).all()
    with pytest.raises(RuntimeError, match=r"n_samples\[0\] = 200"):
        nm.speaker_encoder_packed(audio, [0, 1761], [200, 1761])
    with pytest.raises(ValueError, match="ends at float"):
        nm.speaker_encoder_packed(audio, [0, 1761], [1761, 1762])
    emb, ws = torch.full((2, 256), 7.0, device="cuda"), torch.empty(need, dtype=torch.uint8, device="cuda")      # the full size is accepted
    assert L.l2s_speaker_encoder_packed(nm._h, audio.data_ptr(), off, (ctypes.c_int64 * 2)(1761, 1000), 2, emb.data_ptr(), ws.data_ptr(), ctypes.c_int64(need), None) == 0
    torch.cuda.synchronize()
    assert ((emb.norm(dim=1) - 1).abs() < NORM_TOL).all()
