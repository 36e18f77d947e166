"""SpeakerEncoder tower.  CPU: the oracle's LSTM tail against torch.nn.LSTM, and the stage-by-stage fp64 restatement
(tests/speaker_tower_torch.py) against the oracle's mel; GPU: HIP vs oracle on the embedding, and every stage on its own (l2s_op_speaker_taps)
against the fp64 restatement of that stage applied to the device's own output of the stage before."""
import ctypes

import numpy as np
import pytest
import torch

import speaker_tower_torch as st
from lip2speech_amd import statespec, synth
from oracle import l2s_oracle as orc


def _spk_sd():
    return synth.synth_state_dict(statespec.speaker_encoder_spec("speaker_encoder."), seed=99)


def _audio(B, N=19456, seed=5, amp=0.2):
    """a sine per clip plus noise a quarter of its amplitude; amp = 0.2: mel peaks near 400 (layer 0 saturated), 0.9: hard saturated, 0.01: the gates' linear range"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(N) / 16000.0
    base = amp * torch.sin(2 * np.pi * (180.0 + 40 * torch.arange(B).view(B, 1)) * t)
    return (base + 0.25 * amp * torch.randn(B, N, generator=g)).float()


def test_oracle_tail_matches_nn_lstm():
    sd = _spk_sd()
    lstm = torch.nn.LSTM(40, 256, 3, batch_first=True)
    lin = torch.nn.Linear(256, 256)
    lstm.load_state_dict({k[len("speaker_encoder.lstm."):]: v for k, v in sd.items() if ".lstm." in k})
    lin.load_state_dict({"weight": sd["speaker_encoder.linear.weight"], "bias": sd["speaker_encoder.linear.bias"]})
    mel = orc.mel40(_audio(3))
    assert mel.shape == (3, 122, 40)
    with torch.no_grad():
        _, (h, _) = lstm(mel)
        want = torch.nn.functional.normalize(torch.relu(lin(h[-1])), p=2, dim=1)
        got = orc.speaker_lstm_tail(sd, mel)
    assert (got - want).abs().max() < 2e-6


@pytest.mark.gpu
def test_speaker_encoder_hip_matches_oracle():
    from model.modules import SpeakerEncoder
    sd = _spk_sd()
    enc = SpeakerEncoder(state_dict={k[len("speaker_encoder."):]: v for k, v in sd.items()}).cuda()
    for B, N in ((3, 19456), (1, 8000), (17, 16000)):
        audio = _audio(B, N)
        emb = enc.inference(audio.cuda())
        with torch.no_grad():
            want = orc.speaker_encoder_inference(sd, audio)
        assert emb.shape == (B, 256) and (emb >= 0).all()
        assert ((emb.norm(dim=1) - 1).abs() < 1e-5).all()
        assert (emb.cpu() - want).abs().max() < 2e-4
    # the embedding feeds Lip2Speech.inference as `speaker_embedding` (demo.py:84-86)


# ------------------------------------------------------------------------------------------------ the fp64 restatement, pinned on the host
def test_stage_restatement_matches_oracle_mel_and_bounds_catch_wrong_ones():
    """tests/speaker_tower_torch.py (frames x Hann, DFT as a matrix product, power, HTK filterbank) gives the oracle's mel40 (torch.stft) in fp64 to
    rounding: measured 3e-15 of a frame's largest band; asserted at 1e-12 (fp64 sums of 400 and 201 terms: a few hundred eps64 at the very most).
    And the stage bounds of the GPU tests below are tight enough to notice an end reflection off by one, a symmetric window, DFT operands rounded
    to bf16 and filterbank rows shifted by one bin: measured 1.4e-2, 5.7e-3, 2.2e-3 and 0.74 of a frame's largest band against a bound of a few 1e-6."""
    for B, N in ((3, 19456), (2, 201), (2, 320), (1, 16079)):
        audio = _audio(B, N).double()
        got, want = st.mel_from_audio(audio), orc.mel40(audio)
        assert got.shape == want.shape == (B, N // 160 + 1, 40)
        rel = ((got - want).abs().amax(dim=2) / want.abs().amax(dim=2)).max().item()
        print(f"restatement vs oracle.mel40 (fp64) B={B} N={N}: {rel:.1e} of the frame's largest band")
        assert rel < 1e-12
    audio = _audio(3)
    R = 3 * st.n_frames(audio.shape[1])
    mel64, mel32 = st.mel_from_audio(audio).view(R, 40), st.mel_from_audio(audio, torch.float32).view(R, 40)
    ok, _, e32 = st.frame_check(mel32, mel64, mel32)
    assert ok and 8 * max(e32, st.EPS32) < 1e-5          # the bound: a few 1e-6 of the frame's largest band
    spec64, spec32 = st.spec(audio), st.spec(audio, torch.float32)
    pw64 = st.power(spec64)
    wrong = {"end reflection off by one": dict(end_off=1), "symmetric window": dict(periodic=False), "DFT operands in bf16": dict(bf16_operands=True),
             "filterbank one bin late": dict(fb_shift=1)}
    for name, kw in wrong.items():
        ok, rel, _ = st.frame_check(st.mel_from_audio(audio, **kw).view(R, 40), mel64, mel32)
        print(f"wrong restatement ({name}): mel moves by {rel:.1e} of the frame's largest band")
        assert not ok and rel > 1e-3, name
        # and at the stage that is wrong, judged as the GPU tests judge it
        if "fb_shift" in kw:
            assert not st.frame_check(st.mel(pw64, fb_shift=1), st.mel(pw64), st.mel(pw64.float()))[0]
        else:
            assert not st.frame_check(st.spec(audio, **kw), spec64, spec32)[0], name


# ------------------------------------------------------------------------------------------------ GPU: each stage on its own
STAGES = ("spec", "power", "mel", "h0", "h1", "h2", "linear", "emb")
_nms = {}


def _nm(**options):
    """NativeModels holding the speaker tower's weights, one per option set (options are per model, set before the weights are packed)."""
    import parity_common as pc
    key = tuple(sorted(options.items()))
    if key not in _nms:
        _nms[key] = pc.fresh_native_model(_spk_sd(), **options)
    return _nms[key]


def _run(nm, audio):
    emb, taps = nm.speaker_encoder_fwd(audio.cuda(), taps=True)
    torch.cuda.synchronize()
    return emb.cpu(), [t.cpu() for t in taps]


def _check_stages(sd, audio, emb, taps, label):
    """Every stage against its fp64 restatement fed the DEVICE's output of the stage before; bound 8 x max(e32, eps32 x S) (speaker_tower_torch.py:
    e32 = what the fp32 torch restatement of the stage loses on the same input).  Prints the deviation of every stage, then asserts them all."""
    B, N = audio.shape
    L = st.n_frames(N)
    spec, power, mel, h0, h1, h2, lin = taps
    assert spec.shape == (B * L, 402) and power.shape == (B * L, 204) and mel.shape == (B * L, 40) and h2.shape == (B, L, 256) and lin.shape == (B, 256)
    res = {}
    res["spec"] = st.frame_check(spec, st.spec(audio), st.spec(audio, torch.float32))
    res["power"] = st.frame_check(power, st.power(spec.double()), st.power(spec))
    res["mel"] = st.frame_check(mel, st.mel(power.double()), st.mel(power))
    x = mel.view(B, L, 40)
    for layer, h in enumerate((h0, h1, h2)):
        res[f"h{layer}"] = st.global_check(h, st.lstm_layer(sd, layer, x.double()), st.lstm_layer(sd, layer, x))
        x = h
    res["linear"] = st.global_check(lin, st.linear_relu(sd, h2[:, -1].double()), st.linear_relu(sd, h2[:, -1]))
    res["emb"] = st.global_check(emb, st.normalise(lin.double()), st.normalise(lin))
    for k in STAGES:
        ok, dev, ref = res[k]
        unit = "of the frame's largest, fp32 torch" if k in ("spec", "power", "mel") else "abs, bound"
        print(f"speaker stage {label} {k:6s}: device {dev:.2e} ({unit} {ref:.2e}) {'ok' if ok else 'EXCEEDS its bound'}")
    assert torch.equal(power[:, 201:], torch.zeros(B * L, 3)), "power columns 201-203 must be exactly 0"
    assert emb.shape == (B, 256) and (emb >= 0).all()
    bad = [k for k in STAGES if not res[k][0]]
    assert not bad, f"{label}: stages beyond 8 x max(e32, eps32 x S): {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("amp", [0.2, 0.9, 0.01])
def test_speaker_stages_amplitude_regimes(amp):
    """(3, 19456) with layer 0 saturated (0.2), hard saturated (0.9) and in the gates' linear range (0.01)."""
    sd, audio = _spk_sd(), _audio(3, amp=amp)
    emb, taps = _run(_nm(), audio)
    _check_stages(sd, audio, emb, taps, f"amp={amp}")
    assert ((emb.norm(dim=1) - 1).abs() < 1e-5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [201, 320, 16079, 16000])
def test_speaker_stages_length_edges(N):
    """the shortest clip the entry accepts (L = 2), a multiple of the hop, one sample short of the next frame and 1 s; clip 1 is all zeros, as the tail
    of a padded batch is: its spec, power and mel must be exactly zero (S = 0 in the frame bound)"""
    sd, audio = _spk_sd(), _audio(2, N)
    audio[1] = 0
    emb, taps = _run(_nm(), audio)
    _check_stages(sd, audio, emb, taps, f"N={N}")
    L = st.n_frames(N)
    assert not taps[2][L:].any() and taps[2][:L].any()


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,x3", [(32, 19456, 1), (33, 19200, 1), (3, 19456, 3), (3, 19456, 0)])
def test_speaker_stages_dft_kernel_switch(B, N, x3):
    """the DFT product (R = B L rows, N = 402, K = 400) moves from the f32 MFMA kernel to the narrow split-bf16 tile from R = 3 969 rows at the default
    "gemm_x3" = 1: R = 3 904 just below, 3 993 just above; "gemm_x3" = 3 forces every addressable GEMM of the tower onto the split-bf16 kernel, 0 none"""
    sd, audio = _spk_sd(), _audio(B, N)
    emb, taps = _run(_nm() if x3 == 1 else _nm(gemm_x3=x3), audio)
    _check_stages(sd, audio, emb, taps, f"B={B} N={N} gemm_x3={x3}")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 15, 16, 17, 48, 49, 97, 112, 193, 200, 385])
def test_speaker_stages_recurrence_batch_forms(B):
    """N = 1 761 (L = 12).  The recurrence (K = 256, LSTM epilogue in the general blocks) changes block shape with the batch: 1x1 blocks up to 96 clips
    (full and ragged 16-row tiles), skinny_rc_kernel<2,1> from 97, <2,2> from 193, <4,2> from 385 - each here with a ragged last row tile"""
    sd, audio = _spk_sd(), _audio(B, 1761)
    emb, taps = _run(_nm(), audio)
    _check_stages(sd, audio, emb, taps, f"B={B} L=12")


@pytest.mark.gpu
def test_speaker_stages_grid_stride_wraparound():
    """(400, 4000): L = 26, R = 10 400 - 4.16 M window elements and 2.12 M power elements, both past the 8 192 x 256 threads of their launches (the
    grid-stride loops wrap), the 4x2 recurrence blocks and the split-bf16 DFT in one call"""
    sd, audio = _spk_sd(), _audio(400, 4000)
    assert 400 * 26 * 400 > 8192 * 256 and 400 * 26 * 204 > 8192 * 256
    emb, taps = _run(_nm(), audio)
    _check_stages(sd, audio, emb, taps, "B=400 N=4000")


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,bad", [(3, 19456, 1), (100, 1761, 17)])
def test_speaker_neighbours_of_a_nan_clip_keep_their_bits(B, N, bad):
    """rows are independent in every product of the tower: with one clip all NaN, every other clip's embedding and taps have the bits of the all-finite
    call (an end reflection reaching into the next clip, or a start reflection into the one before, would not)"""
    audio = _audio(B, N)
    emb0, taps0 = _run(_nm(), audio)
    poisoned = audio.clone()
    poisoned[bad] = float("nan")
    emb1, taps1 = _run(_nm(), poisoned)
    keep = torch.arange(B) != bad
    assert torch.isfinite(emb0).all() and _same_bits(emb0[keep], emb1[keep])
    for name, a, b in zip(STAGES, taps0, taps1):
        a, b = a.reshape(B, -1), b.reshape(B, -1)
        assert torch.isfinite(a).all() and _same_bits(a[keep], b[keep]), name
    assert torch.isnan(taps1[0].reshape(B, -1)[bad]).all()          # and the poison did arrive


@pytest.mark.gpu
def test_speaker_zero_vector_normalises_to_zero():
    """linear.bias = -10: ReLU leaves the zero vector; the oracle's clamp and pool_norm_cat's max(|v|, eps) both give exactly 0, finite"""
    import parity_common as pc
    sd = _spk_sd()
    sd["speaker_encoder.linear.bias"] = torch.full_like(sd["speaker_encoder.linear.bias"], -10.0)
    audio = _audio(3)
    emb, taps = _run(pc.fresh_native_model(sd), audio)
    assert not taps[6].any()
    assert torch.isfinite(emb).all() and not emb.any()
    with torch.no_grad():
        assert not orc.speaker_encoder_inference(sd, audio).any()


@pytest.mark.gpu
def test_speaker_bf16_leg_front_end():
    """a model with "infer_bf16" = 1: the DFT and filterbank products round their operands to bf16 (nearest even) and accumulate in fp32.  spec against the
    fp64 product of the rounded operands - the fp32 frames (audio x fp32 window, one rounding: the same bits on the host) and the fp32 DFT table; mel
    against bf16(device power) x bf16(filterbank); bound 8 x the deviation of an fp32-accumulated torch product of the same rounded operands.  And the
    flag really does something: spec differs from the unrounded product by more than 1e-4 of the frame's largest bin."""
    audio = _audio(3)
    emb, taps = _run(_nm(infer_bf16=1), audio)
    spec, power, mel = taps[:3]
    f16, d16 = st.frames(audio, torch.float32).bfloat16(), st.dft_matrix(torch.float32).bfloat16()
    ok, dev, e32 = st.frame_check(spec, f16.double() @ d16.double(), f16.float() @ d16.float(), floor=0.0)
    print(f"speaker stage bf16 spec  : device {dev:.2e} (of the frame's largest, fp32 torch {e32:.2e}) {'ok' if ok else 'EXCEEDS its bound'}")
    p16, fb16 = power[:, :201].bfloat16(), st.filterbank(torch.float32).bfloat16()
    ok_m, dev_m, e32_m = st.frame_check(mel, p16.double() @ fb16.double(), p16.float() @ fb16.float(), floor=0.0)
    print(f"speaker stage bf16 mel   : device {dev_m:.2e} (of the frame's largest, fp32 torch {e32_m:.2e}) {'ok' if ok_m else 'EXCEEDS its bound'}")
    _, moved, _ = st.frame_check(spec, st.spec(audio), st.spec(audio, torch.float32))
    print(f"speaker stage bf16 spec  : {moved:.2e} of the frame's largest bin from the unrounded product")
    assert ok and ok_m
    assert moved > 1e-4
    assert torch.isfinite(emb).all() and ((emb.norm(dim=1) - 1).abs() < 1e-5).all()


@pytest.mark.gpu
def test_speaker_entry_refuses_short_audio_and_short_workspace():
    """N = 200 (no room for the reflect padding) and a workspace one byte short of l2s_speaker_workspace_bytes: the library's message, `emb` untouched"""
    nm = _nm()
    with pytest.raises(RuntimeError, match="audio shorter than the reflect padding"):
        nm.speaker_encoder_fwd(_audio(2, 200).cuda())
    L = nm._L
    for N, short, msg in ((200, 0, "audio shorter than the reflect padding (200 samples)"), (1761, 1, "speaker-encoder workspace too small")):
        audio = _audio(2, N).cuda()
        emb = torch.full((2, 256), 7.0, device="cuda")
        need = int(L.l2s_speaker_workspace_bytes(2, N))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        rc = L.l2s_speaker_encoder_fwd(nm._h, audio.data_ptr(), 2, N, emb.data_ptr(), ws.data_ptr(), ctypes.c_int64(need - short), None)
        torch.cuda.synchronize()
        assert rc != 0 and msg in L.l2s_last_error().decode()
        assert (emb == 7.0).all()
    ws = torch.empty(int(L.l2s_speaker_workspace_bytes(2, 1761)), dtype=torch.uint8, device="cuda")      # the full size is accepted
    emb, audio = torch.full((2, 256), 7.0, device="cuda"), _audio(2, 1761).cuda()
    assert L.l2s_speaker_encoder_fwd(nm._h, audio.data_ptr(), 2, 1761, emb.data_ptr(), ws.data_ptr(), ctypes.c_int64(ws.numel()), None) == 0
    torch.cuda.synchronize()
    assert ((emb.norm(dim=1) - 1).abs() < 1e-5).all()
