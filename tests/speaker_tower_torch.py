"""Stage-by-stage restatement of the voice speaker tower, for the tests only (nothing under lip2speech_amd/ imports it).

Each function is ONE stage of ``l2s_speaker_encoder_fwd`` from a given input, in the dtype asked for (fp64 = the reference; fp32 = the yardstick of what
fp32 arithmetic costs on the same input): reflect-indexed frames x periodic Hann, the real DFT as a matrix product [cos | sin] (the sign of the
imaginary half is the table's, +sin: the power does not see it), power, the HTK filterbank, one LSTM layer, Linear + ReLU, L2 normalisation.  Tables are
computed in fp64 and then rounded to the working dtype, as the library's packer does.  ``tests/test_speaker_encoder.py`` pins ``mel`` against
``oracle.mel40`` (which goes through ``torch.stft``) and shows that the stage bounds catch four deliberately wrong restatements (the keyword switches).
"""
import math

import torch

from oracle import l2s_oracle as orc

N_FFT, HOP, NF, NFP, NMEL, H = 400, 160, 201, 204, 40, 256
EPS32 = torch.finfo(torch.float32).eps
MARGIN = 8.0      # another summation order and other expf / tanhf roundings than torch's: the margin of the l2s_mel_targets tests


def n_frames(N: int) -> int:
    return N // HOP + 1


def window(dtype=torch.float64, periodic=True) -> torch.Tensor:
    j = torch.arange(N_FFT, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2.0 * math.pi * j / (N_FFT if periodic else N_FFT - 1))).to(dtype)


def dft_matrix(dtype=torch.float64) -> torch.Tensor:
    """(400, 402): column k = cos(2 pi k j / 400), column 201 + k = sin(2 pi k j / 400), k = 0..200 (the angle reduced exactly, k j mod 400)."""
    kj = (torch.arange(NF).view(1, NF) * torch.arange(N_FFT).view(N_FFT, 1)) % N_FFT
    ang = 2.0 * math.pi * kj.double() / N_FFT
    return torch.cat([torch.cos(ang), torch.sin(ang)], dim=1).to(dtype)


def filterbank(dtype=torch.float64, shift=0) -> torch.Tensor:
    """(201, 40) HTK triangles; shift = 1 (a wrong restatement): every row one bin late."""
    fb = orc.htk_mel_filterbank(NF, 0.0, 8000.0, NMEL, 16000)
    if shift:
        fb = torch.roll(fb, shift, dims=0)
    return fb.to(dtype)


def reflect_index(N: int, end_off=0) -> torch.Tensor:
    """(L, 400) sample index of frame l, tap j under centre + reflect padding; end_off = 1 (a wrong restatement): the end reflection as 2 (N - 1) - i + 1."""
    L = n_frames(N)
    i = torch.arange(L).view(L, 1) * HOP + torch.arange(N_FFT).view(1, N_FFT) - N_FFT // 2
    i = torch.where(i < 0, -i, i)
    return torch.where(i >= N, 2 * (N - 1) - i + end_off, i)


def frames(audio: torch.Tensor, dtype=torch.float64, end_off=0, periodic=True) -> torch.Tensor:
    """audio (B, N) -> (B * L, 400) = audio[reflect index] * window, one rounding in `dtype`."""
    B, N = audio.shape
    idx = reflect_index(N, end_off).clamp(max=N - 1)
    return (audio.to(dtype)[:, idx] * window(dtype, periodic)).reshape(B * n_frames(N), N_FFT)


def spec(audio: torch.Tensor, dtype=torch.float64, bf16_operands=False, **wrong) -> torch.Tensor:
    """audio (B, N) -> (B * L, 402) = [re | im]; bf16_operands (a wrong restatement of the fp32 path, and the right one of the bf16 leg given fp32 frames)."""
    f, d = frames(audio, dtype, **wrong), dft_matrix(dtype)
    if bf16_operands:
        f, d = f.bfloat16().to(dtype), d.bfloat16().to(dtype)
    return f @ d


def power(sp: torch.Tensor) -> torch.Tensor:
    """(R, 402) -> (R, 204): re^2 + im^2, columns 201-203 zero."""
    out = sp.new_zeros(sp.shape[0], NFP)
    out[:, :NF] = sp[:, :NF] * sp[:, :NF] + sp[:, NF:] * sp[:, NF:]
    return out


def mel(pw: torch.Tensor, fb_shift=0) -> torch.Tensor:
    """(R, 204) -> (R, 40)."""
    return pw[:, :NF] @ filterbank(pw.dtype, fb_shift)


def mel_from_audio(audio: torch.Tensor, dtype=torch.float64, bf16_operands=False, fb_shift=0, **wrong) -> torch.Tensor:
    B, N = audio.shape
    return mel(power(spec(audio, dtype, bf16_operands, **wrong)), fb_shift).view(B, n_frames(N), NMEL)


def lstm_layer(sd, layer: int, x: torch.Tensor, p="speaker_encoder.") -> torch.Tensor:
    """(B, L, in) -> (B, L, 256): layer `layer` from a zero state, weights of `sd` in x's dtype."""
    B, L, _ = x.shape
    w = [sd[f"{p}lstm.{n}_l{layer}"].to(x.dtype) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    h, c = x.new_zeros(B, H), x.new_zeros(B, H)
    outs = []
    for t in range(L):
        h, c = orc.lstm_cell(x[:, t], h, c, *w)
        outs.append(h)
    return torch.stack(outs, dim=1)


def linear_relu(sd, h_last: torch.Tensor, p="speaker_encoder.") -> torch.Tensor:
    return torch.relu(h_last @ sd[p + "linear.weight"].to(h_last.dtype).t() + sd[p + "linear.bias"].to(h_last.dtype))


def normalise(v: torch.Tensor) -> torch.Tensor:
    return v / torch.clamp(torch.sqrt((v * v).sum(dim=1, keepdim=True)), min=1e-12)


# ---------------------------------------------------------------------------------------------- the stage bounds
def frame_check(got: torch.Tensor, ref64: torch.Tensor, ref32: torch.Tensor, floor=EPS32):
    """Per-frame stages (spec, power, mel: rows are frames).  A frame's deviation is judged by ITS largest reference magnitude S_r, so that a quiet frame
    is not judged by a loud one: |got - ref64| <= 8 * max(e32, eps32) * S_r on every row r, where e32 = max_r |ref32 - ref64|_r / S_r is what fp32
    torch arithmetic loses on the same input.  A frame with S_r = 0 (a silent clip) must be exactly zero.  -> (ok, worst got / S, e32)"""
    got, ref64, ref32 = got.double().cpu(), ref64.double(), ref32.double()
    S = ref64.abs().amax(dim=1)
    live = S > 0
    Sl = torch.where(live, S, torch.ones_like(S))
    e32 = ((ref32 - ref64).abs().amax(dim=1) / Sl)[live].max().item() if live.any() else 0.0
    err = (got - ref64).abs().amax(dim=1)
    rel = (err / Sl)[live].max().item() if live.any() else 0.0
    ok = bool(torch.isfinite(got).all()) and bool((err <= MARGIN * max(e32, floor) * S).all())
    return ok, rel, e32


def global_check(got: torch.Tensor, ref64: torch.Tensor, ref32: torch.Tensor):
    """Hidden sequences, linear and embedding: |got - ref64| <= 8 * max(e32, eps32 * S), S the largest reference magnitude.  -> (ok, worst, bound)"""
    got, ref64, ref32 = got.double().cpu(), ref64.double(), ref32.double()
    S = ref64.abs().max().item()
    e32 = (ref32 - ref64).abs().max().item()
    err = (got - ref64).abs().max().item() if got.numel() else 0.0
    bound = MARGIN * max(e32, EPS32 * S)
    return bool(torch.isfinite(got).all()) and err <= bound, err, bound
