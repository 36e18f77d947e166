"""Log-mel target transform (reference: /root/reference/datasets/spectograms.py:41-59).

The reference wraps ``torchaudio.transforms.MelSpectrogram`` (0.9.0: hann window, centre/reflect padding, power 2,
HTK mel scale, no filterbank normalisation) followed by ``log(clamp(x, 1e-5))``.  torchaudio is not available in this
environment, so the same published algorithm is restated on ``torch.stft``; its parity is therefore UNPINNED
 - it produces training targets, it is not on the measured mel-frames/s path.
"""
from __future__ import annotations

import math

import torch

from ..hparams import create_hparams


def mel_filterbank(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> torch.Tensor:
    """Triangular HTK filters, (n_freqs, n_mels), as torchaudio.functional.create_fb_matrix (norm=None)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.min(down, up), min=0.0)


class MelSpectrogram(torch.nn.Module):
    def __init__(self, hparams=None, n_fft=None, hop_length=None, win_length=None, n_mels=None, f_min=None, f_max=None,
                 sample_rate=None, log=True, backend: str = "auto"):
        """`backend`: "hip" = the device kernel behind `l2s_mel_targets` (mel_targets.hip: one wave per frame, wave-level 1024-point FFT, banded
        filterbank sums); "torch" = the restatement on `torch.stft` below (what the kernel is tested against); "auto" = "hip" for fp32 device
        tensors of a supported shape (n_fft = win = 1024, hop 256, at most 128 mel bands, at least 513 samples), else "torch".  CPU tensors always
        take the torch path."""
        super().__init__()
        assert backend in ("auto", "hip", "torch"), backend
        self.backend = backend
        hp = hparams or create_hparams()
        self.n_fft = n_fft or hp.filter_length
        self.hop = hop_length or hp.hop_length
        self.win = win_length or hp.win_length
        self.sr = sample_rate or hp.sampling_rate
        self.log = log
        n_mels = n_mels or hp.n_mel_channels
        f_min = hp.mel_fmin if f_min is None else f_min
        f_max = hp.mel_fmax if f_max is None else f_max
        self.register_buffer("window", torch.hann_window(self.win, periodic=True))
        self.register_buffer("fb", mel_filterbank(self.n_fft // 2 + 1, f_min, f_max, n_mels, self.sr))
        self.fb_nnz = int((self.fb != 0).sum())

    def _use_hip(self, x: torch.Tensor) -> bool:
        ok = (x.is_cuda and x.dtype == torch.float32 and self.fb.dtype == torch.float32 and self.fb.device == x.device and self.n_fft == 1024 and
              self.win == 1024 and self.hop == 256 and self.fb.shape[1] <= 128 and 0 < self.fb_nnz <= 2048 and x.shape[0] > 0 and x.shape[-1] >= 513 and
              not (x.requires_grad and torch.is_grad_enabled()))              # the kernel has no backward: a waveform that wants a gradient keeps torch's
        if self.backend == "hip" and not ok:
            raise RuntimeError("MelSpectrogram(backend='hip'): needs fp32 device tensors (module on the same device), n_fft = win = 1024, hop 256, "
                               "at most 128 mel bands and at least 513 samples per waveform")
        return ok and self.backend in ("auto", "hip")

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        """(..., N) -> (..., n_mels, N // hop + 1)"""
        shape = waveform.shape
        x = waveform.reshape(-1, shape[-1])
        if self._use_hip(x):
            from .. import native
            R, N = x.shape
            x = x.detach().contiguous()                                            # the rows of a contiguous (R, N) tensor ARE waveforms packed back to back
            mel = native.mel_targets(x.reshape(-1), [r * N for r in range(R)], [N] * R, self.fb, self.fb_nnz, log=self.log, want_audio=False)[0]
            return mel.reshape(*shape[:-1], mel.shape[-2], mel.shape[-1])
        spec = torch.stft(x, self.n_fft, hop_length=self.hop, win_length=self.win, window=self.window, center=True,
                          pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        power = spec.real ** 2 + spec.imag ** 2                                   # (B, n_freqs, L)
        mel = torch.matmul(power.transpose(1, 2), self.fb).transpose(1, 2)         # (B, n_mels, L)
        if self.log:
            mel = torch.log(torch.clamp(mel, min=1e-5))
        return mel.reshape(*shape[:-1], mel.shape[-2], mel.shape[-1])


def spectral_de_normalize(x: torch.Tensor) -> torch.Tensor:
    """exp(x): inverse of the log compression of the targets (spectograms.py:24-39, C = 1)."""
    return torch.exp(x)


class MelSpec2Audio(torch.nn.Module):
    """Log-mel -> waveform, the vocoder `evaluate.py` scores with (reference: datasets/spectograms.py:76-95): exp, then
    torchaudio 0.9.0's ``InverseMelScale`` (non-negative least squares of ``mel = spec @ fb`` by SGD, lr 0.1 / momentum 0.9, random
    start, `max_iters` iterations with the 1e-5 / 1e-8 stopping rules) and ``GriffinLim`` (`max_iters` iterations, momentum 0.99,
    random start, power 2).  torchaudio is absent here: both published algorithms are restated on torch ops (torch.stft/istft on the
    device) - PARITY UNPINNED, and stochastic in the reference as well.  Not part of the mel-frames/s path."""

    def __init__(self, hparams=None, max_iters: int = 256, backend: str = "auto"):
        """`backend`: "hip" = the fused device kernels behind `l2s_inverse_mel` / `l2s_griffin_lim` (vocoder.hip: one wave per mel frame for
        the SGD; wave-level FFTs for Griffin-Lim: one block per clip with the waveform in LDS up to 121 frames, one launch per iteration over
        tiles of frames above); "torch" = the same algorithms as ~5 000 torch launches per call (the restatement the kernels are tested
        against); "auto" = "hip" for device tensors of a supported shape (n_fft = win = 1024, hop 256, at least 5 frames per clip), else
        "torch".  Both draw the same random start iterates in the same order."""
        super().__init__()
        hp = hparams or create_hparams()
        self.n_fft, self.hop, self.win, self.sr = hp.filter_length, hp.hop_length, hp.win_length, hp.sampling_rate
        self.max_iters = max_iters
        self.backend = backend
        self.register_buffer("window", torch.hann_window(self.win, periodic=True))
        self.register_buffer("fb", mel_filterbank(self.n_fft // 2 + 1, hp.mel_fmin, hp.mel_fmax, hp.n_mel_channels, self.sr))
        self.fb_nnz = int((self.fb != 0).sum())

    def _use_hip(self, t: torch.Tensor, L: int) -> bool:
        ok = t.is_cuda and self.n_fft == 1024 and self.win == 1024 and self.hop == 256 and L >= 5 and self.fb_nnz <= 2048
        if self.backend == "hip" and not ok:
            raise RuntimeError("MelSpec2Audio(backend='hip'): needs device tensors, n_fft = win = 1024, hop 256 and at least 5 frames per clip")
        return ok and self.backend in ("auto", "hip")

    # -- clips of unequal length (`lengths=`): every clip exactly as the solo call `self(melspec[b:b+1, :, :L_b], generator)` computes it
    @staticmethod
    def _check_lengths(t: torch.Tensor, lengths) -> list:
        lengths = [int(v) for v in lengths]
        if len(lengths) != t.shape[0] or not lengths or min(lengths) < 2 or max(lengths) > t.shape[-1]:
            raise ValueError(f"lengths: one frame count in [2, {t.shape[-1]}] per clip of the batch of {t.shape[0]}, got {lengths}")
        return lengths

    def _use_hip_lengths(self, t: torch.Tensor, lengths) -> bool:
        """The ragged kernels take the call when every clip is inside the solo kernels' envelope (at least 5 frames)."""
        return self._use_hip(t, min(lengths))

    def _draw_init(self, t: torch.Tensor, L: int, generator) -> torch.Tensor:
        return torch.rand(1, L, self.fb.shape[0], device=t.device, dtype=t.dtype, generator=generator)      # what the solo inverse_mel draws

    def _draw_angles(self, t: torch.Tensor, L: int, generator) -> torch.Tensor:
        return torch.rand(1, self.fb.shape[0], L, 2, device=t.device, dtype=t.dtype, generator=generator)   # what the solo griffin_lim draws

    @staticmethod
    def _pad_blocks(flat: torch.Tensor, lengths, rows: int) -> torch.Tensor:
        """Packed per-clip (rows, L_b) blocks -> (N, rows, max L_b), zeros past each clip."""
        out = flat.new_zeros(len(lengths), rows, max(lengths))
        o = 0
        for b, L in enumerate(lengths):
            out[b, :, :L] = flat[o: o + rows * L].view(rows, L)
            o += rows * L
        return out

    def _inverse_mel_lengths(self, mel: torch.Tensor, generator, lengths) -> torch.Tensor:
        """`inverse_mel(lengths=...)`: mel (N, n_mels, L_pad), clip b its first lengths[b] frames -> (N, n_freqs, max L_b), clip b as the solo call on
        `mel[b:b+1, :, :L_b]` computes it (its own gradient scale, loss mean and stopping rules), zeros behind; the start iterates are drawn clip by clip."""
        lengths = self._check_lengths(mel, lengths)
        if self._use_hip_lengths(mel, lengths):
            from .. import native
            init = torch.cat([self._draw_init(mel, L, generator)[0] for L in lengths], dim=0)
            return self._pad_blocks(native.inverse_mel_ragged(mel, lengths, self.fb, self.fb_nnz, init, self.max_iters), lengths, self.fb.shape[0])
        out = mel.new_zeros(len(lengths), self.fb.shape[0], max(lengths))
        for b, L in enumerate(lengths):
            out[b, :, :L] = self.inverse_mel(mel[b:b + 1, :, :L], generator)[0]
        return out

    def _griffin_lim_lengths(self, power_spec: torch.Tensor, generator, lengths) -> torch.Tensor:
        """`griffin_lim(lengths=...)`: power_spec (N, n_freqs, L_pad) -> (N, hop * (max L_b - 1)), clip b as the solo call on `power_spec[b:b+1, :, :L_b]`
        computes it, exact zeros behind its hop * (L_b - 1) samples; the start angles are drawn clip by clip."""
        lengths = self._check_lengths(power_spec, lengths)
        if self._use_hip_lengths(power_spec, lengths):
            from .. import native
            ang = torch.cat([self._draw_angles(power_spec, L, generator).reshape(-1) for L in lengths])
            packed = torch.cat([power_spec[b, :, :L].reshape(-1) for b, L in enumerate(lengths)])
            return native.griffin_lim_ragged(packed, ang, lengths, self.max_iters, None, self.n_fft, self.hop, 0.99)
        out = power_spec.new_zeros(len(lengths), self.hop * (max(lengths) - 1))
        for b, L in enumerate(lengths):
            out[b, :self.hop * (L - 1)] = self.griffin_lim(power_spec[b:b + 1, :, :L], generator)[0]
        return out

    def _forward_lengths(self, melspec: torch.Tensor, generator, lengths) -> torch.Tensor:
        """`forward(lengths=...)`.  A solo call draws its clip's start spectrum, then its start angles: the draws here come in that order, clip by clip, so
        both routes are the loop of solo calls on the same generator - the torch route literally, the kernels in two ragged launch chains."""
        lengths = self._check_lengths(melspec, lengths)
        if self._use_hip_lengths(melspec, lengths):
            from .. import native
            mel = spectral_de_normalize(melspec.to(torch.float32))
            drawn = [(self._draw_init(mel, L, generator)[0], self._draw_angles(mel, L, generator).reshape(-1)) for L in lengths]
            spec = native.inverse_mel_ragged(mel, lengths, self.fb, self.fb_nnz, torch.cat([d[0] for d in drawn], dim=0), self.max_iters)
            return native.griffin_lim_ragged(spec, torch.cat([d[1] for d in drawn]), lengths, self.max_iters, None, self.n_fft, self.hop, 0.99)
        out = torch.zeros(len(lengths), self.hop * (max(lengths) - 1), device=melspec.device, dtype=torch.float32)
        for b, L in enumerate(lengths):
            out[b, :self.hop * (L - 1)] = self(melspec[b:b + 1, :, :L], generator)[0]
        return out

    # -- torchaudio.transforms.InverseMelScale.forward (0.9.0)
    def inverse_mel(self, mel: torch.Tensor, generator=None, rows_per_call: int = None, lengths=None) -> torch.Tensor:
        """mel (B, n_mels, L) power-mel -> power spectrogram (B, n_freqs, L) >= 0.  The reference's loop reads its loss on the host every
        iteration (`new_loss.item()`) for the two stopping rules; here the rules are evaluated on the device and freeze the iterate from the
        stopping iteration on, so the 256 iterations are enqueued without a single host synchronisation and end at the same iterate.
        `rows_per_call`: the rows are G independent calls of that many rows each (several loader batches vocoded in one pass): the loss mean,
        the 1/(B*L) gradient scale and the stopping rules are per call, exactly as G separate calls would have them.
        `lengths` (a host sequence, one frame count per clip; not with `rows_per_call`): every clip is its own call over its own frames (`_inverse_mel_lengths`)."""
        if lengths is not None:
            assert rows_per_call is None, "lengths makes every clip its own call"
            return self._inverse_mel_lengths(mel, generator, lengths)
        N, _, L = mel.shape
        R = rows_per_call or N
        assert N % R == 0, "rows_per_call must divide the batch"
        G = N // R
        target = mel.transpose(1, 2).reshape(G, R * L, -1)                        # (G, R*L, n_mels)
        spec = torch.rand(G, R * L, self.fb.shape[0], device=mel.device, dtype=mel.dtype, generator=generator)
        if self._use_hip(mel, L):
            from .. import native
            return native.inverse_mel(mel, self.fb, self.fb_nnz, spec.reshape(N * L, -1), self.max_iters, rows_per_call=R)
        vel = torch.zeros_like(spec)
        loss = torch.full((G, 1, 1), float("inf"), device=mel.device, dtype=mel.dtype)
        active = torch.ones((G, 1, 1), device=mel.device, dtype=torch.bool)
        fbt = self.fb.t().contiguous()
        for _ in range(self.max_iters):
            diff = target - spec @ self.fb
            new_loss = diff.pow(2).sum(dim=-1).mean(dim=-1).view(G, 1, 1)
            grad = (-2.0 / (R * L)) * (diff @ fbt)                                # d/dspec of the call's mean over (B, L) of the per-frame squared error
            new_vel = 0.9 * vel + grad                                            # torch.optim.SGD(lr=0.1, momentum=0.9)
            new_spec = (spec - 0.1 * new_vel).clamp_(min=0)
            vel = torch.where(active, new_vel, vel)                               # the update of the iteration that meets a rule is still applied
            spec = torch.where(active, new_spec, spec)
            active = active & ~((new_loss < 1e-5) | ((loss - new_loss).abs() < 1e-8))
            loss = new_loss
        return spec.reshape(N, L, -1).transpose(1, 2)

    # -- torchaudio.functional.griffinlim (0.9.0): power 2, momentum 0.99, rand_init
    def griffin_lim(self, power_spec: torch.Tensor, generator=None, lengths=None) -> torch.Tensor:
        if lengths is not None:
            return self._griffin_lim_lengths(power_spec, generator, lengths)
        mag = power_spec.clamp(min=0).sqrt()                                      # (B, n_freqs, L)
        B, _, L = mag.shape
        length = self.hop * (L - 1)
        ang = torch.view_as_complex(torch.rand(*mag.shape, 2, device=mag.device, dtype=mag.dtype, generator=generator))
        if self._use_hip(power_spec, L):
            from .. import native
            return native.griffin_lim(power_spec, ang, self.max_iters, self.n_fft, self.hop, 0.99)
        momentum = 0.99 / (1 + 0.99)
        prev = torch.zeros_like(ang)
        stft = lambda x: torch.stft(x, self.n_fft, self.hop, self.win, self.window, center=True, pad_mode="reflect",      # noqa: E731
                                    normalized=False, onesided=True, return_complex=True)
        istft = lambda z: torch.istft(z, self.n_fft, self.hop, self.win, self.window, length=length)                      # noqa: E731
        for _ in range(self.max_iters):
            rebuilt = stft(istft(mag * ang))
            ang = rebuilt - prev * momentum
            ang = ang / (ang.abs() + 1e-16)
            prev = rebuilt
        return istft(mag * ang)

    def forward(self, melspec: torch.Tensor, generator=None, rows_per_call: int = None, lengths=None) -> torch.Tensor:
        """(B, n_mels, L) log-mel -> (B, hop*(L-1)) waveform.  `rows_per_call`: see `inverse_mel` (Griffin-Lim is per clip anyway).
        `lengths` (a host sequence, one frame count per clip): -> (B, hop * (max L_b - 1)), clip b exactly the solo call `self(melspec[b:b+1, :, :L_b],
        generator)` in a loop over b on the same generator (pad frames are never read), exact zeros behind its hop * (L_b - 1) samples.  With
        backend "auto" the kernels take device tensors when every L_b >= 5 (`l2s_inverse_mel_ragged`, `l2s_griffin_lim_ragged`: two launch chains for
        the whole batch)."""
        if lengths is not None:
            assert rows_per_call is None, "lengths makes every clip its own call"
            return self._forward_lengths(melspec, generator, lengths)
        mel = spectral_de_normalize(melspec.to(torch.float32))
        return self.griffin_lim(self.inverse_mel(mel, generator, rows_per_call), generator)
