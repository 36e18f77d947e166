"""``SpeakerEncoder`` of the boundary (reference: /root/reference/model/modules/audio.py:110-150).

Holds the ``speaker_encoder.*`` checkpoint tensors (3-layer LSTM(256) + Linear) so demo-style loaders
(``demo.py:33-43``: ``SpeakerEncoder(state_dict=...)`` then ``.inference(audios)``) keep working, and runs
``inference`` on the device through ``l2s_speaker_encoder_fwd``: 40-band mel front-end (DFT and filterbank as GEMMs: the
fp32 MFMA kernel, except that the DFT product moves to the split-bf16 kernel - fp32 operands as three bf16 planes, fp32-grade
sums - from 3 969 frames per call at the default ``gemm_x3`` = 1, and that a model with ``infer_bf16`` rounds the operands of both
to bf16), three LSTM layers on the batch-row LSTM kernel, Linear + ReLU + L2 normalisation.
``inference(x, audio_lengths=...)`` and ``inference_packed(packed)`` run the same tower over clips of UNEQUAL length
(``l2s_speaker_encoder_packed``): every clip's embedding is the one it has alone - nothing past a clip's own end is read, its last
frames reflect at its own end and the recurrence stops at its own last frame - where the plain call, like the reference, runs the
whole batch to the padded length (a shorter clip's embedding then depends on its padding).  Rows travel in the time-major compact
layout of a PackedSequence; the same bits as the solo call up to 96 clips and 3 968 frames per call, to rounding beyond.
The mel front-end restates torchaudio 0.9's published algorithm (third-party, absent here): parity UNPINNED for
that piece; the LSTM/Linear tail is checked against ``torch.nn.LSTM`` in the tests.
"""
import torch

from ... import native, statespec
from ._tree import NativeBacked, ParamTree


class SpeakerEncoder(ParamTree, NativeBacked):
    _key_prefix = "speaker_encoder."

    def __init__(self, state_dict=None):
        ParamTree.__init__(self, statespec.speaker_encoder_spec(""), key_prefix="speaker_encoder.")
        self._init_native()
        for p in self.parameters():
            p.requires_grad_(False)
        if state_dict is not None:
            self.load_state_dict(state_dict, strict=True)

    def inference(self, x: torch.Tensor, audio_lengths=None) -> torch.Tensor:
        """audio (B, n_samples) at 16 kHz -> (B,256) non-negative unit-norm embedding.  ``audio_lengths`` (a host tensor or list of B sample
        counts, each in (200, n_samples]): row b is then the embedding of ``x[b, :audio_lengths[b]]`` alone - nothing past a clip's own end is
        read (``l2s_speaker_encoder_packed`` with offsets b * n_samples).  The lengths stay on the host: no device sync."""
        if self.training:
            self.eval()
        with torch.no_grad():
            if audio_lengths is None:
                return self.native_model().speaker_encoder_fwd(x)
            if x.dim() != 2:
                raise ValueError(f"audio must be (B, n_samples), got {tuple(x.shape)}")
            B, N = x.shape
            lens = native._host_ints(audio_lengths, "audio_lengths")
            if len(lens) != B:
                raise ValueError(f"audio_lengths must hold one length per clip ({B}), got {len(lens)}")
            bad = [(b, n) for b, n in enumerate(lens) if n > N]
            if bad:
                raise ValueError(f"audio_lengths beyond n_samples = {N}: " + ", ".join(f"clip {b}: {n}" for b, n in bad))
            return self.native_model().speaker_encoder_packed(x, [b * N for b in range(B)], lens)

    def inference_packed(self, packed, offsets=None, samples=None) -> torch.Tensor:
        """Waveforms back to back in one device buffer -> (B,256) embeddings in call order, each what ``inference`` gives for that clip alone.
        ``packed``: a ``datasets.PackedAudio`` (what ``device_collate_fn_pad_raw`` and ``LRW(raw_audio=True)`` hand over), or its device buffer
        with the host ``offsets`` / ``samples`` given separately.  No padded copy is built."""
        if offsets is None and samples is None:      # a PackedAudio: its (pinned) host buffer goes over as it is
            packed, offsets, samples = packed.data.to(next(self.parameters()).device, non_blocking=True), packed.offsets, packed.samples
        elif offsets is None or samples is None:
            raise ValueError("pass a PackedAudio, or a device buffer with both offsets and samples")
        if self.training:
            self.eval()
        with torch.no_grad():
            return self.native_model().speaker_encoder_packed(packed, offsets, samples)

    def forward(self, utterances, hidden_init=None):
        raise NotImplementedError("only SpeakerEncoder.inference (the frozen, eval-mode use in demo.py:84) is built on the HIP path")
