"""The model-facing halves of the reference's caller loops, without their I/O:

  * ``demo_clips`` / ``demo_clip`` - demo.py:60-90: per clip, speaker embedding from the VOICE tower (``--encoding voice``), a
                         supplied one or the model's FACE tower (``encoding="face"``, ``--encoding face``), ``net.inference(..., return_attention_map=True)``, truncate to ``output_lengths[0]``.
  * ``evaluate_mels`` / ``evaluate_net`` - evaluate.py:22-51: ``net(..., tf_ratio=1)[1]`` in eval mode over collated batches.
  * ``train_iterations`` - train.py:150-193.

The inference-side loops run on the GROUPED path by default: the loader's batches are prefetched ``group`` at a time into one launch chain
(``l2s_inference_multi`` / ``l2s_forward_eval_multi``) with ``n_inflight`` chains on the GPU (``Lip2Speech.inference_many`` /
``forward_many`` over ``parallel.InflightPool.imap``); results come back in loader order, each bit-identical to the single-batch call.

The reference then vocodes the mels (InverseMelScale + Griffin-Lim, torchaudio) and scores ESTOI (pystoi); both are
third-party, stochastic and out of scope here - these functions return the mels.

``honour_lengths=True`` (off by default, as the reference ignores lengths): the loader's ``video_lengths`` are passed on to the length-masked entry
points (``l2s_inference_masked`` / ``l2s_forward_eval_masked``), and on the voice route the batch's audio lengths go to the speaker tower
(``SpeakerEncoder.inference(audios, audio_lengths=...)``, ``l2s_speaker_encoder_packed``), so a clip's output no longer depends on what it was
padded to or batched with - neither through the video nor through the embedding that conditions every decoder stage.  By default the batches then run
one masked call each, in loader order; with ``group_lengths=True`` as well, batches of unequal length share launch chains as ragged groups:
``demo_clips`` through ``l2s_inference_ragged`` (``Lip2Speech.inference_many_lengths``), ``evaluate_mels`` / ``evaluate_net`` through
``l2s_forward_eval_ragged`` (``Lip2Speech.forward_many_lengths``), where the batches differ in their mel length as well.
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

from . import native


def demo_clip(net, batch, speaker_encoder=None, speaker_embedding: Optional[torch.Tensor] = None, device="cuda", encoding: str = "voice",
              early_stop: bool = False, honour_lengths: bool = False, persist_frames: int = 0, persist_masked: int = 0):
    """``batch`` = one item of ``DataLoader(ds, batch_size=1, collate_fn=test_collate_fn_pad)`` (one iteration of demo.py:60-90): the direct
    ``net.inference`` call, which for one clip takes the library's latency form (the decode loop as one persistent launch, option "persist_decode") -
    a single clip has no grouping to stay consistent with; ``demo_clips`` streams a whole loader through the grouped path instead.
    ``encoding="face"`` (demo.py ``--encoding face``): no embedding is passed, the model takes it from its face tower (``net.vgg_face``).
    ``early_stop``: the decode loop ends once the clip has stopped (model option "early_stop", set on ``net`` for this call and after); the
    returned mel and attention are already truncated to ``output_lengths[0]`` and are the same either way.
    ``honour_lengths``: the batch's ``video_lengths`` go to ``net.inference(video_lengths=...)`` (a batch of several padded clips).
    ``persist_frames``: 0 leaves the model's option "persist_frames" alone (32 unless set); a positive value sets it on ``net`` for this call and
    after - above 32, clips of up to that many frames (80 at the most: a 75-frame GRID clip) take the latency form too (include/l2s.h).
    ``persist_masked``: 0 leaves the model's option "persist_masked" alone (0 unless set: a ``honour_lengths`` call takes the launch-per-phase
    route); a positive value sets it on ``net`` for this call and after - a ``honour_lengths`` batch of up to four clips inside the envelope
    of "persist_decode" / "persist_frames" then takes the latency form too, each clip at its own length."""
    _check_encoding(encoding)
    _set_persist_frames(net, persist_frames)
    _set_persist_masked(net, persist_masked)
    if encoding == "voice" and speaker_embedding is None and speaker_encoder is None:
        raise ValueError("pass a SpeakerEncoder (voice route) or a speaker_embedding")
    (videos, vlen), (audios, alen), _, face_crops, _ = batch
    with torch.no_grad():
        emb = _voice_embedding(encoding, speaker_encoder, speaker_embedding, audios, device, alen if honour_lengths else None)
        face_crops = face_crops.to(device, non_blocking=True) if encoding == "face" else face_crops
        mel, lengths, attn = net.inference(videos.to(device, non_blocking=True), face_crops, speaker_embedding=emb, return_attention_map=True,
                                           early_stop=bool(early_stop), video_lengths=vlen if honour_lengths else None)
    n = int(lengths[0])                                  # synchronises: a timed-out persistent launch is reported here, not handed on as NaN
    native.check_persist_timeouts()
    return mel[:1, :, :n], lengths, attn[:, :n]


def demo_clips(net, batches: Iterable, speaker_encoder=None, speaker_embedding: Optional[torch.Tensor] = None, device="cuda",
               group: int = 8, n_inflight: int = 3, encoding: str = "voice", early_stop: bool = False, honour_lengths: bool = False,
               persist_frames: int = 0, persist_masked: int = 0, group_lengths: bool = False):
    """demo.py:60-90 over a whole loader: per clip the speaker embedding from the VOICE tower (``--encoding voice``) or a supplied one,
    ``net.inference(..., return_attention_map=True)``, truncation to ``output_lengths[0]``.  The clips are advanced ``group`` per launch
    chain with ``n_inflight`` chains on the GPU (``Lip2Speech.inference_many``); yields ``(mel, lengths, attention)`` per clip, in order.
    ``encoding="face"``: the embedding comes from the model's face tower instead.  ``early_stop``: every group's decode loop ends once all of
    its clips have stopped (model option "early_stop", set once on ``net`` before the chains start); the yielded tensors are the same.
    ``honour_lengths``: every batch goes through ``demo_clip`` with its ``video_lengths``, one masked call per batch.
    ``group_lengths`` (with ``honour_lengths``; off by default): the batches - whatever their B and T - run ``group`` per launch chain as ragged
    groups instead (``Lip2Speech.inference_many_lengths``, ``l2s_inference_ragged``): the same clips out, each as it would come out alone.
    ``persist_frames``: as in ``demo_clip``, set once on ``net`` before the first clip (grouped calls themselves never take the persistent
    forms; the option is the model's and holds for its later single-batch calls).
    ``persist_masked``: as in ``demo_clip``, set once on ``net`` before the first clip: with ``honour_lengths`` every batch still goes through
    ``demo_clip``, and its masked call takes the persistent forms where it is inside their envelope (masked calls never do without it)."""
    _check_encoding(encoding)
    _set_persist_frames(net, persist_frames)
    _set_persist_masked(net, persist_masked)
    if encoding == "voice" and speaker_embedding is None and speaker_encoder is None:
        raise ValueError("pass a SpeakerEncoder (voice route) or a speaker_embedding")
    if group_lengths and not honour_lengths:
        raise ValueError("group_lengths groups the length-honouring calls: pass honour_lengths=True as well")
    if honour_lengths and not group_lengths:
        for batch in batches:
            yield demo_clip(net, batch, speaker_encoder, speaker_embedding, device, encoding, early_stop, honour_lengths=True)
        return
    if honour_lengths:
        def ragged_calls():
            for (videos, vlen), (audios, alen), _, face_crops, _ in batches:
                with torch.no_grad():
                    emb = _voice_embedding(encoding, speaker_encoder, speaker_embedding, audios, device, alen)
                yield videos, face_crops, emb, True, {"video_lengths": vlen}

        for mel, lengths, attn in net.inference_many_lengths(ragged_calls(), group=group, n_inflight=n_inflight, early_stop=bool(early_stop)):
            n = int(lengths[0])
            yield mel[:1, :, :n], lengths, attn[:, :n]
        return

    def calls():
        for (videos, _), (audios, _), _, face_crops, _ in batches:
            with torch.no_grad():
                emb = _voice_embedding(encoding, speaker_encoder, speaker_embedding, audios, device)
            yield videos, face_crops, emb, True

    for mel, lengths, attn in net.inference_many(calls(), group=group, n_inflight=n_inflight, early_stop=bool(early_stop)):
        n = int(lengths[0])
        yield mel[:1, :, :n], lengths, attn[:, :n]


def _set_persist_frames(net, persist_frames: int) -> None:
    """Model option "persist_frames" (include/l2s.h): 0 leaves the model's value alone."""
    if persist_frames:
        net.native_model().set_option("persist_frames", int(persist_frames))


def _set_persist_masked(net, persist_masked: int) -> None:
    """Model option "persist_masked" (include/l2s.h): 0 leaves the model's value alone."""
    if persist_masked:
        net.native_model().set_option("persist_masked", int(persist_masked))


def _check_encoding(encoding: str) -> None:
    if encoding not in ("voice", "face"):
        raise ValueError(f"encoding must be 'voice' or 'face' (demo.py --encoding), got {encoding!r}")


def _voice_embedding(encoding, speaker_encoder, speaker_embedding, audios, device, audio_lengths=None):
    """The embedding a caller passes on: none on the face route (the model's face tower computes it), else the supplied one or the voice tower's.
    ``audio_lengths`` (the ``honour_lengths`` callers pass the batch's): the tower runs each clip over its own samples only
    (``SpeakerEncoder.inference(audios, audio_lengths=...)``), so the embedding of a padded clip is the one it has alone."""
    if encoding == "face":
        return None
    if speaker_embedding is not None:
        return speaker_embedding
    if speaker_encoder is None:
        return None
    if audio_lengths is not None:
        return speaker_encoder.inference(audios.to(device, non_blocking=True), audio_lengths=audio_lengths)
    return speaker_encoder.inference(audios.to(device, non_blocking=True))


def _evaluate_outputs(net, batches: Iterable, speaker_encoder, device, group: int, n_inflight: int, encoding: str = "voice",
                      honour_lengths: bool = False, group_lengths: bool = False):
    """The eval-mode ``net(..., tf_ratio=1)`` of evaluate.py:32-38 for every collated batch (``train_collate_fn_pad`` layout), on the grouped
    path: yields ``(batch, outputs)`` in loader order.  ``honour_lengths``: one ``net(...)`` call per batch with the model's
    ``honour_video_lengths`` switched on for the loop (``l2s_forward_eval_masked``).  ``group_lengths`` (with ``honour_lengths``; off by default):
    the batches - whatever their B, T and mel length - run ``group`` per launch chain as ragged groups instead
    (``Lip2Speech.forward_many_lengths``, ``l2s_forward_eval_ragged``): the same outputs, every clip as it would come out alone."""
    if group_lengths and not honour_lengths:
        raise ValueError("group_lengths groups the length-honouring calls: pass honour_lengths=True as well")
    if honour_lengths and group_lengths:
        kept = []

        def ragged_calls():
            for batch in batches:
                (videos, vlen), (audios, alen), (melspecs, mlen, _gate), face_crops = batch
                kept.append(batch)
                with torch.no_grad():
                    emb = _voice_embedding(encoding, speaker_encoder, None, audios, device, alen)
                yield videos, face_crops, audios, melspecs, vlen, alen, mlen, 1, {"speaker_embedding": emb}

        for out in net.forward_many_lengths(ragged_calls(), group=group, n_inflight=n_inflight):
            yield kept.pop(0), out
        return
    if honour_lengths:
        was = net.honour_video_lengths
        net.honour_video_lengths = True
        try:
            for batch in batches:
                (videos, vlen), (audios, alen), (melspecs, mlen, _gate), face_crops = batch
                with torch.no_grad():
                    emb = _voice_embedding(encoding, speaker_encoder, None, audios, device, alen)
                    yield batch, net(videos, face_crops, audios, melspecs, vlen, alen, mlen, 1, speaker_embedding=emb)
        finally:
            net.honour_video_lengths = was
        return
    kept = []

    def calls():
        for batch in batches:
            (videos, vlen), (audios, alen), (melspecs, mlen, _gate), face_crops = batch
            kept.append(batch)
            with torch.no_grad():
                emb = _voice_embedding(encoding, speaker_encoder, None, audios, device)
            yield videos, face_crops, audios, melspecs, vlen, alen, mlen, 1, {"speaker_embedding": emb}

    for out in net.forward_many(calls(), group=group, n_inflight=n_inflight):
        yield kept.pop(0), out


def evaluate_mels(net, batches: Iterable, speaker_encoder=None, device="cuda", group: int = 8, n_inflight: int = 3,
                  encoding: str = "voice", honour_lengths: bool = False, group_lengths: bool = False) -> List[torch.Tensor]:
    """Post-net mels of ``net(..., tf_ratio=1)[1]`` for every collated batch (``train_collate_fn_pad`` layout; evaluate.py:32-38), ``group``
    loader batches per launch chain (``l2s_forward_eval_multi``), ``n_inflight`` chains in flight.  ``honour_lengths`` / ``group_lengths``: as in
    ``_evaluate_outputs`` - one masked call per batch, or ragged groups of ``group`` batches (``l2s_forward_eval_ragged``)."""
    was_training = net.training
    net.eval()
    try:
        return [out[1] for _, out in _evaluate_outputs(net, batches, speaker_encoder, device, group, n_inflight, encoding, honour_lengths, group_lengths)]
    finally:
        net.train(was_training)


def evaluate_net(net, batches: Iterable, speaker_encoder=None, device="cuda", max_iters: int = 256, sampling_rate: int = None,
                 group: int = 8, n_inflight: int = 3, timings: Optional[dict] = None, vocoder_backend: str = "auto", metric: str = "auto",
                 encoding: str = "voice", honour_lengths: bool = False, group_lengths: bool = False, vocode_lengths: bool = False,
                 vocoder_generator=None) -> float:
    """Mean ESTOI of the vocoded predictions against the ground-truth audio (reference: evaluate.py:22-51): `net(..., tf_ratio=1)[1]`
    -> `MelSpec2Audio` (InverseMelScale + Griffin-Lim, `max_iters` each) -> `stoi(gt, pred, fs, extended=True)` per clip.  Vocoder and
    metric are restatements of third-party algorithms (parity unpinned); the mels come from the HIP path, `group` loader batches per launch
    chain, and the next groups' chains run while this thread vocodes and scores.  `timings` (a dict) receives the wall seconds spent waiting
    for the model, in the vocoder and in the metric.  `encoding="face"`: the speaker embedding comes from the model's face tower.
    `honour_lengths` / `group_lengths`: as in `evaluate_mels`.
    `vocode_lengths` (with `honour_lengths`; off by default): the tail honours the lengths too (`_evaluate_net_vocode_lengths`) - clip b of a batch is vocoded
    over its own `melspec_lengths[b]` frames and scored over its own samples against its own ground truth, as `demo.py` treats a clip, and a pass holds
    up to `group` batches whatever their mel and audio widths.  `vocoder_generator` (that route only): the generator the vocoder's start iterates are
    drawn from, clip by clip in loader order - with it a clip's score depends on neither its batch nor its pass; None draws from the device's default
    generator, which the model's Gumbel noise shares."""
    _check_encoding(encoding)
    if group_lengths and not honour_lengths:
        raise ValueError("group_lengths groups the length-honouring calls: pass honour_lengths=True as well")
    if vocode_lengths and not honour_lengths:
        raise ValueError("vocode_lengths vocodes and scores every clip at its own length: pass honour_lengths=True as well")
    if vocode_lengths:
        return _evaluate_net_vocode_lengths(net, batches, speaker_encoder, device, max_iters, sampling_rate, group, n_inflight, timings, vocoder_backend, metric,
                                            encoding, group_lengths, vocoder_generator)
    import time
    from .datasets.spectrograms import MelSpec2Audio
    from .hparams import create_hparams
    from . import native
    from .metrics import estoi_device, stoi
    hp = create_hparams()
    fs = sampling_rate or hp.sampling_rate
    vocoder = MelSpec2Audio(hp, max_iters=max_iters, backend=vocoder_backend).to(device)
    scores = []
    was_training = net.training
    net.eval()
    t = {"model_wait_s": 0.0, "vocoder_s": 0.0, "estoi_s": 0.0, "clips": 0}
    def vocode_and_score(pending):
        """One vocoder pass over the mels of up to `group` loader batches, then ESTOI per clip.  On the device path (`metric="hip"`, default
        where the shapes allow: vocoder.hip) the vocoder is three launches per pass (plus one per Griffin-Lim iteration past 121 mel frames) and the metric one block per clip - the predictions never
        leave the GPU, one (N,) score vector comes back per group; `metric="host"` scores with the numpy restatement like the reference."""
        t1 = time.perf_counter()
        same = all(m.shape[0] == pending[0][1].shape[0] for _, m in pending)
        if same:        # InverseMelScale's SGD normalises by the call's own B*L: the loader batches stay separate calls inside the one pass
            pred_dev = vocoder(torch.cat([m for _, m in pending], dim=0), rows_per_call=pending[0][1].shape[0])
        else:
            pred_dev = torch.cat([vocoder(m) for _, m in pending], dim=0)
        n = min(min(a.shape[1] for a, _ in pending), pred_dev.shape[1])      # the device branch only (all audio lengths equal there)
        on_device = metric != "host" and pred_dev.is_cuda and all(a.shape[1] == pending[0][0].shape[1] for a, _ in pending) and \
            -(-n * 10000 // fs) <= native.ESTOI_MAX_SAMPLES
        if metric == "hip" and not on_device:
            raise RuntimeError(f"evaluate_net(metric='hip'): needs device predictions and clips of at most {native.ESTOI_MAX_SAMPLES} samples at 10 kHz (4.8 s)")
        if on_device:
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            gt_dev = torch.cat([a[:, :n] for a, _ in pending], dim=0).to(pred_dev.device, non_blocking=True).float().contiguous()
            scores.extend(float(v) for v in estoi_device(gt_dev, pred_dev[:, :n].contiguous(), fs).cpu())
            native.check_persist_timeouts()
            row = gt_dev.shape[0]
        else:
            pred = pred_dev.cpu().numpy()
            t2 = time.perf_counter()
            row = 0
            for audios, m in pending:      # per loader batch, like the reference's loop: a batch's score does not depend on which batches share its group
                gt = audios.numpy() if not audios.is_cuda else audios.cpu().numpy()
                n_b = min(gt.shape[1], pred.shape[1])
                for i in range(gt.shape[0]):
                    scores.append(stoi(gt[i, :n_b], pred[row + i, :n_b], fs, extended=True))
                row += gt.shape[0]
        t3 = time.perf_counter()
        t["vocoder_s"] += t2 - t1
        t["estoi_s"] += t3 - t2
        t["clips"] += row

    try:
        with torch.no_grad():
            t0 = time.perf_counter()
            pending = []
            for batch, out in _evaluate_outputs(net, batches, speaker_encoder, device, group, n_inflight, encoding, honour_lengths, group_lengths):
                mel = out[1]
                # a pass holds batches of one mel shape AND one audio width: batches padded to different audio lengths are then scored per
                # equal-width run (on the device where the metric runs there) - a batch's score does not depend on which batches share its group
                if pending and (len(pending) == max(1, group) or pending[0][1].shape[1:] != mel.shape[1:] or
                                pending[0][0].shape[1] != batch[1][0].shape[1]):
                    t["model_wait_s"] += time.perf_counter() - t0
                    vocode_and_score(pending)
                    pending = []
                    t0 = time.perf_counter()
                pending.append((batch[1][0], mel))
            t["model_wait_s"] += time.perf_counter() - t0
            if pending:
                vocode_and_score(pending)
    finally:
        net.train(was_training)
    if timings is not None:
        timings.update(t)
    return sum(scores) / max(1, len(scores))


def _evaluate_net_vocode_lengths(net, batches, speaker_encoder, device, max_iters, sampling_rate, group, n_inflight, timings, vocoder_backend, metric,
                                 encoding, group_lengths, generator) -> float:
    """`evaluate_net(honour_lengths=True, vocode_lengths=True)`: the model half as `_evaluate_outputs` runs it; then, per pass of up to `group` loader batches
    (whatever their shapes), ONE ragged vocoder call (`MelSpec2Audio.forward(lengths=...)`: `l2s_inverse_mel_ragged` + `l2s_griffin_lim_ragged`) over every
    clip's own L_b = `melspec_lengths[b]` frames and ONE ragged metric call (`estoi_device(lengths=...)`: `l2s_estoi_ragged`) over every clip's own
    n_b = min(audio_lengths[b], hop (L_b - 1)) samples.  Each clip is vocoded and scored as it would be alone, so its score does not depend on which clips
    share its pass.  `metric="host"`: the numpy `stoi` scores the same per-clip slices.  `timings` also receives the per-clip scores ("scores")."""
    import time
    from .datasets.spectrograms import MelSpec2Audio
    from .hparams import create_hparams
    from .metrics import FS, estoi_device, stoi
    hp = create_hparams()
    fs = sampling_rate or hp.sampling_rate
    vocoder = MelSpec2Audio(hp, max_iters=max_iters, backend=vocoder_backend).to(device)
    scores = []
    t = {"model_wait_s": 0.0, "vocoder_s": 0.0, "estoi_s": 0.0, "clips": 0}

    def vocode_and_score(pending):
        t1 = time.perf_counter()
        mlens = [int(v) for _, _, mlen, _ in pending for v in mlen]
        n_clips, l_max = len(mlens), max(mlens)
        mel = pending[0][3].new_zeros(n_clips, pending[0][3].shape[1], l_max)       # the pass's clips in one padded tensor: what pads it is never read
        row = 0
        for _, _, _, m in pending:
            w = min(m.shape[2], l_max)
            mel[row: row + m.shape[0], :, :w] = m[:, :, :w]
            row += m.shape[0]
        pred_dev = vocoder(mel, generator=generator, lengths=mlens)
        alens = [int(v) for _, alen, _, _ in pending for v in alen]
        n = [min(a, vocoder.hop * (L - 1)) for a, L in zip(alens, mlens)]
        on_device = metric != "host" and pred_dev.is_cuda and max(-(-v * FS // fs) for v in n) <= native.ESTOI_MAX_SAMPLES
        if metric == "hip" and not on_device:
            raise RuntimeError(f"evaluate_net(metric='hip'): needs device predictions and clips of at most {native.ESTOI_MAX_SAMPLES} samples at 10 kHz (4.8 s)")
        pitch = max(n)
        if on_device:
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            gt_dev = pred_dev.new_zeros(n_clips, pitch)
            row = 0
            for audios, _, _, _ in pending:
                w = min(audios.shape[1], pitch)
                gt_dev[row: row + audios.shape[0], :w] = audios[:, :w].to(pred_dev.device, non_blocking=True)
                row += audios.shape[0]
            scores.extend(float(v) for v in estoi_device(gt_dev, pred_dev[:, :pitch].contiguous(), fs, lengths=n).cpu())
            native.check_persist_timeouts()
        else:
            pred = pred_dev.cpu().numpy()
            t2 = time.perf_counter()
            row = 0
            for audios, _, _, _ in pending:
                gt = audios.numpy() if not audios.is_cuda else audios.cpu().numpy()
                for i in range(gt.shape[0]):
                    scores.append(stoi(gt[i, :n[row + i]], pred[row + i, :n[row + i]], fs, extended=True))
                row += gt.shape[0]
        t3 = time.perf_counter()
        t["vocoder_s"] += t2 - t1
        t["estoi_s"] += t3 - t2
        t["clips"] += n_clips

    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            t0 = time.perf_counter()
            pending = []
            for batch, out in _evaluate_outputs(net, batches, speaker_encoder, device, group, n_inflight, encoding, True, group_lengths):
                if len(pending) == max(1, group):       # nothing else ends a pass: batches of any mel and audio width share it
                    t["model_wait_s"] += time.perf_counter() - t0
                    vocode_and_score(pending)
                    pending = []
                    t0 = time.perf_counter()
                pending.append((batch[1][0], batch[1][1], batch[2][1], out[1]))
            t["model_wait_s"] += time.perf_counter() - t0
            if pending:
                vocode_and_score(pending)
    finally:
        net.train(was_training)
    if timings is not None:
        timings.update(t)
        timings["scores"] = list(scores)
    return sum(scores) / max(1, len(scores))


def vocode_clips(mels, max_iters: int = 256, generator=None, backend: str = "auto"):
    """The vocoder of demo.py over the clips `demo_clips` yields: `mels` a list of (1, n_mels, n_i) log-mels of unequal length -> a list of (hop (n_i - 1),)
    waveforms from ONE ragged vocoder pass (`MelSpec2Audio.forward(lengths=...)`), each what `MelSpec2Audio(max_iters=max_iters, backend=backend)(mel_i,
    generator)` returns for the clips in list order on the same generator."""
    from .datasets.spectrograms import MelSpec2Audio
    mels = list(mels)
    if not mels:
        return []
    lengths = [int(m.shape[-1]) for m in mels]
    vocoder = MelSpec2Audio(max_iters=max_iters, backend=backend).to(mels[0].device)
    padded = mels[0].new_zeros(len(mels), mels[0].shape[-2], max(lengths))
    for i, m in enumerate(mels):
        padded[i, :, :lengths[i]] = m.reshape(m.shape[-2], lengths[i])
    with torch.no_grad():
        wave = vocoder(padded, generator=generator, lengths=lengths)
    return [wave[i, :vocoder.hop * (n - 1)] for i, n in enumerate(lengths)]


def reconstruction_losses(outputs, targets) -> dict:
    """`Loss.forward` (train_utils/losses.py:35-79) on torch tensors, attached to autograd: KLD of the content distribution against the
    uniform one, MSE of the pre- and (x10) post-net mels, BCE-with-logits of the stop tokens."""
    import torch.nn.functional as F
    mel_target, gate_target = targets
    mel, mel_post, stop, qy = outputs[0], outputs[1], outputs[2], outputs[5]
    return {"KLD": torch.sum(qy * torch.log(qy * qy.shape[-1] + 1e-20), dim=-1).mean(),
            "mel_loss": F.mse_loss(mel, mel_target),
            "postnet_mel_loss": 10 * F.mse_loss(mel_post, mel_target),
            "gate_loss": F.binary_cross_entropy_with_logits(stop.reshape(-1, 1), gate_target.reshape(-1, 1))}


def train_iterations(net, batches: List, n_iters: int, speaker_encoder=None, tf_ratio: float = 0.0, lr: float = 1e-4, weight_decay: float = 1e-6,
                     grad_clip: float = 1.0, fused_optimizer: bool = True, device="cuda", bf16: bool = False,
                     encoding: str = "voice", honour_lengths: bool = False, honour_mel_lengths: bool = False) -> List[dict]:
    """The model-facing half of `train.py`'s loop (train.py:102-104,150-193): `net.train()`; cycle through the collated batches
    (`tf_ratio += 0.1` every 10 epochs); forward -> 4-term loss -> `backward()` -> gradient all-reduce when a process group is up
    (one process per GPU) -> clip at `grad_clip` -> AdamW(amsgrad) on the decoder and encoder groups.  Returns the per-iteration loss
    log (python floats; the `.item()` calls are this loop's only host synchronisations, like the reference's `loss_log`).
    `bf16=True`: the training entry points run their GEMMs with bf16 operands (option "train_bf16", include/l2s.h).  `encoding="face"`: the
    speaker embedding comes from the model's face tower (train.py's own call passes none); it is a constant of the step, as in the reference.
    `honour_lengths=True` (off by default, as the reference ignores lengths): the batches are ZERO-padded and their `video_lengths` go to the
    length-masked training entry points (`honour_video_lengths` and `train_video_lengths` switched on for the loop; include/l2s.h "training with
    per-clip video lengths") - every clip is encoded, attended to and differentiated as it would be alone.  Those entry points run on running
    statistics, so the loop keeps the model in eval() mode - every BatchNorm frozen, as when fine-tuning - and draws the five dropout sites itself
    (`training.draw_dropout`, handed in through `dropout_masks=`); `bf16` is refused with it.
    `honour_mel_lengths=True` (needs `honour_lengths`): the batches' `melspec_lengths` go to the post-net and to the criterion as well (`train_mel_lengths`
    switched on for the loop; include/l2s.h "training with per-clip mel lengths") - every clip's loss covers its own mel frames and content rows, and
    the batch loss is the mean over the clips."""
    _check_encoding(encoding)
    from .losses import Loss
    from .training import AdamWAmsgrad, GradAllReducer, draw_dropout
    if honour_lengths and bf16:
        raise NotImplementedError("honour_lengths: option \"train_bf16\" with video_lengths is not supported (include/l2s.h)")
    if honour_mel_lengths and not honour_lengths:
        raise NotImplementedError("honour_mel_lengths needs honour_lengths: the mel lengths are the other half of the same padding")
    net.train(not honour_lengths)
    switches = (net.honour_video_lengths, net.train_video_lengths, net.train_mel_lengths)
    if honour_lengths:
        net.honour_video_lengths = net.train_video_lengths = True
    if honour_mel_lengths:
        net.train_mel_lengths = True
    flat = net._train_state()
    # reduced-precision training (the reference's switch is hparams.fp16_run = apex O2, train.py:106-107,180-191): here bf16 OPERANDS in the
    # GEMMs / Conv1d stacks of encoder, prologue and post-net on the bf16 matrix cores, fp32 accumulation, fp32 master weights, fp32 loop
    net.native_model().set_option("train_bf16", 1 if bf16 else 0)
    reducer = GradAllReducer(flat.grad)          # no-op without a process group; both optimizer routes reduce (ranks must not diverge)
    # the decoder's buckets (the flat buffer holds the decoder group first) are reduced while the encoder backward still runs: the model's
    # backward calls this hook as soon as every decoder gradient is final (same overlap as bench.py --mode train)
    n_dec_buckets = reducer.buckets_covering(net._n_decoder_elems())
    net.__dict__["_on_decoder_grads"] = lambda: reducer.start(0, n_dec_buckets)
    reconstruction_criterion = Loss()
    if fused_optimizer:
        optim = AdamWAmsgrad(flat, lr=lr, weight_decay=weight_decay)
    else:
        dec, enc = net.trainable_groups()
        optim = torch.optim.AdamW([{"params": dec}, {"params": enc}], lr=lr, weight_decay=weight_decay, amsgrad=True)
    log, epoch, pos = [], 0, 0
    for _ in range(n_iters):
        if pos == len(batches):
            pos, epoch = 0, epoch + 1
            if epoch % 10 == 0:
                tf_ratio += 0.1
        (videos, vlen), (audios, alen), (melspecs, mlen, gates), face_crops = batches[pos]
        pos += 1
        emb = _voice_embedding(encoding, speaker_encoder, None, audios, device)
        drop = draw_dropout(videos.shape[0], videos.shape[2], melspecs.shape[2], device) if honour_lengths else None
        outputs = net(videos.to(device), face_crops.to(device) if face_crops is not None else None, audios.to(device), melspecs.to(device), vlen, alen,
                      mlen, tf_ratio, speaker_embedding=emb, dropout_masks=drop)
        losses = reconstruction_criterion(outputs, (melspecs.to(device), gates.to(device)), dict(), **({"melspec_lengths": mlen} if honour_mel_lengths else {}))
        loss = sum(losses.values())
        optim.zero_grad()
        loss.backward()
        reducer.start(n_dec_buckets)                 # the encoder's buckets; the decoder's are already travelling
        if fused_optimizer:
            grad_norm = optim.step(max_norm=grad_clip, grad_mul=reducer.wait())
            net.mark_weights_changed()
        else:
            mul = reducer.wait()
            if mul != 1.0:
                flat.grad.mul_(mul)                  # average over ranks before the clip (train.py:191 clips the reduced gradient)
            grad_norm = torch.nn.utils.clip_grad_norm_(net.parameters(), grad_clip)
            optim.step()
        rec = {k: float(v.detach()) for k, v in losses.items()}
        rec.update(loss=float(loss.detach()), grad_norm=float(grad_norm), tf_ratio=tf_ratio, epoch=epoch)
        log.append(rec)
    net.__dict__["_on_decoder_grads"] = None
    net.honour_video_lengths, net.train_video_lengths, net.train_mel_lengths = switches
    return log
