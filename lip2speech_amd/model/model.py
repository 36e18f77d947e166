"""``Lip2Speech`` / ``get_network`` - the drop-in boundary (reference: /root/reference/model/model.py:13-72).

``get_network(mode)`` returns an ``nn.Module`` with ``.encoder``, ``.decoder``, ``.vgg_face`` attributes,
``forward(...)`` returning the reference's list of 7 and ``inference(...)`` returning
``(mel, output_lengths[, attention])``, so train.py / evaluate.py / demo.py style callers work unchanged.
``inference`` with a supplied ``speaker_embedding`` runs as ONE native call (``l2s_inference``: encoder,
prologue, 300-step loop and post-net enqueued back to back on the current stream).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from .. import native, statespec
from .modules import Decoder, FaceRecognizer, VideoExtractor
from .modules._tree import NativeBacked

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


class _HipTrainStep(torch.autograd.Function):
    """`Lip2Speech.forward` as ONE autograd node (reference: model.py:20-41 + decoder.py:320-379 under loss.backward(), train.py:184):
    forward runs the HIP kernels with tapes; backward runs the HIP backward (post-net, BPTT through the loop, prologue, encoder) and
    deposits every encoder/decoder parameter gradient in the flat gradient buffer the parameters' `.grad` alias.  `anchor` is any
    parameter of the model - it only makes autograd call `backward`."""

    @staticmethod
    def forward(ctx, anchor, model, video, emb, gumbel, mels, mask, drop, lens=None, mlens=None):
        # lens (`Lip2Speech.train_video_lengths`): the host lengths of a ZERO-padded batch - the three stages that see the video run their *_masked
        # entry points (include/l2s.h "training with per-clip video lengths"), forward and backward.  mlens (`Lip2Speech.train_mel_lengths`): the host mel
        # lengths - the post-net runs its *_masked entry points ("training with per-clip mel lengths"): rows s >= S_b of mel are zeroed, of mel_post zeros
        nm = model.native_model()
        B, _, T, _, _ = video.shape
        S = mels.shape[2]
        drop = drop or {}
        ctx.bn_batch = bool(model.training)                 # nn.Module.train(): batch statistics + running-statistics update (in the bound buffers)
        nm.train_set_bn(ctx.bn_batch)
        pdrop = native.postnet_drop_pack(drop["post"]) if drop.get("post") is not None else None
        vis, _, etape = nm.train_encoder_fwd(video, emb, video_lengths=lens)
        real = None
        if lens is not None:                                # (B,T,1): frames a clip has; the multipliers of its pad rows are never read
            real = (torch.arange(T, device=video.device)[None, :] < torch.as_tensor(list(lens), device=video.device)[:, None]).unsqueeze(2)
        if drop.get("feat") is not None:                    # F.dropout(self.encoder(video_frames), 0.1, self.training), model.py:26
            if real is None:
                vis[:, :, :768] *= drop["feat"]
            else:
                vis[:, :, :768] = torch.where(real, vis[:, :, :768] * drop["feat"], torch.zeros((), device=video.device))
        state, dis, ptape = nm.train_prologue_fwd(vis, emb, gumbel, video_lengths=lens)
        teacher = None
        if mask is not None:
            bos = model.decoder.BOS.detach().to(torch.float32).reshape(1, 1, -1).expand(B, 1, -1)
            teacher = torch.cat([bos, mels.detach().to(torch.float32).permute(0, 2, 1)[:, :S - 1]], dim=1).contiguous()
        (mel, stop, logits), sctx = nm.train_steps_fwd(state, B, T, S, teacher, mask, drop=drop, video_lengths=lens)
        mel_post, post_tape = nm.train_postnet_fwd(mel, pdrop, mel_lengths=mlens)
        ctx.model, ctx.tapes = model, (video, emb, vis, etape, state, ptape, sctx, mel, post_tape, pdrop, drop.get("feat"))
        ctx.lens, ctx.real, ctx.mlens = lens, real, mlens
        ctx.mark_non_differentiable(logits)
        if ctx.bn_batch:
            model._count_batch()
        return mel.permute(0, 2, 1).contiguous(), mel_post, stop.unsqueeze(2), logits, dis

    @staticmethod
    def backward(ctx, dmel_cf, dmel_post, dstop, _dlogits, ddis):
        model = ctx.model
        nm = model.native_model()
        nm.train_set_bn(ctx.bn_batch)
        video, emb, vis, etape, state, ptape, sctx, mel, post_tape, pdrop, fdrop = ctx.tapes
        B, S = mel.shape[0], mel.shape[1]
        flat = model._flat
        # a fused zero_grad() just zeroed the buffer and nothing has written it through torch since (FlatBuffer.cleared_version): nothing to
        # accumulate.  A manual p.grad.add_(), an all-reduce or another graph's backward in between bumps the version -> the accumulate path
        live = model._grads_live() and not flat.is_cleared()
        flat.mark_written()
        prev = flat.grad.clone() if live else None                    # gradient accumulation across backward() calls
        n_dec = model._n_decoder_elems()
        z = lambda g, ref: torch.zeros_like(ref) if g is None else g  # noqa: E731
        wbuf = nm.train_pack_weights(video.device)
        dmel = nm.train_postnet_bwd(mel, z(dmel_post, mel.permute(0, 2, 1)), post_tape, pdrop, mel_lengths=ctx.mlens)
        if dmel_cf is not None:
            dmel += dmel_cf.permute(0, 2, 1)
        sg = nm.train_steps_bwd(sctx, dmel, z(dstop, mel[:, :, :1]).reshape(B, S), wbuf=wbuf)
        dvis = nm.train_prologue_bwd(vis, emb, state, ptape, sg, dcontent_dis=ddis, wbuf=wbuf, video_lengths=ctx.lens)
        if fdrop is not None:
            if ctx.real is None:
                dvis[:, :, :768] *= fdrop
            else:
                dvis[:, :, :768] = torch.where(ctx.real, dvis[:, :, :768] * fdrop, torch.zeros((), device=dvis.device))
        # every decoder gradient is final here (the flat buffer holds the decoder group first): a data-parallel caller's hook starts the
        # all-reduce of those buckets now, under the encoder backward (train.py:184-193's hook point; bench.py --mode train does the same)
        if prev is not None:
            flat.grad[:n_dec] += prev[:n_dec]
        hook = model.__dict__.get("_on_decoder_grads")
        if hook is not None:
            hook()
        nm.train_encoder_bwd(video, dvis, etape, video_lengths=ctx.lens)
        if prev is not None:
            flat.grad[n_dec:] += prev[n_dec:]
        model._attach_grads()
        return (None,) * 10


class Lip2Speech(NativeBacked):
    _key_prefix = ""

    def __init__(self):
        super().__init__()
        self._init_native()
        self.vgg_face = FaceRecognizer()
        self.encoder = VideoExtractor()
        self.decoder = Decoder()
        # Off (the default): `video_lengths` is ignored as in the reference, whatever hparams.mask_padding says (nothing reads that).  On: eval-mode
        # `forward` hands the `video_lengths` it receives to `l2s_forward_eval_masked` - every clip of a ZERO-padded batch then comes out as it would
        # alone (include/l2s.h "per-clip video lengths").  A call that wants gradients raises NotImplementedError unless `train_video_lengths` is on too.
        self.honour_video_lengths = False
        # Off (the default): as above.  On, together with `honour_video_lengths`: a differentiable `forward` hands its `video_lengths` to the
        # l2s_train_*_masked_fwd / _masked_bwd entry points (include/l2s.h "training with per-clip video lengths") - the model that is trained is then the function of
        # the weights that is evaluated and served with lengths honoured.  Running statistics only: the module must be in eval() mode (dropout then
        # comes through `dropout_masks=`); train() mode - batch statistics - is refused by name, as the library refuses it.
        self.train_video_lengths = False
        # Off (the default): the post-net of a differentiable `forward` runs over all S frames of every clip, as in the reference.  On, together with the two
        # switches above: it hands `melspec_lengths` to l2s_train_postnet_masked_fwd / _masked_bwd (include/l2s.h "training with per-clip mel lengths") - a
        # clip's post-net sees zeros past its own last frame, mel_post is zeros there; give the same lengths to `Loss.forward(melspec_lengths=)`.
        # Running statistics only, like `train_video_lengths`: train() mode is refused by name.
        self.train_mel_lengths = False
        # one packed weight blob for the whole path; the sub-modules borrow it while they live inside this model
        self.encoder.__dict__["_native_parent"] = self
        self.decoder.__dict__["_native_parent"] = self

    def _collect_tensors(self):
        sd = self.state_dict(keep_vars=True)
        return {k: v for k, v in sd.items() if k.startswith(("encoder.", "decoder."))}

    # ------------------------------------------------------------------ training state
    def trainable_groups(self):
        """The optimizer's parameter groups as train.py:102-104 builds them: decoder, then encoder."""
        return [list(self.decoder.parameters()), list(self.encoder.parameters())]

    def _train_state(self):
        """Lazy: re-home the decoder/encoder parameters into one flat fp32 buffer (+ a flat gradient buffer) and bind both to the library."""
        if self.__dict__.get("_flat") is None:
            from ..training import FlatBuffer
            flat = FlatBuffer(self.trainable_groups())
            self.__dict__["_flat"] = flat
            names = {id(p): "decoder." + n for n, p in self.decoder.named_parameters()}
            names.update({id(p): "encoder." + n for n, p in self.encoder.named_parameters()})
            self.__dict__["_flat_names"] = [names[id(p)] for p in flat.params]
            grads = {}
            for p, key in zip(flat.params, self._flat_names):
                off = flat.offsets[id(p)]
                grads[key] = flat.grad[off:off + p.numel()].view_as(p)
                p.grad = None
            self.__dict__["_grad_views"] = grads
            # the (re)load below also builds the device-side refresh map (a per-model option: other models keep the cheap load)
            nm = self.__dict__.get("_native") or native.NativeModel()
            nm.set_option("refresh_map", 1)
            self.__dict__["_native"] = nm
            self.__dict__["_native_sig"] = None
            nm = self.native_model()
            bound = {k: p.data for k, p in zip(self._flat_names, flat.params)}
            bound.update({k: v for k, v in self._tensors().items() if k not in bound and v.is_floating_point()})   # buffers: BN statistics, pos_table
            nm.train_bind(bound, grads)
            self.__dict__["_refresh_on_device"] = True
        return self._flat

    def _n_decoder_elems(self) -> int:
        """Elements of the decoder group = the leading range of the flat parameter / gradient buffers."""
        if self.__dict__.get("_n_dec") is None:
            self.__dict__["_n_dec"] = sum(p.numel() for p in self.decoder.parameters())
        return self.__dict__["_n_dec"]

    def _count_batch(self):
        """num_batches_tracked += 1 on every BatchNorm (what nn.BatchNorm does in train mode; the running statistics themselves are updated
        by the kernels)."""
        if self.__dict__.get("_nbt") is None:
            self.__dict__["_nbt"] = [b for n, b in self.named_buffers() if n.endswith("num_batches_tracked") and n.startswith(("encoder.", "decoder."))]
        if self._nbt:
            torch._foreach_add_(self._nbt, 1)

    def _grads_live(self) -> bool:
        return any(p.grad is not None for p in self._flat.params)

    def _attach_grads(self):
        for p, key in zip(self._flat.params, self._flat_names):
            p.grad = self._grad_views[key]

    def _speaker(self, face_frames, speaker_embedding):
        if speaker_embedding is not None:
            return speaker_embedding
        return self.vgg_face.inference(face_frames[:, 0, :, :, :])

    def forward(self, video_frames, face_frames, audio_frames, melspecs, video_lengths, audio_lengths, melspec_lengths,
                tf_ratio, speaker_embedding=None, gumbel_noise=None, dropout_masks=None):
        masked = bool(self.honour_video_lengths) and video_lengths is not None
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.decoder.parameters())
        mel_masked = bool(self.train_mel_lengths) and (self.training or wants_grad)
        if mel_masked:
            if not (self.honour_video_lengths and self.train_video_lengths):
                raise NotImplementedError("train_mel_lengths: needs `honour_video_lengths` and `train_video_lengths` switched on as well (the mel lengths are the "
                                          "other half of the same padding)")
            if self.training:
                raise NotImplementedError("train_mel_lengths: train() mode normalises with batch statistics, and the length-masked post-net runs on running "
                                          "statistics only (batch_stats = 1 with mel_lengths is refused, include/l2s.h); call in eval() mode and hand the "
                                          "dropout multipliers in through dropout_masks=")
            if video_lengths is None or melspec_lengths is None:
                raise ValueError("train_mel_lengths: video_lengths and melspec_lengths are both needed")
        if masked and (self.training or wants_grad):
            if not self.train_video_lengths:
                raise NotImplementedError("honour_video_lengths: a training call takes the length-masked entry points (l2s_train_*_masked_fwd / _masked_bwd, include/l2s.h) only "
                                          "with `train_video_lengths` switched on as well; otherwise use it in eval() mode under torch.no_grad()")
            if self.training:
                raise NotImplementedError("train_video_lengths: train() mode normalises with batch statistics, and the length-masked training entry points "
                                          "run on running statistics only (batch_stats = 1 with video_lengths is refused, include/l2s.h); call in eval() "
                                          "mode and hand the dropout multipliers in through dropout_masks=")
            if not wants_grad:
                raise NotImplementedError("train_video_lengths: no gradient is wanted here; the forward-only length-masked route is eval() mode under torch.no_grad()")
        if wants_grad:
            return self._forward_train(video_frames, face_frames, melspecs, video_lengths, tf_ratio, speaker_embedding, gumbel_noise, dropout_masks,
                                       honour_lengths=masked, melspec_lengths=melspec_lengths if mel_masked else None)
        if self.training:
            # a no_grad call on a train()-mode module: the feature dropout of model.py:26 is live - the staged route through the sub-modules
            video_features = F.dropout(self.encoder(video_frames), 0.1, True)
            emb = self._speaker(face_frames, speaker_embedding)
            vis = native.build_visual(video_features, emb)
            face = emb.unsqueeze(1).expand(-1, vis.shape[1], -1)
            outputs = self.decoder(vis, face, melspecs, video_lengths, melspec_lengths, tf_ratio, gumbel_noise=gumbel_noise)
            return outputs + [video_lengths]
        job = self._forward_job(video_frames, face_frames, melspecs, video_lengths, tf_ratio, speaker_embedding, gumbel_noise)
        out = self.native_model().forward_eval(job["video"], job["emb"], job["gumbel"], job["S"], teacher=job.get("teacher"), teacher_mask=job.get("mask"),
                                               video_lengths=video_lengths if masked else None)
        return job["finish"](out)

    def _forward_job(self, video_frames, face_frames, melspecs, video_lengths, tf_ratio, speaker_embedding=None, gumbel_noise=None):
        """One eval-mode `forward` call as a job of the native path (`l2s_forward_eval`; model.py:23-40 + decoder.py:320-379): the speaker
        embedding, the Gumbel noise (drawn on the device unless supplied) and the scheduled-sampling mask (one host `torch.rand(1)` per
        step) are fixed here, in the reference's order; `finish` shapes the native outputs into the reference's list of 7."""
        dev = self.decoder.BOS.device
        with torch.no_grad():
            video = video_frames.to(dev, non_blocking=True)
            emb = self._speaker(face_frames.to(dev, non_blocking=True) if face_frames is not None else None,
                                speaker_embedding.to(dev, non_blocking=True) if speaker_embedding is not None else None)
            B, _, T, _, _ = video.shape
            S = melspecs.shape[2]
            if gumbel_noise is None:
                gumbel_noise = Decoder.draw_gumbel(B * native.min_T(T), dev)
            mask = Decoder.sampling_mask(S, tf_ratio)
            job = {"entry": "forward", "video": video, "emb": emb, "gumbel": gumbel_noise.to(dev, non_blocking=True), "S": S, "mask": mask}
            if mask is not None:
                job["teacher"] = self.decoder.teacher_frames(melspecs.to(dev, non_blocking=True))
        job["finish"] = lambda o: [o[0], o[1], o[2].unsqueeze(2), emb, o[3], o[4], video_lengths]
        return job

    def _inference_job(self, video_frames, face_frames, speaker_embedding=None, return_attention_map=False, gumbel_noise=None, video_lengths=None):
        """`video_lengths` given: a job of the ragged route (`l2s_inference_ragged`), validated here - before the batch is staged on the device."""
        lens = None
        if video_lengths is not None:
            lens = list(native.video_lengths_array(video_lengths, video_frames.shape[0], video_frames.shape[2]))
        dev = self.decoder.BOS.device
        with torch.no_grad():
            video = video_frames.to(dev, non_blocking=True)
            emb = self._speaker(face_frames.to(dev, non_blocking=True) if face_frames is not None else None,
                                speaker_embedding.to(dev, non_blocking=True) if speaker_embedding is not None else None)
            B, _, T, _, _ = video.shape
            if gumbel_noise is None:
                gumbel_noise = Decoder.draw_gumbel(B * native.min_T(T), dev)
        job = {"entry": "inference", "video": video, "emb": emb, "gumbel": gumbel_noise.to(dev, non_blocking=True),
               "S": self.decoder.hparams.max_decoder_steps, "want_attn": bool(return_attention_map),
               "finish": (lambda o: (o[0], o[1], o[2])) if return_attention_map else (lambda o: (o[0], o[1]))}
        if lens is not None:
            job["entry"], job["video_lengths"] = "inference_ragged", lens
        return job

    # ------------------------------------------------------------------ loader-driven callers: G batches per launch chain, chains in flight
    def pool(self, group: int = 8, n_inflight: int = 3):
        """The `parallel.InflightPool` of this model's weight blob (cached per shape of concurrency)."""
        from ..parallel import InflightPool
        nm = self.native_model()
        pools = self.__dict__.setdefault("_pools", {})
        key = (group, n_inflight)
        if key not in pools or pools[key].model is not nm:      # a re-packed / replaced NativeModel: the old pool (and its blob) is dropped
            pools[key] = InflightPool(model=nm, n_inflight=n_inflight, group=group, device=self.decoder.BOS.device)
        for k in [k for k, v in pools.items() if v.model is not nm]:
            del pools[k]
        return pools[key]

    @staticmethod
    def _call(item):
        """An item of `*_many`: the positional arguments of the single-batch method, optionally followed by a dict of keyword arguments."""
        if isinstance(item, dict):
            return (), item
        item = tuple(item)
        if item and isinstance(item[-1], dict):
            return item[:-1], item[-1]
        return item, {}

    def set_early_stop(self, early_stop: Optional[bool]) -> None:
        """Option "early_stop" of this model's native handle (include/l2s.h): `None` leaves it alone.  The option is per MODEL, not per call: a
        model shared by several threads (`inference_many`'s chains, a serving pool) should set it once, before the threads start."""
        if early_stop is not None:
            self.native_model().set_option("early_stop", 1 if early_stop else 0)

    def inference_many(self, calls, group: int = 8, n_inflight: int = 3, early_stop: Optional[bool] = None):
        """`inference` over a stream of batches - the loop of demo.py:60-90 - with `group` batches advanced per launch chain
        (`l2s_inference_multi`) and `n_inflight` chains on the GPU at once.  `calls` is any iterable (e.g. a generator over a DataLoader) of
        argument tuples `(video_frames, face_frames[, speaker_embedding[, return_attention_map[, gumbel_noise]]])`, optionally ending in a
        dict of keyword arguments; inputs may live on the host (they are copied on the pool's copy stream, one group ahead).  Yields, in
        order, exactly what `inference(*call)` returns for each - bit-identical when the Gumbel noise is supplied.
        `early_stop`: `None` leaves the model's option alone, `True` / `False` sets it ONCE for the model before the first chain starts (every
        chain of the pool drives this one model): the decode loop of a group then ends once all its clips have stopped, and frames at or
        past a clip's length are exact zeros (`inference`)."""
        self.native_model()
        self.set_early_stop(early_stop)
        prep = lambda item: (lambda a, k: self._inference_job(*a, **k))(*self._call(item))      # noqa: E731
        return self.pool(group, n_inflight).imap(calls, prep)

    def inference_many_lengths(self, calls, group: int = 8, n_inflight: int = 3, early_stop: Optional[bool] = None):
        """`inference(..., video_lengths=)` over a stream of batches whose B and T differ - a loader that pads every batch to its own longest clip
        (GRID, AVSpeech, in-the-wild clips) - with `group` batches, at most 256 clips, advanced per launch chain as a ragged group
        (`l2s_inference_ragged`) and `n_inflight` chains on the GPU at once.  `calls`: as for `inference_many`, every item with `video_lengths=` in its
        trailing dict (required: without lengths the batches could not share a chain).  Yields, in order, what `inference(*call)` returns for each:
        every clip as it would come out alone, the encoder run on the real frames only.  `early_stop`: as in `inference_many`."""
        self.native_model()
        self.set_early_stop(early_stop)

        def prep(item):
            a, k = self._call(item)
            if k.get("video_lengths") is None:
                raise ValueError("inference_many_lengths: every call needs video_lengths= (use inference_many for batches whose lengths are ignored)")
            k = {key: v for key, v in k.items() if key != "early_stop"}
            return self._inference_job(*a, **k)
        return self.pool(group, n_inflight).imap(calls, prep)

    def forward_many(self, calls, group: int = 8, n_inflight: int = 3):
        """Eval-mode `forward` over a stream of batches - the loop of evaluate.py:22-51 (`net(..., tf_ratio=1)` per DataLoader batch) - on the
        grouped path (`l2s_forward_eval_multi`).  `calls`: iterable of `forward`'s argument tuples `(video_frames, face_frames, audio_frames,
        melspecs, video_lengths, audio_lengths, melspec_lengths, tf_ratio)`, optionally ending in a dict (`speaker_embedding=`,
        `gumbel_noise=`).  Yields the reference's list of 7 per call, in order, bit-identical to `forward(*call)` under `torch.no_grad()`.
        Batches group when they share shape, S and scheduled-sampling mask (always at tf_ratio = 1: no step is teacher-forced)."""
        if self.training:
            raise RuntimeError("forward_many is the evaluate path: call .eval() first (train() mode trains through forward / backward)")
        if self.honour_video_lengths:
            raise NotImplementedError("honour_video_lengths: the grouped entry points have no length-masked form (include/l2s.h); call forward per batch, "
                                      "or forward_many_lengths for free-running batches (tf_ratio = 1)")
        self.native_model()

        def prep(item):
            a, k = self._call(item)
            video, face, _audio, mels, vlen, _alen, _mlen, tf = a
            return self._forward_job(video, face, mels, vlen, tf, **k)
        return self.pool(group, n_inflight).imap(calls, prep)

    def forward_many_lengths(self, calls, group: int = 8, n_inflight: int = 3):
        """Eval-mode `forward` WITH its `video_lengths` honoured over a stream of batches whose B, T and mel length differ - evaluate.py's loop over a
        loader that pads every batch to its own longest clip and its own longest mel - with `group` batches, at most 256 clips, advanced per launch chain
        as an evaluate-shaped ragged group (`l2s_forward_eval_ragged`) and `n_inflight` chains on the GPU at once: the twin of `inference_many_lengths`.
        `calls`: as for `forward_many`; every call needs its `video_lengths` (B integers in [7, T]) and a `tf_ratio` whose scheduled-sampling draws force
        no step (evaluate.py's tf_ratio = 1; the draws are made as `forward` makes them, so the host RNG is consumed alike) - a call that teacher-forces
        a step raises `ValueError`: it keeps its own `forward` call.  Yields the reference's list of 7 per call, in order, each what `forward(*call)`
        gives with `honour_video_lengths` on - every clip as it would come out alone.  Does not read the `honour_video_lengths` attribute."""
        if self.training:
            raise RuntimeError("forward_many_lengths is the evaluate path: call .eval() first (train() mode trains through forward / backward)")
        self.native_model()

        def prep(item):
            a, k = self._call(item)
            video, face, _audio, mels, vlen, _alen, _mlen, tf = a
            return self._forward_ragged_job(video, face, mels, vlen, tf, **k)
        return self.pool(group, n_inflight).imap(calls, prep)

    def _forward_ragged_job(self, video_frames, face_frames, melspecs, video_lengths, tf_ratio, speaker_embedding=None, gumbel_noise=None):
        """`_forward_job` as a job of the ragged evaluate route (`l2s_forward_eval_ragged`): the lengths are validated before the batch is staged on the
        device, the scheduled-sampling draws are made as `forward` makes them and must force no step."""
        if video_lengths is None:
            raise ValueError("forward_many_lengths: every call needs video_lengths (use forward_many for batches whose lengths are ignored)")
        lens = list(native.video_lengths_array(video_lengths, video_frames.shape[0], video_frames.shape[2]))
        job = self._forward_job(video_frames, face_frames, melspecs, video_lengths, tf_ratio, speaker_embedding, gumbel_noise)
        if job["mask"] is not None:
            raise ValueError(f"forward_many_lengths: tf_ratio = {tf_ratio} teacher-forces a step - the ragged evaluate call is free-running (tf_ratio = 1); "
                             "call forward for this batch")
        job["entry"], job["video_lengths"] = "forward_ragged", lens
        return job

    def _forward_train(self, video_frames, face_frames, melspecs, video_lengths, tf_ratio, speaker_embedding, gumbel_noise, dropout_masks=None,
                       honour_lengths=False, melspec_lengths=None):
        """The differentiable route (train.py:167-184): same outputs as `forward`, attached to autograd through `_HipTrainStep`.
        In `train()` mode the five dropout sites of the reference are active (multipliers drawn on the device by `training.draw_dropout`
        and handed to the kernels as inputs, or supplied through `dropout_masks=`); in `eval()` mode they are off (the configuration the
        reference gradient goldens pin).  BatchNorm follows the module mode too: batch statistics with running-statistics updates in
        `train()`, running statistics in `eval()` (per process: no cross-rank synchronisation, like the single-device reference)."""
        self._train_state()
        with torch.no_grad():
            emb = self._speaker(face_frames, speaker_embedding).to(torch.float32).contiguous()
        B, _, T, _, _ = video_frames.shape
        S = melspecs.shape[2]
        if gumbel_noise is None:
            gumbel_noise = Decoder.draw_gumbel(B * native.min_T(T), video_frames.device)
        mask, consumed = [], 0
        for _ in range(S):                                   # scheduled sampling, one torch.rand(1) per step (decoder.py:355-357)
            take = bool(torch.rand(1) > tf_ratio) and consumed < int(tf_ratio * S)
            consumed += int(take)
            mask.append(1 if take else 0)
        drop = dropout_masks
        if drop is None and self.training:
            from ..training import draw_dropout
            drop = draw_dropout(B, T, S, video_frames.device)
        # `honour_lengths` (forward: both switches on): checked on the host before anything reaches the device
        lens = native.video_lengths_array(video_lengths, B, T) if honour_lengths else None
        mlens = native.mel_lengths_array(melspec_lengths, B, S) if melspec_lengths is not None else None      # `train_mel_lengths`: likewise
        mel, mel_post, stop, attn, dis = _HipTrainStep.apply(self.decoder.BOS, self, video_frames.detach().to(torch.float32).contiguous(), emb,
                                                             gumbel_noise.detach().to(torch.float32).contiguous(), melspecs, mask if any(mask) else None, drop, lens, mlens)
        if mlens is not None:      # what `Loss.forward(melspec_lengths=)` reads: the video lengths this call honoured, marked as such
            video_lengths = torch.as_tensor(video_lengths).detach().clone()
            video_lengths.l2s_honoured = True
        return [mel, mel_post, stop, emb, attn, dis, video_lengths]

    def inference(self, video_frames, face_frames, speaker_embedding=None, return_attention_map=False, gumbel_noise=None, early_stop=None,
                  video_lengths=None, **kwargs):
        """The reference's `Lip2Speech.inference` (model.py:43-59).  `early_stop` (not in the reference; default `None` = leave the model's option
        "early_stop" as it is, off unless set): `True` / `False` sets the option for this MODEL before the call.  On: the decode loop ends once
        every clip of the batch has crossed its stop token (plus the post-net's 10-frame margin) instead of running all `max_decoder_steps`;
        `output_lengths` and every frame below a clip's length are what the full loop gives, the frames at or past it - which every caller
        drops - come back as exact zeros.  A model shared by threads should set it once (`set_early_stop`), not per call.
        `video_lengths` (not read by the reference, whose signature takes it through `**kwargs`; default `None` = lengths ignored as there): the
        frame count of every clip of a batch ZERO-padded to T, B integers in [7, T] - the call then runs `l2s_inference_masked`, and every clip
        comes out as it would alone (its attention columns past its length are zeros).  Other keyword arguments are accepted and ignored,
        as by the reference."""
        self.set_early_stop(early_stop)
        with torch.no_grad():
            emb = self._speaker(face_frames, speaker_embedding)
            B, _, T, _, _ = video_frames.shape
            if gumbel_noise is None:
                gumbel_noise = Decoder.draw_gumbel(B * native.min_T(T), video_frames.device)
            mel, lengths, attn = self.native_model().inference(
                video_frames, emb, gumbel_noise, S=self.decoder.hparams.max_decoder_steps, want_attn=return_attention_map, video_lengths=video_lengths)
        if return_attention_map:
            return mel, lengths, attn
        return mel, lengths


def inference_pool(net: "Lip2Speech", n_inflight: int = 2, group: int = 4):
    """Throughput serving for a loaded model: a `parallel.InflightPool` over the model's own packed weight blob.  `pool.map(
    [(video, speaker_embedding, gumbel_noise), ...])` advances `group` independent batches per launch chain (`l2s_inference_multi`) with
    `n_inflight` chains on the GPU at once (2.4x the one-at-a-time throughput on one MI355X at group 8) and returns
    `(mel, output_lengths, attention)` per batch, each identical to `net.inference` on that batch."""
    from ..parallel import InflightPool
    return InflightPool(model=net.native_model(), n_inflight=n_inflight, group=group)


def get_network(mode):
    assert mode in ("train", "test")
    model = Lip2Speech()
    return model.train() if mode == "train" else model.eval()
