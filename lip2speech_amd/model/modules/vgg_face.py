"""Face speaker tower (reference: /root/reference/model/modules/vgg_face.py:12-60).

The reference wraps the third-party ``facenet_pytorch.InceptionResnetV1(pretrained='casia-webface')`` and a projection
Linear(512,512) -> GELU -> Linear(512,256).  ``Lip2Speech.forward`` / ``inference`` take the speaker embedding from it whenever the caller
passes none (model.py:47-50: train.py, evaluate.py and demo.py ``--encoding face`` all do so).

Checkpoints: a reference checkpoint carries the tower's tensors as ``vgg_face.resnet.*`` / ``vgg_face.projection_layer.*`` and
``demo.py:38`` loads it with ``strict=True``.  This module is a container for them: whatever keys a checkpoint holds under its
prefix are adopted on load (as buffers of nested sub-modules, same names, same values), so strict loading succeeds and
``state_dict()`` hands them back unchanged - a checkpoint saved here loads strictly in the reference again.

Once the adopted tensors form the tower's full used set (``statespec.face_tower_spec`` without ``resnet.logits.*`` and the
``num_batches_tracked`` counters), ``inference`` / ``forward`` run on the device through ``l2s_face_encoder_fwd`` (face_tower.hip) on a
library model that holds only these keys, packed lazily and re-packed when a tensor changes.  The architecture is restated from the
published package (absent here): parity against facenet_pytorch is unpinned; the reference's glue is pinned by a golden.
"""
import threading

import torch
from torch import nn

from ... import native, statespec

# the keys the tower computes with: name (without the "vgg_face." prefix) -> shape
# one lock for every FaceRecognizer: forward_many / inference_many may reach the lazy pack from several threads.  Module-level, so that an
# instance holds nothing that cannot be deep-copied or pickled
_PACK_LOCK = threading.Lock()

_USED = {k: tuple(shape) for k, shape, kind in statespec.face_tower_spec("")
         if kind != "bn_nbt" and not k.startswith("resnet.logits.")}


class _Held(nn.Module):
    """Nested name-space of adopted tensors (no arithmetic)."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("inert container of third-party face-tower tensors")


class FaceRecognizer(nn.Module):
    def __init__(self):
        super().__init__()
        self.__dict__["_face_native"] = None
        self.__dict__["_face_sig"] = None
        self.__dict__["_face_tensors"] = None

    def __getstate__(self):
        """copy.deepcopy / pickle / torch.save: the tensors travel, the packed library model (a device handle) does not - a copy packs its own"""
        state = super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__
        state = dict(state)
        state["_face_native"] = None
        state["_face_sig"] = None
        state["_face_tensors"] = None
        return state

    def _adopt(self, name: str, value: torch.Tensor):
        node = self
        parts = name.split(".")
        for part in parts[:-1]:
            if part not in node._modules:
                node.add_module(part, _Held())
            node = node._modules[part]
        if parts[-1] not in node._buffers:
            node.register_buffer(parts[-1], value.detach().clone())

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for key, value in state_dict.items():
            if key.startswith(prefix) and isinstance(value, torch.Tensor):
                self._adopt(key[len(prefix):], value)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self.__dict__["_face_tensors"] = None

    def _apply(self, fn, *a, **k):
        self.__dict__["_face_tensors"] = None
        return super()._apply(fn, *a, **k)

    def _used_tensors(self):
        """The used set by key, checked against the tower's shapes; raises naming the first missing / misshapen key."""
        cached = self.__dict__.get("_face_tensors")
        if cached is not None:
            return cached
        held = dict(self.named_buffers())
        if not held:
            raise RuntimeError("FaceRecognizer needs the third-party facenet_pytorch tower, which is outside this "
                               "path; pass speaker_embedding=... (the --encoding voice route, demo.py:84-86)")
        out = {}
        for key, shape in _USED.items():
            t = held.get(key)
            if t is None:
                raise RuntimeError(f"FaceRecognizer: missing tensor vgg_face.{key} (expected shape {shape})")
            if tuple(t.shape) != shape:
                raise RuntimeError(f"FaceRecognizer: tensor vgg_face.{key} has shape {tuple(t.shape)}, expected {shape}")
            out["vgg_face." + key] = t
        self.__dict__["_face_tensors"] = out
        return out

    def native_model(self) -> native.NativeModel:
        """The library model of the tower (only vgg_face.* keys), packed on first use and again whenever a tensor changed."""
        with _PACK_LOCK:
            tensors = self._used_tensors()
            sig = tuple((t.data_ptr(), t._version) for t in tensors.values())
            if self.__dict__["_face_native"] is None or sig != self.__dict__["_face_sig"]:
                nm = self.__dict__["_face_native"] or native.NativeModel()
                nm.load(tensors, list(tensors.keys()))
                self.__dict__["_face_native"] = nm
                self.__dict__["_face_sig"] = sig
            return self.__dict__["_face_native"]

    def forward(self, x):
        """(B,3,160,160) faces on the device -> (B,256) pre-ReLU projection (vgg_face.py:28-50).  Eval-only: BatchNorm always uses the
        running statistics and nothing is differentiable (no_grad), whatever the module's mode.  The reference's forward in train() mode would
        use batch statistics and let gradients reach last_linear / last_bn; Lip2Speech only ever calls `inference`, which is eval + no_grad there too."""
        self._used_tensors()
        with torch.no_grad():
            return self.native_model().face_encoder_fwd(x, want_proj=True)[1]

    def inference(self, x):
        """(B,3,160,160) faces on the device -> (B,256) normalize(relu(projection)) (vgg_face.py:52-60); the strided face_frames[:, 0]
        view is read as it is."""
        if self.training:
            self.eval()
        self._used_tensors()
        if not x.is_cuda:
            raise RuntimeError("the face tower runs on the GPU: move face_frames to cuda (no CPU fallback)")
        with torch.no_grad():
            return self.native_model().face_encoder_fwd(x)
