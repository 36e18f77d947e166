#!/usr/bin/env python
"""Generate tests/golden/face_tower_b2.npz by running THE REFERENCE'S OWN FaceRecognizer (model/modules/vgg_face.py).

Runs only in the build container (needs /root/reference, read-only).  The reference module imports third-party packages that are not
installed here; stub modules are registered for them before it is loaded: ``facenet_pytorch`` exposes the CPU restatement of
``InceptionResnetV1`` (tests/face_tower_torch.py), ``cv2`` / ``torchaudio.transforms`` / ``matplotlib.pyplot`` are empty (the reference
only imports them).  The synthetic tower and projection weights (lip2speech_amd.synth.synth_face_state_dict) are loaded into the reference
module, and its ``forward`` / ``inference`` run on 2 synthetic faces (synth.synth_faces, regenerated from a seed on every host, not stored).
What this pins is the reference's glue: the stage order, the projection without ReLU in ``forward``, ReLU + L2 normalisation in
``inference``.  The trunk itself is the restatement (parity against facenet_pytorch is unpinned).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_face_goldens.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"

from lip2speech_amd import synth          # noqa: E402
import face_tower_torch as ft              # noqa: E402


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


def load_reference_face():
    sys.dont_write_bytecode = True
    _stub("facenet_pytorch", InceptionResnetV1=ft.InceptionResnetV1)
    _stub("cv2")
    ta = _stub("torchaudio")
    ta.transforms = _stub("torchaudio.transforms")
    if importlib.util.find_spec("matplotlib") is None:
        mpl = _stub("matplotlib")
        mpl.pyplot = _stub("matplotlib.pyplot", winter=None)
    spec = importlib.util.spec_from_file_location("ref_vgg_face", f"{REF}/model/modules/vgg_face.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference_face()
    net = ref.FaceRecognizer()
    sd = synth.synth_face_state_dict()
    net.load_state_dict({k[len("vgg_face."):]: v for k, v in sd.items()}, strict=True)
    net = net.double().eval()
    faces = synth.synth_faces(2)[:, 0].double()
    taps = {}
    with torch.no_grad():
        proj = net(faces)
        emb = net.inference(faces)
        # the pooled 1792-vector and last_bn's output of the same module's trunk
        feat = net.resnet.features(faces, taps)
        pooled = net.resnet.avgpool_1a(feat).view(2, -1)
        bn = net.resnet.last_bn(net.resnet.last_linear(pooled))
    # cross-check the test restatement of the glue against the reference module
    tower = ft.load_tower(sd, dtype=torch.float64)
    with torch.no_grad():
        d = max((tower(faces) - proj).abs().max().item(), (tower.inference(faces) - emb).abs().max().item())
    print(f"restatement vs reference FaceRecognizer: max|d| {d:.3e}")
    assert d < 1e-12
    out = os.path.join(HERE, "face_tower_b2.npz")
    np.savez_compressed(out, proj=proj.float().numpy(), emb=emb.float().numpy(), pooled=pooled.float().numpy(), last_bn=bn.float().numpy())
    print(f"wrote {out}: proj std {proj.std().item():.3f}, pooled std {pooled.std().item():.3f}")


if __name__ == "__main__":
    main()
