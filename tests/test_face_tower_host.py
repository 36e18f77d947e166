"""Face speaker tower, CPU side: the key table, the test restatement against the golden of the reference's own FaceRecognizer, the
synthetic weights' numeric regime, the adopting container and the declared C-ABI.  No device needed."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import face_tower_torch as ft                     # noqa: E402
from lip2speech_amd import statespec, synth      # noqa: E402


@pytest.fixture(scope="module")
def face_sd():
    return synth.synth_face_state_dict()


def test_spec_has_the_tables_keys_and_shapes():
    spec = statespec.face_tower_spec("vgg_face.")
    keys = [k for k, _, _ in spec]
    assert len(keys) == len(set(keys)) == 720
    resnet = [(k, s, kind) for k, s, kind in spec if k.startswith("vgg_face.resnet.")]
    assert len(resnet) == 716 and sum(kind == "bn_nbt" for _, _, kind in resnet) == 112
    floats = sum(int(np.prod(s)) if kind != "bn_nbt" else 1 for _, s, kind in resnet)
    assert floats == 28_937_311
    assert floats - 10575 * 512 - 10575 == 23_512_336
    # the restatement's own state_dict is the same table
    tower = ft.FaceTower()
    want = {k: tuple(v.shape) for k, v in tower.state_dict().items()}
    assert {k[len("vgg_face."):]: tuple(s) for k, s, _ in spec} == want
    shapes = dict((k, tuple(s)) for k, s, _ in spec)
    assert shapes["vgg_face.resnet.repeat_2.3.branch1.1.conv.weight"] == (128, 128, 1, 7)
    assert shapes["vgg_face.resnet.block8.branch1.2.conv.weight"] == (192, 192, 3, 1)
    assert shapes["vgg_face.resnet.logits.weight"] == (10575, 512)
    assert shapes["vgg_face.projection_layer.2.weight"] == (256, 512)


def test_default_synth_state_dict_unchanged():
    """The committed goldens hang on synth_state_dict()'s default output: same keys, same bits as before the face tower's kinds were added
    (SHA-256 over the sorted keys and their fp32 / int64 bytes), and no vgg_face.* key among them."""
    import hashlib
    sd = synth.synth_state_dict()
    assert not any(k.startswith("vgg_face.") for k in sd)
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].numpy().tobytes())
    assert h.hexdigest() == "dce6dfb8d9611470022f57c06d4fa6d64b1e46c28fa1c4926ec926815e44b128"


def test_fresh_and_loaded_networks_deep_copy_and_pickle(face_sd):
    """copy.deepcopy and torch.save of the whole module keep working (a best-model copy, EMA, saving the module): the face tower's pack
    lock is module-level and its packed library model is not part of the state."""
    import copy
    import io
    from model.model import get_network
    net = get_network("test")
    copy.deepcopy(net)
    torch.save(net, io.BytesIO())
    net.load_state_dict({**synth.synth_state_dict(seed=3), **face_sd}, strict=True)
    twin = copy.deepcopy(net)
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), twin.state_dict().values()))
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert set(back.state_dict()) == set(net.state_dict())
    assert len(back.vgg_face._used_tensors()) == 606


def test_restatement_reproduces_the_reference_golden(face_sd):
    g = np.load(os.path.join(HERE, "golden", "face_tower_b2.npz"))
    faces = synth.synth_faces(2)[:, 0].double()
    tower = ft.load_tower(face_sd, dtype=torch.float64)
    taps = {}
    with torch.no_grad():
        proj = tower.run(faces, taps)
        emb = tower.inference(faces)
    for name, got in (("proj", proj), ("emb", emb), ("pooled", taps["pooled"]), ("last_bn", taps["last_bn"])):
        assert (got.float() - torch.from_numpy(g[name])).abs().max().item() <= 1e-6, name


def test_synthetic_tower_stays_order_one(face_sd):
    tower = ft.load_tower(face_sd)
    taps = {}
    with torch.no_grad():
        tower.run(synth.synth_faces(2)[:, 0], taps)
    for name in ("conv2d_4b", "repeat_1", "mixed_6a", "repeat_2", "mixed_7a", "block8", "pooled"):
        sd = taps[name].std().item()
        assert 0.05 <= sd <= 20, (name, sd)


def test_full_face_set_round_trips_strictly(face_sd):
    from model.model import get_network
    ck = dict(synth.synth_state_dict(seed=3))
    ck.update(face_sd)
    net = get_network("test")
    res = net.load_state_dict(ck, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = net.state_dict()
    assert set(out) == set(ck) and all(torch.equal(out[k], ck[k]) for k in ck)
    get_network("test").load_state_dict(out, strict=True)


def test_partial_set_names_the_missing_key(face_sd):
    from model.model import get_network
    net = get_network("test")
    with pytest.raises(RuntimeError, match="speaker_embedding"):        # nothing adopted: the message of the voice route
        net.vgg_face.inference(torch.zeros(1, 3, 160, 160))
    gone = "vgg_face.resnet.repeat_2.4.branch1.2.bn.running_var"
    net.load_state_dict({**synth.synth_state_dict(seed=3), **{k: v for k, v in face_sd.items() if k != gone}}, strict=False)
    with pytest.raises(RuntimeError, match=re.escape(gone) + r".*\(128,\)"):
        net.vgg_face.inference(torch.zeros(1, 3, 160, 160))


def test_cpu_faces_raise(face_sd):
    from model.model import get_network
    net = get_network("test")
    net.load_state_dict({**synth.synth_state_dict(seed=3), **face_sd}, strict=True)
    with pytest.raises(RuntimeError, match="GPU"):
        net.vgg_face.inference(torch.zeros(1, 3, 160, 160))


def test_header_declares_the_face_entry_points():
    text = open(os.path.join(ROOT, "include", "l2s.h")).read()
    assert re.search(r"int64_t\s+l2s_face_workspace_bytes\s*\(\s*int B,\s*int H,\s*int W\s*\)", text)
    assert re.search(r"int\s+l2s_face_encoder_fwd\s*\(\s*l2s_model\* m,\s*const float\* faces,\s*int64_t batch_stride", text)
    diag = open(os.path.join(ROOT, "include", "l2s_diag.h")).read()
    assert "l2s_op_face_conv2d(" in diag and "l2s_op_face_taps(" in diag
    from lip2speech_amd import native
    assert {"l2s_face_workspace_bytes", "l2s_face_encoder_fwd"} <= set(native.ABI_SYMBOLS)
    assert {"l2s_op_face_conv2d", "l2s_op_face_taps"} <= set(native.DIAG_SYMBOLS)
