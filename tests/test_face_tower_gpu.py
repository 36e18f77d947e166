"""Face speaker tower on the MI355X (face_tower.hip): the Conv2d operator over every geometry of the tower, stage taps, embeddings against
the fp64 CPU restatement, the reference golden through net.vgg_face, batch independence, and the reference's call shapes without a
speaker embedding (eval, grouped evaluate, one training step)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import face_tower_torch as ft                # noqa: E402
from lip2speech_amd import synth            # noqa: E402

pytestmark = pytest.mark.gpu

NMAX = 32


@pytest.fixture(scope="module")
def face_sd():
    return synth.synth_face_state_dict()


@pytest.fixture(scope="module")
def faces():
    return synth.synth_faces(NMAX)                # (32, 2, 3, 160, 160); face_frames[:, 0] is the tower's input


@pytest.fixture(scope="module")
def ref64(face_sd, faces):
    """fp64 restatement: proj, emb and the stage taps of the 32 faces (rows are independent: a prefix is the smaller batch)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    tower = ft.load_tower(face_sd, dtype=torch.float64)
    taps = {}
    with torch.no_grad():
        proj = tower.run(faces[:, 0].double(), taps)
    emb = F.normalize(F.relu(proj), p=2, dim=1)
    return proj, emb, taps


@pytest.fixture(scope="module")
def face_model(face_sd):
    from model.modules import FaceRecognizer
    fr = FaceRecognizer()
    fr.load_state_dict({k[len("vgg_face."):]: v for k, v in face_sd.items()}, strict=True)
    return fr.cuda()


# every Conv2d geometry of the table: (Cin, Cout, (kh, kw), stride, (ph, pw), H)
GEOMS = [(32, 32, (3, 3), 1, (0, 0), 79), (32, 64, (3, 3), 1, (1, 1), 77), (64, 80, (1, 1), 1, (0, 0), 38), (80, 192, (3, 3), 1, (0, 0), 38),
         (192, 256, (3, 3), 2, (0, 0), 36), (256, 96, (1, 1), 1, (0, 0), 17), (32, 32, (3, 3), 1, (1, 1), 17), (96, 256, (1, 1), 1, (0, 0), 17),
         (256, 384, (3, 3), 2, (0, 0), 17), (192, 192, (3, 3), 1, (1, 1), 17), (192, 256, (3, 3), 2, (0, 0), 17),
         (896, 256, (1, 1), 1, (0, 0), 8), (128, 128, (1, 7), 1, (0, 3), 8), (128, 128, (7, 1), 1, (3, 0), 8), (256, 896, (1, 1), 1, (0, 0), 8),
         (896, 768, (1, 1), 1, (0, 0), 8), (256, 384, (3, 3), 2, (0, 0), 8), (256, 256, (3, 3), 2, (0, 0), 8), (256, 256, (3, 3), 1, (1, 1), 8),
         (1792, 384, (1, 1), 1, (0, 0), 3), (192, 192, (1, 3), 1, (0, 1), 3), (192, 192, (3, 1), 1, (1, 0), 3), (384, 1792, (1, 1), 1, (0, 0), 3)]


def _conv_ref(x_nchw, w, scale, shift, stride, pad, res=None, relu=True):
    y = F.conv2d(x_nchw.double(), w.double(), stride=stride, padding=pad) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}k{g[2][0]}{g[2][1]}s{g[3]}p{g[4][0]}{g[4][1]}h{g[5]}")
def test_conv2d_operator(geom):
    from lip2speech_amd import native
    cin, cout, (kh, kw), stride, pad, H = geom
    g = torch.Generator().manual_seed(cin * 7 + cout + kh * 3 + H)
    B = 3
    x = torch.randn(B, cin, H, H, generator=g)
    w = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
    scale, shift = 0.5 + torch.rand(cout, generator=g), 0.2 * torch.randn(cout, generator=g)
    Ho = (H + 2 * pad[0] - kh) // stride + 1
    Wo = (H + 2 * pad[1] - kw) // stride + 1
    for res, relu in ((None, True), (torch.randn(B, cout, Ho, Wo, generator=g), False)):
        want = _conv_ref(x, w, scale, shift, stride, pad, res, relu)
        got = native.op_face_conv2d(x.permute(0, 2, 3, 1).contiguous().cuda(), w.cuda(), scale.cuda(), shift.cuda(), stride, pad,
                                    res=res.permute(0, 2, 3, 1).contiguous().cuda() if res is not None else None, relu=relu)
        err = (got.cpu().double() - want).abs().max().item() / want.abs().max().item()
        assert err <= 1e-5, err


def test_conv2d_stem_from_strided_view():
    from lip2speech_amd import native
    g = torch.Generator().manual_seed(11)
    crops = torch.rand(4, 2, 3, 160, 160, generator=g) * 2 - 1
    w = torch.randn(32, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5
    scale, shift = 0.5 + torch.rand(32, generator=g), 0.2 * torch.randn(32, generator=g)
    dev = crops.cuda()[:, 0]
    assert not dev.is_contiguous() and dev.stride(0) == 2 * 3 * 160 * 160
    got = native.op_face_conv2d(dev, w.cuda(), scale.cuda(), shift.cuda(), 2, (0, 0), nchw=True)
    want = _conv_ref(crops[:, 0], w, scale, shift, 2, (0, 0))
    err = (got.cpu().double() - want).abs().max().item() / want.abs().max().item()
    assert got.shape == (4, 79, 79, 32) and err <= 1e-5, err


def test_stage_taps_b2(face_model, faces, ref64):
    _, _, taps = ref64
    nm = face_model.native_model()
    emb, proj, outs = nm.face_encoder_fwd(faces[:2, 0].cuda(), want_proj=True, taps=True)
    names = ["conv2d_4b", "repeat_1", "mixed_6a", "repeat_2", "mixed_7a", "block8", "pooled", "last_bn"]
    for name, got in zip(names, outs):
        want = taps[name][:2]
        if want.dim() == 4:
            want = want.permute(0, 2, 3, 1)
        d = (got.cpu().double() - want).abs().max().item()
        assert d <= 1e-4 * max(1.0, want.abs().max().item()), (name, d)


@pytest.mark.parametrize("B", [1, 2, 8, 32])
def test_embeddings_against_fp64(face_model, faces, ref64, B):
    proj64, emb64, _ = ref64
    emb, proj = face_model.native_model().face_encoder_fwd(faces[:B, 0].cuda(), want_proj=True)
    d_emb = (emb.cpu().double() - emb64[:B]).abs().max().item()
    d_proj = (proj.cpu().double() - proj64[:B]).abs().max().item()
    print(f"B={B}: max|d| emb {d_emb:.2e} proj {d_proj:.2e}")
    assert d_emb <= 1e-4 and d_proj <= 1e-4
    assert torch.equal(face_model(faces[:B, 0].cuda()), proj)


def test_reference_golden_through_vgg_face(face_sd):
    from model.model import get_network
    g = np.load(os.path.join(HERE, "golden", "face_tower_b2.npz"))
    net = get_network("test")
    net.load_state_dict({**synth.synth_state_dict(), **face_sd}, strict=True)
    net = net.cuda()
    crops = synth.synth_faces(2).cuda()
    emb = net.vgg_face.inference(crops[:, 0])
    proj = net.vgg_face(crops[:, 0])
    assert (emb.cpu() - torch.from_numpy(g["emb"])).abs().max().item() <= 1e-4
    assert (proj.cpu() - torch.from_numpy(g["proj"])).abs().max().item() <= 1e-4
    assert not net.vgg_face.training


def test_batch_independence_and_strided_view(face_model, faces):
    nm = face_model.native_model()
    crops = faces.cuda()
    big = nm.face_encoder_fwd(crops[:, 0])
    small = nm.face_encoder_fwd(crops[8:16, 0])
    assert torch.equal(big[8:16], small)
    assert torch.equal(nm.face_encoder_fwd(crops[:, 0].contiguous()), big)


def test_cpu_faces_raise(face_model, faces):
    with pytest.raises(RuntimeError):
        face_model.inference(faces[:2, 0])
    with pytest.raises(RuntimeError):
        face_model.native_model().face_encoder_fwd(faces[:2, 0])


# ------------------------------------------------------------------------------------------------ the reference's call shapes
B, T, S = 2, 29, 24


@pytest.fixture(scope="module")
def full_net(face_sd):
    from model.model import get_network
    net = get_network("test")
    net.load_state_dict({**synth.synth_state_dict(), **face_sd}, strict=True)
    return net.cuda().eval()


def _clip():
    video = synth.synth_video(B, T, tag="video-face")
    gum = synth.synth_gumbel(B * 4, tag="gumbel-face")
    mels = synth.synth_mels(B, S, tag="mel-face")
    crops = synth.synth_faces(B, tag="crops-face")
    return video, gum, mels, crops


def test_forward_and_inference_without_embedding(full_net):
    video, gum, mels, crops = (t.cuda() for t in _clip())
    lens = torch.full((B,), T, device="cuda")
    emb = full_net.vgg_face.inference(crops[:, 0])
    with torch.no_grad():
        a = full_net(video, crops, None, mels, lens, None, None, 1, gumbel_noise=gum)
        b = full_net(video, crops, None, mels, lens, None, None, 1, speaker_embedding=emb, gumbel_noise=gum)
    assert torch.equal(a[3], emb)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y)
    i1 = full_net.inference(video, crops, gumbel_noise=gum)
    i2 = full_net.inference(video, crops, speaker_embedding=emb, gumbel_noise=gum)
    for x, y in zip(i1, i2):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y)


def test_evaluate_mels_face_route(full_net):
    from lip2speech_amd import callers
    video, gum, mels, crops = _clip()
    audio = torch.zeros(B, 256 * (S - 1))
    gate = torch.zeros(B, S)
    batch = ((video, torch.full((B,), T)), (audio, torch.full((B,), audio.shape[1])), (mels, torch.full((B,), S), gate), crops)
    emb = full_net.vgg_face.inference(crops[:, 0].cuda())

    class Given:
        def inference(self, a):
            return emb

    torch.manual_seed(5)
    face = callers.evaluate_mels(full_net, [batch, batch], encoding="face", group=2)
    torch.manual_seed(5)
    given = callers.evaluate_mels(full_net, [batch, batch], speaker_encoder=Given(), group=2)
    assert len(face) == 2 and all(torch.equal(x, y) for x, y in zip(face, given))


def test_train_step_face_route(face_sd):
    from model.model import get_network
    from lip2speech_amd import callers
    video, gum, mels, crops = _clip()
    audio = torch.zeros(B, 256 * (S - 1))
    gate = torch.zeros(B, S)
    gate[:, S - 1] = 1.0
    batch = ((video, torch.full((B,), T)), (audio, torch.full((B,), audio.shape[1])), (mels, torch.full((B,), S), gate), crops)
    runs = []
    for encoding in ("face", "given"):
        net = get_network("train")
        net.load_state_dict({**synth.synth_state_dict(), **face_sd}, strict=True)
        net = net.cuda()
        emb = net.vgg_face.inference(crops[:, 0].cuda())

        class Given:
            def inference(self, a):
                return emb

        torch.manual_seed(3)
        if encoding == "face":
            log = callers.train_iterations(net, [batch], 1, tf_ratio=0.5, encoding="face")
        else:
            log = callers.train_iterations(net, [batch], 1, speaker_encoder=Given(), tf_ratio=0.5)
        torch.cuda.synchronize()
        runs.append((log[0]["loss"], net._flat.grad.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])
