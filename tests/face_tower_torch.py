"""CPU restatement of the face tower, for the tests only (nothing under lip2speech_amd/ imports it).

facenet_pytorch 2.5.2's ``InceptionResnetV1`` (the reference's ``vgg_face.py:16``), restated from the package's published structure with
its state_dict key names, plus the reference's own projection (``vgg_face.py:22-26``).  Runs in fp32 or fp64 (``.double()``).  The package is
not importable here, so parity against it is unpinned; the reference's glue is pinned by ``tests/golden/face_tower_b2.npz``.
"""
import torch
import torch.nn.functional as F
from torch import nn


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, kernel_size, stride, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=0.001, momentum=0.1, affine=True)
        self.relu = nn.ReLU(inplace=False)

    def forward(self, x):
        return self.relu(self.bn(self.conv(x)))


class Block35(nn.Module):
    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = scale
        self.branch0 = BasicConv2d(256, 32, 1, 1)
        self.branch1 = nn.Sequential(BasicConv2d(256, 32, 1, 1), BasicConv2d(32, 32, 3, 1, 1))
        self.branch2 = nn.Sequential(BasicConv2d(256, 32, 1, 1), BasicConv2d(32, 32, 3, 1, 1), BasicConv2d(32, 32, 3, 1, 1))
        self.conv2d = nn.Conv2d(96, 256, kernel_size=1, stride=1)
        self.relu = nn.ReLU(inplace=False)

    def forward(self, x):
        out = torch.cat((self.branch0(x), self.branch1(x), self.branch2(x)), 1)
        return self.relu(self.conv2d(out) * self.scale + x)


class Block17(nn.Module):
    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = scale
        self.branch0 = BasicConv2d(896, 128, 1, 1)
        self.branch1 = nn.Sequential(BasicConv2d(896, 128, 1, 1), BasicConv2d(128, 128, (1, 7), 1, (0, 3)), BasicConv2d(128, 128, (7, 1), 1, (3, 0)))
        self.conv2d = nn.Conv2d(256, 896, kernel_size=1, stride=1)
        self.relu = nn.ReLU(inplace=False)

    def forward(self, x):
        out = torch.cat((self.branch0(x), self.branch1(x)), 1)
        return self.relu(self.conv2d(out) * self.scale + x)


class Block8(nn.Module):
    def __init__(self, scale=1.0, noReLU=False):
        super().__init__()
        self.scale = scale
        self.noReLU = noReLU
        self.branch0 = BasicConv2d(1792, 192, 1, 1)
        self.branch1 = nn.Sequential(BasicConv2d(1792, 192, 1, 1), BasicConv2d(192, 192, (1, 3), 1, (0, 1)), BasicConv2d(192, 192, (3, 1), 1, (1, 0)))
        self.conv2d = nn.Conv2d(384, 1792, kernel_size=1, stride=1)
        if not noReLU:
            self.relu = nn.ReLU(inplace=False)

    def forward(self, x):
        out = self.conv2d(torch.cat((self.branch0(x), self.branch1(x)), 1)) * self.scale + x
        return out if self.noReLU else self.relu(out)


class Mixed_6a(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = BasicConv2d(256, 384, 3, 2)
        self.branch1 = nn.Sequential(BasicConv2d(256, 192, 1, 1), BasicConv2d(192, 192, 3, 1, 1), BasicConv2d(192, 256, 3, 2))
        self.branch2 = nn.MaxPool2d(3, stride=2)

    def forward(self, x):
        return torch.cat((self.branch0(x), self.branch1(x), self.branch2(x)), 1)


class Mixed_7a(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = nn.Sequential(BasicConv2d(896, 256, 1, 1), BasicConv2d(256, 384, 3, 2))
        self.branch1 = nn.Sequential(BasicConv2d(896, 256, 1, 1), BasicConv2d(256, 256, 3, 2))
        self.branch2 = nn.Sequential(BasicConv2d(896, 256, 1, 1), BasicConv2d(256, 256, 3, 1, 1), BasicConv2d(256, 256, 3, 2))
        self.branch3 = nn.MaxPool2d(3, stride=2)

    def forward(self, x):
        return torch.cat((self.branch0(x), self.branch1(x), self.branch2(x), self.branch3(x)), 1)


class InceptionResnetV1(nn.Module):
    """Eval-mode structure of facenet_pytorch's InceptionResnetV1 (classify=False); ``pretrained`` only sets the logits width (no download)."""

    def __init__(self, pretrained=None, classify=False, num_classes=None, dropout_prob=0.6, device=None):
        super().__init__()
        self.pretrained = pretrained
        self.classify = classify
        if num_classes is None:
            num_classes = {"vggface2": 8631, "casia-webface": 10575}.get(pretrained, 10575)
        self.conv2d_1a = BasicConv2d(3, 32, 3, 2)
        self.conv2d_2a = BasicConv2d(32, 32, 3, 1)
        self.conv2d_2b = BasicConv2d(32, 64, 3, 1, 1)
        self.maxpool_3a = nn.MaxPool2d(3, stride=2)
        self.conv2d_3b = BasicConv2d(64, 80, 1, 1)
        self.conv2d_4a = BasicConv2d(80, 192, 3, 1)
        self.conv2d_4b = BasicConv2d(192, 256, 3, 2)
        self.repeat_1 = nn.Sequential(*[Block35(scale=0.17) for _ in range(5)])
        self.mixed_6a = Mixed_6a()
        self.repeat_2 = nn.Sequential(*[Block17(scale=0.10) for _ in range(10)])
        self.mixed_7a = Mixed_7a()
        self.repeat_3 = nn.Sequential(*[Block8(scale=0.20) for _ in range(5)])
        self.block8 = Block8(noReLU=True)
        self.avgpool_1a = nn.AdaptiveAvgPool2d(1)
        self.dropout = nn.Dropout(dropout_prob)
        self.last_linear = nn.Linear(1792, 512, bias=False)
        self.last_bn = nn.BatchNorm1d(512, eps=0.001, momentum=0.1, affine=True)
        self.logits = nn.Linear(512, num_classes)

    def forward(self, x):
        x = self.features(x)
        x = self.last_bn(self.last_linear(self.dropout(self.avgpool_1a(x)).view(x.shape[0], -1)))
        if self.classify:
            return self.logits(x)
        return F.normalize(x, p=2, dim=1)

    def features(self, x, taps=None):
        """conv2d_1a .. block8; taps (a dict) receives the stage outputs the device hook reports."""
        for name in ("conv2d_1a", "conv2d_2a", "conv2d_2b", "maxpool_3a", "conv2d_3b", "conv2d_4a", "conv2d_4b",
                     "repeat_1", "mixed_6a", "repeat_2", "mixed_7a", "repeat_3", "block8"):
            x = getattr(self, name)(x)
            if taps is not None:
                taps[name] = x
        return x


class FaceTower(nn.Module):
    """The reference's FaceRecognizer arithmetic (vgg_face.py:28-60) over the restated trunk: forward = pre-ReLU projection,
    inference = normalize(relu(projection))."""

    def __init__(self):
        super().__init__()
        self.resnet = InceptionResnetV1(pretrained="casia-webface")
        self.projection_layer = nn.Sequential(nn.Linear(512, 512), nn.GELU(), nn.Linear(512, 256))

    def run(self, x, taps=None):
        feat = self.resnet.features(x, taps)
        pooled = self.resnet.avgpool_1a(feat).view(x.shape[0], -1)
        bn = self.resnet.last_bn(self.resnet.last_linear(pooled))
        proj = self.projection_layer(bn)
        if taps is not None:
            taps["pooled"] = pooled
            taps["last_bn"] = bn
        return proj

    def forward(self, x):
        return self.run(x)

    def inference(self, x):
        return F.normalize(F.relu(self.run(x)), p=2, dim=1)


def load_tower(sd, prefix="vgg_face.", dtype=torch.float32) -> FaceTower:
    """A FaceTower in eval mode holding the `prefix`ed tensors of `sd` (strict)."""
    t = FaceTower()
    t.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)
    return t.to(dtype).eval()
