"""Unit-by-unit view of the video trunk (16 ShuffleNet units, conv_last, pooling) for the tests only (nothing under lip2speech_amd/ imports it).

The RIGHT arithmetic is the oracle's own: ``orc.shuffle_unit`` / ``orc._pw`` / ``orc.frontend3d`` with the weights cast by ``orc.to_dtype`` - fp64 is the
reference, fp32 the yardstick of what fp32 arithmetic costs on the same input.  This module adds only the layout of the taps of ``l2s_op_encoder_taps``
(channels last, one row per frame for the bound), the bound itself (``frame_check`` / ``global_check`` of tests/speaker_tower_torch.py, imported, not
copied) and four deliberately WRONG restatements of a unit (keyword ``wrong``) with which tests/test_encoder_stages_host.py shows that the bound notices
the errors the trunk kernels can make.
"""
import torch
import torch.nn.functional as F

from oracle import l2s_oracle as orc
from speaker_tower_torch import EPS32, MARGIN, frame_check, global_check      # noqa: F401  (re-exported: the tests take the bound from here)

N_UNITS = 16
TAP_FRONTEND, TAP_LAST = 0, N_UNITS + 1
N_TAPS = N_UNITS + 2
WRONG = ("pad_before_pw1", "swap_channels", "drop_low_plane", "scale_one_value")

_cast = {}


def cast(sd, dtype):
    """orc.to_dtype(sd, dtype), kept per (state dict, dtype): the suite's synthetic checkpoint is one session-wide object."""
    key = (id(sd), dtype)
    if key not in _cast:
        _cast[key] = (sd, orc.to_dtype(sd, dtype))      # holding sd keeps its id from being reused
    return _cast[key][1]


def unit_prefix(u: int) -> str:
    return f"encoder.trunk.0.{u}."


def tap(u: int) -> int:
    """tap index of unit u's output"""
    return 1 + u


def nchw(t: torch.Tensor) -> torch.Tensor:
    """a tap (NF, h, h, C) -> the oracle's layout (NF, C, h, h)"""
    return t.permute(0, 3, 1, 2).contiguous()


def rows(x: torch.Tensor) -> torch.Tensor:
    """the oracle's (NF, C, h, h) -> one row per frame in the tap's element order, (NF, h * h * C)"""
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)


# ---------------------------------------------------------------------------------------------- wrong restatements
def _truncated_two_planes(w: torch.Tensor) -> torch.Tensor:
    """fp32 -> hi + mid of the truncating three-way bf16 split (encoder_kernels.hip su_split2): the lowest plane, at most 2^-16 of the value, is lost"""
    w = w.float().contiguous()
    hi = (w.view(torch.int32) & -65536).view(torch.float32)
    r = w - hi
    mid = (r.view(torch.int32) & -65536).view(torch.float32)
    return hi + mid


def _unit_pad_before_pw1(x, sd, p):
    """shuffle_unit with banch2's depthwise conv padding the INPUT of pw1 instead of its output: the border taps read relu(bn(0)) where they must read 0"""
    stride2 = (p + "banch1.0.weight") in sd
    x2 = x if stride2 else x[:, x.shape[1] // 2:]
    r = orc._pw(F.pad(x2, (1, 1, 1, 1)), sd, p + "banch2.0", p + "banch2.1")
    w = sd[p + "banch2.3.weight"]
    r = orc.batchnorm_eval(F.conv2d(r, w, stride=2 if stride2 else 1, padding=0, groups=w.shape[0]), sd, p + "banch2.4")
    r = orc._pw(r, sd, p + "banch2.5", p + "banch2.6")
    if stride2:
        left = orc._pw(orc._dw(x, sd, p + "banch1.0", p + "banch1.1", 2), sd, p + "banch1.2", p + "banch1.3")
    else:
        left = x[:, :x.shape[1] // 2]
    return orc.channel_shuffle2(torch.cat([left, r], dim=1))


def unit(sd, u: int, x: torch.Tensor, dtype=torch.float64, wrong=None) -> torch.Tensor:
    """Unit u on x (NF, C, h, h) in `dtype`: orc.shuffle_unit.  wrong = one of WRONG:
    pad_before_pw1   the depthwise conv pads pw1's input, not its output (the bug the comment at su_dw_s2 warns of)
    swap_channels    the two output channels of largest mean magnitude change places after the shuffle (a mis-cut shuffle; a fixed pair may be dead)
    drop_low_plane   the unit's pointwise weights without their lowest bf16 plane
    scale_one_value  the largest value of the last frame times (1 + 1e-4)"""
    assert wrong is None or wrong in WRONG, wrong
    p, x, sdd = unit_prefix(u), x.to(dtype), cast(sd, dtype)
    if wrong == "pad_before_pw1":
        return _unit_pad_before_pw1(x, sdd, p)
    if wrong == "drop_low_plane":
        sdd = dict(sdd)
        for conv in ("banch2.0", "banch2.5", "banch1.2"):
            if p + conv + ".weight" in sd:
                sdd[p + conv + ".weight"] = _truncated_two_planes(sd[p + conv + ".weight"]).to(dtype)
    out = orc.shuffle_unit(x, sdd, p)
    if wrong == "swap_channels":
        a, b = out.abs().mean(dim=(0, 2, 3)).topk(2).indices.tolist()
        out = out.clone()
        out[:, [a, b]] = out[:, [b, a]]
    if wrong == "scale_one_value":
        out = out.clone()
        last = out[-1].reshape(-1)
        last[last.abs().argmax()] *= 1.0 + 1e-4
    return out


# ---------------------------------------------------------------------------------------------- the other stages
def frontend(sd, video: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """(B, 3, T, H, W) -> (B * T, 24, H/4, H/4)"""
    return orc.frontend3d(video.to(dtype), cast(sd, dtype))


def conv_last(sd, x: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """unit 15's output (NF, 464, h, h) -> conv_last + BN + ReLU as the tap holds it, (NF * h * h, 768)"""
    y = orc._pw(x.to(dtype), cast(sd, dtype), "encoder.trunk.1.0", "encoder.trunk.1.1")
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def pool_norm(last: torch.Tensor, NF: int) -> torch.Tensor:
    """the conv_last tap (NF * h * h, 768) -> feat rows (NF, 768): the mean over the map, then the L2 norm over the channels (oracle.encoder_forward's last two lines)"""
    x = last.view(NF, -1, last.shape[1]).mean(dim=1)
    return x / torch.clamp(torch.sqrt((x * x).sum(dim=1, keepdim=True)), min=1e-12)


# ---------------------------------------------------------------------------------------------- the bounds
def map_check(got_rows: torch.Tensor, ref64: torch.Tensor, ref32: torch.Tensor):
    """A map stage: `got_rows` (NF, ...) in tap order against the oracle-layout references (NF, C, h, h).  frame_check with one row per frame:
    |got - ref64| <= 8 * max(e32, eps32) * S_frame.  -> (ok, worst deviation / S_frame, e32)"""
    return frame_check(got_rows.reshape(got_rows.shape[0], -1), rows(ref64), rows(ref32))


def unit_check(sd, u: int, x_in: torch.Tensor, got: torch.Tensor):
    """unit u's tap `got` (NF, h, h, C) against the fp64 unit applied to `x_in`, the tap of the stage before (NF, h_in, h_in, C_in)"""
    x = nchw(x_in.cpu())
    return map_check(got, unit(sd, u, x), unit(sd, u, x, torch.float32))


def last_check(sd, x15: torch.Tensor, got: torch.Tensor):
    """the conv_last tap against the fp64 pointwise conv of unit 15's tap, one row per frame"""
    NF, x = x15.shape[0], nchw(x15.cpu())
    return frame_check(got.reshape(NF, -1), conv_last(sd, x).reshape(NF, -1), conv_last(sd, x, torch.float32).reshape(NF, -1))


def feat_check(last: torch.Tensor, feat: torch.Tensor):
    """feat (B, T, 768) against the fp64 mean + normalise of the conv_last tap; global_check -> (ok, worst, bound)"""
    NF = feat.shape[0] * feat.shape[1]
    last = last.cpu()
    return global_check(feat.reshape(NF, -1), pool_norm(last.double(), NF), pool_norm(last, NF))
