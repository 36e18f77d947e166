"""Host-side checks of what tests/test_gemm_bwd_op_gpu.py relies on (no GPU): the fp64 reference of tests/gemm_bwd_common.py against plain autograd and
against the written-out sums, the exactness condition and the consistency of every row of the edge table, the buffer layouts, and the parser of the
launch recorder's records (`native.gemm_bwd_record_dict`, `l2s_gemm_bwd_record` of include/l2s_diag.h)."""
import ctypes
import os
import re

import pytest
import torch

import gemm_bwd_common as gb
from lip2speech_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("B,T,Cin,Nout,k,stride,pad", [(2, 9, 6, 5, 5, 1, 2), (1, 3, 4, 3, 5, 1, 2), (2, 29, 4, 3, 7, 7, 0), (2, 11, 3, 4, 3, 3, 0), (2, 7, 5, 6, 1, 1, 0)])
def test_reference_is_conv1d_autograd(B, T, Cin, Nout, k, stride, pad):
    """the descriptor -> dense Conv1d reading and the packed layouts (dZ and X channel-last, Wp[n][tap * Cin + ci]): the helper's result equals what
    `loss.backward()` leaves on a Conv1d's weight and input, and the sums written out element by element"""
    gen = torch.Generator().manual_seed(B * 100 + k)
    x = torch.randint(-8, 9, (B, Cin, T), generator=gen).double().requires_grad_(True)
    w = torch.randint(-8, 9, (Nout, Cin, k), generator=gen).double().requires_grad_(True)
    y = torch.nn.functional.conv1d(x, w, stride=stride, padding=pad)
    Tz = y.shape[2]
    dz = torch.randint(-8, 9, y.shape, generator=gen).double()
    y.backward(dz)
    dz_cl, x_cl = dz.permute(0, 2, 1).reshape(B * Tz, Nout), x.detach().permute(0, 2, 1).reshape(B * T, Cin)
    wp = w.detach().permute(0, 2, 1).reshape(Nout, k * Cin)
    d = gb.dw_desc(B, T, Cin, Nout, k, stride, pad)
    assert (d["M"], d["N"], d["K"], d["Tz"]) == (Nout, k * Cin, B * Tz, Tz)
    got = gb.reference(d, dz_cl.float(), x_cl.float())
    assert torch.equal(got, w.grad.permute(0, 2, 1).reshape(Nout, k * Cin))
    want = torch.zeros(Nout, k * Cin, dtype=torch.float64)
    for b in range(B):
        for t in range(Tz):
            for tap in range(k):
                tx = t * stride + tap - pad
                if 0 <= tx < T:
                    want[:, tap * Cin:(tap + 1) * Cin] += torch.outer(dz[b, :, t], x.detach()[b, :, tx])
    assert torch.equal(got, want)
    if stride == 1:
        d = gb.dx_desc(B, T, Cin, Nout, k, pad)
        assert (d["M"], d["N"], d["K"], d["Tz"], d["padp"]) == (B * T, Cin, k * Nout, Tz, k - 1 - pad)
        got = gb.reference(d, dz_cl.float(), wp.float())
        assert torch.equal(got, x.grad.permute(0, 2, 1).reshape(B * T, Cin))
        want = torch.zeros(B, T, Cin, dtype=torch.float64)
        for t in range(Tz):
            for tap in range(k):
                tx = t + tap - pad
                if 0 <= tx < T:
                    want[:, tx] += dz[:, :, t] @ wp[:, tap * Cin:(tap + 1) * Cin]
        assert torch.equal(got, want.reshape(B * T, Cin))


def test_edge_table_rows_are_exact_and_consistent():
    """every row: integers that describe one Conv1d (geometry asserts), the exactness condition lim * lim * K * |alpha| + max|C0| < 2^24, integers that
    bf16 holds exactly, a name of its own; the rows reach every <VEC> form of the three kernels (each runs in f32 and bf16: all twelve instances), every
    launch function, clipped and empty slices, accumulate, the c_T form and strided operands"""
    table = gb.edge_table()
    names = [L["name"] for L in table]
    assert len(set(names)) == len(names)
    for L in table + [r[0] for r in gb.refusal_table()]:
        for d in [L["d"]] + ([L["d2"]] if L["pair"] else []):
            gb.geometry(d)
        assert gb.exactness_margin(L) < 2 ** 24, L["name"]
        assert L["lim"] <= 256                      # 8 significand bits
        if L["pair"]:
            assert L["d"]["mode"] == gb.DW and L["d2"]["mode"] == gb.DX and L["d"]["K"] == L["d2"]["M"]
    assert {gb.instance(L, b) for L in table for b in (0, 1)} == gb.ALL_INSTANCES
    assert {L["entry"] for L in table} == {0, 1, 2}
    by = {L["name"]: L for L in table}
    assert gb.used_splits(by["dw58_k97_s7"]) == 4 and gb.used_splits(by["dw58_k97_s3"]) == 3 and gb.used_splits(by["dw58_k97_s1"]) == 1
    nkt = (33408 + 31) // 32
    per = (nkt + 255) // 256
    assert per == 5 and (nkt + per - 1) // per == 209                          # 209 live slices, 47 empty
    assert gb.used_splits(by["dx_conv_k3_b2t9c24n20_s12_acc"]) == 2            # K = 60: two K tiles cap twelve slices
    assert by["dx_vecsize_unaligned"]["d"]["N"] % 4 == 0 and gb.expected_vec(by["dx_vecsize_unaligned"]) == 0
    assert all(n in by for n in gb.RANDOM_CASES) and len(gb.RANDOM_CASES) == 6
    assert {by[n]["d"]["K"] for n in gb.RANDOM_CASES} >= {5632, 400}


def test_layout_and_expected_buffer():
    """the output region follows ldc and c_T / c_seq_stride; `expected` changes nothing outside it"""
    L = next(x for x in gb.edge_table() if x["name"] == "dx_cT_k3")
    d = L["d"]
    (H,) = gb.build(L, seed=1)
    first, idx, n = H["lay"]["c"]
    assert first == gb.GUARD and n == gb.GUARD + 2 * 29 * 16 + gb.GUARD
    assert idx.shape == (18, 48) and int(idx[9, 0]) == first + 29 * 16 and int(idx[1, 0]) == first + 48
    ref = gb.reference(d, H["a"], H["b"])
    out = gb.expected(H, ref)
    mask = torch.ones(n, dtype=torch.bool)
    mask[idx.reshape(-1)] = False
    assert int(mask.sum()) == 2 * gb.GUARD + 2 * 2 * 16                        # guards + frames 27, 28 of both clips
    assert torch.equal(out[mask], H["C"].double()[mask])
    assert torch.equal(out[idx], H["C"].double()[idx] + ref)                   # accumulate = 1
    assert float(out.abs().max()) < 2 ** 24 and torch.equal(out, out.round())
    # a strided, offset, unaligned case: dense operands come back out of their buffers where the descriptor says
    L = next(x for x in gb.edge_table() if x["name"] == "dx_nonvec_strided")
    (H,) = gb.build(L, seed=2)
    fa, ia, na = H["lay"]["a"]
    assert fa == 2 and na == 2 + 32 * 30 + 22 and torch.equal(H["a"][5], H["A"][2 + 5 * 30:2 + 5 * 30 + 22])
    assert not bool((H["C"] != gb.SENTINEL).any())
    # the halves of a pair read ONE dZ
    L = next(x for x in gb.edge_table() if x["name"] == "pair58_k97_s3")
    hw, hx = gb.build(L, seed=3)
    assert hx.get("shared_A") and hx["A"] is hw["A"]


def _struct_fields(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l2s_diag.h")).read(), flags=re.S)
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            out += [(ctype, f.strip()) for f in rest.split(",")]
    return out


def test_record_parser_matches_the_header():
    """the ctypes mirrors have the header's fields in the header's order and no padding; a record filled field by field parses into the same values;
    de-duplication ignores the name and the precision, nothing else"""
    want = [("int64_t", "c_seq_stride")] + [("int32_t", k) for k in native.GEMM_BWD_INTS] + [("float", "alpha")]
    assert _struct_fields("l2s_gemm_bwd_desc") == want
    assert [n for n, _ in native.GemmBwdDesc._fields_] == [k for _, k in want]
    assert _struct_fields("l2s_gemm_bwd_record") == [("l2s_gemm_bwd_desc", "d[2]")] + [("int32_t", k) for k in ("entry", "splits_asked", "splits", "vec", "bf16", "pair")] + [
        ("int32_t", "align[2][3]"), ("char", "name[40]")]
    assert ctypes.sizeof(native.GemmBwdDesc) == 8 + 4 * 18 == 80
    assert ctypes.sizeof(native.GemmBwdRecord) == 2 * 80 + 4 * 6 + 4 * 6 + 40
    assert tuple(gb.INTS) == tuple(native.GEMM_BWD_INTS) and (gb.DX, gb.DW) == (native.BWD_DX, native.BWD_DW)
    r = native.GemmBwdRecord()
    dw, dx = gb.dw_desc(1, 97, 58, 60, ldc=64), gb.dx_desc(1, 18, 48, 16, ldc=48, accumulate=1, alpha=-2.0, c_T=9, c_seq_stride=2 ** 33 + 464)
    r.d[0], r.d[1] = native.gemm_bwd_desc(**dw), native.gemm_bwd_desc(**dx)
    r.entry, r.splits_asked, r.splits, r.vec, r.bf16, r.pair = 2, 7, 4, 0, 1, 1
    for h, al in enumerate(((4, 8, 12), (0, 12, 4))):
        for i, a in enumerate(al):
            r.align[h][i] = a
    r.name = b"train_bwd_encoder_dw_dx"
    R = native.gemm_bwd_record_dict(r)
    assert R["d"] == dw and R["d2"] == dx and R["align"] == (4, 8, 12) and R["align2"] == (0, 12, 4)
    assert (R["entry"], R["splits_asked"], R["splits"], R["vec"], R["bf16"], R["pair"], R["name"]) == (2, 7, 4, 0, 1, 1, "train_bwd_encoder_dw_dx")
    # the raw bytes are where the header puts them: c_seq_stride of the second descriptor, the first align word, the name
    raw = bytes(r)
    assert int.from_bytes(raw[80:88], "little") == 2 ** 33 + 464 and int.from_bytes(raw[184:188], "little") == 4 and raw[208:231] == b"train_bwd_encoder_dw_dx"
    r.pair = 0
    S = native.gemm_bwd_record_dict(r)
    assert "d2" not in S and "align2" not in S
    other = dict(R, name="another_site", bf16=0, vec=1, splits=9)
    assert gb.dedup_key(other) == gb.dedup_key(R)
    for change in (dict(entry=1), dict(splits_asked=8), dict(align=(0, 8, 12)), dict(d=dict(dw, ldc=68)), dict(d2=dict(dx, alpha=1.0)), dict(d2=dict(dx, c_seq_stride=464))):
        assert gb.dedup_key(dict(R, **change)) != gb.dedup_key(R), change
    L = gb.from_record(R)
    assert gb.used_splits(L) == 4 and gb.expected_vec(L) == 0 and gb.instance(L, True) == ("pair", 0, 1)
