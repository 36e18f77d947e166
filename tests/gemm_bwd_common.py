"""Shared by tests/test_gemm_bwd_op_gpu.py and tests/test_gemm_bwd_op_host.py: one backward GEMM of gemm_bwd.hip as a LAUNCH - a descriptor (the integers
of BwdGemmP), the three operands' address alignment, the launch function it goes through and the K slices asked for - with its fp64 reference.

A launch is a dict in the format of `native.gemm_bwd_record_dict` (what the launch recorder yields), so a recorded launch and a row of the edge table
below are replayed by the same code:
    d, align, entry (0 launch_gemm_bwd, 1 launch_gemm_bwd_splitk, 2 launch_gemm_bwd_dw_dx), splits_asked, pair, and for a pair d2, align2
plus, in table rows only, "off" / "off2": extra column offsets (floats, multiples of 4) of A, B, C inside their buffers, "lim" (operand range) and "name".

Reference: the descriptor is read back as the dense Conv1d it stands for - dZ (B,Tz,Nout), X (B,Tx,Cin), Wp [Nout][taps*Cin] with k = tap*Cin + ci - and
its gradient is taken by fp64 autograd through torch.nn.functional.conv1d.  `layout` embeds the dense operands into buffers of the described row
pitches and offsets and says where in the output buffer the M x N result lives (ldc, and c_T / c_seq_stride where set); everything else in the
output buffer must keep its pre-fill bit for bit.

Exactness: with integer operands of magnitude <= lim and integer pre-fill, every product, partial sum and slice sum is an integer below 2^24 when
lim * lim * K * |alpha| + max|C0| < 2^24, so fp32 accumulation is exact in ANY order, and - small integers being exact in bf16 - so is the bf16 form."""
import torch

DX, DW = 0, 1
SENTINEL = -77777.5                       # exact in fp32 and no integer: no result of an exact case can equal it
TK = 32                                   # K tile of gemm_bwd.hip: slices are whole K tiles
INTS = ("mode", "M", "N", "K", "lda", "ldb", "ldc", "Tx", "Tz", "taps", "stride", "pad", "padp", "Nout", "Cin", "c_T", "accumulate")


# ------------------------------------------------------------------------------------------------ descriptors (as bwd_dx / bwd_dw of gemm_bwd.hip write them)
def dx_desc(B, Tx, Cin, Nout, taps=1, pad=0, lda=None, ldb=None, ldc=None, accumulate=0, alpha=1.0, c_T=0, c_seq_stride=0):
    Tz = Tx + 2 * pad - taps + 1
    return dict(mode=DX, M=B * Tx, N=Cin, K=taps * Nout, lda=lda or Nout, ldb=ldb or taps * Cin, ldc=ldc or Cin, Tx=Tx, Tz=Tz, taps=taps, stride=1, pad=pad,
                padp=taps - 1 - pad, Nout=Nout, Cin=Cin, c_T=c_T, c_seq_stride=c_seq_stride, accumulate=accumulate, alpha=float(alpha))


def dw_desc(B, Tx, Cin, Nout, taps=1, stride=1, pad=0, lda=None, ldb=None, ldc=None, accumulate=0, alpha=1.0):
    Tz = (Tx + 2 * pad - taps) // stride + 1
    return dict(mode=DW, M=Nout, N=taps * Cin, K=B * Tz, lda=lda or Nout, ldb=ldb or Cin, ldc=ldc or taps * Cin, Tx=Tx, Tz=Tz, taps=taps, stride=stride, pad=pad,
                padp=0, Nout=Nout, Cin=Cin, c_T=0, c_seq_stride=0, accumulate=accumulate, alpha=float(alpha))


def launch(name, d, entry=0, splits=0, align=(0, 0, 0), off=(0, 0, 0), pair=None, align2=(0, 0, 0), off2=(0, 0, 0), lim=8):
    L = dict(name=name, d=d, align=tuple(align), off=tuple(off), entry=entry, splits_asked=splits, pair=0, lim=lim)
    if pair is not None:
        L.update(pair=1, entry=2, d2=pair, align2=tuple(align2), off2=tuple(off2))
    return L


# ------------------------------------------------------------------------------------------------ what a descriptor stands for
def geometry(d):
    """The dense Conv1d behind a descriptor: (B, Tx, Tz, Cin, Nout, taps, stride, pad) - and the consistency of its integers"""
    taps, stride, pad, Tx, Tz, Cin, Nout = d["taps"], d["stride"], d["pad"], d["Tx"], d["Tz"], d["Cin"], d["Nout"]
    if d["mode"] == DX:
        assert stride == 1 and d["N"] == Cin and d["K"] == taps * Nout and d["M"] % Tx == 0, d
        assert Tz == Tx + 2 * pad - taps + 1 and d["padp"] == taps - 1 - pad, d
        B = d["M"] // Tx
    else:
        assert d["M"] == Nout and d["N"] == taps * Cin and d["K"] % Tz == 0 and d["c_T"] == 0, d
        assert Tz == (Tx + 2 * pad - taps) // stride + 1, d
        B = d["K"] // Tz
    return B, Tx, Tz, Cin, Nout, taps, stride, pad


def operand_shapes(d):
    """(rows, columns) of the dense A and B operands and of the result"""
    B, Tx, Tz, Cin, Nout, taps, _, _ = geometry(d)
    if d["mode"] == DX:
        return (B * Tz, Nout), (Nout, taps * Cin), (d["M"], d["N"])
    return (B * Tz, Nout), (B * Tx, Cin), (d["M"], d["N"])


def reference(d, a, b):
    """fp64 autograd through F.conv1d on the dense operands a, b (any float dtype, any device) -> the M x N result WITHOUT alpha, fp64"""
    B, Tx, Tz, Cin, Nout, taps, stride, pad = geometry(d)
    F = torch.nn.functional
    dz = a.double().reshape(B, Tz, Nout).permute(0, 2, 1)                                  # (B, Nout, Tz): the gradient of the conv's output
    if d["mode"] == DX:
        w = b.double().reshape(Nout, taps, Cin).permute(0, 2, 1).contiguous()              # canonical (Nout, Cin, taps)
        x = torch.zeros(B, Cin, Tx, dtype=torch.float64, device=a.device, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv1d(x, w, stride=1, padding=pad), x, dz)
        return g.permute(0, 2, 1).reshape(B * Tx, Cin)
    x = b.double().reshape(B, Tx, Cin).permute(0, 2, 1).contiguous()
    w = torch.zeros(Nout, Cin, taps, dtype=torch.float64, device=a.device, requires_grad=True)
    y = F.conv1d(x, w, stride=stride, padding=pad)
    assert y.shape[2] == Tz
    (g,) = torch.autograd.grad(y, w, dz)
    return g.permute(0, 2, 1).reshape(Nout, taps * Cin)                                    # [n][tap * Cin + ci]


# ------------------------------------------------------------------------------------------------ buffers
GUARD = 64                                # floats of pre-fill in front of and behind every output region (a multiple of 4: alignment is kept)


def _in_layout(rows, cols, ld, align, off):
    """an input operand inside a flat buffer: (first element, index of every dense element, buffer length)"""
    assert align % 4 == 0 and off % 4 == 0 and ld >= cols
    first = align // 4 + off
    idx = first + torch.arange(rows).unsqueeze(1) * ld + torch.arange(cols).unsqueeze(0)
    return first, idx, first + (rows - 1) * ld + cols


def layout(d, align=(0, 0, 0), off=(0, 0, 0)):
    """Where the dense operands and the result sit: per operand "a", "b", "c" a (first, idx, length) triple.  The output buffer carries GUARD floats in
    front, the whole described extent - every row to its full pitch ldc, every clip to its full c_seq_stride in the c_T form - and GUARD floats behind"""
    (ra, ca), (rb, cb), (M, N) = operand_shapes(d)
    out = {"a": _in_layout(ra, ca, d["lda"], align[0], off[0]), "b": _in_layout(rb, cb, d["ldb"], align[1], off[1])}
    assert align[2] % 4 == 0 and off[2] % 4 == 0 and d["ldc"] >= N
    first = GUARD + align[2] // 4 + off[2]
    m = torch.arange(M)
    if d["c_T"] > 0:
        assert M % d["c_T"] == 0 and d["c_seq_stride"] >= (d["c_T"] - 1) * d["ldc"] + N
        row0 = (m // d["c_T"]) * d["c_seq_stride"] + (m % d["c_T"]) * d["ldc"]
        extent = (M // d["c_T"]) * d["c_seq_stride"]
    else:
        row0 = m * d["ldc"]
        extent = M * d["ldc"]
    idx = first + row0.unsqueeze(1) + torch.arange(N).unsqueeze(0)
    assert idx.unique().numel() == idx.numel(), "output elements overlap"
    out["c"] = (first, idx, first + int(extent) + GUARD)
    return out


def ints(gen, n, lim):
    return torch.randint(-lim, lim + 1, (n,), generator=gen, dtype=torch.int64).to(torch.float32)


def exactness_margin(L):
    """lim * lim * K * |alpha| + max|C0| for every half of the launch (C0: integers of magnitude <= lim where the half accumulates, else none)"""
    lim = L["lim"]
    return max(lim * lim * d["K"] * abs(d["alpha"]) + (lim if d["accumulate"] else 0) for d in ([L["d"]] + ([L["d2"]] if L["pair"] else [])))


def build(L, seed, random_data=False):
    """Host-side buffers of one launch: per half a dict of flat fp32 buffers "A", "B", "C" (inputs: integers in [-lim, lim] everywhere, gaps between
    the rows included, so that a read from a wrong column is not a read of zero; C: SENTINEL, or integers where the half accumulates), their layouts and
    the dense operands "a", "b".  The two halves of a pair share dZ when they describe it alike, as every pair of the model does.
    random_data: normal operands, dZ scaled by K^-0.5 for DW and the weight by K^-0.5 for DX (unit-scale results; each half of a pair then has a dZ
    of its own, scaled for its own K)."""
    gen = torch.Generator().manual_seed(seed)
    halves = []
    for h, (d, al, of) in enumerate([(L["d"], L["align"], L.get("off", (0, 0, 0)))] + ([(L["d2"], L["align2"], L.get("off2", (0, 0, 0)))] if L["pair"] else [])):
        lay = layout(d, al, of)
        H = dict(d=d, lay=lay)
        for key, name in (("a", "A"), ("b", "B")):
            n = lay[key][2]
            if random_data:
                buf = torch.randn(n, generator=gen)
                if (key == "a") == (d["mode"] == DW):
                    buf = buf * d["K"] ** -0.5
            else:
                buf = ints(gen, n, L["lim"])
            H[name] = buf
        if h == 1 and not random_data and halves[0]["lay"]["a"][1].shape == lay["a"][1].shape and halves[0]["d"]["lda"] == d["lda"] and halves[0]["lay"]["a"][0] == lay["a"][0]:
            H["A"], H["shared_A"] = halves[0]["A"], True
        n = lay["c"][2]
        H["C"] = ints(gen, n, L["lim"]) if d["accumulate"] and not random_data else torch.full((n,), SENTINEL)
        if d["accumulate"] and random_data:
            H["C"] = torch.randn(n, generator=gen)
        H["a"], H["b"] = H["A"][lay["a"][1]], H["B"][lay["b"][1]]
        halves.append(H)
    return halves


def expected(H, ref):
    """The whole output buffer after the launch, fp64: the pre-fill with alpha * ref written (or added) at the result's elements"""
    d, idx = H["d"], H["lay"]["c"][1]
    out = H["C"].double().clone()
    v = d["alpha"] * ref.cpu()
    out[idx] = out[idx] + v if d["accumulate"] else v
    return out


def used_splits(L):
    """slices that run: the K tiles cap what was asked for (launch_gemm_bwd_splitk / launch_gemm_bwd_dw_dx); 1 = no partial matrices"""
    if L["entry"] == 0:
        return 1
    return max(1, min(L["splits_asked"], (L["d"]["K"] + TK - 1) // TK))


def vec_ok(d, align):
    """bwd_vec_ok of gemm_bwd.hip: 16-byte operand loads need aligned A and B, row pitches and the contiguous dimensions in multiples of 4"""
    v = align[0] % 16 == 0 and align[1] % 16 == 0 and d["lda"] % 4 == 0 and d["ldb"] % 4 == 0 and d["Cin"] % 4 == 0 and d["N"] % 4 == 0
    return v and (d["Nout"] % 4 == 0 if d["mode"] == DX else d["M"] % 4 == 0)


def expected_vec(L):
    v = vec_ok(L["d"], L["align"])
    return int(v and vec_ok(L["d2"], L["align2"])) if L["pair"] else int(v)


def instance(L, bf16):
    """(kernel, VEC, BF16) of the twelve instances"""
    return ("pair" if L["pair"] else ("dx", "dw")[L["d"]["mode"]], expected_vec(L), int(bool(bf16)))


ALL_INSTANCES = {(k, v, b) for k in ("dx", "dw", "pair") for v in (0, 1) for b in (0, 1)}


def dedup_key(R):
    """a recorded launch without its name and without the precision it ran in: what decides the arithmetic and the addressing"""
    def dk(d):
        return tuple(d[k] for k in INTS) + (d["c_seq_stride"], d["alpha"])
    return (R["entry"], R["splits_asked"], R["pair"], dk(R["d"]), tuple(R["align"])) + ((dk(R["d2"]), tuple(R["align2"])) if R["pair"] else ())


def from_record(R, lim=8):
    """a recorded launch as a replayable one"""
    L = dict(R)
    L.update(lim=lim, off=(0, 0, 0), off2=(0, 0, 0))
    return L


# ------------------------------------------------------------------------------------------------ (b) the edge table
def edge_table():
    T = []
    add = lambda *a, **k: T.append(launch(*a, **k))      # noqa: E731
    # DW, taps = 1, non-VEC: 58 channels, 97 rows = four K tiles, the last ragged.  3 slices: per = 2, the third slice is empty; 7 is clipped to 4
    for s in (1, 3, 4, 7):
        add(f"dw58_k97_s{s}", dw_desc(1, 97, 58, 58), entry=1, splits=s)
        add(f"pair58_k97_s{s}", dw_desc(1, 97, 58, 58), splits=s, pair=dx_desc(1, 97, 58, 58))
    # DW at the encoder's slice geometry: 33 408 rows in 256 slices (per = 5: 209 live, 47 empty); 33 409: the last tile holds one row
    for K in (33408, 33409):
        add(f"dw58_k{K}_s256", dw_desc(1, K, 58, 58), entry=1, splits=256, lim=4)
        add(f"pair58_k{K}_s256", dw_desc(1, K, 58, 58), splits=256, pair=dx_desc(1, K, 58, 58), lim=4)
    # DW, VEC: full tiles, and ragged row and column tiles in multiples of 4
    add("dw_vec_64x64x96", dw_desc(1, 96, 64, 64))
    add("dw_vec_132x68x100", dw_desc(1, 100, 68, 132))
    add("dw_vec_132x68x100_s3", dw_desc(1, 100, 68, 132), entry=1, splits=3)
    add("pair_vec_132x68x100_s2", dw_desc(1, 100, 68, 132), splits=2, pair=dx_desc(1, 100, 68, 132))
    # DW, Conv1d: (B, T, Cin, Nout, k, stride, pad); the second has fewer frames than taps, the third is Content.agg's stride == taps, pad 0 form
    for B, Tn, Cin, Nout, k, st, pad in ((2, 9, 16, 20, 5, 1, 2), (1, 3, 16, 8, 5, 1, 2), (2, 29, 16, 8, 7, 7, 0), (2, 11, 48, 12, 11, 1, 5)):
        add(f"dw_conv_b{B}t{Tn}c{Cin}n{Nout}k{k}s{st}p{pad}", dw_desc(B, Tn, Cin, Nout, k, st, pad))
    # DX, Conv1d, stride 1: plain, and split into an ldc > N output with accumulate.  Cin 80 / Nout 64: two column tiles, the second ragged, taps that
    # start on K-tile boundaries; Cin 24 / Nout 20: tap boundaries inside the 32-row K tiles (every 20 rows), one ragged column tile
    for k in (3, 5, 7, 11):
        for B, Tn in ((2, 9), (2, 3)):
            for Cin, Nout in ((80, 64), (24, 20)):
                base = f"dx_conv_k{k}_b{B}t{Tn}c{Cin}n{Nout}"
                add(base, dx_desc(B, Tn, Cin, Nout, k, k // 2))
                for s in (2, 5, min(16, 4 * k)):
                    add(f"{base}_s{s}_acc", dx_desc(B, Tn, Cin, Nout, k, k // 2, ldc=Cin + 12, accumulate=1), entry=1, splits=s)
    # the model's two longest Conv1d input-gradient reductions: MultiHop k = 11 (K = 5632, 16 slices) and the post-net's last layer (K = 400, 5 slices)
    add("dx_conv_k11_n512_K5632_s16_acc", dx_desc(2, 9, 64, 512, 11, 5, ldc=96, accumulate=1), entry=1, splits=16)
    add("dx_conv_k5_n80_K400_s5", dx_desc(2, 9, 64, 80, 5, 2), entry=1, splits=5)
    # DX, taps = 1, non-VEC; and a VEC-sized case with every pointer one float off 16 bytes: vec = 0, still exact
    add("dx_r70n58c24", dx_desc(1, 70, 24, 58))
    add("dx_r33n22c58", dx_desc(1, 33, 58, 22))
    add("dx_r70n58c24_s2", dx_desc(1, 70, 24, 58), entry=1, splits=2)
    add("dx_vecsize_unaligned", dx_desc(1, 64, 64, 64), align=(4, 4, 4))
    add("dw_vecsize_unaligned", dw_desc(1, 64, 64, 64), align=(4, 4, 4))
    # DX, c_T form: Content.agg's linear map on the (B * Lj, k * C) view of (B, T, C); frames Lj * k .. T - 1 of each clip stay untouched
    for k in (1, 3, 5, 7):
        Lj = 29 // k
        d = dx_desc(1, 2 * Lj, k * 16, 16, ldc=k * 16, accumulate=1, c_T=Lj, c_seq_stride=29 * 16)
        add(f"dx_cT_k{k}", d)
    # strided and offset operands
    add("dx_lda_gt_nout_coloff", dx_desc(1, 70, 48, 32, lda=64), off=(32, 0, 0))                       # weight_ih_l0 + 256, lda 512
    add("dw_ldb_gt_cin_coloff", dw_desc(1, 70, 32, 48, ldb=96), off=(0, 40, 0))                        # tp.cat + 2560, ldb 4608
    add("dx_ldb_gt_cin_coloff", dx_desc(1, 70, 48, 32, ldb=160), off=(0, 32, 0))                       # W + 512, ldb 2560
    add("dw_ldc_gt_n_coloff", dw_desc(1, 70, 32, 48, ldc=96), off=(0, 0, 16))                          # gw + 512, ldc 2560
    add("dx_ldc_gt_n_coloff_s3_acc", dx_desc(1, 70, 48, 96, ldc=144, accumulate=1), entry=1, splits=3, off=(0, 0, 80))      # dcat + 2560, ldc 4608
    add("dx_nonvec_strided", dx_desc(1, 33, 58, 22, lda=30, ldb=61, ldc=63), align=(8, 12, 4))
    # alpha
    add("dx_alpha_m2", dx_desc(2, 9, 24, 20, 5, 2, alpha=-2.0, accumulate=1))
    add("dw_alpha_m2_s2", dw_desc(1, 97, 58, 58, alpha=-2.0), entry=1, splits=2)
    return T


def refusal_table():
    """(launch, the rule's text in l2s_last_error)"""
    return [
        (launch("refuse_unaligned_taps", dx_desc(2, 9, 24, 20, 5, 2), align=(4, 0, 0)), "unaligned operands are supported for 1x1 layers only"),
        (launch("refuse_splitk_cT", dx_desc(1, 18, 48, 64, ldc=48, c_T=9, c_seq_stride=29 * 16), entry=1, splits=2), "split-K: plain row-major output only"),
        (launch("refuse_pair_taps", dw_desc(2, 9, 16, 20, 5, 1, 2), splits=1, pair=dx_desc(2, 9, 16, 20, 5, 2)), "dW + dX pair: 1x1 layers, plain outputs"),
    ]


RANDOM_CASES = ("dx_conv_k11_n512_K5632_s16_acc", "dx_conv_k5_n80_K400_s5", "pair58_k33409_s256", "dw_conv_b2t11c48n12k11s1p5", "dx_cT_k3", "dw_vec_132x68x100_s3")
