"""The split-bf16 GEMM family (gemm_x3.hip) on the 16x16x32 MFMA shape: lane mapping, 32-k accumulation, the re-planned LDS stages.  `-m gpu`.

Everything goes through the operator entries native.op_gemm / native.op_conv1d with x3=True (forced: every addressable shape runs the split-bf16
kernel; the wide 128x256 tile wherever N % 256 == 0 and K, Cin % 16 == 0, else the narrow 128x128 one), in three forms: the default, x3_narrow
(the narrow tile everywhere) and x3_dma (the weight operand as pre-split planes by LDS-DMA; the flag is ignored where the wide tile does not apply).

The first three groups are EXACT by construction - every product and every partial sum is representable in fp32, so the result must equal the
fp64 / int64 product bit for bit whatever the summation order - and so catch a misplaced operand or a dropped / doubled k without a tolerance."""
import pytest
import torch

from lip2speech_amd import native
import parity_common as pc

pytestmark = pytest.mark.gpu

FORMS = ({}, {"x3_narrow": True}, {"x3_dma": True})
K0S = (0, 7, 8, 15, 16, 23, 24, 31, 32, 47)


def _three_plane_values(n, seed):
    """fp32 values with 24 significant bits spread over all three bf16 planes: (1 + 2^-10 + 2^-23) x a small odd integer, rounded to fp32 once
    (the fp32 value is the operand; the reference multiplies exactly that)."""
    g = torch.Generator().manual_seed(seed)
    odd = (2 * torch.randint(0, 8, (n,), generator=g) + 1).double() * (2 * torch.randint(0, 2, (n,), generator=g) - 1).double()
    v = ((1.0 + 2.0 ** -10 + 2.0 ** -23) * odd).float()
    hi = (v.view(torch.int32) & -65536).view(torch.float32)
    mid = ((v - hi).view(torch.int32) & -65536).view(torch.float32)
    assert bool(((hi != 0) & (mid != 0) & ((v - hi - mid) != 0)).all())      # all three planes carry bits
    return v


def _small_ints(shape, seed, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("swap", [False, True], ids=["A_one_hot", "W_one_hot"])
@pytest.mark.parametrize("M,N,K", [(17, 80, 48), (129, 256, 48), (1, 1, 4), (33, 257, 400)])
def test_operand_placement_exact(M, N, K, swap):
    """One operand is one-hot in k (one non-zero per row, at k0, with bits in all three planes), the other has entries in {0, +-1, +-2}: every
    output is a single exact product.  k0 sweeps the edges of the 8-k lane groups, of the 16-k half steps and of the 32-k accumulation."""
    rows_hot, rows_int = (N, M) if swap else (M, N)
    ints = _small_ints((rows_int, K), 7 * M + N + K, -2, 2)
    for k0 in sorted({k for k in K0S + (K - 1,) if k < K}):
        hot = torch.zeros(rows_hot, K)
        hot[:, k0] = _three_plane_values(rows_hot, 1000 * k0 + M + N)
        A, W = (ints, hot) if swap else (hot, ints)
        ref = A.double() @ W.double().t()
        assert bool((ref.float().double() == ref).all())
        for form in FORMS:
            out = native.op_gemm(A.cuda(), W.cuda(), x3=True, **form)
            assert torch.equal(out.cpu().double(), ref), (k0, form, pc.maxdiff(out, ref))


@pytest.mark.parametrize("K", [4, 16, 20, 36, 48, 400, 1028])
def test_sum_structure_exact(K):
    """Dense integer operands in [-8, 8]: |sum| <= 64 K < 2^24, so fp32 accumulation is exact in any order and the result is the int64 product.
    M = 130: two row tiles, the second ragged; N = 256: the wide tile applies wherever K is a multiple of 16, and there the three forms agree
    bitwise (here trivially, through the exact reference; asserted on its own all the same)."""
    M, N = 130, 256
    A, W = _small_ints((M, K), K, -8, 8), _small_ints((N, K), K + 1, -8, 8)
    ref = A.long() @ W.long().t()
    outs = [native.op_gemm(A.cuda(), W.cuda(), x3=True, **form) for form in FORMS]
    for form, out in zip(FORMS, outs):
        assert torch.equal(out.cpu().long(), ref) and torch.equal(out.cpu(), ref.float()), (form, pc.maxdiff(out, ref))
    if K % 16 == 0:
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("B,T,Ci,Co,k,st,pad", [(2, 9, 80, 512, 5, 1, 2),        # K = 400: the taps straddle the 32-k steps (Cin = 5 x 16)
                                                 (2, 11, 48, 256, 3, 1, 1),       # K = 144
                                                 (1, 3, 512, 80, 5, 1, 2),        # T shorter than the taps, narrow tile
                                                 (2, 29, 512, 512, 7, 7, 0)])     # strided, unpadded
def test_conv1d_addressing_exact(B, T, Ci, Co, k, st, pad):
    """Integer-valued data (|x| <= 8, |w| <= 8: |sum| <= 64 * 3584 < 2^24): the implicit-Conv1d addressing checked exactly against conv1d in fp64."""
    X = _small_ints((B, T, Ci), T + k, -8, 8)
    Wt = _small_ints((Co, Ci, k), Ci + k, -8, 8)
    Wp = Wt.permute(0, 2, 1).reshape(Co, k * Ci).contiguous()
    ref = torch.nn.functional.conv1d(X.double().permute(0, 2, 1), Wt.double(), stride=st, padding=pad).permute(0, 2, 1)
    for form in FORMS:
        out = native.op_conv1d(X.cuda(), Wp.cuda(), taps=k, stride=st, pad=pad, x3=True, **form)
        assert torch.equal(out.cpu().double(), ref), (form, pc.maxdiff(out, ref))


def test_two_source_rows_through_prologue(synth_sd):
    """The two-segment A rows of the MultiHop launches (a_split / a_gap; the operator entries do not expose them): decoder_prologue at B = 2, T = 29
    with the split-bf16 kernels forced onto every GEMM they can address ("gemm_x3" = 3), against the golden K / V taps at the bounds of
    test_prologue_matches_oracle; the narrow tile everywhere ("gemm_x3" = 7) gives the same bits.
    What this does NOT cover: the model's only two-segment launch (the V bottleneck) has a_split = 512, an EVEN multiple of 16, and runs as split-K
    slices, so an A split that falls inside a 32-k step (an odd multiple of 16) is not exercised here, and nothing in the test shows which tile a
    slice ran on.  The half-step straddle itself is covered through Cin = 80 and Cin = 48 in test_conv1d_addressing_exact, which takes the same
    uniform half-step path as the split does."""
    g, _, emb = pc.lrw2_inputs()
    B, T = 2, 29
    vis = native.build_visual(g["feat"].cuda(), emb.cuda())
    fields = []
    for mode in (3, 7):
        nm = pc.fresh_native_model(synth_sd, gemm_x3=mode)
        state, _ = nm.decoder_prologue(vis, emb.cuda(), g["gumbel"].cuda())
        fields.append([native.state_field(state, B, T, f, (B, T, 512)).clone() for f in (native.ST_ENC, native.ST_K, native.ST_V)])
    enc, k, v = fields[0]
    assert pc.maxdiff(enc, g["oracle_enc"]) < 2e-5
    assert pc.maxdiff(k, g["oracle_k"].permute(0, 2, 1)) < 5e-5
    assert pc.maxdiff(v, g["oracle_v"]) < 5e-5
    for a, b in zip(*fields):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,N,K", [(257, 384, 1028), (130, 129, 36), (300, 256, 400)])
def test_random_data(M, N, K):
    """The rule of test_gemm_split_bf16_operator: the gate of the f32-MFMA kernel against the fp64 product, and an error no larger than 1.5x that
    kernel's own."""
    torch.manual_seed(M + N)
    A = torch.randn(M, K).cuda()
    W = (torch.randn(N, K) / K ** 0.5).cuda()
    ref = A.double() @ W.double().t()
    e32 = pc.maxdiff(native.op_gemm(A, W), ref)
    for form in FORMS:
        e3 = pc.maxdiff(native.op_gemm(A, W, x3=True, **form), ref)
        print(f"M {M} N {N} K {K} {form}: split-bf16 {e3:.3e}, f32 {e32:.3e}")
        assert e3 < 2e-5 and e3 <= 1.5 * e32 + 1e-7, (form, e3, e32)
