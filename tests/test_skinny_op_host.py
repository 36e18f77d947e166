"""Host side of the batch-row operator test (tests/test_skinny_op_gpu.py): the wrapper's frag16 packing, and which kernels its sweep reaches.  No GPU."""
import pytest
import torch

from lip2speech_amd import native
import skinny_op_common as sk


@pytest.fixture(scope="module")
def table():
    return sk.load_table()


@pytest.fixture(scope="module")
def D():
    return native.diag()


def _frag16_index_ref(row, k, K):
    """l2s_common.h frag16_index, transcribed with the divisions and remainders of its comment: F[(rt*(K/16) + c)*256 + l*4 + e] = X[16*rt + (l&15)][16*c + 4*(l>>4) + e]"""
    rt, i, c, q, e = row // 16, row % 16, k // 16, (k % 16) // 4, k % 4
    lane = q * 16 + i
    return (rt * (K // 16) + c) * 256 + lane * 4 + e


@pytest.mark.parametrize("R,K", [(1, 16), (13, 80), (16, 16), (17, 96), (49, 256), (200, 80), (33, 1024)])
def test_frag16_pack_and_unpack_invert_each_other(R, K):
    """ragged rows (no multiple of 16) and column counts with 1, 5, 6, 16 and 64 chunks: element by element against the formula, padded rows zero, and the
    round trip in both directions"""
    X = torch.randn(R, K, generator=torch.Generator().manual_seed(R * 1000 + K))
    F = native.frag16_pack(X)
    Rp = (R + 15) // 16 * 16
    assert F.shape == (Rp * K,)
    for r in sorted({0, R - 1, R // 2, min(15, R - 1), min(16, R - 1)}):
        for k in range(K):
            assert F[_frag16_index_ref(r, k, K)] == X[r, k] and native.frag16_index(r, k, K) == _frag16_index_ref(r, k, K)
    back = native.frag16_unpack(F, Rp, K)
    assert torch.equal(back[:R], X) and torch.equal(back[R:], torch.zeros(Rp - R, K))
    assert torch.equal(native.frag16_pack(back), F)                       # unpack then pack: the same buffer
    idx = native.frag16_index(torch.arange(Rp).view(-1, 1), torch.arange(K).view(1, -1), K).reshape(-1)
    assert torch.equal(idx.sort().values, torch.arange(Rp * K))           # a permutation of the buffer: no two elements share a slot
    wide = native.frag16_pack(X, rows=R + 16)                             # more padded rows on request
    assert wide.numel() == (Rp + 16) * K and torch.equal(native.frag16_unpack(wide, R, K), X)


@pytest.mark.parametrize("H", [4, 256, 512])
def test_lstm_row_permutation(H):
    """packed row 4 * unit + gate holds PyTorch's row gate * H + unit, and back"""
    perm = native.lstm_perm_rows(H)
    assert perm.shape == (4 * H,) and torch.equal(perm.sort().values, torch.arange(4 * H))
    for unit in (0, 1, H // 2, H - 1):
        for gate in range(4):
            assert perm[4 * unit + gate] == gate * H + unit
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(4 * H)
    gate, unit = torch.arange(4).view(-1, 1), torch.arange(H).view(1, -1)
    assert torch.equal(inv.view(4, H), 4 * unit + gate)
    W = torch.randn(4 * H, 16, generator=torch.Generator().manual_seed(H))
    assert torch.equal(W[perm][inv], W)


def test_sweep_reaches_every_unstamped_kernel(table, D):
    """Coverage as a condition: the kernels the GPU test launches (the same generator) are exactly the non-refused, non-stamped names of the recorded table"""
    cases = sk.sweep(D, table)
    reached = {sk.kernel_of(line) for _, _, _, line, _, _ in cases if not line.startswith("ERROR ")}
    # the recorded names outside the stamped section (the stamped builds are named by table["stamped"] alone), refusals aside
    forms = set()
    for site in table["sites"]:
        for rv in table["table"][site]:
            for cell in table["rowvecs"][rv]:
                c = table["cells"][cell]
                forms |= {c} if isinstance(c, int) else {f for per_chain in c for f in ([per_chain] if isinstance(per_chain, int) else per_chain)}
    want = {table["kernels"][table["forms"][f][0]] for f in forms}
    want = {k for k in want if not k.startswith("ERROR ")}
    assert not any("_timed" in k for k in want) and len(set(table["kernels"]) - want) == 7      # one refusal and the six stamped builds
    assert len(want) == 96 and reached == want, (sorted(want - reached), sorted(reached - want))
    assert any(line.startswith("ERROR ") for _, _, _, line, _, _ in cases)      # and the refused launches are in the sweep too
    assert {site for site, *_ in cases} == set(table["sites"]) and len(table["sites"]) == 12
    print(f"{len(cases)} launches reach {len(reached)} kernels")
