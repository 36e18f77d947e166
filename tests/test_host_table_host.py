"""The per-clip tables (csrc/host_table.h), the parts that need no GPU: every workspace sizer whose table moved onto the builder returns at least what the
formula it replaced gives - the formulas are written out here as arithmetic, for small shapes and at the limits - and the builder's alignment rule, its
offsets and its sizes-only mode through the diagnostic library's `l2s_op_table_layout` (no upload: dst is None)."""
import ctypes
from collections import Counter

import pytest

from lip2speech_amd import native

H = W = 88
VOC, D_EMB, N_MELS = 501, 256, 80
SPK_MAX_CLIPS, SPK_MAX_ROWS = 1048560, 4194240      # L2S_SPK_MAX_CLIPS, L2S_SPK_MAX_ROWS


def al(n):
    return (n + 255) // 256 * 256


def pad16(n):
    return (n + 15) // 16 * 16


@pytest.mark.parametrize("B,T,S", [(1, 7, 1), (2, 29, 77), (16, 75, 300), (63, 50, 10), (64, 8, 300), (65, 7, 3), (256, 29, 77)])
def test_masked_sizer_is_not_below_the_old_formula(B, T, S):
    L = native.lib()
    assert L.l2s_workspace_bytes_masked(B, T, H, W, S) >= L.l2s_workspace_bytes(B, T, H, W, S) + al(2 * B * 4) + 256


def ragged_old(batch_B, T, S):
    """the old formula for batches of ONE padded length T (then the chain's own part is l2s_workspace_bytes at N clips): length table, the gathered
    embeddings and Gumbel rows, N clip records of 24 bytes, the pair map"""
    N = sum(batch_B)
    return (native.lib().l2s_workspace_bytes(N, T, H, W, S) + al(2 * N * 4) + 256 + al(N * D_EMB * 4) + al(N * native.min_T(T) * VOC * 4) + al(N * 24)
            + al(N * ((T + 1) // 2) * 4))


@pytest.mark.parametrize("batch_B,T,S", [([1], 7, 1), ([2, 3], 29, 77), ([5, 6], 8, 4), ([32] * 8, 7, 2), ([32] * 8, 75, 300), ([21] * 6, 50, 9)])
def test_ragged_sizers_are_not_below_the_old_formulas(batch_B, T, S):
    G, N = len(batch_B), sum(batch_B)
    lens = [T] * N
    assert native.ragged_plan(batch_B, [T] * G, lens)[2] == N
    assert native.workspace_bytes_ragged(batch_B, [T] * G, H, W, S) >= ragged_old(batch_B, T, S)
    # the evaluate route adds its staging buffers and N records of 32 bytes to the ragged group's workspace at Smax
    batch_S = [max(1, S - g) for g in range(G)]
    assert native.forward_eval_ragged_plan(batch_B, [T] * G, batch_S)[4:] == (N, T, S)
    rows = N * S
    staging = 2 * al(rows * N_MELS * 4) + al(rows * 4) + al(rows * T * 4) + al(N * native.min_T(T) * VOC * 4) + al(N * 32)
    assert native.workspace_bytes_eval_ragged(batch_B, [T] * G, batch_S, H, W) >= ragged_old(batch_B, T, S) + staging


@pytest.mark.parametrize("samples", [[201], [16000], [201, 48000, 16000], [3200 * k + 201 for k in range(17)], [201] * SPK_MAX_CLIPS,
                                     [319] * (SPK_MAX_CLIPS - 1) + [160 * (SPK_MAX_ROWS - 2 * (SPK_MAX_CLIPS - 1) - 1)]])
def test_speaker_packed_sizer_is_not_below_the_old_formula(samples):
    B = len(samples)
    _, _, row0, L_max, R = native.speaker_packed_plan(samples)
    assert R == sum(n // 160 + 1 for n in samples) and len(row0) == L_max + 1
    floats = R * (400 + 402 + 204 + 40 + 1024 + 256 * 2) + pad16(B) * 256 * 3 + B * 256 * 2 + 64 * 16
    old = floats * 4 + al((B * 4 + L_max + 1) * 4) + (1 << 12)      # the table: B records of 16 bytes, then L_max + 1 words
    assert native.lib().l2s_speaker_workspace_bytes_packed((ctypes.c_int64 * B)(*samples), B) >= old


VOCODER_TABLES = [[5], [5, 8], [5, 8, 9, 77, 130], [122, 145, 188, 300], [5] * 42, [7] * 43, [5] * 65535, [256] * 65535]


@pytest.mark.parametrize("lengths", VOCODER_TABLES, ids=lambda t: f"N{len(t)}L{t[-1]}")
def test_vocoder_ragged_sizers_are_not_below_the_old_formulas(lengths):
    L, N, frames = native.lib(), len(lengths), sum(lengths)
    for iters in (0, 4):
        solo = sum(c * L.l2s_inverse_mel_workspace_bytes(1, n, 80, 513, 1, iters) for n, c in Counter(lengths).items())
        got = native.inverse_mel_ragged_workspace_bytes(lengths, 80, 513, iters)
        assert got >= 256 + 2 * al(N * 8) + al((N + 1) * 4) + solo      # two int64 arrays and the row prefix sums, each rounded up, and the solo sizers
        assert got >= solo
    GL_LDK = 520
    assert L.l2s_griffin_lim_workspace_bytes(1, 5) == 5 * GL_LDK * 4 + 2 * 5 * GL_LDK * 8 + 512
    got = native.griffin_lim_ragged_workspace_bytes(lengths)
    assert got >= 512 + al((3 * N + 3) * 4) + frames * GL_LDK * 4 + frames * 3 * GL_LDK * 8 + 512 * N
    assert got >= sum(c * L.l2s_griffin_lim_workspace_bytes(1, n) for n, c in Counter(lengths).items())
    n_res = [4000 + 3 * n for n in lengths]
    solo = sum(c * L.l2s_estoi_workspace_bytes_long(1, n) for n, c in Counter(n_res).items())
    got = native.estoi_ragged_workspace_bytes(n_res)
    assert got >= 256 + al((4 * N + 30) * 4) + solo and got >= solo


@pytest.mark.parametrize("n_a,n_b", [(0, 0), (0, 3), (1, 1), (2, 1), (3, 4), (7, 0), (959, 2), (960, 1), (961, 960)])
def test_builder_aligns_each_segment_to_its_element(n_a, n_b):
    a, b = list(range(1, n_a + 1)), [(k + 1) << 33 for k in range(n_b)]
    off_a, off_b, words = native.op_table_layout(a, b)
    assert off_a == 0 and off_b == n_a + n_a % 2 and off_b % 2 == 0      # the int64 segment starts at the next even word: 8 bytes
    assert words == off_b + 2 * n_b
    assert native.op_table_layout(a, b, fill=False) == (off_a, off_b, words)      # the sizers' mode: the same offsets and total, and no data is read
