"""The carrier of the per-clip tables on the GPU (csrc/host_table.h; `l2s_op_upload_table` / `l2s_op_table_layout` of the diagnostic library): words built on
the host reach device memory through kernel arguments, native.TABLE_CHUNK per launch - exactly the n words asked for, at any destination offset, across
chunk boundaries, and with no host buffer that has to outlive the call."""
import ctypes

import pytest
import torch

from lip2speech_amd import native

pytestmark = pytest.mark.gpu

C = native.TABLE_CHUNK
SENTINEL = -0x5A5A5A5B
OFFSET = 1021              # words before the table: not a multiple of 64 (nor of 2)


def test_round_trip_at_the_chunk_boundaries():
    sizes = [1, 2, C - 1, C, C + 1, 2 * C, 2 * C + 3]
    bufs, patterns = [], []
    for n in sizes:
        buf = torch.full((OFFSET + n + 777,), SENTINEL, dtype=torch.int32, device="cuda")
        pattern = [(k * 2654435761 + n) % (1 << 31) - (k & 1) * (1 << 30) for k in range(n)]
        host = (ctypes.c_int32 * n)(*pattern)
        native.op_upload_table(host, n, buf, OFFSET)
        ctypes.memset(host, 0xEE, 4 * n)      # the call has returned, the stream has not been synchronised: the words travelled in the kernel arguments
        del host
        bufs.append(buf)
        patterns.append(pattern)
    torch.cuda.synchronize()
    for n, buf, pattern in zip(sizes, bufs, patterns):
        got = buf.cpu()
        assert got[OFFSET:OFFSET + n].tolist() == pattern, n
        assert bool((got[:OFFSET] == SENTINEL).all()) and bool((got[OFFSET + n:] == SENTINEL).all()), n


def test_built_table_lands_where_the_builder_says():
    """an odd number of int32 words, then an int64 segment: the builder pads one word, and the uploaded table holds both segments at the returned offsets"""
    a = [3 * k + 1 for k in range(C - 1)]                      # 959 words: the int64 segment starts at word 960, the second launch's first
    b = [(k + 1) * (1 << 33) + k for k in range(5)]
    buf = torch.full((2 * C,), SENTINEL, dtype=torch.int32, device="cuda")
    off_a, off_b, words = native.op_table_layout(a, b, dst=buf)
    torch.cuda.synchronize()
    assert (off_a, off_b, words) == (0, C, C + 10)
    got = buf.cpu()
    assert got[:C - 1].tolist() == a and int(got[C - 1]) == 0      # the pad word is a zero
    assert got[off_b:words].view(torch.int64).tolist() == b
    assert bool((got[words:] == SENTINEL).all())
