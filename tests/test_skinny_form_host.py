"""Which kernel every batch-row launch takes (skinny.hip skinny_form + the dispatcher's table), pinned on the host: no GPU, nothing is launched.

tests/golden/skinny_forms.json was recorded from the dispatcher of the commit BEFORE skinny_form existed (its launch macros turned into a recorder that
keeps the kernel with its template arguments, grid, block and dynamic LDS), over the cross product of: the call sites of l2s_api.hip (the batches as it
builds them) x rows on both sides of every threshold x 1-3 launch chains x weight planes present / absent x the defaults and, one at a time, every option
value the GPU suite sets; plus the two stamped builds at 256 rows.  l2s_op_skinny_form (libl2s_diag.so) must answer every row with the recorded line.
The file keeps each distinct name, form, [chains][planes] cell and [rows] vector once and the table as indices into them (a planes pair of equal
entries is stored as that entry, a cell of six equal entries as that entry).
A refused case holds "ERROR " and the error text; the hook answers with "ERROR " and the text launch_skinny sets for its caller.  The bracketed tail of
such a text is the source of the failed condition (L2S_REQUIRE appends it), which moved with the code, so the comparison is on the text in front of it."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = 2


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(ROOT, "tests", "golden", "skinny_forms.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def D():
    from lip2speech_amd import native
    return native.diag()


def _form(D, model, groups, planes, B, chains, stamped=(0, 0)):
    flat = []
    for g in groups:
        flat += g[:6] + [1 if planes and g[5] == LSTM else 0, g[6]]
    arr = (ctypes.c_int * len(flat))(*flat)
    out = ctypes.create_string_buffer(512)
    rc = D.l2s_op_skinny_form(model, len(groups), arr, B, chains, stamped[0], stamped[1], out, len(out))
    assert rc == 0, D.l2s_last_error()
    return out.value.decode()


def _model(D, options):
    h = ctypes.c_void_p()
    assert D.l2s_model_create(ctypes.byref(h)) == 0
    for name, value in options:
        assert D.l2s_model_set_option(h, name.encode(), value) == 0, name
    return h


def _line(table, form):
    """a recorded form as the line the hook writes: forms hold [kernel, grid x, y, z, block, lds], or [refusal text]"""
    f = table["forms"][form]
    k = table["kernels"][f[0]]
    return k if len(f) == 1 else f"{k} grid=({f[1]},{f[2]},{f[3]}) block={f[4]} lds={f[5]}"


def _cell(table, cell, ci, pi):
    """the form of cells[cell][chains][planes]; a planes pair of equal entries is stored as that entry, a cell of six equal entries as that entry"""
    c = table["cells"][cell]
    c = c[ci] if isinstance(c, list) else c
    return c[pi] if isinstance(c, list) else c


def _same(got, want):
    if want.startswith("ERROR "):      # a refusal: the text l2s_last_error gives the caller of the refused launch, compared in front of the condition's source
        return got.endswith("]") and got.split(" [")[0] == want.split(" [")[0]
    return got == want


def test_every_recorded_launch_keeps_its_form(table, D):
    bad, n = [], 0
    for oi, options in enumerate(table["options"]):
        m = _model(D, options)
        try:
            for site, groups in table["sites"].items():
                rowvec = table["rowvecs"][table["table"][site][oi]]
                for bi, B in enumerate(table["rows"]):
                    for ci, chains in enumerate(table["chains"]):
                        for pi, planes in enumerate(table["planes"]):
                            want = _line(table, _cell(table, rowvec[bi], ci, pi))
                            got = _form(D, m, groups, planes, B, chains)
                            n += 1
                            if not _same(got, want):
                                bad.append((site, options, B, chains, planes, got, want))
        finally:
            D.l2s_model_destroy(m)
    assert n == len(table["options"]) * len(table["sites"]) * 17 * 3 * 2 and len(table["sites"]) == 12 and len(table["options"]) == 33
    assert not bad, f"{len(bad)} of {n} launches changed form; the first: {bad[:5]}"


def test_stamped_builds_keep_their_form(table, D):
    bad = []
    m = _model(D, [])
    try:
        for site, groups in table["sites"].items():
            for fi, flags in enumerate(table["stamped_flags"]):
                for ci, chains in enumerate(table["chains"]):
                    for pi, planes in enumerate(table["planes"]):
                        want = _line(table, _cell(table, table["stamped"][site][fi], ci, pi))
                        got = _form(D, m, groups, planes, table["stamped_rows"], chains, flags)
                        if not _same(got, want):
                            bad.append((site, flags, chains, planes, got, want))
    finally:
        D.l2s_model_destroy(m)
    assert table["stamped_rows"] == 256 and table["stamped_flags"] == [[1, 0], [0, 1]]
    assert not bad, f"{len(bad)} stamped launches changed form; the first: {bad[:5]}"


def test_the_recording_covers_the_case_list(table):
    """the list itself: nothing dropped from it when the table is regenerated"""
    assert table["rows"] == [1, 16, 17, 48, 49, 64, 96, 97, 112, 113, 176, 192, 193, 208, 224, 256, 512]
    assert table["chains"] == [1, 2, 3] and sorted(table["planes"]) == [0, 1]
    want = [[]] + [[[n, v]] for n, vs in (
        ("skinny_static", (1,)), ("skinny_sized", (0,)), ("skinny_split", (1, 3)), ("skinny_split8", (2,)), ("skinny_flat", (0,)),
        ("skinny_rc_jb", (2, 4, 15, 28, 44)), ("skinny_rc", (11, 21, 22, 42, 33)), ("skinny_rc_multi", (11, 21, 22, 42, 33)), ("lstm_x3", (0, 1, 2, 3, 4)),
        ("flat_half", (0, 2)), ("half_min_mts", (0,)), ("flat_xcd", (1,)), ("hoist_vproj", (0, 1))) for v in vs]
    assert table["options"] == want
    assert list(table["sites"]) == ["bilstm_step", "phase_a_unfolded", "phase_a_folded_step0", "phase_a_folded", "step_attention_proj", "phase_d_k1536",
                                    "phase_d_k1280", "phase_d_k1024_sum", "phase_d_k1024_unfolded", "phase_e", "step_fc_out_stop", "spk_lstm_step"]
    assert any(k.startswith("ERROR ") for k in table["kernels"])
    for site in table["sites"]:
        assert len(table["table"][site]) == len(table["options"]) and len(table["stamped"][site]) == 2
    assert all(len(v) == 17 for v in table["rowvecs"]) and all(isinstance(c, int) or (len(c) == 3 and all(isinstance(x, int) or len(x) == 2 for x in c)) for c in table["cells"])
