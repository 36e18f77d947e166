"""The sweep of the batch-row operator tests, shared by tests/test_skinny_op_host.py (which kernels it reaches) and tests/test_skinny_op_gpu.py (what they
compute): call site x rows x launch chains x weight planes x option set, reduced to one launch per distinct (site, rows, planes, kernel line).

The call sites and the option sets are those of tests/golden/skinny_forms.json - the list lives there and nowhere else; which kernel a combination takes is
asked of l2s_op_skinny_form (libl2s_diag.so), which launches nothing and needs no device."""
import ctypes
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = 2
# 16-row tiles 1, 1, 4, 8, 11, 13, 32: ragged on purpose (no count but 1 is a multiple of 16); {1, 4, 8, 11, 32} tiles is the smallest set at which the
# recorded table reaches every unstamped kernel instance, 200 rows add the partial row block of a 4x2 block (13 tiles = 3 blocks + 1 tile)
ROWS = (1, 13, 49, 113, 170, 200, 500)
CHAINS = (1, 2, 3)
PLANES = (0, 1)
X3_FAMILIES = ("skinny_rc4x_kernel", "skinny_rc8x_kernel", "skinny_rc4h_kernel", "skinny_sp_kernel")      # the split-bf16 LSTM blocks


def load_table():
    with open(os.path.join(ROOT, "tests", "golden", "skinny_forms.json")) as f:
        return json.load(f)


def diag_model(D, options):
    """a diag model that only carries options (never finalised): what l2s_op_skinny_form and l2s_op_skinny read the form rule's inputs from"""
    h = ctypes.c_void_p()
    assert D.l2s_model_create(ctypes.byref(h)) == 0
    for name, value in options:
        assert D.l2s_model_set_option(h, name.encode(), value) == 0, name
    return h


def form_line(D, model, groups, planes, B, chains):
    """the answer of l2s_op_skinny_form for a site's groups ([nchunks x 4, ntiles, epi, a_sum set]); the planes go to the LSTM groups, as in the product"""
    flat = []
    for g in groups:
        flat += g[:6] + [1 if planes and g[5] == LSTM else 0, g[6]]
    arr = (ctypes.c_int * len(flat))(*flat)
    out = ctypes.create_string_buffer(512)
    rc = D.l2s_op_skinny_form(model, len(groups), arr, B, chains, 0, 0, out, len(out))
    assert rc == 0, D.l2s_last_error()
    return out.value.decode()


def kernel_of(line):
    """the kernel with its template arguments, without the launch shape"""
    return line if line.startswith("ERROR ") else line.split(" grid=")[0]


def is_x3(line):
    return line.startswith(X3_FAMILIES)


def sweep(D, table, sites=None):
    """-> a list of (site, rows, planes, line, options, chains): every distinct (site, rows, planes, kernel line) of the cross product - the line under
    "skinny_static" kept apart from the same line without it - with the first option set and chain count that lead to it.  planes is 0 for a site without an LSTM group: nothing there takes them."""
    seen, out = set(), []
    models = [diag_model(D, options) for options in table["options"]]
    try:
        for site, groups in table["sites"].items():
            if sites is not None and site not in sites:
                continue
            has_lstm = any(g[5] == LSTM for g in groups)
            for B in ROWS:
                for planes in (PLANES if has_lstm else (0,)):
                    for options, m in zip(table["options"], models):
                        for chains in CHAINS:
                            line = form_line(D, m, groups, planes, B, chains)
                            # "skinny_static" is the one option that changes the code a kernel of the same name runs (SkinnyP::layout picks the
                            # compile-time segment layouts inside the general blocks): such a launch counts as a form of its own
                            key = (site, B, planes, line, any(name == "skinny_static" and value for name, value in options))
                            if key not in seen:
                                seen.add(key)
                                out.append((site, B, planes, line, options, chains))
    finally:
        for m in models:
            D.l2s_model_destroy(m)
    return out
