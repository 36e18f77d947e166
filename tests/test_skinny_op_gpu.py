"""What the batch-row ("skinny") kernels compute, one launch at a time, against fp64.  `-m gpu`.

tests/golden/skinny_forms.json pins WHICH kernel a launch takes; this file pins what each of them computes.  Every call site of l2s_api.hip (the groups of
the JSON's "sites") is launched through `native.op_skinny` -> `l2s_op_skinny` -> `launch_skinny` - the product's validation, form rule and dispatch table -
at 1, 13, 49, 113, 170, 200 and 500 rows, once per distinct (rows, planes, kernel line) of the sweep of tests/skinny_op_common.py (1078 launches that reach
all 96 unstamped kernel instances: tests/test_skinny_op_host.py), and every row of every output is compared with plain fp64 torch on the unpacked tensors.

Gates
  * every form: max |d| < 2e-5 on these unit-scale outputs (the operator gate of test_gemm_operator, at larger K than any here);
  * split-bf16 forms (rc4x, rc8x, rc4h, sp): also error <= 1.5 x the f32 form's error on the same launch + 1e-7 (the rule of test_gemm_split_bf16_operator);
  * within one (site, rows): all f32 forms give the same bits, and all split-bf16 forms give the same bits;
  * no sentinel survives inside [B] x [N]; nothing is written at rows >= B or at columns >= N;
  * a launch that l2s_op_skinny_form refuses is refused by the op with the same text, and writes nothing;
  * the early-stop twin: the plain kernel's bits while es_step < *es_end, nothing written from es_step >= *es_end on.
The largest split-bf16 / f32 error ratio seen on the MI355X is recorded in the docstring of test_site_against_fp64."""
import pytest
import torch

from lip2speech_amd import native
import skinny_op_common as sk

pytestmark = pytest.mark.gpu

NONE, RELU, SILU, PSINE = range(4)
GATE = 2e-5
SENT = native.SKINNY_SENTINEL
TABLE = sk.load_table()
SITES = list(TABLE["sites"])

# what the JSON's integers leave open, per group of each call site (l2s_api.hip): the activation, the valid columns, the addends
_FIRST = [dict(act=PSINE, N=256), dict(act=PSINE, N=512, addrow=True), dict(act=SILU, N=256)]      # prenet layer 1, Q + pos, content Q
DETAIL = {
    "bilstm_step": [dict(H=512, pre=True), dict(H=512, pre=True)],
    "phase_a_unfolded": _FIRST, "phase_a_folded_step0": _FIRST, "phase_a_folded": _FIRST + [dict(yfrag=False)],
    "step_attention_proj": [dict(act=NONE, N=256, add=True)],
    "phase_d_k1536": [dict(H=512)], "phase_d_k1280": [dict(H=512)], "phase_d_k1024_sum": [dict(H=512)], "phase_d_k1024_unfolded": [dict(H=512)],
    "phase_e": [dict(H=512)],
    "step_fc_out_stop": [dict(yfrag=True)],
    "spk_lstm_step": [dict(H=256, pre=True)],
}


def make_groups(site_groups, detail, B, seed):
    """the op's group dicts for one call site at B rows, on the device: seeded randn activations, weights randn / sqrt(K), |c_prev| <= 1, every addend of order 1"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen).cuda()
    out = []
    for (n0, n1, n2, n3, ntiles, epi, a_sum), det in zip(site_groups, detail):
        segs = [16 * n for n in (n0, n1, n2, n3) if n]
        K = sum(segs)
        N = {sk.LSTM: 16 * ntiles, native.SK_MEL: 81}.get(epi, det.get("N"))
        g = dict(epi=epi, ntiles=ntiles, a=[rn(B, k) for k in segs], W=rn(N, K) / K ** 0.5, bias=rn(N))
        if a_sum:
            g["a_sum"] = rn(B, segs[1])
        if epi == sk.LSTM:
            H = det["H"]
            # the new hidden state lands at a column offset inside a wider frag16 buffer; both plain copies are asked for
            g.update(H=H, c_prev=(torch.rand(B, H, generator=gen) * 2 - 1).cuda(), h_out_K=H + 64, h_out_off=32, h_seq=True, h_plain=True)
            if det.get("pre"):
                g["pre"] = rn(B, 4 * H)
        elif epi == native.SK_MEL:
            g.update(stop_const=rn(B), yfrag=det["yfrag"])
        else:
            g.update(act=det["act"], actw=rn(N))
            if det.get("add"):
                g["add"] = rn(B, N)
            if det.get("addrow"):
                g["addrow"] = rn(N)
            if epi == native.SK_PLAIN:
                g["ldo"] = N + 16         # spare columns in every row: a write at a column >= N shows as a lost sentinel
        out.append(g)
    return out


def reference(groups):
    """plain fp64 torch on the unpacked tensors -> per group {output name: [B][columns]}"""
    refs = []
    for g in groups:
        a = [x.double() for x in g["a"]]
        if g.get("a_sum") is not None:
            a[1] = a[1] + g["a_sum"].double()
        v = torch.cat(a, dim=1) @ g["W"].double().t() + g["bias"].double()
        if g["epi"] == sk.LSTM:
            if g.get("pre") is not None:
                v = v + g["pre"].double()
            i, f, gg, o = v.chunk(4, dim=1)
            c = torch.sigmoid(f) * g["c_prev"].double() + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            refs.append(dict(c_out=c, h_out=h, h_seq=h, h_plain=h))
        elif g["epi"] == native.SK_MEL:
            r = dict(mel=v[:, :80], stop=(v[:, 80] + g["stop_const"].double()).unsqueeze(1))
            if g["yfrag"]:
                r["yfrag"] = v[:, :80]
            refs.append(r)
        else:
            v = [v, v.relu(), v * torch.sigmoid(v), torch.sin(v) * g["actw"].double()][g["act"]]
            if g.get("add") is not None:
                v = v + g["add"].double()
            if g.get("addrow") is not None:
                v = v + g["addrow"].double()
            refs.append(dict(out=v))
    return refs


def check_against(outs, refs, groups, B):
    """-> the largest |d| over every output of the launch; asserts that the outputs are written exactly on [B] x [their columns]"""
    worst = 0.0
    for gi, (o, r, g) in enumerate(zip(outs, refs, groups)):
        assert set(o) == set(r), (set(o), set(r))
        for name, ref in r.items():
            full = o[name]
            c0 = g["h_out_off"] if name == "h_out" else 0
            got = full[:B, c0:c0 + ref.shape[1]]
            assert not (got == SENT).any(), f"group {gi} {name}: {(got == SENT).sum().item()} elements inside [B] x [N] were never written"
            mask = torch.ones_like(full, dtype=torch.bool)
            mask[:B, c0:c0 + ref.shape[1]] = False
            stray = (full != SENT) & mask
            assert not stray.any(), f"group {gi} {name}: writes outside [B] x [N] at {stray.nonzero()[:4].tolist()}"
            worst = max(worst, (got.double() - ref).abs().max().item())
    return worst


def same_bits(a, b):
    return all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in x)


def untouched(outs):
    return all((t == SENT).all().item() for o in outs for t in o.values())


_model_cache = {}


def model_for(D, options):
    key = tuple(map(tuple, options))
    if key not in _model_cache:
        _model_cache[key] = sk.diag_model(D, options)
    return _model_cache[key]


def run_case(D, groups, prepared, B, planes, options, chains, refused=None, es=None):
    gs = [dict(g, planes=bool(planes and g["epi"] == sk.LSTM)) for g in groups]
    pr = prepared[1 if planes else 0]
    native.set_thread_chains(chains)
    try:
        return native.op_skinny(model_for(D, options), gs, B, es=es, refused=refused, prepared=pr)
    finally:
        native.set_thread_chains(1)


def prepare_both(groups, B):
    """the packed inputs without and with the plane buffers of the LSTM groups (the same tensors otherwise)"""
    plain = native.op_skinny_prepare(groups, B)
    with_planes = native.op_skinny_prepare([dict(g, planes=g["epi"] == sk.LSTM) for g in groups], B) if any(g["epi"] == sk.LSTM for g in groups) else plain
    return plain, with_planes


@pytest.mark.parametrize("site", SITES)
def test_site_against_fp64(site):
    """Every kernel form the sweep finds for this call site, at every row count, all rows against fp64.

    Measured on the MI355X, largest |d| against fp64 over all rows and forms: the first-phase launches 2.2e-6 (f32), attention_proj 8.6e-7, fc_out + stop 7.5e-7,
    the LSTM launches 8.0e-7 on the f32 forms and 6.0e-7 on the split-bf16 forms (BiLSTM step 5.3e-7 / 4.5e-7, speaker LSTM 3.9e-7, f32 only: K = 256 has no
    split-bf16 layout).  Largest split-bf16 / f32 error ratio: 1.02 (layer 0 with the summed segment at 113 rows; 0.48 - 0.98 elsewhere)."""
    D = native.diag()
    cases = sk.sweep(D, TABLE, sites=[site])
    site_groups, detail = TABLE["sites"][site], DETAIL[site]
    assert len(site_groups) == len(detail)
    worst_f32 = worst_x3 = worst_ratio = 0.0
    n_launch = n_refused = 0
    for B in sk.ROWS:
        groups = make_groups(site_groups, detail, B, seed=1000 * SITES.index(site) + B)
        refs = reference(groups)
        prepared = prepare_both(groups, B)
        first = {}       # x3? -> (outputs, error, line) of the first form of that arithmetic at this (site, rows)
        pending_x3 = []
        for _, rows, planes, line, options, chains in cases:
            if rows != B:
                continue
            if line.startswith("ERROR "):
                refused = []
                outs = run_case(D, groups, prepared, B, planes, options, chains, refused=refused)
                torch.cuda.synchronize()
                assert len(refused) == 1 and refused[0].endswith("]") and refused[0].split(" [")[0] == line[len("ERROR "):].split(" [")[0], (refused, line)
                assert untouched(outs), f"{site} B={B} {options}: a refused launch wrote to its outputs"
                n_refused += 1
                continue
            outs = run_case(D, groups, prepared, B, planes, options, chains)
            err = check_against(outs, refs, groups, B)
            n_launch += 1
            x3 = sk.is_x3(line)
            assert err < GATE, f"{site} B={B} {line} {options} chains={chains}: max |d| {err:.2e}"
            if x3 not in first:
                first[x3] = (outs, err, line)
            else:
                assert same_bits(outs, first[x3][0]), f"{site} B={B}: {line} ({options}, chains={chains}) and {first[x3][2]} give different bits"
            if x3:
                pending_x3.append((err, line))
        if pending_x3:
            assert False in first, f"{site} B={B}: no f32 form to compare the split-bf16 forms with"
            e32 = first[False][1]
            for e3, line in pending_x3:
                assert e3 <= 1.5 * e32 + 1e-7, f"{site} B={B} {line}: split-bf16 error {e3:.2e} against f32 {e32:.2e}"
            worst_ratio = max(worst_ratio, max(e for e, _ in pending_x3) / e32)
            worst_x3 = max(worst_x3, max(e for e, _ in pending_x3))
            print(f"  {site} B={B}: f32 {e32:.2e}  split-bf16 {pending_x3[0][0]:.2e}  ratio {pending_x3[0][0] / e32:.2f}")
        worst_f32 = max(worst_f32, first[False][1])
    print(f"{site}: {n_launch} launches, {n_refused} refused; max |d| f32 forms {worst_f32:.2e}, split-bf16 forms {worst_x3:.2e}, largest ratio {worst_ratio:.2f}")
    assert n_launch + n_refused == len(cases)


@pytest.mark.parametrize("act", [NONE, RELU, SILU, PSINE])
@pytest.mark.parametrize("epi", [native.SK_PLAIN, native.SK_FRAG])
def test_every_activation(act, epi):
    """One extra group per activation (no call site uses ReLU), K = 512, with a column count that is no multiple of 16 (N = 250 in 16 tiles: the last tile's
    columns >= N stay unwritten) and both addends, at 13 and 200 rows, one and three chains."""
    D = native.diag()
    for B in (13, 200):
        gen = torch.Generator().manual_seed(77 + B + act)
        rn = lambda *s: torch.randn(*s, generator=gen).cuda()
        N, K = 250, 512
        g = dict(epi=epi, ntiles=16, a=[rn(B, K)], W=rn(N, K) / K ** 0.5, bias=rn(N), act=act, actw=rn(N), add=rn(B, N), addrow=rn(N))
        refs = reference([g])
        want = None
        for chains in (1, 3):
            native.set_thread_chains(chains)
            try:
                outs = native.op_skinny(model_for(D, []), [g], B)
            finally:
                native.set_thread_chains(1)
            err = check_against(outs, refs, [g], B)
            print(f"  act {act} epi {epi} B={B} chains={chains}: max |d| {err:.2e}")
            assert err < GATE
            want = want or outs
            assert same_bits(outs, want)


@pytest.mark.parametrize("site", ["phase_e", "phase_a_folded"])
def test_early_stop_twin(site):
    """The early-stop twin of the kernel (SkinnyBatch::es_end set) at 200 rows, one LSTM launch and one first-phase launch, default options at one and three
    chains, planes present: the plain entry's bits while es_step < *es_end, every output still the sentinel from es_step >= *es_end on."""
    D = native.diag()
    B = 200
    site_groups, detail = TABLE["sites"][site], DETAIL[site]
    groups = make_groups(site_groups, detail, B, seed=4242 + SITES.index(site))
    prepared = prepare_both(groups, B)
    refs = reference(groups)
    for chains in (1, 3):
        plain = run_case(D, groups, prepared, B, 1, [], chains)
        assert check_against(plain, refs, groups, B) < GATE
        for end, step in ((0, -1), (-3, -4)):
            live = run_case(D, groups, prepared, B, 1, [], chains, es=(end, step))
            assert same_bits(live, plain), f"{site} chains={chains}: the early-stop twin at step {step} < end {end} differs from the plain kernel"
        for end, step in ((-3, -3), (-3, -1), (0, 0)):
            dead = run_case(D, groups, prepared, B, 1, [], chains, es=(end, step))
            assert untouched(dead), f"{site} chains={chains}: the early-stop twin wrote at step {step} >= end {end}"
