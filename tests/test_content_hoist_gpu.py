"""The hoisted content projection of the decode step's LSTM layer 0 (option "hoist_vproj" = 3, the default for clips of at most 8 content slots).  `-m gpu`.

Layer 0 of the folded step used to run K = 1024 on [content | prenet + a.V' | h0] with content = alpha @ value.  `value` is fixed for the call, so
W_ih[:, content] (alpha @ value) = sum_j alpha_j (W_ih[:, content] value_j): the prologue computes P = value W_ih[:, content]^T once (the state's
L2S_ST_CP table), the attention launch stores alpha instead of content, layer 0 runs K = 768 on [prenet + a.V' | h0] and its cell threads add
sum_j alpha_j P_j after the K-slice partials and before the bias.  tests/test_content_hoist_host.py pins the algebra; this file pins the launches."""
import pytest
import torch

from lip2speech_amd import native, synth
import parity_common as pc
import skinny_op_common as sk

pytestmark = pytest.mark.gpu

H = 512
SITE = "phase_d_k768_hoist"
# the new call site in the integers of tests/golden/skinny_forms.json "sites" ([nchunks x 4, ntiles, epi, a_sum set]): an empty segment 0, the summed
# prenet + a.V' segment, h0; 128 tiles of 16 gate rows; the LSTM epilogue
SITE_GROUPS = [[0, 16, 32, 0, 128, sk.LSTM, 1]]


def _layer0_case(B, m, seed):
    """synthetic operands of one layer-0 launch on B rows with m content slots, and the float64 restatement of the UNHOISTED formula"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen).cuda()
    W_ih, W_hh, bias = rn(4 * H, 512) / 32.0, rn(4 * H, 512) / 32.0, rn(4 * H)          # [content 256 | u 256], randn / sqrt(K = 1024)
    value, alpha = rn(B, m, 256), torch.softmax(rn(B, m) * 2.0, dim=1)                   # rows of alpha sum to 1
    p2, o, h0 = rn(B, 256), rn(B, 256), rn(B, H)
    c0 = (torch.rand(B, H, generator=gen) * 2 - 1).cuda()
    cc64 = torch.bmm(alpha.double().unsqueeze(1), value.double()).squeeze(1)
    gates = torch.cat([cc64, p2.double() + o.double()], dim=1) @ W_ih.double().t() + h0.double() @ W_hh.double().t() + bias.double()
    i, f, g, og = gates.chunk(4, dim=1)
    c = torch.sigmoid(f) * c0.double() + torch.sigmoid(i) * torch.tanh(g)
    h = torch.sigmoid(og) * torch.tanh(c)
    # = 2: content = alpha @ value as the attention launch forms it (an fmaf chain in fp32, j ascending), then K = 1024 with the summed segment
    cc32 = torch.zeros(B, 256, device="cuda")
    for j in range(m):
        cc32 = torch.addcmul(cc32.double(), alpha[:, j:j + 1].double(), value[:, j].double()).float()      # one rounding per term, as fmaf
    old = dict(epi=sk.LSTM, ntiles=128, a=[cc32, p2, h0], a_sum=o, W=torch.cat([W_ih, W_hh], dim=1), bias=bias, H=H, c_prev=c0, planes=True)
    # = 3: P = value W_ih[:, content]^T in fp32 (the prologue's f32 GEMM stands behind it in the product), slot fastest at pitch ceil4(m), alpha padded to 8
    pitch = (m + 3) // 4 * 4
    P = torch.zeros(B, 4 * H, pitch, device="cuda")
    P[:, :, :m] = torch.einsum("bjk,nk->bnj", value.double(), W_ih[:, :256].double()).float()
    al8 = torch.zeros(B, 8, device="cuda")
    al8[:, :m] = alpha
    new = dict(epi=sk.LSTM, ntiles=128, a=[p2.new_zeros(B, 0), p2, h0], a_sum=o, W=torch.cat([W_ih[:, 256:], W_hh], dim=1), bias=bias, H=H, c_prev=c0,
               planes=True, hoist_p=P, hoist_alpha=al8)
    return old, new, dict(c_out=c, h_out=h)


def _err(outs, ref, B):
    return max((outs[0][k][:B].double() - ref[k]).abs().max().item() for k in ("c_out", "h_out"))


@pytest.mark.parametrize("rows,chains", [(3, 2), (16, 2), (192, 2), (256, 2), (192, 1), (256, 1)])
@pytest.mark.parametrize("m", [4, 7])
def test_layer0_launch_against_fp64(rows, chains, m):
    """One layer-0 launch, the K = 768 form with the hoisted term and the K = 1024 form, against a float64 restatement of the unhoisted formula: a partial
    tile, one tile, and the first and the benchmark's row counts that take the shared-panel form under two chains (also alone).  m = 4 is the benchmark's
    table pitch, m = 7 the 8-float pitch.  The inference launch stores the new cell and hidden state, not the gates: they are compared through both.
    The new form may err at most twice as much as the old one on the same inputs (one more rounding stage); a layout or order bug shows as 1e-3 or worse.

    Measured on the MI355X, max |d| against fp64 over c and h: the K = 768 hoisted form 2.6e-7 - 5.4e-7, the K = 1024 form 3.1e-7 - 6.2e-7 on the same inputs;
    ratio new / old 0.71 - 1.00 at m = 4 and 1.00 - 1.40 at m = 7 (largest at 3 rows)."""
    D = native.diag()
    old, new, ref = _layer0_case(rows, m, seed=100 * rows + m)
    model = sk.diag_model(D, [])
    native.set_thread_chains(chains)
    try:
        e_old = _err(native.op_skinny(model, [old], rows), ref, rows)
        out_new = native.op_skinny(model, [new], rows)
        e_new = _err(out_new, ref, rows)
    finally:
        native.set_thread_chains(1)
        D.l2s_model_destroy(model)
    print(f"layer 0, {rows} rows, {chains} chains, m = {m}: max |d| against fp64  K=1024 form {e_old:.3e}  K=768 hoisted form {e_new:.3e}  ratio {e_new / e_old:.2f}")
    for k in ("c_out", "h_out"):
        full = out_new[0][k]
        assert not (full[:rows] == native.SKINNY_SENTINEL).any() and (full[rows:] == native.SKINNY_SENTINEL).all(), k      # written exactly on the rows
    assert e_new <= 2.0 * e_old


@pytest.mark.parametrize("rows", [192, 256])
def test_block_forms_of_the_new_site_agree(rows):
    """skinny_sp (three chains, default), rc4h ("lstm_x3" = 3) and rc8x (a chain alone) run the new site with the same bits; so do the small-block forms."""
    D = native.diag()
    _, new, _ = _layer0_case(rows, 4, seed=7 + rows)
    prepared = native.op_skinny_prepare([new], rows)
    outs, lines = {}, {}
    for name, options, chains in (("sp", [], 3), ("rc4h", [("lstm_x3", 3)], 3), ("rc8x", [], 1), ("rc8x_22", [("skinny_rc", 22)], 1), ("rc4x_11", [("lstm_x3", 1), ("skinny_rc", 11)], 1)):
        model = sk.diag_model(D, options)
        lines[name] = sk.form_line(D, model, SITE_GROUPS, 1, rows, chains)
        native.set_thread_chains(chains)
        try:
            outs[name] = native.op_skinny(model, [new], rows, prepared=prepared)
        finally:
            native.set_thread_chains(1)
            D.l2s_model_destroy(model)
    print(lines)
    # (a chain alone takes the eight-wave blocks: 4x2 at 256 rows, 2x2 at 192, where 4x2 blocks would leave a quarter of the CUs idle)
    assert lines["sp"].startswith("skinny_sp_kernel<7>") and lines["rc4h"].startswith("skinny_rc4h_kernel<4, 2, 7")
    assert lines["rc8x"].startswith("skinny_rc8x_kernel<4, 2, 7" if rows == 256 else "skinny_rc8x_kernel<2, 2, 7")
    assert lines["rc8x_22"].startswith("skinny_rc8x_kernel<2, 2, 7") and lines["rc4x_11"].startswith("skinny_rc4x_kernel<1, 1, 7")
    for name in outs:
        for k in ("c_out", "h_out"):
            assert torch.equal(outs[name][0][k], outs["sp"][0][k]), (name, k)


@pytest.fixture(scope="module")
def models(synth_sd):
    """the default model (hoist_vproj = 3) and one on the K = 1024 form, both of the diagnostic build"""
    return pc.fresh_native_model(synth_sd, diag=True), pc.fresh_native_model(synth_sd, hoist_vproj=2)


def _inputs(B, T, tag):
    return synth.synth_video(B, T, tag=tag).cuda(), synth.synth_speaker_embedding(B, tag=tag).cuda(), synth.synth_gumbel(B * native.min_T(T), tag=tag).cuda()


def test_end_to_end_against_k1024_form(models):
    """B = 2, T = 29, S = 24: the default against "hoist_vproj" = 2 - equal lengths, mel_post within the 1e-3 gate of the fp32 goldens."""
    new, old = models
    v, e, g = _inputs(2, 29, "hoist-e2e")
    a, b = new.inference(v, e, g, S=24, want_attn=True), old.inference(v, e, g, S=24, want_attn=True)
    d = pc.maxdiff(a[0], b[0])
    print(f"default (K = 768, hoisted content) against hoist_vproj = 2, B = 2, T = 29, S = 24: max |d mel_post| {d:.3e}")
    assert torch.equal(a[1], b[1]) and d < 1e-3
    assert not torch.equal(a[0], b[0])      # another order of the same sums: the new form did run


def test_masked_clip_equals_its_solo_call(models):
    """Lengths [13, 29] (one and four content slots) padded to T = 29: each clip is its solo call at T = len, bit for bit, under the new form."""
    new, _ = models
    T, S, lens = 29, 12, [13, 29]
    v, e, g = _inputs(2, T, "hoist-mask")
    for b, L in enumerate(lens):
        v[b, :, L:] = 0
    got = new.inference(v, e, g, S=S, want_attn=True, video_lengths=lens)
    for b, L in enumerate(lens):
        mT, mL = native.min_T(T), native.min_T(L)
        solo = new.inference(v[b:b + 1, :, :L].contiguous(), e[b:b + 1], g[b * mT:b * mT + mL].contiguous(), S=S, want_attn=True)
        assert torch.equal(got[0][b], solo[0][0]) and torch.equal(got[1][b], solo[1][0]) and torch.equal(got[2][b, :, :L], solo[2][0]), (b, L)


def test_long_clips_fall_back_to_k1024(models):
    """T = 63 (nine content slots): the default is "hoist_vproj" = 2, bit for bit; T = 56 (eight slots) still takes the new form."""
    new, old = models
    v, e, g = _inputs(2, 63, "hoist-t63")
    a, b = new.inference(v, e, g, S=8), old.inference(v, e, g, S=8)
    assert native.min_T(63) == 9 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    v, e, g = _inputs(2, 56, "hoist-t56")
    a, b = new.inference(v, e, g, S=8), old.inference(v, e, g, S=8)
    d = pc.maxdiff(a[0], b[0])
    print(f"T = 56 (m = 8, table pitch 8): max |d mel_post| against hoist_vproj = 2 {d:.3e}")
    assert native.min_T(56) == 8 and not torch.equal(a[0], b[0]) and d < 1e-3 and torch.equal(a[1], b[1])
    assert new.step_site(SITE, 3) == [g_[:6] + [1, g_[6]] for g_ in SITE_GROUPS]      # the site the default launches at m <= 8


def test_grouped_batches_equal_single_calls(models):
    """inference_multi of two batches of three clips: each batch is its single call, bit for bit (six rows: the small-row forms carry the term too)."""
    new, _ = models
    batches = [_inputs(3, 29, f"hoist-grp{i}") for i in range(2)]
    want = [tuple(t.clone() for t in new.inference(*b, S=12, want_attn=True)) for b in batches]
    got = new.inference_multi(batches, S=12, want_attn=True)
    for a, w in zip(got, want):
        assert torch.equal(a[0], w[0]) and torch.equal(a[1], w[1]) and torch.equal(a[2], w[2])


def test_nan_clip_stays_alone(models):
    """One clip's video set to NaN, B = 3: the other clips keep their bits."""
    new, _ = models
    v, e, g = _inputs(3, 29, "hoist-nan")
    want = new.inference(v, e, g, S=12)[0].clone()
    v2 = v.clone()
    v2[1] = float("nan")
    got = new.inference(v2, e, g, S=12)[0]
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("rows", [3, 256])
def test_site_integers(models, rows):
    """The new site's groups are the integers written in this file (weight planes present); every existing site is held by tests/test_step_sites_gpu.py."""
    new, _ = models
    assert new.step_site(SITE, rows) == [[0, 16, 32, 0, 128, sk.LSTM, 1, 1]]
