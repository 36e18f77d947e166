"""The decode loop at MANY rows per launch, every row against the fp64 oracle.

The launches of 176 - 512 rows - the benchmark's own forms: skinny_sp_kernel, skinny_rc4h_kernel, the 4x2 blocks, skinny_flat_kernel<.., 2> - were compared
with each other bit for bit (test_half_cu_block_forms_same_bits, test_lstm_shared_panel_gpu.py) and with a reference on rows 0-1 only.  Here the whole loop
runs at 113 - 512 rows on soft attention weights (tests/test_soft_attention.py: both temperatures x 1e-3, so that every frame's weight counts), from a `vis`
built of L2-normalised random features and synthetic embeddings - no encoder - and mel frames, stop logits and attention weights of ALL rows are held to the
fp64 oracle on the same inputs.  Stop-derived lengths are not compared: min |stop| is about 7e-5 on these inputs, inside STOP_MARGIN.

The fp32 oracle's own distance from the fp64 one is printed next to each case's errors (measured on the CPU, (rows, T) -> mel / attention: (208, 8) 1.4e-7 /
1.4e-6, (513, 8) 1.8e-7 / 1.3e-6, (256, 29) 1.1e-7 / 6.1e-7); the gates are those of test_soft_attention.py."""
import pytest
import torch

from lip2speech_amd import native, synth
from oracle import l2s_oracle as orc
import parity_common as pc
import skinny_op_common as sk
from test_soft_attention import ATTN_TOL, assert_soft, content_m, decoder_oracle, soft_model, soft_state_dict

gpu = pytest.mark.gpu

# (rows, T, S, chains): 8, 13, 16 and 32 row tiles; 200 rows leave the 4x2 blocks a partial row block and a ragged last tile; three chains = the half-CU forms
CASES = [(113, 8, 4, 1), (200, 8, 4, 1), (200, 8, 4, 3), (256, 29, 4, 1), (256, 29, 4, 3), (512, 8, 4, 3)]
F32_CASE = (200, 8, 4, 3)            # also on a model with "lstm_x3" = 0: the f32 forms get an all-rows anchor
MEL_STOP_TOL = 1e-4
# the batch-row launches of the prologue's BiLSTM recurrence and of one folded decode step under the default options (l2s_api.hip), by their names in
# skinny_forms.json
STEP_SITES = ("bilstm_step", "phase_a_folded_step0", "phase_a_folded", "phase_d_k1024_sum", "phase_e", "step_fc_out_stop")


def test_cases_reach_the_many_row_forms():
    """Host side (no GPU): over CASES the launches of the BiLSTM step and of the decode step take the shared-panel and half-CU LSTM blocks, the eight-wave 4x2 split-bf16 block and the flat
    first phase in both its straight-line forms (eight waves alone, four waves under overlap)."""
    D = native.diag()
    table = sk.load_table()
    m = sk.diag_model(D, [])
    try:
        reached = {sk.kernel_of(sk.form_line(D, m, table["sites"][site], 1, rows, chains)) for rows, _, _, chains in CASES for site in STEP_SITES}
    finally:
        D.l2s_model_destroy(m)
    for want in ("skinny_sp_kernel", "skinny_rc4h_kernel", "skinny_rc8x_kernel<4, 2, "):
        assert any(k.startswith(want) for k in reached), (want, sorted(reached))
    flat = {k.split(", ")[2] for k in reached if k.startswith("skinny_flat_kernel<")}      # <S8, S4, STATIC, stamped>
    assert {"1", "2"} <= flat, sorted(reached)


_oracle = {}


def inputs_and_oracle(sd, rows, T, S):
    """seeded inputs and the fp64 oracle's loop on them (cached per shape: the chain counts and models share it), with the fp32 oracle's spread"""
    key = (rows, T, S)
    if key not in _oracle:
        tag = f"rows{rows}_{T}"
        feat = torch.nn.functional.normalize(torch.randn(rows, T, 768, generator=torch.Generator().manual_seed(rows * 100 + T)), dim=2)
        emb, gum = synth.synth_speaker_embedding(rows, tag=tag), synth.synth_gumbel(rows * content_m(T), tag=tag)
        ref = decoder_oracle(sd, feat, emb, gum, S)
        assert_soft(ref)
        with torch.no_grad():
            st = orc.decoder_prologue(sd, orc.build_visual(feat, emb), emb, gum)
            mel32, stop32, attn32 = orc.decode_loop(sd, st, S)
        spread = (pc.maxdiff(mel32.permute(0, 2, 1), ref["mel"]), pc.maxdiff(stop32, ref["stop"]), pc.maxdiff(attn32, ref["attn"]))
        _oracle[key] = (feat, emb, gum, ref, spread)
    return _oracle[key]


def run_loop(nm, feat, emb, gum, rows, T, S, chains):
    vis = orc.build_visual(feat, emb).contiguous().cuda()
    native.set_thread_chains(chains)
    try:
        state, _ = nm.decoder_prologue(vis, emb.cuda(), gum.cuda())
        mel, stop, attn = nm.decode_steps(state, rows, T, S, want_attn=True)
        torch.cuda.synchronize()
    finally:
        native.set_thread_chains(1)
    return mel, stop, attn


def check_all_rows(tag, out, ref, spread):
    mel, stop, attn = out
    d_mel, d_stop, d_attn = pc.maxdiff(mel.permute(0, 2, 1), ref["mel"]), pc.maxdiff(stop, ref["stop"]), pc.maxdiff(attn, ref["attn"])
    print(f"{tag}: max |d| over all rows mel {d_mel:.2e} stop {d_stop:.2e} attention {d_attn:.2e}  (fp32 oracle: {spread[0]:.2e} {spread[1]:.2e} {spread[2]:.2e}; "
          f"largest attention weight {ref['attn'].max().item():.3f}, min |stop| {ref['stop'].abs().min().item():.1e})")
    assert d_mel < MEL_STOP_TOL and d_stop < MEL_STOP_TOL, (tag, d_mel, d_stop)
    assert d_attn < ATTN_TOL, (tag, d_attn)


@gpu
@pytest.mark.parametrize("rows,T,S,chains", CASES)
def test_decode_loop_all_rows_against_fp64(synth_sd, rows, T, S, chains):
    """HIP prologue + decode_steps under the default options, all rows.  Measured on the MI355X, max |d| mel / stop / attention (fp32 oracle's spread):
    113 rows 7.4e-8 / 6.9e-8 / 8.7e-8 (1.2e-7 / 6.5e-8 / 1.3e-6); 200 rows, one and three chains, 1.1e-7 / 6.3e-8 / 7.4e-8 (1.2e-7 / 8.1e-8 / 1.4e-6);
    256 rows T = 29, one and three chains, 5.6e-8 / 6.7e-8 / 5.6e-8 (1.1e-7 / 8.4e-8 / 1.0e-6); 512 rows 1.0e-7 / 5.7e-8 / 8.6e-8 (1.1e-7 / 8.4e-8 / 1.6e-6)."""
    sd = soft_state_dict(synth_sd)
    feat, emb, gum, ref, spread = inputs_and_oracle(sd, rows, T, S)
    out = run_loop(soft_model(sd), feat, emb, gum, rows, T, S, chains)
    check_all_rows(f"rows {rows} T {T} S {S} chains {chains}", out, ref, spread)


@gpu
def test_decode_loop_all_rows_f32_forms(synth_sd):
    """the same on a model with "lstm_x3" = 0: the LSTM launches on the f32 matrix pipe"""
    rows, T, S, chains = F32_CASE
    sd = soft_state_dict(synth_sd)
    feat, emb, gum, ref, spread = inputs_and_oracle(sd, rows, T, S)
    out = run_loop(soft_model(sd, lstm_x3=0), feat, emb, gum, rows, T, S, chains)
    check_all_rows(f"rows {rows} T {T} S {S} chains {chains} lstm_x3=0", out, ref, spread)
