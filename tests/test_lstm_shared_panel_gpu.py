"""Option "lstm_x3" = 4 on the GPU: the decode step's two K = 1024 LSTM launches as one eight-wave block per CU (64 rows x 64 gate columns) whose two
column halves share one activation panel through LDS (csrc/skinny_dev.h skinny_block_sp).  The form changes no arithmetic, so everything the staged
loop hands back - mel, stop, attention and the state buffer with the final h / c of both LSTM layers - is compared BITWISE against the half-CU form
("lstm_x3" = 3) on the same inputs, through the diagnostic library's l2s_decode_steps with three chains hinted.  Which form a call launched is read
from the block-stamp log (kind 4 = the shared-panel blocks, kind 1 = the other split-bf16 LSTM blocks)."""
import pytest
import torch

import parity_common as pc
from lip2speech_amd import native, synth

pytestmark = pytest.mark.gpu

T, S = 8, 4             # step 0 takes the BOS path, steps 1-3 the folded one
BMAX = 256
SP_KIND, LSTM_KIND = 4, 1


@pytest.fixture(scope="module")
def ctx(synth_sd):
    model = pc.fresh_native_model(synth_sd, diag=True, persist_decode=0)
    gen = torch.Generator().manual_seed(1024)
    vis = (0.5 * torch.randn(BMAX, T, 1024, generator=gen)).cuda()
    emb = synth.synth_speaker_embedding(BMAX, tag="sp").cuda()
    gum = synth.synth_gumbel(BMAX * native.min_T(T), tag="sp").cuda()
    log = torch.zeros(1 + 3 * 65536, dtype=torch.int64, device="cuda")
    return {"model": model, "vis": vis, "emb": emb, "gum": gum, "log": log, "sd": synth_sd, "states": {}}


def _state(ctx, model, B):
    """The prologue's state for the first B rows (rows are independent), computed once per B and never changed: every run gets a clone."""
    if B not in ctx["states"]:
        m = native.min_T(T)
        ctx["states"][B], _ = model.decoder_prologue(ctx["vis"][:B].contiguous(), ctx["emb"][:B].contiguous(), ctx["gum"][:B * m].contiguous())
    return ctx["states"][B]


def _run(ctx, model, B, x3, state=None):
    """One staged loop with three chains hinted; returns (mel, stop, attn, state after the loop) and the set of block kinds that ran."""
    D, log = native.diag(), ctx["log"]
    st = (_state(ctx, model, B) if state is None else state).clone()
    model.set_option("lstm_x3", x3)
    native.set_thread_chains(3)
    try:
        log[0] = 0
        native.check(D.l2s_op_stamp_log(log.data_ptr(), (log.numel() - 1) // 3), D)
        mel, stop, attn = model.decode_steps(st, B, T, S, want_attn=True)
        torch.cuda.synchronize()
    finally:
        native.check(D.l2s_op_stamp_log(None, 0), D)
        native.set_thread_chains(1)
        model.set_option("lstm_x3", 4)      # the default
    n = int(log[0].item())
    assert 0 < n <= (log.numel() - 1) // 3
    kinds = set(((log[1:1 + 3 * n].view(n, 3)[:, 2] >> 60) & 0xF).tolist())
    print(f"B = {B}, lstm_x3 = {x3}: {n} block records, kinds {sorted(kinds)}")
    return (mel, stop, attn, st), kinds


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B", [192, 208, 200, 256])      # 12 row tiles: the threshold; 13: a row block of one tile; padded rows; the bench's rows
def test_shared_panel_bits(ctx, B):
    ref, k3 = _run(ctx, ctx["model"], B, 3)
    new, k4 = _run(ctx, ctx["model"], B, 4)
    assert LSTM_KIND in k3 and SP_KIND not in k3
    assert SP_KIND in k4 and LSTM_KIND not in k4          # both LSTM launches of every step took the new form
    assert ref[0].isfinite().all() and ref[0].abs().max() > 0
    assert _same(ref, new)


def test_below_threshold_keeps_old_form(ctx):
    ref, k3 = _run(ctx, ctx["model"], 176, 3)
    new, k4 = _run(ctx, ctx["model"], 176, 4)             # 11 row tiles < "half_min_mts" = 12
    assert SP_KIND not in k4 and LSTM_KIND in k4 and k3 == k4
    assert _same(ref, new)


def test_one_chain_keeps_old_form(ctx):
    """Without the chains hint the option changes nothing: a chain that has the chip to itself keeps the eight-wave blocks."""
    D, log, model = native.diag(), ctx["log"], ctx["model"]
    st = _state(ctx, model, 192).clone()
    model.set_option("lstm_x3", 4)
    try:
        log[0] = 0
        native.check(D.l2s_op_stamp_log(log.data_ptr(), (log.numel() - 1) // 3), D)
        out = model.decode_steps(st, 192, T, S, want_attn=True)
        torch.cuda.synchronize()
    finally:
        native.check(D.l2s_op_stamp_log(None, 0), D)
        model.set_option("lstm_x3", 4)      # the default
    n = int(log[0].item())
    kinds = set(((log[1:1 + 3 * n].view(n, 3)[:, 2] >> 60) & 0xF).tolist())
    assert SP_KIND not in kinds and LSTM_KIND in kinds
    ref, _ = _run(ctx, model, 192, 3)
    assert _same(ref[:3], out)


def test_early_stop_symbols(ctx):
    model = ctx["model"]
    model.set_option("early_stop", 1)
    try:
        ref, k3 = _run(ctx, model, 208, 3)
        new, k4 = _run(ctx, model, 208, 4)
    finally:
        model.set_option("early_stop", 0)
    assert SP_KIND in k4 and SP_KIND not in k3
    assert _same(ref, new)


def test_second_instance_other_addresses(ctx):
    """Another model (its own weight blob and planes), another state buffer and another workspace: the same bits."""
    first, _ = _run(ctx, ctx["model"], 200, 4)
    other = pc.fresh_native_model(ctx["sd"], diag=True, persist_decode=0)
    pad = torch.empty(3 << 20, dtype=torch.uint8, device="cuda")      # shifts what the allocator hands out next
    state2 = _state(ctx, ctx["model"], 200).clone()
    other._tls.ws = torch.empty(int(native.diag().l2s_workspace_bytes(200, T, 96, 96, S)) + 4096, dtype=torch.uint8, device="cuda")
    second, k4 = _run(ctx, other, 200, 4, state=state2)
    assert SP_KIND in k4
    assert second[3].data_ptr() != first[3].data_ptr() and other._h.value != ctx["model"]._h.value
    assert _same(first, second)
    del pad
