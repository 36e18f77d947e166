"""The algebra behind option "hoist_vproj" = 3, on the CPU: the content columns of LSTM layer 0 commute with the content soft-max.

The oracle's decode step (oracle/l2s_oracle.py decode_loop, decoder.py:262-271 and 353-375) feeds cc = alpha @ value straight into lstm_cell as the first
256 input columns: no bias and no nonlinearity sits between the two, so

    W_ih0[:, :256] (sum_j alpha_j value_j)  =  sum_j alpha_j (W_ih0[:, :256] value_j)

and the bracket on the right is fixed for the call.  Here the oracle's own functions run one step on the synthetic checkpoint's prologue state, and the
gates they give are compared with the hoisted form: K = 768 on [u | h0] plus sum_j alpha_j P_j with P = value W_ih0[:, :256]^T."""
import torch

from lip2speech_amd import synth
from oracle import l2s_oracle as orc

P_ = "decoder."


def _slots(T):
    """content slots of a T-frame clip: the stride-7 branch of Content.agg is the shortest map (decoder.py:239-260)"""
    return (T - 7) // 7 + 1


def _gates_both_ways(sd, alpha, value, u, h0):
    w_ih, w_hh = sd[P_ + "decoder_rnn.weight_ih_l0"], sd[P_ + "decoder_rnn.weight_hh_l0"]
    b_ih, b_hh = sd[P_ + "decoder_rnn.bias_ih_l0"], sd[P_ + "decoder_rnn.bias_hh_l0"]
    # the oracle's path: Content.forward, then the first line of lstm_cell
    cc = torch.bmm(alpha.unsqueeze(1), value).squeeze(1)
    x = torch.cat([cc, u], dim=1)
    literal = x @ w_ih.t() + b_ih + h0 @ w_hh.t() + b_hh
    # the hoisted path: the per-call table, the K = 768 product, sum_j alpha_j P_j
    P = torch.einsum("bjk,nk->bnj", value, w_ih[:, :256])                         # (B, 2048, m)
    hoisted = torch.cat([u, h0], dim=1) @ torch.cat([w_ih[:, 256:], w_hh], dim=1).t() + torch.einsum("bj,bnj->bn", alpha, P) + b_ih + b_hh
    # what the terms of one gate add up to in magnitude: the yardstick of the float32 bound
    mag = (torch.cat([cc, u], dim=1).abs() @ w_ih.abs().t() + b_ih.abs() + h0.abs() @ w_hh.abs().t() + b_hh.abs()
           + torch.einsum("bj,bnj->bn", alpha.abs(), torch.einsum("bjk,nk->bnj", value.abs(), w_ih[:, :256].abs())))
    return literal, hoisted, mag


def _operands(dtype, B=3, T=29, steps=2, seed=5):
    """alpha, value, u, h0 of the oracle's decode loop at step `steps` on the synthetic checkpoint (random visual features stand for the encoder)"""
    sd = orc.to_dtype(synth.synth_state_dict(), dtype)
    gen = torch.Generator().manual_seed(seed)
    vis = torch.randn(B, T, 1024, generator=gen).to(dtype)
    emb = torch.nn.functional.normalize(torch.randn(B, 256, generator=gen), dim=1).to(dtype)
    gumbel = synth.synth_gumbel(B * _slots(T), tag="hoist-host").to(dtype)
    with torch.no_grad():
        st = orc.decoder_prologue(sd, vis, emb, gumbel)
        alphas = []
        orc.decode_loop(sd, st, steps, alphas=alphas)
    value = st["value"]
    assert value.shape == (B, _slots(T), 256) and alphas[-1].shape == (B, _slots(T))
    # u and h0 of a step: any operands of the right shape pin the algebra; take them at the scale the step sees
    u = torch.randn(B, 256, generator=gen).to(dtype)
    h0 = torch.tanh(torch.randn(B, 512, generator=gen)).to(dtype)
    return sd, alphas[-1], value, u, h0


def test_hoisted_algebra_float64():
    sd, alpha, value, u, h0 = _operands(torch.float64)
    assert torch.allclose(alpha.sum(dim=1), torch.ones(alpha.shape[0], dtype=torch.float64), atol=1e-12)
    literal, hoisted, _ = _gates_both_ways(sd, alpha, value, u, h0)
    rel = ((literal - hoisted).abs().max() / literal.abs().max()).item()
    print(f"float64: max |literal - hoisted| / max |gate| = {rel:.3e}")
    assert rel <= 1e-12


def test_hoisted_algebra_float32():
    """the same in float32: the two orders differ by rounding only - at most 4 eps32 x the sum of the magnitudes of a gate's terms"""
    sd, alpha, value, u, h0 = _operands(torch.float32)
    literal, hoisted, mag = _gates_both_ways(sd, alpha, value, u, h0)
    eps = torch.finfo(torch.float32).eps
    worst = ((literal - hoisted).abs() / (eps * mag)).max().item()
    print(f"float32: max |literal - hoisted| = {worst:.3f} eps32 x sum |terms|")
    assert worst <= 4.0


def test_value_is_fixed_for_the_call():
    """the table can be computed once: the decode loop never writes the content values (the state's `value` is the same tensor before and after)"""
    sd = orc.to_dtype(synth.synth_state_dict(), torch.float64)
    gen = torch.Generator().manual_seed(9)
    vis, emb = torch.randn(2, 29, 1024, generator=gen, dtype=torch.float64), torch.randn(2, 256, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        st = orc.decoder_prologue(sd, vis, emb, synth.synth_gumbel(2 * _slots(29), tag="hoist-host2").double())
        before = st["value"].clone()
        orc.decode_loop(sd, st, 3)
    assert torch.equal(st["value"], before)
