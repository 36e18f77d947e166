"""Training with per-clip mel lengths (include/l2s.h "training with per-clip mel lengths"; running statistics): l2s_loss_lengths and the
l2s_train_postnet_masked_fwd / _masked_bwd entry points against the unmasked ones, a float64 restatement of the contract and the fp64 oracle.

Shapes: 96 x 96 frames, B = 4, T = 22, S = 8, video lengths [7, 13, 22, 16], mel lengths [8, 1, 5, 7]: a full clip, a one-frame clip, a clip whose padding
lies wholly inside the post-net's stacked 10-frame halo, a clip with a single pad row.  B = 17 at T = 14, S = 3 puts clip boundaries inside a 64-row GEMM tile.
Mixed teacher mask and all five dropout sites on unless a test says otherwise.  The rig, the inputs and the error measure are tests/test_masked_train_gpu.py's.

How the bound of `test_as_alone` is set: as there, it is MEASURED.  The same comparison - a batch against the fp64 sum of its clips alone through the
unmasked entry points - on an UNPADDED batch (every clip T frames and S mel frames, unmasked on both sides) gives per tensor class what the reordering of
the fp32 sums costs; the masked step gets 4 x that.  One run's values: profiles/masked_mel_errors.txt."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_common as pc          # noqa: E402
from lip2speech_amd import synth    # noqa: E402
from test_masked_train_gpu import CLASSES, MASK as MASK6, OracleGoldens, Rig, equal_all, inputs, klass, min_T      # noqa: E402

pytestmark = pytest.mark.gpu

LENS, MLENS, T, S = [7, 13, 22, 16], [8, 1, 5, 7], 22, 8
MASK = np.concatenate([MASK6, np.array([1, 0], dtype=np.uint8)])          # (8,): mixed teacher forcing (step 0 always takes BOS)
NAN = float("nan")


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    assert len(r.grads) == 308
    return r


def gate_of(mlens, S):
    """The collates' gate target: 1 from frame S_b - 1 on."""
    g = torch.zeros(len(mlens), S, device="cuda")
    for b, n in enumerate(mlens):
        g[b, n - 1:] = 1.0
    return g


def clip_of(d, b, T, n, S, sb):
    """Clip b of a batch alone at T = n, S = sb: its frames, its first min_T(n) Gumbel rows, its first sb target frames, its rows of every dropout multiplier
    and upstream gradient."""
    m, mb = min_T(T), min_T(n)
    rows = slice(b * m, b * m + mb)
    c = dict(video=d["video"][b:b + 1, :, :n].contiguous(), emb=d["emb"][b:b + 1], gum=d["gum"][rows].contiguous(), mels=d["mels"][b:b + 1, :, :sb].contiguous())
    dr = d["drop"]
    c["drop"] = None if dr is None else dict(feat=dr["feat"][b:b + 1, :n].contiguous(), prenet=dr["prenet"][:sb, b:b + 1].contiguous(),
                                             attn=dr["attn"][:sb, b:b + 1, :n].contiguous(), rnn=dr["rnn"][:sb, b:b + 1].contiguous(),
                                             post=[p[b:b + 1, :, :sb].contiguous() for p in dr["post"]])
    u = d["up"]
    c["up"] = dict(dmel_post=u["dmel_post"][b:b + 1, :, :sb].contiguous(), dmel=u["dmel"][b:b + 1, :sb].contiguous(), dstop=u["dstop"][b:b + 1, :sb].contiguous(),
                   ddis=u["ddis"][rows].contiguous())
    return c


def step(rig, d, mask=MASK, lens=None, mlens=None, route="up"):
    """One training step through the staged entry points.  route "up": fed the explicit upstream gradients of `d` (with `mlens`, those of the loop - dmel, dstop -
    are cut to zeros at pad steps, as the loss gives them; dmel_post goes in as it is); route "loss": through training.loss_terms (gate: 1 from S_b - 1 on).
    Returns outputs, state gradients and a copy of all 308 gradients."""
    from lip2speech_amd import native
    from lip2speech_amd.training import loss_terms
    nm = rig.nm
    video, emb = d["video"], d["emb"]
    B, _, T, _, _ = video.shape
    S = d["mels"].shape[2]
    drop = d["drop"] or {}
    for g in rig.grads.values():
        g.zero_()
    real = None
    if lens is not None:
        real = (torch.arange(T, device="cuda")[None, :] < torch.tensor(lens, device="cuda")[:, None]).unsqueeze(2)
    vis_enc, feat, etape = nm.train_encoder_fwd(video, emb, video_lengths=lens)
    vis = vis_enc.clone()
    if drop.get("feat") is not None:
        vis[:, :, :768] = vis[:, :, :768] * drop["feat"] if real is None else torch.where(real, vis[:, :, :768] * drop["feat"], torch.zeros((), device="cuda"))
    state, dis, ptape = nm.train_prologue_fwd(vis, emb, d["gum"], video_lengths=lens)
    teacher = None
    if mask is not None and mask[:S].any():
        bos = rig.bound["decoder.BOS"].reshape(1, 1, 80).expand(B, 1, 80)
        teacher = torch.cat([bos, d["mels"].permute(0, 2, 1)[:, :S - 1]], dim=1).contiguous()
    (mel, stop, logits), ctx = nm.train_steps_fwd(state, B, T, S, teacher, mask[:S] if teacher is not None else None, drop=drop, video_lengths=lens)
    pdrop = native.postnet_drop_pack(drop["post"]) if drop.get("post") is not None else None
    mel_post, post_tape = nm.train_postnet_fwd(mel, pdrop, mel_lengths=mlens)
    out = {}
    if route == "loss":
        out["loss"], g = loss_terms(mel.permute(0, 2, 1).contiguous(), mel_post, stop, dis, d["mels"], gate_of(mlens if mlens is not None else [S] * B, S),
                                    mel_lengths=mlens, video_lengths=lens if mlens is not None else None)
        up = dict(dmel_post=g["mel_post"], dmel=g["mel"].permute(0, 2, 1), dstop=g["stop"], ddis=g["content_dis"])
        out.update({"g_" + k: v for k, v in g.items()})
    else:
        up = dict(d["up"])
        if mlens is not None:
            pad = torch.arange(S, device="cuda")[None, :] >= torch.tensor(mlens, device="cuda")[:, None]
            up["dmel"] = up["dmel"].masked_fill(pad.unsqueeze(2), 0.0)
            up["dstop"] = up["dstop"].masked_fill(pad, 0.0)
    wbuf = nm.train_pack_weights(video.device)
    dmel = nm.train_postnet_bwd(mel, up["dmel_post"], post_tape, pdrop, mel_lengths=mlens)
    out["dmel_postnet"] = dmel.clone()
    dmel += up["dmel"]
    sg = nm.train_steps_bwd(ctx, dmel, up["dstop"], wbuf=wbuf)
    dvis = nm.train_prologue_bwd(vis, emb, state, ptape, sg, dcontent_dis=up["ddis"], wbuf=wbuf, video_lengths=lens)
    dvis_out = dvis.clone()
    if drop.get("feat") is not None:
        dvis[:, :, :768] = dvis[:, :, :768] * drop["feat"] if real is None else torch.where(real, dvis[:, :, :768] * drop["feat"], torch.zeros((), device="cuda"))
    nm.train_encoder_bwd(video, dvis, etape, video_lengths=lens)
    torch.cuda.synchronize()
    out.update(mel=mel, mel_post=mel_post, stop=stop, logits=logits, dis=dis, vis=vis_enc, feat=feat, dvis=dvis_out)
    out.update(sg)
    return out, {k: g.clone() for k, g in rig.grads.items()}


# ------------------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("B,T,S", [(4, 22, 8), (17, 14, 3), (1, 14, 6)])
def test_full_lengths_are_the_unmasked_bits(rig, B, T, S):
    """All S_b = S and len_b = T: outputs, loss terms, the four loss gradients and all 308 parameter gradients are bit-identical to the unmasked route."""
    rig.bind()
    d = inputs(B, T, S, f"mm-full-{B}")
    for route in ("up", "loss"):
        o0, g0 = step(rig, d, route=route)
        o1, g1 = step(rig, d, lens=[T] * B, mlens=[S] * B, route=route)
        assert equal_all(o0, o1) == [] and equal_all(g0, g1) == [], route
        assert all(torch.isfinite(v).all() for v in g1.values())
    assert rig.nm.calls["l2s_train_postnet_masked_fwd"] >= 2 and rig.nm.calls["l2s_train_postnet_masked_bwd"] >= 2
    # per_clip beside the dispatch to l2s_loss's own launches: every clip's terms, whose mean over the clips is the batch's
    from lip2speech_amd.training import loss_terms
    args = (o1["mel"].permute(0, 2, 1).contiguous(), o1["mel_post"], o1["stop"], o1["dis"], d["mels"], gate_of([S] * B, S))
    loss, g, pcl = loss_terms(*args, mel_lengths=[S] * B, video_lengths=[T] * B, per_clip=True)
    assert torch.equal(loss, o1["loss"]) and all(torch.equal(g[k], o1["g_" + k]) for k in g)
    assert (pcl.double().mean(0) - loss[:4].double()).abs().max() < 2e-6 * loss[:4].abs().max()


# ------------------------------------------------------------------------------------------------------------------------------ 2
def loss64(mel, mel_post, tgt, stop, gate, dis, mlens, mbs):
    """The contract in float64 on the device: per clip over its own extent, the mean over the clips; gradients of the summed batch loss."""
    B, _, S = mel.shape
    m, V = dis.shape[0] // B, dis.shape[1]
    per = torch.zeros(B, 4, dtype=torch.float64, device="cuda")
    g = dict(mel=torch.zeros_like(mel, dtype=torch.float64), mel_post=torch.zeros_like(mel, dtype=torch.float64), stop=torch.zeros_like(stop, dtype=torch.float64),
             content_dis=torch.zeros_like(dis, dtype=torch.float64))
    for b, (sb, mb) in enumerate(zip(mlens, mbs)):
        t = tgt[b, :, :sb].double()
        d0, d1 = mel[b, :, :sb].double() - t, mel_post[b, :, :sb].double() - t
        x, y = stop[b, :sb].double(), gate[b, :sb].double()
        q = dis[b * m:b * m + mb].double()
        lr = torch.log(q * V + 1e-20)
        per[b, 0], per[b, 1] = (d0 * d0).mean(), 10 * (d1 * d1).mean()
        per[b, 2] = (x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean()
        per[b, 3] = (q * lr).sum(1).mean()
        g["mel"][b, :, :sb] = 2 * d0 / (B * 80 * sb)
        g["mel_post"][b, :, :sb] = 20 * d1 / (B * 80 * sb)
        g["stop"][b, :sb] = (torch.sigmoid(x) - y) / (B * sb)
        g["content_dis"][b * m:b * m + mb] = (lr + q * V / (q * V + 1e-20)) / (B * mb)
    terms = per.mean(0)
    return torch.cat([terms, terms.sum()[None]]), per, g


@pytest.mark.parametrize("B,S,Tp,mlens,vlens", [(4, 8, 22, MLENS, LENS), (3, 60, 64, [60, 37, 1], [64, 7, 30])])
def test_loss_kernel_alone(B, S, Tp, mlens, vlens):
    """l2s_loss_lengths against the float64 restatement: the five terms and per_clip within 2e-6 relative (fp64 sums, one fp32 rounding at the end: about
    1.2e-7 expected), gradients within 1e-6 of each tensor's max, exact zeros at pad positions and unused content rows, NaN at every never-read position
    changes no bit, two runs give equal bits.  The second shape strides a clip's 80 x S positions and m x 501 content entries over its blocks more than once."""
    from lip2speech_amd.training import loss_terms
    m, mbs = min_T(Tp), [min_T(v) for v in vlens]
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + S)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)      # noqa: E731
    tgt = synth.synth_mels(B, S, tag="mm-loss").cuda()
    mel, mel_post, stop = tgt + rnd(B, 80, S), tgt + 0.5 * rnd(B, 80, S), 2 * rnd(B, S)
    dis = torch.softmax(3 * rnd(B * m, 501), dim=1)
    for b, mb in enumerate(mbs):
        dis[b * m + mb:(b + 1) * m] = 0.0      # unused content slots: the masked prologue writes zero rows
    gate = gate_of(mlens, S)
    loss, gr, pcl = loss_terms(mel, mel_post, stop, dis, tgt, gate, mel_lengths=mlens, video_lengths=vlens, per_clip=True)
    want, per, g64 = loss64(mel, mel_post, tgt, stop, gate, dis, mlens, mbs)
    rel = ((loss.double() - want).abs() / want.abs()).max().item()
    rel_pc = ((pcl.double() - per).abs() / per.abs()).max().item()
    gerr = {k: ((gr[k].double() - g64[k]).abs().max() / g64[k].abs().max()).item() for k in gr}
    print(f"loss kernel B={B} S={S}: terms rel {rel:.3e}, per_clip rel {rel_pc:.3e} (bound 2e-6), gradients / tensor max {({k: f'{v:.3e}' for k, v in gerr.items()})} (bound 1e-6)")
    assert rel < 2e-6 and rel_pc < 2e-6, (loss, want)
    assert all(v < 1e-6 for v in gerr.values()), gerr
    for b, (sb, mb) in enumerate(zip(mlens, mbs)):
        assert (gr["mel"][b, :, sb:] == 0).all() and (gr["mel_post"][b, :, sb:] == 0).all() and (gr["stop"][b, sb:] == 0).all()
        assert (gr["content_dis"][b * m + mb:(b + 1) * m] == 0).all()
    assert all(torch.isfinite(v).all() for v in gr.values())
    # without per_clip and without gradients: the same five terms
    assert torch.equal(loss_terms(mel, mel_post, stop, dis, tgt, gate, want_grads=False, mel_lengths=mlens, video_lengths=vlens)[0], loss)
    # poison every never-read position; two runs
    mel, mel_post, stop, tgt, gate, dis = (t.clone() for t in (mel, mel_post, stop, tgt, gate, dis))
    for b, (sb, mb) in enumerate(zip(mlens, mbs)):
        for t in (mel, mel_post, tgt):
            t[b, :, sb:] = NAN
        stop[b, sb:] = NAN
        gate[b, sb:] = NAN
        dis[b * m + mb:(b + 1) * m] = NAN
    for _ in range(2):
        loss2, gr2, pcl2 = loss_terms(mel, mel_post, stop, dis, tgt, gate, mel_lengths=mlens, video_lengths=vlens, per_clip=True)
        assert torch.equal(loss2, loss) and torch.equal(pcl2, pcl) and equal_all(gr, gr2) == []


# ------------------------------------------------------------------------------------------------------------------------------ 3
def alone_errors(rig, d, T, lens, mlens, masked, route, mask=MASK):
    """test_masked_train_gpu.alone_errors with mel lengths: the batch (masked: through the masked entry points at the lengths; else unmasked, `lens` = all T and
    `mlens` = all S) against its clips ALONE through the UNMASKED entry points at B = 1, T = len_b, S = S_b, summed in fp64 - with weight 1 / B on the loss
    route, where the clip alone carries its own 1 / (80 S_b) and the batch is the mean over the clips.  Same measures: forward rows max |d| / max |ref|;
    gradients per class max over tensors of max |d| / (max |ref| + 1e-5 x the class's largest gradient entry)."""
    B = len(lens)
    S = d["mels"].shape[2]
    ob, gb = step(rig, d, mask=mask, lens=lens if masked else None, mlens=mlens if masked else None, route=route)
    w = 1.0 / B if route == "loss" else 1.0
    ref = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in gb.items()}
    fwd, terms = {}, torch.zeros(5, dtype=torch.float64)
    for b, (n, sb) in enumerate(zip(lens, mlens)):
        oc, gc = step(rig, clip_of(d, b, T, n, S, sb), mask=mask, route=route)
        for k in ref:
            ref[k] += w * gc[k].double()
        if route == "loss":
            terms += w * oc["loss"].double().cpu()
        m, mb = min_T(T), min_T(n)
        for name, got, want in (("mel", ob["mel"][b, :sb], oc["mel"][0]), ("mel_post", ob["mel_post"][b, :, :sb], oc["mel_post"][0]), ("stop", ob["stop"][b, :sb], oc["stop"][0]),
                                ("logits", ob["logits"][b, :sb, :n], oc["logits"][0]), ("dis", ob["dis"][b * m:b * m + mb], oc["dis"]),
                                ("dvis", ob["dvis"][b, :n], w * oc["dvis"][0])):
            e = (got.double() - want.double()).abs().max().item() / max(want.abs().max().item(), 1e-30)
            fwd[name] = max(fwd.get(name, 0.0), e)
    scale = {c: max(ref[k].abs().max().item() for k in ref if klass(k) == c) for c in CLASSES}
    err = {c: 0.0 for c in CLASSES}
    for k in ref:
        c = klass(k)
        e = (gb[k].double() - ref[k]).abs().max().item() / (ref[k].abs().max().item() + 1e-5 * scale[c])
        err[c] = max(err[c], e)
    err.update({"fwd:" + k: v for k, v in fwd.items()})
    if route == "loss":
        err["loss terms"] = ((ob["loss"].double().cpu() - terms).abs() / terms.abs()).max().item()
    return err, ob, gb


@pytest.fixture(scope="module")
def baseline(rig):
    """An UNPADDED batch of 4 clips of 22 frames and 8 mel frames against its own clips alone, unmasked entry points on both sides, per route."""
    rig.bind()
    base = {}
    for route in ("up", "loss"):
        base[route], _, _ = alone_errors(rig, inputs(4, T, S, "mm-base"), T, [T] * 4, [S] * 4, masked=False, route=route)
        print(f"baseline, route {route} (unpadded batch vs its clips alone):", {k: f"{v:.3e}" for k, v in base[route].items()})
    return base


def check_against_baseline(err, base):
    bad = {k: (v, base[k]) for k, v in err.items() if v > 4.0 * base[k]}
    assert not bad, f"masked step further from its clips alone than 4 x the unpadded baseline: {bad}"


@pytest.mark.parametrize("route", ["up", "loss"])
def test_as_alone(rig, baseline, route):
    """Forward rows < S_b and gradients of the masked step against the clips alone (unmasked, B = 1, T = len_b, S = S_b), summed in fp64; bound = 4 x the measured
    baseline (module docstring; one run's values: profiles/masked_mel_errors.txt).  "up": explicit upstream gradients (post-net and loop); "loss": the whole step
    through l2s_loss_lengths, whose terms are the mean over the clips of each clip's own."""
    rig.bind()
    d = inputs(len(LENS), T, S, "mm-alone", lens=LENS)
    err, ob, gb = alone_errors(rig, d, T, LENS, MLENS, masked=True, route=route)
    print(f"masked lens={LENS} mel lens={MLENS}, route {route}:", {k: f"{v:.3e}" for k, v in err.items()})
    assert all(torch.isfinite(v).all() for v in gb.values())
    check_against_baseline(err, baseline[route])


# ------------------------------------------------------------------------------------------------------------------------------ 4
def test_fp64_oracle(rig):
    """oracle/l2s_oracle.py autograd on each clip ALONE (fp64) with mels[b, :, :S_b] and gate[b, :S_b], all four terms weighted 1 / B, against the masked step
    through training.model_forward_backward(mel_lengths=): check_grads of tests/test_grad_goldens.py at its own tolerances (3e-3 / 6e-3 / 6e-3, saturated floor);
    loss terms within 2e-5 relative, forward rows within 1e-3.  Dropout off (the oracle has none); mixed teacher mask."""
    from lip2speech_amd.training import model_forward_backward
    from oracle import l2s_oracle as orc
    from test_grad_goldens import check_grads
    rig.bind()
    B, m = len(LENS), min_T(T)
    d = inputs(B, T, S, "mm-oracle", lens=LENS, dropout=False)
    gate = gate_of(MLENS, S)
    for g in rig.grads.values():
        g.zero_()
    out = model_forward_backward(rig.nm, d["video"], d["emb"], d["gum"], d["mels"], gate, teacher_mask=torch.from_numpy(MASK.astype(bool)),
                                 bos=rig.bound["decoder.BOS"], video_lengths=LENS, mel_lengths=MLENS)
    torch.cuda.synchronize()
    sd64 = {k: (v.double().requires_grad_(True) if k in rig.grads else (v.double() if v.is_floating_point() else v)) for k, v in rig.sd.items()}
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    terms_sum = np.zeros(4)
    for b, (n, sb) in enumerate(zip(LENS, MLENS)):
        mb = min_T(n)
        mels_b = d["mels"][b:b + 1, :, :sb].cpu().double()
        outs = orc.forward_eval(sd64, d["video"][b:b + 1, :, :n].cpu().double(), d["emb"][b:b + 1].cpu().double(), mels_b,
                                d["gum"][b * m:b * m + mb].cpu().double(), teacher_mask=torch.from_numpy(MASK[:sb].astype(bool)))
        t = orc.loss_terms(outs, mels_b, gate[b:b + 1, :sb].cpu().double())
        ((t[0] + t[1] + t[2] + t[3]) / B).backward()
        terms_sum += np.array([x.item() for x in t[:4]]) / B
        assert pc.maxdiff(out["mel"][b, :, :sb], outs[0][0]) < 1e-3 and pc.maxdiff(out["mel_post"][b, :, :sb], outs[1][0]) < 1e-3
        assert pc.maxdiff(out["stop"][b, :sb], outs[2][0, :, 0]) < 1e-3
    got = out["loss"].cpu().double().numpy()
    assert np.abs(got[:4] - terms_sum).max() < 2e-5 * np.abs(terms_sum).max(), (got, terms_sum)
    z = OracleGoldens({k: sd64[k].grad for k in rig.grads})
    check_grads(z, z.index, rig.grads, z.keys, rel_norm=3e-3, rel_proj=6e-3, rel_full=6e-3)


# ------------------------------------------------------------------------------------------------------------------------------ 5
def test_never_read_and_exact_positions(rig):
    """mel_post[b, :, S_b:] and the pad rows of the post-net's dmel are exact zeros; NaN in the post-net dropout multipliers at pad rows and in the caller's
    dmel_post at pad positions changes no bit of any output or gradient; same bits run to run."""
    rig.bind()
    d = inputs(len(LENS), T, S, "mm-nan", lens=LENS)
    o0, g0 = step(rig, d, lens=LENS, mlens=MLENS)
    o0b, g0b = step(rig, d, lens=LENS, mlens=MLENS)
    assert equal_all(o0, o0b) == [] and equal_all(g0, g0b) == [], "not deterministic"
    for b, sb in enumerate(MLENS):
        for p in d["drop"]["post"]:
            p[b, :, sb:] = NAN
        d["up"]["dmel_post"][b, :, sb:] = NAN
    o1, g1 = step(rig, d, lens=LENS, mlens=MLENS)
    assert equal_all(o0, o1) == [] and equal_all(g0, g1) == []
    assert all(torch.isfinite(v).all() for v in g1.values())
    for b, sb in enumerate(MLENS):
        assert (o1["mel_post"][b, :, sb:] == 0).all() and (o1["mel"][b, sb:] == 0).all()
        assert (o1["dmel_postnet"][b, sb:] == 0).all()
        assert torch.isfinite(o1["mel_post"][b, :, :sb]).all() and o1["mel_post"][b, :, :sb].abs().max() > 0
    for k in ("mel", "mel_post", "stop", "dmel_postnet", "dvis", "dk", "dv", "dckey", "dcval", "dh_init", "de_c"):
        assert torch.isfinite(o1[k]).all(), k


# ------------------------------------------------------------------------------------------------------------------------------ 6
def test_b17_crosses_the_row_tile(rig):
    """17 clips at T = 14, S = 3, mel lengths cycling 1, 2, 3 (B * S = 51 rows: every clip boundary lies inside one 64-row GEMM tile): finite, the exact
    positions, and as alone within the bound of test_as_alone: 4 x the same quantity for an unpadded batch - here of THIS shape, 17 clips of 14 frames and
    3 mel frames through the unmasked entry points against its clips alone.  (The 4-clip baseline does not carry over: from 17 rows on the prologue's
    backward sums its second 16-row tile in another order than a clip alone, video lengths or not - dvis is bit-identical at B = 4 and 1e-6 off at B = 17.)"""
    rig.bind()
    B, Tp, Sp = 17, 14, 3
    lens = [7 + (3 * b) % 8 for b in range(B)]
    mlens = [1 + b % 3 for b in range(B)]
    base, _, _ = alone_errors(rig, inputs(B, Tp, Sp, "mm-b17-base"), Tp, [Tp] * B, [Sp] * B, masked=False, route="up", mask=MASK[:Sp])
    print("baseline, B = 17 (unpadded batch vs its clips alone):", {k: f"{v:.3e}" for k, v in base.items()})
    d = inputs(B, Tp, Sp, "mm-b17", lens=lens)
    err, o, g = alone_errors(rig, d, Tp, lens, mlens, masked=True, route="up", mask=MASK[:Sp])
    print("B = 17, mel lens cycling 1, 2, 3:", {k: f"{v:.3e}" for k, v in err.items()})
    assert all(torch.isfinite(v).all() for v in g.values())
    for b, sb in enumerate(mlens):
        assert (o["mel_post"][b, :, sb:] == 0).all() and (o["dmel_postnet"][b, sb:] == 0).all()
    check_against_baseline(err, base)


# ------------------------------------------------------------------------------------------------------------------------------ 7
def test_batch_statistics_and_bf16_are_refused_by_name(rig):
    """In the library (RuntimeError of the masked post-net calls) and in the Python layer (the model's switch in
    train() mode, train_iterations with bf16; their host halves are in tests/test_masked_mel_host.py)."""
    from lip2speech_amd import callers
    from model.model import get_network
    rig.bind()
    mel = torch.randn(2, 4, 80, device="cuda")
    ok, tape = rig.nm.train_postnet_fwd(mel.clone(), mel_lengths=[4, 2])
    rig.nm.train_set_bn(True, 0.1)
    try:
        with pytest.raises(RuntimeError, match="batch_stats = 1"):
            rig.nm.train_postnet_fwd(mel.clone(), mel_lengths=[4, 2])
        with pytest.raises(RuntimeError, match="batch_stats = 1"):
            rig.nm.train_postnet_bwd(mel, torch.zeros(2, 80, 4, device="cuda"), tape, mel_lengths=[4, 2])
    finally:
        rig.nm.train_set_bn(False)
    rig.nm.set_option("train_bf16", 1)
    try:
        with pytest.raises(RuntimeError, match="train_bf16"):
            rig.nm.train_postnet_fwd(mel.clone(), mel_lengths=[4, 2])
        with pytest.raises(RuntimeError, match="train_bf16"):
            rig.nm.train_postnet_bwd(mel, torch.zeros(2, 80, 4, device="cuda"), tape, mel_lengths=[4, 2])
    finally:
        rig.nm.set_option("train_bf16", 0)
    assert torch.equal(rig.nm.train_postnet_fwd(mel.clone(), mel_lengths=[4, 2])[0], ok)
    with pytest.raises(RuntimeError, match=r"mel_lengths\[1\] = 5 is outside \[1, S = 4\]"):      # the library's own check, past the wrapper's
        rig.nm._check(rig.nm._L.l2s_train_postnet_masked_fwd(rig.nm._h, mel.data_ptr(), 2, 4, tape.data_ptr(), ok.data_ptr(), None, None,
                                                             (__import__("ctypes").c_int32 * 2)(4, 5)))
    net = get_network("train").cuda()
    net.honour_video_lengths = net.train_video_lengths = net.train_mel_lengths = True
    with pytest.raises(NotImplementedError, match="train_mel_lengths: train\\(\\) mode"):
        net(torch.zeros(1, 3, 8, 96, 96, device="cuda"), None, None, torch.zeros(1, 80, 4, device="cuda"), torch.tensor([8]), None, torch.tensor([3]), 1.0,
            speaker_embedding=torch.zeros(1, 256, device="cuda"))
    with pytest.raises(NotImplementedError, match="train_bf16"):
        callers.train_iterations(net, [], 0, honour_lengths=True, honour_mel_lengths=True, bf16=True)


# ------------------------------------------------------------------------------------------------------------------------------ 8
def model_batches():
    """Two synthetic batches of unequal mel length (S = 8 and S = 6), both zero-padded to T = 22."""
    out = []
    for tag, Sp, vl, ml in (("mm-model-a", 8, LENS, MLENS), ("mm-model-b", 6, [22, 9, 14, 7], [6, 3, 6, 2])):
        B = len(vl)
        video = synth.synth_video(B, T, tag=tag)
        for b, n in enumerate(vl):
            video[b, :, n:] = 0.0
        mels = synth.synth_mels(B, Sp, tag=tag)
        gate = gate_of(ml, Sp).cpu()
        audio = torch.zeros(B, 256 * (Sp - 1))
        out.append(((video, torch.tensor(vl)), (audio, torch.full((B,), audio.shape[1])), (mels, torch.tensor(ml), gate), None))
    return out


def fresh_net():
    from model.model import get_network
    net = get_network("train").cuda()
    net.load_state_dict({k: v for k, v in synth.synth_state_dict().items() if k.startswith(("encoder.", "decoder."))}, strict=False)
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    return net


def test_model_level_three_optimizer_steps():
    """`Lip2Speech` through `callers.train_iterations(honour_lengths=True, honour_mel_lengths=True)`, three optimizer steps over two batches of unequal mel
    length: finite, the masked post-net and l2s_loss_lengths routes taken, the switches restored; the four loss terms of every step equal, bit for bit, a
    hand-driven `training.model_forward_backward(mel_lengths=)` + AdamWAmsgrad loop with the same draws; and they differ from the honour_mel_lengths=False run."""
    from lip2speech_amd import callers, native
    from lip2speech_amd.model.modules.decoder import Decoder
    from lip2speech_amd.training import AdamWAmsgrad, draw_dropout, model_forward_backward
    batches = model_batches()
    emb = synth.synth_speaker_embedding(4, tag="mm-model")

    class Spk:
        def inference(self, a):
            return emb.to(a.device)
    keys = ("mel_loss", "postnet_mel_loss", "gate_loss", "KLD")
    logs = {}
    for mel_on in (True, False):
        net = fresh_net()
        log = callers.train_iterations(net, batches, 3, speaker_encoder=Spk(), tf_ratio=0.5, honour_lengths=True, honour_mel_lengths=mel_on)
        calls = net.native_model().calls
        want = 3 if mel_on else 0
        assert calls["l2s_train_postnet_masked_fwd"] == want and calls["l2s_train_postnet_masked_bwd"] == want, dict(calls)
        assert net.honour_video_lengths is False and net.train_video_lengths is False and net.train_mel_lengths is False and not net.training
        assert all(np.isfinite(r["loss"]) and np.isfinite(r["grad_norm"]) for r in log)
        logs[mel_on] = [[r[k] for k in keys] for r in log]
    assert all(a != b for a, b in zip(logs[True], logs[False])), "honour_mel_lengths changed nothing"
    # the same three steps by hand
    net = fresh_net()
    net.eval()
    flat = net._train_state()
    optim = AdamWAmsgrad(flat, lr=1e-4, weight_decay=1e-6)
    hand = []
    for it in range(3):
        (video, vlen), _, (mels, mlen, gate), _ = batches[it % 2]
        B, Sp = video.shape[0], mels.shape[2]
        drop = draw_dropout(B, T, Sp, "cuda")
        gum = Decoder.draw_gumbel(B * native.min_T(T), torch.device("cuda"))
        mask, consumed = [], 0
        for _ in range(Sp):
            take = bool(torch.rand(1) > 0.5) and consumed < int(0.5 * Sp)
            consumed += int(take)
            mask.append(take)
        nm = net.native_model()
        nm.train_set_bn(False)
        optim.zero_grad()
        out = model_forward_backward(nm, video.cuda(), emb.cuda(), gum, mels.cuda(), gate.cuda(), teacher_mask=torch.tensor(mask) if any(mask) else None,
                                     bos=net.decoder.BOS.detach(), drop=drop, video_lengths=[int(v) for v in vlen], mel_lengths=mlen)
        optim.step(max_norm=1.0, grad_mul=1.0)
        net.mark_weights_changed()
        hand.append([float(v) for v in out["loss"][:4]])
    assert hand == logs[True], (hand, logs[True])


# ------------------------------------------------------------------------------------------------------------------------------ timing script
def test_timing_script_runs_at_its_smallest_setting():
    """timing/masked_mel/time_masked_mel.py (-> profiles/masked_mel_times.txt) runs end to end: two clips of 1 - 3 mel frames, one round of one call."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, B="2", S="3", LO="1", ROUNDS="1", REPS="1")
    env.pop("PARENT_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(root, "timing", "masked_mel", "time_masked_mel.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "masked, true lengths" in r.stdout and "masked, all lengths = S" in r.stdout
    line = next(l for l in r.stdout.splitlines() if "all lengths = S" in l and "bit-identical" in l)
    assert line.rstrip().endswith("True"), line      # all lengths = S: the unmasked calls' loss terms, bit for bit
