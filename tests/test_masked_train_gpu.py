"""Training with per-clip video lengths (include/l2s.h "training with per-clip video lengths"; running statistics): the l2s_train_*_masked_fwd / _masked_bwd
entry points against the unmasked ones.

Shapes: 96 x 96 frames, S = 6, LENS = [7, 13, 22, 16] zero-padded to T = 22 (m_b = 1, 1, 3, 2: the minimum length and a full-length clip); one clip of 9 frames
padded to 14; B = 17 at T = 14, S = 3 (crosses the 16-row tile).  Mixed teacher mask and all five dropout sites on unless a test says otherwise.

How the bound of `test_as_alone` is set: it is MEASURED by the test itself, not chosen.  A batch and the sum of its clips alone are two orders of the same
fp32 sums, whatever the lengths; so the same comparison on an UNPADDED batch (all clips of T frames, the unmasked entry points against themselves at B = 1)
gives, per tensor class, what that reordering costs: the baseline.  The masked path gets 4 x the baseline - it adds one more row-count-dependent choice of
kernel form (the trunk runs at sum(len_b) frames) and the scatter order of the sums.  The measured values of one run are in profiles/masked_train_errors.txt."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_common as pc          # noqa: E402
from lip2speech_amd import synth    # noqa: E402

pytestmark = pytest.mark.gpu

LENS, T, S = [7, 13, 22, 16], 22, 6
MASK = np.array([0, 1, 0, 1, 1, 0], dtype=np.uint8)          # mixed teacher forcing (step 0 always takes BOS)
is_buf = lambda k: k.endswith(("running_mean", "running_var", "num_batches_tracked", "pos_table"))      # noqa: E731


def min_T(n):
    return n // 7


class Rig:
    """The cached model with every encoder / decoder tensor bound and a gradient slot per parameter."""
    def __init__(self):
        self.sd = synth.synth_state_dict()
        self.nm = pc.native_model(self.sd)
        self.bound = {k: v.clone().cuda() for k, v in self.sd.items() if k.startswith(("encoder.", "decoder.")) and v.is_floating_point()}
        self.grads = {k: torch.zeros_like(v) for k, v in self.bound.items() if not is_buf(k)}
        self.bind()

    def bind(self):
        self.nm.train_bind(self.bound, self.grads)
        self.nm.train_set_bn(False)


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    assert len(r.grads) == 308
    return r


def inputs(B, T, S, tag, lens=None, dropout=True):
    """Synthetic batch; with `lens` the pad frames of the video are exact zeros (the contract).  Upstream gradients are inputs too: the same rows go to the
    batch and to the clips alone."""
    from lip2speech_amd.training import draw_dropout
    m = min_T(T)
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, tag)))
    d = dict(video=synth.synth_video(B, T, tag=tag).cuda(), emb=synth.synth_speaker_embedding(B, tag=tag).cuda(), gum=synth.synth_gumbel(B * m, tag=tag).cuda(),
             mels=synth.synth_mels(B, S, tag=tag).cuda())
    if lens is not None:
        for b, n in enumerate(lens):
            d["video"][b, :, n:] = 0.0
    d["drop"] = draw_dropout(B, T, S, "cuda", generator=g) if dropout else None
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)      # noqa: E731
    d["up"] = dict(dmel_post=rnd(B, 80, S), dmel=rnd(B, S, 80), dstop=rnd(B, S), ddis=rnd(B * m, 501) * 1e-2)
    return d


def clip_of(d, b, T, n, S):
    """Clip b of a batch alone at T = n: its frames, its first min_T(n) Gumbel rows, its rows of every dropout multiplier and upstream gradient."""
    m, mb = min_T(T), min_T(n)
    rows = slice(b * m, b * m + mb)
    c = dict(video=d["video"][b:b + 1, :, :n].contiguous(), emb=d["emb"][b:b + 1], gum=d["gum"][rows].contiguous(), mels=d["mels"][b:b + 1])
    dr = d["drop"]
    c["drop"] = None if dr is None else dict(feat=dr["feat"][b:b + 1, :n].contiguous(), prenet=dr["prenet"][:, b:b + 1].contiguous(),
                                             attn=dr["attn"][:, b:b + 1, :n].contiguous(), rnn=dr["rnn"][:, b:b + 1].contiguous(),
                                             post=[p[b:b + 1].contiguous() for p in dr["post"]])
    u = d["up"]
    c["up"] = dict(dmel_post=u["dmel_post"][b:b + 1].contiguous(), dmel=u["dmel"][b:b + 1].contiguous(), dstop=u["dstop"][b:b + 1].contiguous(),
                   ddis=u["ddis"][rows].contiguous())
    return c


def step(rig, d, mask=MASK, lens=None):
    """One training step through the staged entry points, fed explicit upstream gradients.  Returns outputs, state gradients and a copy of all 308 gradients."""
    from lip2speech_amd import native
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
    mel_post, post_tape = nm.train_postnet_fwd(mel, pdrop)
    up = d["up"]
    wbuf = nm.train_pack_weights(video.device)
    dmel = nm.train_postnet_bwd(mel, up["dmel_post"], post_tape, pdrop)
    dmel += up["dmel"]
    sg = nm.train_steps_bwd(ctx, dmel, up["dstop"], wbuf=wbuf)
    dvis = nm.train_prologue_bwd(vis, emb, state, ptape, sg, dcontent_dis=up["ddis"], wbuf=wbuf, video_lengths=lens)
    dvis_out = dvis.clone()
    if drop.get("feat") is not None:
        dvis[:, :, :768] = dvis[:, :, :768] * drop["feat"] if real is None else torch.where(real, dvis[:, :, :768] * drop["feat"], torch.zeros((), device="cuda"))
    nm.train_encoder_bwd(video, dvis, etape, video_lengths=lens)
    torch.cuda.synchronize()
    out = dict(mel=mel, mel_post=mel_post, stop=stop, logits=logits, dis=dis, vis=vis_enc, feat=feat, dvis=dvis_out)
    out.update(sg)
    return out, {k: g.clone() for k, g in rig.grads.items()}


def equal_all(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


# ------------------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("B,T,S", [(4, 22, 6), (17, 14, 3), (1, 14, 6)])
def test_full_lengths_are_the_unmasked_bits(rig, B, T, S):
    """All lengths = T: outputs, the tapes' visible outputs and all 308 gradients are bit-identical to the unmasked entry points."""
    rig.bind()
    d = inputs(B, T, S, f"mt-full-{B}")
    o0, g0 = step(rig, d)
    o1, g1 = step(rig, d, lens=[T] * B)
    assert equal_all(o0, o1) == [] and equal_all(g0, g1) == []
    assert all(torch.isfinite(v).all() for v in g1.values())


# ------------------------------------------------------------------------------------------------------------------------------ 2
CLASSES = ("encoder.", "decoder.postnet.", "decoder.")


def klass(k):
    return next(c for c in CLASSES if k.startswith(c))


def alone_errors(rig, d, T, lens, masked):
    """The batch (masked: through the masked entry points at the lengths; else unmasked, every clip of T frames) against its clips ALONE through the UNMASKED
    entry points at B = 1, T = len_b, summed in fp64.  -> per class: forward rows max |d| / max |ref|; gradients max over tensors of
    max |d| / (max |ref| + 1e-5 x the class's largest gradient entry) - a tensor whose gradient is the rounding residue of sums of class-sized terms (the
    saturated attention path) cannot be compared relative to itself."""
    S = d["mels"].shape[2]
    ob, gb = step(rig, d, lens=lens if masked else None)
    ref = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in gb.items()}
    fwd = {}
    for b, n in enumerate(lens):
        oc, gc = step(rig, clip_of(d, b, T, n, S))
        for k in ref:
            ref[k] += gc[k].double()
        m, mb = min_T(T), min_T(n)
        for name, got, want in (("mel", ob["mel"][b], oc["mel"][0]), ("mel_post", ob["mel_post"][b], oc["mel_post"][0]), ("stop", ob["stop"][b], oc["stop"][0]),
                                ("logits", ob["logits"][b, :, :n], oc["logits"][0]), ("dis", ob["dis"][b * m:b * m + mb], oc["dis"]),
                                ("dvis", ob["dvis"][b, :n], oc["dvis"][0])):
            e = (got.double() - want.double()).abs().max().item() / max(want.abs().max().item(), 1e-30)
            fwd[name] = max(fwd.get(name, 0.0), e)
    scale = {c: max(ref[k].abs().max().item() for k in ref if klass(k) == c) for c in CLASSES}
    err = {c: 0.0 for c in CLASSES}
    for k in ref:
        c = klass(k)
        e = (gb[k].double() - ref[k]).abs().max().item() / (ref[k].abs().max().item() + 1e-5 * scale[c])
        err[c] = max(err[c], e)
    err.update({"fwd:" + k: v for k, v in fwd.items()})
    return err, ob, gb


@pytest.fixture(scope="module")
def baseline(rig):
    """An UNPADDED batch of 4 clips of 22 frames against its own clips alone, unmasked entry points on both sides."""
    rig.bind()
    err, _, _ = alone_errors(rig, inputs(4, T, S, "mt-base"), T, [T] * 4, masked=False)
    print("baseline (unpadded batch vs its clips alone):", {k: f"{v:.3e}" for k, v in err.items()})
    return err


@pytest.mark.parametrize("lens,Tp", [(LENS, 22), ([9], 14)])
def test_as_alone(rig, baseline, lens, Tp):
    """Forward rows and gradients of the masked step against the clips alone (unmasked, B = 1, T = len_b), summed in fp64; bound = 4 x the measured baseline
    (module docstring; one run's values: profiles/masked_train_errors.txt)."""
    rig.bind()
    d = inputs(len(lens), Tp, S, f"mt-alone-{Tp}", lens=lens)
    err, ob, gb = alone_errors(rig, d, Tp, lens, masked=True)
    print(f"masked lens={lens} T={Tp}:", {k: f"{v:.3e}" for k, v in err.items()})
    assert all(torch.isfinite(v).all() for v in gb.values())
    bad = {k: (v, baseline[k]) for k, v in err.items() if v > 4.0 * baseline[k]}
    assert not bad, f"masked step further from its clips alone than 4 x the unpadded baseline: {bad}"


# ------------------------------------------------------------------------------------------------------------------------------ 3
class OracleGoldens:
    """The fields check_grads reads, computed from a dict of fp64 gradients."""
    def __init__(self, grads):
        from test_grad_goldens import projection_vector
        self.keys = list(grads)
        self.index = {k: i for i, k in enumerate(self.keys)}
        flat = {k: g.detach().double().cpu().numpy().ravel() for k, g in grads.items()}
        self.d = {"grad_norm": np.array([np.sqrt((flat[k] ** 2).sum()) for k in self.keys]),
                  "grad_proj": np.array([(flat[k] * projection_vector(k, flat[k].size)).sum() for k in self.keys])}
        self.d.update({"grad:" + k: flat[k] for k in self.keys if flat[k].size <= 2048})
        self.files = list(self.d)

    def __getitem__(self, k):
        return self.d[k]


def test_fp64_oracle(rig):
    """oracle/l2s_oracle.py autograd on each clip ALONE (fp64), summed with the weights the batch loss gives each clip, against the masked step: check_grads of
    tests/test_grad_goldens.py at its own tolerances (3e-3 / 6e-3 / 6e-3, saturated floor).  Dropout off (the oracle has none); mixed teacher mask.
    Loss weights: the three per-frame terms are means over B clips -> 1/B each; KLD is the mean over all B*m rows, of which clip b owns m_b -> m_b/(B*m)."""
    from lip2speech_amd.training import model_forward_backward
    from oracle import l2s_oracle as orc
    from test_grad_goldens import check_grads
    rig.bind()
    B, m = len(LENS), min_T(T)
    d = inputs(B, T, S, "mt-oracle", lens=LENS, dropout=False)
    gate = torch.zeros(B, S, device="cuda")
    gate[:, S - 1] = 1.0
    for g in rig.grads.values():
        g.zero_()
    out = model_forward_backward(rig.nm, d["video"], d["emb"], d["gum"], d["mels"], gate, teacher_mask=torch.from_numpy(MASK.astype(bool)),
                                 bos=rig.bound["decoder.BOS"], video_lengths=LENS)
    torch.cuda.synchronize()
    sd64 = {k: (v.double().requires_grad_(True) if k in rig.grads else (v.double() if v.is_floating_point() else v)) for k, v in rig.sd.items()}
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    total, terms_sum = 0.0, np.zeros(4)
    for b, n in enumerate(LENS):
        mb = min_T(n)
        outs = orc.forward_eval(sd64, d["video"][b:b + 1, :, :n].cpu().double(), d["emb"][b:b + 1].cpu().double(), d["mels"][b:b + 1].cpu().double(),
                                d["gum"][b * m:b * m + mb].cpu().double(), teacher_mask=torch.from_numpy(MASK.astype(bool)))
        t = orc.loss_terms(outs, d["mels"][b:b + 1].cpu().double(), gate[b:b + 1].cpu().double())
        w = np.array([1.0 / B, 1.0 / B, 1.0 / B, mb / (B * m)])
        ((t[0] + t[1] + t[2]) / B + t[3] * (mb / (B * m))).backward()
        terms_sum += w * np.array([x.item() for x in t[:4]])
        assert pc.maxdiff(out["mel"][b], outs[0][0]) < 1e-3 and pc.maxdiff(out["mel_post"][b], outs[1][0]) < 1e-3
        assert pc.maxdiff(out["stop"][b], outs[2][0, :, 0]) < 1e-3
    got = out["loss"].cpu().double().numpy()
    assert np.abs(got[:4] - terms_sum).max() < 2e-5 * np.abs(terms_sum).max(), (got, terms_sum)
    z = OracleGoldens({k: sd64[k].grad for k in rig.grads})
    check_grads(z, z.index, rig.grads, z.keys, rel_norm=3e-3, rel_proj=6e-3, rel_full=6e-3)


# ------------------------------------------------------------------------------------------------------------------------------ 4
def test_never_read_and_exact_positions(rig):
    """NaN in every never-read position (feature and attention dropout multipliers at pad positions, Gumbel rows >= m_b) leaves every output and gradient
    bit-identical; the exact-zero and -inf positions of the contract; same bits run to run."""
    rig.bind()
    d = inputs(len(LENS), T, S, "mt-nan", lens=LENS)
    o0, g0 = step(rig, d, lens=LENS)
    o0b, g0b = step(rig, d, lens=LENS)
    assert equal_all(o0, o0b) == [] and equal_all(g0, g0b) == [], "not deterministic"
    m = min_T(T)
    nan = float("nan")
    for b, n in enumerate(LENS):
        d["drop"]["feat"][b, n:] = nan
        d["drop"]["attn"][:, b, n:] = nan
        d["gum"][b * m + min_T(n):(b + 1) * m] = nan
        d["up"]["ddis"][b * m + min_T(n):(b + 1) * m] = nan
    o1, g1 = step(rig, d, lens=LENS)
    assert equal_all(o0, o1) == [] and equal_all(g0, g1) == []
    assert all(torch.isfinite(v).all() for v in g1.values())
    for b, n in enumerate(LENS):
        mb = min_T(n)
        assert torch.isneginf(o1["logits"][b, :, n:]).all() and torch.isfinite(o1["logits"][b, :, :n]).all()
        assert (o1["dis"][b * m + mb:(b + 1) * m] == 0).all() and (o1["dis"][b * m:b * m + mb].sum(1) - 1).abs().max() < 1e-5
        assert (o1["vis"][b, n:, :768] == 0).all() and (o1["feat"][b, n:] == 0).all() and torch.equal(o1["vis"][b, :, 768:], d["emb"][b].expand(T, 256))
        assert (o1["dvis"][b, n:] == 0).all() and (o1["dk"][b, n:] == 0).all() and (o1["dv"][b, n:] == 0).all()
        assert (o1["dckey"][b, mb:] == 0).all() and (o1["dcval"][b, mb:] == 0).all()
    for k in ("mel", "mel_post", "stop", "dvis", "dk", "dv", "dckey", "dcval", "dh_init", "de_c"):
        assert torch.isfinite(o1[k]).all(), k


def test_b17_crosses_the_row_tile(rig):
    """17 clips of 7 .. 14 frames at T = 14, S = 3: the exact positions, finite gradients, and clip 16 (row 16: the second 16-row tile) as alone within the
    bound of test_as_alone's forward rows (rounding level: 1e-4 of the row's scale, the staged-route bound of the masked inference tests)."""
    rig.bind()
    B, Tp, Sp = 17, 14, 3
    lens = [7 + (3 * b) % 8 for b in range(B)]
    d = inputs(B, Tp, Sp, "mt-b17", lens=lens)
    o, g = step(rig, d, lens=lens)
    assert all(torch.isfinite(v).all() for v in g.values())
    for b, n in enumerate(lens):
        assert torch.isneginf(o["logits"][b, :, n:]).all() and (o["dvis"][b, n:] == 0).all() and (o["dk"][b, n:] == 0).all()
    b, n = 16, lens[16]
    oc, _ = step(rig, clip_of(d, b, Tp, n, Sp))
    for k in ("mel", "mel_post", "stop"):
        assert pc.maxdiff(o[k][b], oc[k][0]) < 1e-4 * max(1.0, oc[k].abs().max().item()), k
    assert pc.maxdiff(o["dvis"][b, :n], oc["dvis"][0]) < 1e-3 * oc["dvis"].abs().max().item()


# ------------------------------------------------------------------------------------------------------------------------------ refusals on the device side
def test_batch_statistics_and_bf16_are_refused_by_name(rig):
    rig.bind()
    d = inputs(1, 14, 3, "mt-refuse", lens=[9])
    rig.nm.train_set_bn(True, 0.1)
    try:
        with pytest.raises(RuntimeError, match="batch_stats = 1"):
            rig.nm.train_encoder_fwd(d["video"], d["emb"], video_lengths=[9])
        with pytest.raises(RuntimeError, match="batch_stats = 1"):
            rig.nm.train_prologue_fwd(torch.zeros(1, 14, 1024, device="cuda"), d["emb"], d["gum"], video_lengths=[9])
    finally:
        rig.nm.train_set_bn(False)
    rig.nm.set_option("train_bf16", 1)
    try:
        with pytest.raises(RuntimeError, match="train_bf16"):
            rig.nm.train_encoder_fwd(d["video"], d["emb"], video_lengths=[9])
    finally:
        rig.nm.set_option("train_bf16", 0)
    with pytest.raises(RuntimeError, match=r"video_lengths\[0\] = 15"):      # the library's own check, past the wrapper's
        rig.nm._check(rig.nm._L.l2s_train_encoder_masked_fwd(rig.nm._h, d["video"].data_ptr(), 1, 14, 96, 96, d["emb"].data_ptr(), None,
                                                            torch.empty(1, 14, 768, device="cuda").data_ptr(), torch.empty(64, device="cuda").data_ptr(), None,
                                                            (__import__("ctypes").c_int32 * 1)(15)))


# ------------------------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("fused", [True, False])
def test_model_level_three_optimizer_steps(fused):
    """`Lip2Speech` with both switches on, three optimizer steps through `callers.train_iterations(honour_lengths=True)` (fused AdamW and torch's): the step
    runs, takes the masked entry points and is deterministic.  (eval() mode: the masked entry points run on running
    statistics; the loop draws the dropout multipliers itself.)"""
    from model.model import get_network
    from lip2speech_amd import callers
    B = len(LENS)
    video = synth.synth_video(B, T, tag="mt-model")
    for b, n in enumerate(LENS):
        video[b, :, n:] = 0.0
    emb = synth.synth_speaker_embedding(B, tag="mt-model")
    mels = synth.synth_mels(B, S, tag="mt-model")
    gate = torch.zeros(B, S)
    gate[:, -1] = 1.0
    audio = torch.zeros(B, 256 * (S - 1))
    batch = ((video, torch.tensor(LENS)), (audio, torch.full((B,), audio.shape[1])), (mels, torch.full((B,), S), gate), None)

    class Spk:
        def inference(self, a):
            return emb.to(a.device)
    logs = []
    for _ in range(2):
        net = get_network("train").cuda()
        net.load_state_dict({k: v for k, v in synth.synth_state_dict().items() if k.startswith(("encoder.", "decoder."))}, strict=False)
        torch.manual_seed(11)
        torch.cuda.manual_seed(11)
        log = callers.train_iterations(net, [batch], 3, speaker_encoder=Spk(), tf_ratio=0.5, fused_optimizer=fused, honour_lengths=True)
        calls = net.native_model().calls
        for st in ("encoder", "prologue", "steps"):
            assert calls[f"l2s_train_{st}_masked_fwd"] == 3 and calls[f"l2s_train_{st}_masked_bwd"] == 3, dict(calls)
        assert net.honour_video_lengths is False and net.train_video_lengths is False and not net.training
        assert all(np.isfinite(r["loss"]) and np.isfinite(r["grad_norm"]) for r in log)
        logs.append([r["loss"] for r in log])
    assert logs[0] == logs[1], "the masked training step is not deterministic"


# ------------------------------------------------------------------------------------------------------------------------------ timing script
def test_timing_script_runs_at_its_smallest_setting():
    """timing/masked_train/time_masked_train.py (-> profiles/masked_train_times.txt) runs end to end: two clips of 7 - 14 frames, S = 3, one round of one step."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, B="2", S="3", LO="7", HI="14", ROUNDS="1", REPS="1")
    env.pop("PARENT_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(root, "timing", "masked_train", "time_masked_train.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "masked step, true lengths" in r.stdout and "masked step, all lengths = T" in r.stdout
    line = next(l for l in r.stdout.splitlines() if "all lengths = T" in l and "bit-identical" in l)
    assert line.rstrip().endswith("True"), line      # all lengths = T: the unmasked step's loss terms, bit for bit
