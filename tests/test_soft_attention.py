"""The decoder's attention at SOFT weights and on long clips, against the fp64 oracle.  `-m gpu`.

With the synthetic checkpoint the location attention is one-hot to fp32 precision (tau = 23.2 MULTIPLIES the logits, decoder.py:268,416):
a kernel that drops every frame but the argmax from the soft-max sum or from a @ v gives the same bits there.  A trained checkpoint learns
its own q, k and tau and does not attend one-hot, so these tests scale both temperatures down (`soft_state_dict`) until the largest weight
is well below 0.5 - asserted on the oracle's own output in every test, so that a change to the synthetic checkpoint cannot quietly bring
the one-hot regime back - and compare the attention weights element by element.

The decoder runs from the HIP encoder's features (the oracle takes the same features in fp64): the clips here reach T = 300 frames, where
the CPU encoder would dominate the run time, and the encoder has tests of its own.

Tolerances: at SOFT = 1e-3 the fp32 oracle's attention weights differ from the fp64 oracle's by at most 6.4e-7 (B=2, T=29, 40 steps; 3.9e-7 at
T=65, 2.6e-7 at T=118, 1.9e-7 at T=300) and its content weights by 5.6e-8; ATTN_TOL = 1e-5 is fifteen times that spread.  Mel frames: MEL_TOL
as in test_gpu_parity.py (the fp32-vs-fp64 spread of the mel frames is 5e-8).
"""
import pytest
import torch

from lip2speech_amd import native, synth
from oracle import l2s_oracle as orc
import parity_common as pc

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-3
ATTN_TOL = 1e-5
SOFT = 1e-3                 # factor on decoder.temperature and decoder.content.temperature
STOP_MARGIN = 1e-4          # output lengths are compared for clips whose stop logits all keep this distance from 0


def soft_state_dict(sd, factor=SOFT):
    """The synthetic checkpoint with both attention temperatures scaled by `factor` (everything else the same tensors)."""
    out = dict(sd)
    out["decoder.temperature"] = sd["decoder.temperature"] * factor
    out["decoder.content.temperature"] = sd["decoder.content.temperature"] * factor
    return out


@pytest.fixture(scope="module")
def soft_sd(synth_sd):
    return soft_state_dict(synth_sd)


_models = {}


def soft_model(sd, persist=0, **options):
    """A NativeModel of its own on the soft checkpoint (cached per option set)."""
    key = (persist, tuple(sorted(options.items())))
    if key not in _models:
        _models[key] = pc.fresh_native_model(sd, persist_decode=persist, **options)
    return _models[key]


def content_m(T):
    return min((T - k) // k + 1 for k in (1, 3, 5, 7))


def clip_inputs(B, T, S, tag):
    tag = f"soft{B}_{T}_{S}_{tag}"
    return (synth.synth_video(B, T, tag=tag), synth.synth_speaker_embedding(B, tag=tag), synth.synth_gumbel(B * content_m(T), tag=tag),
            synth.synth_mels(B, S, tag=tag))


def decoder_oracle(sd, feat, emb, gum, S, teacher_mask=None, mels=None):
    """fp64 oracle of prologue -> S-step loop -> post-net from the given encoder features: mel (B,80,S), mel_post, stop (B,S), attention
    weights (B,S,T), logits (B,S,T), content weights (B,S,m)."""
    sd64 = orc.to_dtype(sd, torch.float64)
    emb64 = emb.double()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        st = orc.decoder_prologue(sd64, orc.build_visual(feat.double(), emb64), emb64, gum.double())
        teacher = None
        if teacher_mask is not None:
            teacher = torch.cat([sd64["decoder.BOS"].view(1, 1, -1).expand(feat.shape[0], -1, -1), mels.double().permute(0, 2, 1)], dim=1)
        al = []
        mel, stop, logits = orc.decode_loop(sd64, st, S, teacher=teacher, teacher_mask=teacher_mask, return_logits=True, alphas=al)
        mel_cf = mel.permute(0, 2, 1)
        post = orc.postnet(sd64, mel_cf) + mel_cf
    return dict(mel=mel_cf, post=post, stop=stop, attn=torch.softmax(logits, dim=-1), logits=logits, alpha=torch.stack(al, dim=1))


def assert_soft(ref):
    """The precondition of every test here: the oracle's attention is far from one-hot (content weights too, where m > 1: at m = 1 the
    content soft-max is identically 1)."""
    assert ref["attn"].max().item() < 0.5, f"attention is not soft: max weight {ref['attn'].max().item():.3f}"
    if ref["alpha"].shape[-1] > 1:
        assert ref["alpha"].max().item() < 0.5, f"content attention is not soft: max weight {ref['alpha'].max().item():.3f}"


def assert_lengths(lengths, stop_ref, S):
    clear = stop_ref.abs().min(dim=1).values > STOP_MARGIN
    want = orc.output_lengths_from_stop(stop_ref, S)
    assert torch.equal(lengths.cpu()[clear], want[clear]), (lengths.cpu(), want, clear)


# (B, T, S): the attention block's path boundaries - projected values through LDS at T <= 32, the one-wave soft-max at T <= 64, the 8-wave
# block_max8 / block_sum8 soft-max beyond; m = T // 7 content keys: 16 at T = 112..118, the long-m content block from T = 119 (m = 17) to
# T = 300 (m = 42); B = 17 and 33 take two and three 16-row tiles
FWD_CASES = [(1, 7, 40), (2, 29, 40), (3, 32, 40), (4, 32, 24), (1, 33, 40), (2, 64, 40), (3, 65, 40), (2, 75, 40), (1, 112, 40), (3, 118, 40),
             (17, 29, 24), (33, 65, 16), (2, 119, 40), (1, 120, 40), (3, 119, 24), (3, 120, 24), (2, 300, 60), (1, 300, 24), (3, 300, 16)]
# launch = the suite's launch-per-phase loop; shipped = the library's own options (persistent decode loop for <= 4 clips of <= 32 frames,
# persistent BiLSTM for <= 2 clips) - the same as the launch path beyond those sizes, so only run where it differs
FWD_PARAMS = [pytest.param(B, T, S, route, id=f"B{B}-T{T}-S{S}-{route}") for B, T, S in FWD_CASES
              for route in (("launch", "shipped") if B <= 4 else ("launch",))]


@pytest.mark.parametrize("B,T,S,route", FWD_PARAMS)
def test_soft_inference_and_forward_eval_match_oracle(soft_sd, B, T, S, route):
    """l2s_inference (mel_post, lengths, attention weights) and l2s_forward_eval (mel, mel_post, stop, logits) at soft weights."""
    nm = soft_model(soft_sd, pc.SHIPPED_PERSIST if route == "shipped" else 0)
    video, emb, gum, _ = clip_inputs(B, T, S, "fwd")
    feat = nm.encoder_fwd(video.cuda())
    ref = decoder_oracle(soft_sd, feat.cpu(), emb, gum, S)
    assert_soft(ref)
    mel_post, lengths, attn = nm.inference(video.cuda(), emb.cuda(), gum.cuda(), S=S, want_attn=True)
    assert pc.maxdiff(mel_post, ref["post"]) < MEL_TOL
    d_attn = pc.maxdiff(attn, ref["attn"])
    assert d_attn < ATTN_TOL, f"attention weights: max |d| {d_attn:.2e}"
    assert_lengths(lengths, ref["stop"], S)
    mel, post, stop, logits, _ = nm.forward_eval(video.cuda(), emb.cuda(), gum.cuda(), S)
    assert pc.maxdiff(mel, ref["mel"]) < 1e-4 and pc.maxdiff(post, ref["post"]) < MEL_TOL
    assert pc.maxdiff(stop, ref["stop"]) < 1e-4
    assert pc.maxdiff(logits, ref["logits"]) / ref["logits"].abs().max().item() < 1e-5
    assert pc.maxdiff(torch.softmax(logits.cpu().double(), dim=-1), ref["attn"]) < ATTN_TOL


@pytest.mark.parametrize("B,T", [(2, 119), (3, 300)])
def test_soft_teacher_forced_long_clips(soft_sd, B, T):
    """forward_eval with scheduled sampling (a random step mask) on clips past 16 content keys."""
    S = 48
    nm = soft_model(soft_sd)
    video, emb, gum, mels = clip_inputs(B, T, S, "tf")
    mask = torch.rand(S, generator=torch.Generator().manual_seed(T)) < 0.5
    teacher = torch.cat([soft_sd["decoder.BOS"].view(1, 1, -1).expand(B, -1, -1), mels.permute(0, 2, 1)[:, :S - 1]], dim=1).contiguous()
    feat = nm.encoder_fwd(video.cuda())
    ref = decoder_oracle(soft_sd, feat.cpu(), emb, gum, S, teacher_mask=mask, mels=mels)
    assert_soft(ref)
    mel, post, stop, logits, _ = nm.forward_eval(video.cuda(), emb.cuda(), gum.cuda(), S, teacher=teacher.cuda(), teacher_mask=mask.numpy())
    assert pc.maxdiff(mel, ref["mel"]) < 1e-4 and pc.maxdiff(post, ref["post"]) < MEL_TOL and pc.maxdiff(stop, ref["stop"]) < 1e-4
    assert pc.maxdiff(torch.softmax(logits.cpu().double(), dim=-1), ref["attn"]) < ATTN_TOL


@pytest.mark.parametrize("B", [2, 32])
def test_soft_attention_block_forms_same_bits(soft_sd, B):
    """The attention block forms of include/l2s_diag.h at soft weights: values through LDS or one column per thread ("attn_lds" 2 / 0),
    and the zero-weight skip ("attn_skip0" 2: with no weight exactly 0 it fetches every frame, four per round, t ascending).  DESIGN.md and
    test_gpu_parity.py hold them to the default form's bits; here every frame's weight counts, so an order or a dropped frame would show."""
    T, S = 29, 40
    video, emb, gum, _ = clip_inputs(B, T, S, "forms")
    base = soft_model(soft_sd, diag=True)
    feat = base.encoder_fwd(video.cuda())
    ref = decoder_oracle(soft_sd, feat.cpu(), emb, gum, S)
    assert_soft(ref)
    want = base.inference(video.cuda(), emb.cuda(), gum.cuda(), S=S, want_attn=True)
    assert pc.maxdiff(want[0], ref["post"]) < MEL_TOL and pc.maxdiff(want[2], ref["attn"]) < ATTN_TOL
    for opts in ({"attn_lds": 0}, {"attn_lds": 2}, {"attn_lds": 0, "attn_skip0": 0}, {"attn_lds": 2, "attn_skip0": 2}, {"attn_skip0": 2}):
        got = soft_model(soft_sd, **opts).inference(video.cuda(), emb.cuda(), gum.cuda(), S=S, want_attn=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[1], want[1]), opts


@pytest.mark.parametrize("hoist", [0, 1])
def test_soft_hoist_vproj_forms_match_oracle(soft_sd, hoist):
    """attention_proj on the values (K = 1280 layer 0) / a @ v through W_ih W_ap (K = 1536): other orders of the same sums, against the oracle."""
    B, T, S = 3, 29, 40
    nm = soft_model(soft_sd, hoist_vproj=hoist)
    video, emb, gum, _ = clip_inputs(B, T, S, "hoist")
    feat = nm.encoder_fwd(video.cuda())
    ref = decoder_oracle(soft_sd, feat.cpu(), emb, gum, S)
    assert_soft(ref)
    mel_post, lengths, attn = nm.inference(video.cuda(), emb.cuda(), gum.cuda(), S=S, want_attn=True)
    assert pc.maxdiff(mel_post, ref["post"]) < MEL_TOL and pc.maxdiff(attn, ref["attn"]) < ATTN_TOL
    assert_lengths(lengths, ref["stop"], S)


def test_soft_graph_replay_same_bits(soft_sd):
    """"use_graph": the decode loop replayed from a captured hipGraph - the same kernels in the same order, the same bits."""
    B, T, S = 2, 65, 40
    video, emb, gum, _ = clip_inputs(B, T, S, "graph")
    want = soft_model(soft_sd).inference(video.cuda(), emb.cuda(), gum.cuda(), S=S, want_attn=True)
    graph = soft_model(soft_sd, use_graph=1)
    for _ in range(2):                                     # capture, then replay
        got = graph.inference(video.cuda(), emb.cuda(), gum.cuda(), S=S, want_attn=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("B,T", [(1, 7), (2, 29), (4, 32)])
def test_soft_persistent_decode_loop_against_launch_path(soft_sd, B, T):
    """pdecode.hip (one persistent launch for the whole loop, its own soft-max) against the launch-per-phase loop at soft weights."""
    S = 40
    video, emb, gum, _ = clip_inputs(B, T, S, "pdec")
    launch = soft_model(soft_sd).inference(video.cuda(), emb.cuda(), gum.cuda(), S=S, want_attn=True)
    pers = soft_model(soft_sd, pc.SHIPPED_PERSIST).inference(video.cuda(), emb.cuda(), gum.cuda(), S=S, want_attn=True)
    torch.cuda.synchronize()
    native.check_persist_timeouts()
    if native.persist_available():
        assert not torch.equal(pers[0], launch[0]), "persist_decode=4 inside its envelope, yet the launch path ran"
    assert pc.maxdiff(pers[0], launch[0]) < MEL_TOL
    assert pc.maxdiff(pers[2], launch[2]) < ATTN_TOL

