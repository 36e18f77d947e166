"""SHA-256 of the outputs of the routes through the stage builders (csrc/decoder_stages.h: decoder prologue and post-net) that hash_inference.py,
hash_train_step.py and hash_step_routes.py do not reach, at the smallest shapes that still take each branch: the persistent BiLSTM route of the prologue
(B = 2, T = 8; plain and length-masked under "persist_masked"), the launch-route prologue under "infer_bf16" (B = 3), the inference post-net on the
tap-split (B = 3, S = 6) and plain (S = 300: 900 rows) routes and, on the diagnostic build only, windowed under "overlap_postnet"; the step-table path of
the post-net (forward_eval_ragged, two batches of one clip); the training post-net with and without dropout masks and batch statistics; the training
prologue and one whole training step under batch statistics (gradients and running statistics).  A change that claims the same bits must leave every
line unchanged.  L2S_LIB=<other build> python tools/hash_stage_routes.py for the A/B.  -> profiles/stage_builder_hashes.txt"""
import os, sys, hashlib, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lip2speech_amd import native, synth, training
h = lambda *ts: hashlib.sha256(b"".join(t.detach().cpu().numpy().tobytes() for t in ts if t is not None)).hexdigest()[:16]
sd = synth.synth_state_dict()
print(os.environ.get("L2S_LIB", "default"))


def model(**options):
    nm = native.NativeModel()
    for k, v in options.items(): nm.set_option(k, v)
    nm.load({k: v.cuda() for k, v in sd.items()}, list(sd.keys()))
    return nm


def visual(B, T):
    feat = torch.nn.functional.normalize(torch.randn(B, T, 768, generator=torch.Generator().manual_seed(11)), dim=2).cuda()
    emb = synth.synth_speaker_embedding(B, tag="stages").cuda()
    return native.build_visual(feat, emb), emb, synth.synth_gumbel(B * native.min_T(T), tag="stages").cuda()


T = 8
# prologue: the persistent BiLSTM (two clips, default options), the same length-masked, and the launch route on the bf16 leg
vis, emb, gum = visual(2, T)
print(f"  decoder_prologue B=2 T={T} persistent BiLSTM: sha256 {h(*model().decoder_prologue(vis, emb, gum))}")
print(f"  decoder_prologue B=2 T={T} persistent BiLSTM, lengths 8,7, persist_masked=1: sha256 "
      f"{h(*model(persist_masked=1).decoder_prologue(vis, emb, gum, video_lengths=[8, 7]))}")
vis3, emb3, gum3 = visual(3, T)
print(f"  decoder_prologue B=3 T={T} infer_bf16=1: sha256 {h(*model(persist_decode=0, infer_bf16=1).decoder_prologue(vis3, emb3, gum3))}")

# inference post-net: one K slice per tap (18 rows), plain (900 rows), windowed under the decode loop (diagnostic build)
nm = model()
for S in (6, 300):
    mel = synth.synth_mels(3, S, tag="stages").permute(0, 2, 1).contiguous().cuda()
    print(f"  postnet B=3 S={S}: sha256 {h(*nm.postnet(mel, want_cf=True))}")
if os.path.basename(native.LIB_PATH) == os.path.basename(native.DIAG_LIB_PATH):
    video = synth.synth_video(3, T, tag="stages").cuda()
    print(f"  inference B=3 T={T} S=300 overlap_postnet=1: sha256 {h(*model(persist_decode=0, overlap_postnet=1).inference(video, emb3, gum3, S=300))}")
else:
    print("  inference overlap_postnet=1: skipped (the option exists in the diagnostic build only: L2S_LIB=diag)")

# the post-net over a step table: two batches of one clip, T = 7 and 8, S = 5 and 6, 88 x 88
batches = []
for g, Tg in enumerate((7, 8)):
    batches.append((synth.synth_video(1, Tg, H=88, W=88, tag=f"stages{g}").cuda(), synth.synth_speaker_embedding(1, tag=f"stages{g}").cuda(),
                    synth.synth_gumbel(native.min_T(Tg), tag=f"stages{g}").cuda()))
out = nm.forward_eval_ragged(batches, [[7], [8]], [5, 6])
print(f"  forward_eval_ragged T=7,8 S=5,6: sha256 {h(*[t for o in out for t in o])}")

# training: post-net, prologue and one whole step at B = 2, S = 5
B, S = 2, 5
tm = model()
bound = {k: v.clone().cuda() for k, v in sd.items() if k.startswith(("encoder.", "decoder.")) and v.is_floating_point()}
is_buf = lambda k: k.endswith(("running_mean", "running_var", "pos_table"))
grads = {k: torch.zeros_like(v) for k, v in bound.items() if not is_buf(k)}
tm.train_bind(bound, grads)
mel = synth.synth_mels(B, S, tag="stages").permute(0, 2, 1).contiguous().cuda()
g = torch.Generator().manual_seed(5)
drop = native.postnet_drop_pack([((torch.rand(B, C, S, generator=g) < 0.5).float() * 2).cuda() for C in (512, 512, 512, 512, 80)])
for bn in (True, False):
    tm.train_set_bn(bn, 0.1)
    for name, d in (("no masks", None), ("dropout masks", drop)):
        print(f"  train_postnet_fwd B={B} S={S} batch statistics {int(bn)}, {name}: sha256 {h(*tm.train_postnet_fwd(mel, d))}")
tm.train_set_bn(True, 0.1)
state, dis, ptape = tm.train_prologue_fwd(vis, emb, gum)
decoder_bn = sorted(k for k in bound if k.endswith(("running_mean", "running_var")) and k.startswith(("decoder.K.", "decoder.V.", "decoder.content.agg.")))
assert len(decoder_bn) == 24, decoder_bn
print(f"  train_prologue_fwd B={B} T={T} batch statistics: sha256 {h(state, dis, ptape)}, running statistics {h(*[bound[k] for k in decoder_bn])}")
video = synth.synth_video(B, T, tag="stages").cuda(); mels = synth.synth_mels(B, S, tag="stages").cuda()
gate = torch.zeros(B, S, device="cuda"); gate[:, -1] = 1
torch.manual_seed(3)
out = training.model_forward_backward(tm, video, emb, gum, mels, gate, drop=training.draw_dropout(B, T, S, "cuda"))
print(f"  training step B={B} T={T} S={S} batch statistics: outputs sha256 {h(*[out[k] for k in ('loss', 'mel', 'mel_post', 'stop')])}, "
      f"gradients {h(*[grads[k] for k in sorted(grads)])}")
torch.cuda.synchronize()
