"""SHA-256 of the outputs of the routes through the step builders (csrc/decode_step.h) that hash_inference.py and hash_train_step.py do not reach, at the
smallest shapes that still take every branch: decoder_prologue + decode_steps at B = 3 (the padded rows of a 16-row tile live), T = 8, S = 6 on the
launch-per-phase loop - folded, "fold_step_weights" = 0, a teacher mask that mixes forced and free steps (step 0 and the last step forced), per-clip
lengths (8, 7, 8), "early_stop" = 1, "lstm_x3" = 0; the voice tower padded and packed at two clips of unequal length; train_prologue_fwd +
train_steps_fwd outputs and tapes at B = 2, S = 5 with and without dropout masks.  A change that claims the same bits must leave every line unchanged.
L2S_LIB=<other build> python tools/hash_step_routes.py for the A/B.  -> profiles/step_builder_hashes.txt"""
import os, sys, hashlib, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lip2speech_amd import native, synth, statespec
h = lambda *ts: hashlib.sha256(b"".join(t.detach().cpu().numpy().tobytes() for t in ts if t is not None)).hexdigest()[:16]
sd = synth.synth_state_dict()
print(os.environ.get("L2S_LIB", "default"))


def model(sd, **options):
    nm = native.NativeModel()
    nm.set_option("persist_decode", 0)      # the launch-per-phase loop: three clips would otherwise take the persistent one
    for k, v in options.items(): nm.set_option(k, v)
    nm.load({k: v.cuda() for k, v in sd.items()}, list(sd.keys()))
    return nm


B, T, S = 3, 8, 6
feat = torch.nn.functional.normalize(torch.randn(B, T, 768, generator=torch.Generator().manual_seed(11)), dim=2).cuda()
emb = synth.synth_speaker_embedding(B, tag="routes").cuda(); gum = synth.synth_gumbel(B * native.min_T(T), tag="routes").cuda()
teacher = synth.synth_mels(B, S, tag="routes").permute(0, 2, 1).contiguous().cuda()      # (B, S, 80)
vis = native.build_visual(feat, emb)


def decode(name, nm, **kw):
    lens = kw.get("video_lengths")
    state, dis = nm.decoder_prologue(vis, emb, gum, video_lengths=lens)
    mel, stop, attn = nm.decode_steps(state, B, T, S, want_attn=True, **kw)
    torch.cuda.synchronize()
    print(f"  decode B={B} T={T} S={S} {name}: sha256 {h(state, dis, mel, stop, attn)}")


nm = model(sd)
decode("folded", nm)
decode("folded, attention logits", nm, attn_logits=True)
decode("teacher mask 1,0,0,1,0,1", nm, teacher=teacher, teacher_mask=[1, 0, 0, 1, 0, 1])
decode("lengths 8,7,8", nm, video_lengths=[8, 7, 8])
decode("lengths 8,7,8, teacher mask 1,0,0,1,0,1", nm, teacher=teacher, teacher_mask=[1, 0, 0, 1, 0, 1], video_lengths=[8, 7, 8])
decode("fold_step_weights=0", model(sd, fold_step_weights=0))
decode("fold_step_weights=0, teacher mask 1,0,0,1,0,1", model(sd, fold_step_weights=0), teacher=teacher, teacher_mask=[1, 0, 0, 1, 0, 1])
decode("early_stop=1", model(sd, early_stop=1))
decode("early_stop=1, lengths 8,7,8", model(sd, early_stop=1), video_lengths=[8, 7, 8])
decode("lstm_x3=0", model(sd, lstm_x3=0))

# the voice tower: two clips of 3200 and 1000 samples (21 and 7 frames), padded call on the zero-padded pair and the packed call
spk = model(synth.synth_state_dict(statespec.speaker_encoder_spec("speaker_encoder."), seed=99))
audio = synth.synth_audio(2, 3200, tag="routes").cuda()
audio[1, 1000:] = 0
print(f"  voice tower padded (2, 3200): sha256 {h(spk.speaker_encoder_fwd(audio))}")
print(f"  voice tower packed 3200 + 1000: sha256 {h(spk.speaker_encoder_packed(audio, [0, 3200], [3200, 1000]))}")

# training forward: prologue and loop with their tapes, B = 2, S = 5
B, S = 2, 5
tm = model(sd)
bound = {k: v.clone().cuda() for k, v in sd.items() if k.startswith(("encoder.", "decoder.")) and v.is_floating_point()}
grads = {k: torch.zeros_like(v) for k, v in bound.items() if not k.endswith(("running_mean", "running_var", "pos_table"))}
tm.train_bind(bound, grads)
state, dis, ptape = tm.train_prologue_fwd(vis[:B].contiguous(), emb[:B].contiguous(), gum[:B * native.min_T(T)].contiguous())
torch.cuda.synchronize()
print(f"  train_prologue_fwd B={B} T={T}: sha256 {h(state, dis, ptape)}")
g = torch.Generator().manual_seed(5)
drop = {"prenet": (torch.rand(S, B, 256, generator=g) < 0.5).float() * 2, "attn": (torch.rand(S, B, T, generator=g) < 0.9).float() / 0.9,
        "rnn": (torch.rand(S, B, 512, generator=g) < 0.9).float() / 0.9}
drop = {k: v.cuda() for k, v in drop.items()}
tch = teacher[:B, :S].contiguous()
for name, kw in (("free-running", {}), ("teacher mask 1,0,1,0,1", dict(teacher=tch, teacher_mask=[1, 0, 1, 0, 1])),
                 ("teacher mask 1,0,1,0,1, dropout masks", dict(teacher=tch, teacher_mask=[1, 0, 1, 0, 1], drop=drop)),
                 ("free-running, dropout masks", dict(drop=drop))):
    (mel, stop, logits), ctx = tm.train_steps_fwd(state, B, T, S, **kw)
    torch.cuda.synchronize()
    print(f"  train_steps_fwd B={B} S={S} {name}: sha256 {h(mel, stop, logits, ctx['tape'])}")
tf = model(sd, fold_step_weights=0)
tf.train_bind(bound, grads)
(mel, stop, logits), ctx = tf.train_steps_fwd(state, B, T, S, teacher=tch, teacher_mask=[1, 0, 1, 0, 1], drop=drop)
torch.cuda.synchronize()
print(f"  train_steps_fwd B={B} S={S} fold_step_weights=0, teacher mask 1,0,1,0,1, dropout masks: sha256 {h(mel, stop, logits, ctx['tape'])}")
