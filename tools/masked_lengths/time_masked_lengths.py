"""Cost of the length-masked entry points (include/l2s.h "per-clip video lengths"): l2s_inference against l2s_inference_masked on the same padded
batch - B = 16 clips with lengths uniform in [25, 75] zero-padded to the batch maximum (BASELINE.json config 4's shape), S = 300 - with ALL lengths
= T, so that both calls do the same arithmetic and the difference is the masking machinery: the length table, the BiLSTM row kernels, the masked
copy / pooling, the length-masked attention blocks, and the launch-per-phase route.  A second line gives the masked call at the clips' true lengths.
`PARENT_LIB=<path to a libl2s_hip.so built from the parent commit>`: that build's unmasked call is timed in the same process, interleaved with this
build's (has the default path moved?), and so is its masked call at the true lengths (has the masked route moved?).  ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the
REPS calls; per variant the median of the rounds and the spread (max - min).  `B=`, `S=`, `ROUNDS=`, `REPS=`.
-> profiles/masked_lengths_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native, synth
from tools import abtime

REPS = int(os.environ.get("REPS", 10))
ROUNDS = int(os.environ.get("ROUNDS", 7))
B = int(os.environ.get("B", 16))
S = int(os.environ.get("S", 300))
LO, HI = 25, 75


def main():
    lens = [int(v) for v in synth.synth_clip_lengths(B, LO, HI, "masked-times")]
    T = max(lens)
    video = synth.synth_padded_video(B, lens, tag="masked-times").cuda()
    emb = synth.synth_speaker_embedding(B, tag="masked-times").cuda()
    gum = synth.synth_gumbel(B * native.min_T(T), tag="masked-times").cuda()
    this = abtime.synth_model()
    variants = [("this build, l2s_inference", lambda: this.inference(video, emb, gum, S=S)),
                ("this build, l2s_inference_masked, all lengths = T", lambda: this.inference(video, emb, gum, S=S, video_lengths=[T] * B)),
                ("this build, l2s_inference_masked, true lengths", lambda: this.inference(video, emb, gum, S=S, video_lengths=lens))]
    parent = next((abtime.synth_model(lib) for _, lib in abtime.libs_from_env("PARENT_LIB", native._load)), None)
    if parent is not None:
        variants.insert(0, ("parent build, l2s_inference", lambda: parent.inference(video, emb, gum, S=S)))
        variants.append(("parent build, l2s_inference_masked, true lengths", lambda: parent.inference(video, emb, gum, S=S, video_lengths=lens)))
    print(f"B = {B} clips, lengths {sorted(lens)} zero-padded to T = {T}, S = {S}; {ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; "
          f"median of the rounds, spread = max - min")
    t, outs = abtime.rounds(variants, ROUNDS, REPS)          # the warm-up call covers every shape and route
    ref = outs[1 if parent is not None else 0]
    for (name, _), o in zip(variants, outs):
        print(f"  {name:<52} mel_post bit-identical to this build's l2s_inference: {torch.equal(o[0], ref[0])}")
    med = abtime.report(variants, t, ratio="this build's l2s_inference", base=1 if parent is not None else 0)
    if parent is not None:
        lo, hi = min(t[0]), max(t[0])
        print(f"default path: this build's l2s_inference median {med[1]:.3f} ms; the parent build's rounds span [{lo:.3f}, {hi:.3f}] ms -> "
              f"{'inside' if lo <= med[1] <= hi else 'OUTSIDE'} the parent's spread")
        print(f"masked route, true lengths: both builds bit-identical: {torch.equal(outs[3][0], outs[4][0])}; this build's median {med[3]:.3f} ms, the parent "
              f"build's rounds span [{min(t[4]):.3f}, {max(t[4]):.3f}] ms -> {'inside or below' if abtime.not_above(t[3], t[4]) else 'ABOVE'} the parent's span")


if __name__ == "__main__":
    main()
