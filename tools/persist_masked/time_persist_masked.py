"""Option "persist_masked" (include/l2s.h): what the persistent forms buy a masked call.  One l2s_inference_masked at S = 300 on a model with the
option off (the masked launch-per-phase route: the parent's code unchanged) against a model with it on (pdecode.hip's length-masked instantiations),
both at persist_decode = 4, persist_frames = 80, for
  B = 2 [40, 75] padded to 75;  B = 4 [27, 50, 62, 75] padded to 75;  B = 4 [26, 34, 42, 50] padded to 50;  B = 2 [13, 29] padded to 29.
In the same process: the UNMASKED persistent call of two 75-frame clips (what do lengths cost on this route?), and
`PARENT_LIB=<path to a libl2s_hip.so built from the parent commit>`: an unmasked B = 2, T = 29 call of that build interleaved with this build's (has the
default path moved?).  Per shape: ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the REPS
calls; per variant the median of the rounds and the spread (max - min).  A row says "faster beyond the spread" only where option-off's median minus
option-on's exceeds the two spreads added.  `LENS=40-75,27-50-62-75,...`: other length lists (each padded to its maximum; the unmasked call rides on
the first), `S=`, `ROUNDS=`, `REPS=`.
-> profiles/persist_masked_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native, synth
from tools import abtime

REPS = int(os.environ.get("REPS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 7))
S = int(os.environ.get("S", 300))
SHAPES = [[int(v) for v in s.split("-")] for s in os.environ.get("LENS", "40-75,27-50-62-75,26-34-42-50,13-29").split(",")]
BASE = dict(persist_decode=4, persist_frames=80)


def inputs(lens, T, tag):
    B = len(lens)
    video = synth.synth_video(B, T, tag=tag)
    for b, n in enumerate(lens):
        video[b, :, n:] = 0
    return video.cuda(), synth.synth_speaker_embedding(B, tag=tag).cuda(), synth.synth_gumbel(B * native.min_T(T), tag=tag).cuda()


def main():
    off = abtime.synth_model(**BASE)
    on = abtime.synth_model(persist_masked=1, **BASE)
    print(f"l2s_inference_masked, S = {S}, persist_decode = 4, persist_frames = 80; persistent forms available on this device: {native.persist_available()}; "
          f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; ms per call: median of the rounds (spread = max - min)")
    for lens in SHAPES:
        T = max(lens)
        video, emb, gum = inputs(lens, T, f"pmt{len(lens)}_{T}")
        variants = [("persist_masked = 0", lambda: off.inference(video, emb, gum, S=S, video_lengths=lens)),
                    ("persist_masked = 1", lambda: on.inference(video, emb, gum, S=S, video_lengths=lens))]
        if lens is SHAPES[0]:
            variants.append((f"unmasked T = {T}, persistent", lambda: on.inference(video, emb, gum, S=S)))
        t, outs = abtime.rounds(variants, ROUNDS, REPS)
        print(f"B = {len(lens)} {str(lens):18s} padded to {T:2d}")
        med = abtime.report(variants, t)
        gain, spread = med[0] - med[1], (max(t[0]) - min(t[0])) + (max(t[1]) - min(t[1]))
        verdict = (f"x{med[0] / med[1]:.2f}, {gain * 1e3 / S:5.2f} us per step saved, {'faster' if gain > spread else 'NOT faster'} beyond the spread "
                   f"({gain:.3f} against {spread:.3f}); same bits as the launch route: {torch.equal(outs[0][0], outs[1][0])}")
        print(f"    {verdict}")
    parent = next((abtime.synth_model(lib, persist_decode=4) for _, lib in abtime.libs_from_env("PARENT_LIB", native._load)), None)
    if parent is not None:
        video, emb, gum = inputs([29, 29], 29, "pmt-parent")
        variants = [("this build", lambda: off.inference(video, emb, gum, S=S)), ("parent build", lambda: parent.inference(video, emb, gum, S=S))]
        t, outs = abtime.rounds(variants, ROUNDS, REPS)
        lo, hi = min(t[1]), max(t[1])
        print("B = 2 unmasked T = 29 (default path)")
        m = abtime.report(variants, t)[0]
        print(f"    same bits: {torch.equal(outs[0][0], outs[1][0])}; "
              f"this build's median {'inside' if lo <= m <= hi else 'OUTSIDE'} the parent's rounds [{lo:.3f}, {hi:.3f}]")
    torch.cuda.synchronize()
    print(f"persistent launches that gave up: {native.persist_timeouts()}")


if __name__ == "__main__":
    main()
