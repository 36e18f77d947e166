"""Option "persist_frames" (include/l2s.h): what the long-clip forms of the persistent decode loop buy.  One l2s_inference at S = 300 for
B in {1, 2, 4} clips of T in {29, 50, 75} frames on a model with the option at its default (32: clips of more than 32 frames take the launch-per-phase
route) against a model with it at 75 (they take pdecode.hip's long forms; 29-frame clips take the short forms either way).
`PARENT_LIB=<path to a libl2s_hip.so built from the parent commit>`: that build's call is timed in the same process for the T = 29 rows, interleaved
with this build's (has the short path moved?).  Per (B, T): ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round,
HIP events around the REPS calls; per variant the median of the rounds and the spread (max - min).  A row says "faster" only where the whole span of
the option-on rounds lies below the whole span of the option-off rounds.  `BS=1,2,4`, `TS=29,50,75`, `S=`, `ROUNDS=`, `REPS=`.
-> profiles/persist_long_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native, synth
from tools import abtime

REPS = int(os.environ.get("REPS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 7))
S = int(os.environ.get("S", 300))
BS = [int(v) for v in os.environ.get("BS", "1,2,4").split(",")]
TS = [int(v) for v in os.environ.get("TS", "29,50,75").split(",")]
FRAMES = 75


def main():
    off = abtime.synth_model(persist_decode=4)
    on = abtime.synth_model(persist_decode=4, persist_frames=FRAMES)
    parent = next((abtime.synth_model(lib, persist_decode=4) for _, lib in abtime.libs_from_env("PARENT_LIB", native._load)), None)
    print(f"l2s_inference, S = {S}, persist_decode = 4; persistent forms available on this device: {native.persist_available()}; "
          f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; ms per call: median of the rounds (spread = max - min)")
    for B in BS:
        for T in TS:
            tag = f"plt{B}_{T}"
            video, emb = synth.synth_video(B, T, tag=tag).cuda(), synth.synth_speaker_embedding(B, tag=tag).cuda()
            gum = synth.synth_gumbel(B * native.min_T(T), tag=tag).cuda()
            variants = [("persist_frames = 32", lambda: off.inference(video, emb, gum, S=S)), (f"persist_frames = {FRAMES}", lambda: on.inference(video, emb, gum, S=S))]
            if parent is not None and T <= 32:
                variants.append(("parent build", lambda: parent.inference(video, emb, gum, S=S)))
            t, outs = abtime.rounds(variants, ROUNDS, REPS)          # the warm-up call covers every shape and route
            print(f"B = {B} T = {T:3d}")
            med = abtime.report(variants, t)
            if T <= 32:
                same = all(torch.equal(o[0], outs[0][0]) for o in outs)
                verdict = f"short forms on every variant, same bits: {same}"
                if parent is not None:
                    lo, hi = min(t[2]), max(t[2])
                    verdict += f"; this build's median {'inside' if lo <= med[1] <= hi else 'OUTSIDE'} the parent's rounds [{lo:.3f}, {hi:.3f}]"
            else:
                faster = abtime.wholly_under(t[1], t[0])
                verdict = (f"x{med[0] / med[1]:.2f}, {(med[0] - med[1]) * 1e3 / S:5.2f} us per step saved, "
                           f"{'faster beyond the spread' if faster else 'NOT faster beyond the spread'}; same bits as the launch route: {torch.equal(outs[0][0], outs[1][0])}")
            print(f"    {verdict}")
    torch.cuda.synchronize()
    print(f"persistent launches that gave up: {native.persist_timeouts()}")


if __name__ == "__main__":
    main()
