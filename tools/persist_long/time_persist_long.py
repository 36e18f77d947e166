"""Option "persist_frames" (include/l2s.h): what the long-clip forms of the persistent decode loop buy.  One l2s_inference at S = 300 for
B in {1, 2, 4} clips of T in {29, 50, 75} frames on a model with the option at its default (32: clips of more than 32 frames take the launch-per-phase
route) against a model with it at 75 (they take pdecode.hip's long forms; 29-frame clips take the short forms either way).
`PARENT_LIB=<path to a libl2s_hip.so built from the parent commit>`: that build's call is timed in the same process for the T = 29 rows, interleaved
with this build's (has the short path moved?).  Per (B, T): ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round,
HIP events around the REPS calls; per variant the median of the rounds and the spread (max - min).  A row says "faster" only where the whole span of
the option-on rounds lies below the whole span of the option-off rounds.
-> profiles/persist_long_times.txt (stdout)

Lives in a sub-directory of tools/ (like masked_lengths/ and early_stop/): the flat tools/ inventory is pinned by tests/test_tools_smoke.py."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from lip2speech_amd import native, synth

REPS = int(os.environ.get("REPS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 7))
S = int(os.environ.get("S", 300))
BS = [int(v) for v in os.environ.get("BS", "1,2,4").split(",")]
TS = [int(v) for v in os.environ.get("TS", "29,50,75").split(",")]
FRAMES = 75


def model(library=None, **options):
    sd = synth.synth_state_dict()
    nm = native.NativeModel(library)
    for k, v in options.items():
        nm.set_option(k, v)
    nm.load({k: v.cuda() for k, v in sd.items()}, list(sd.keys()))
    return nm


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def main():
    off = model(persist_decode=4)
    on = model(persist_decode=4, persist_frames=FRAMES)
    parent_path = os.environ.get("PARENT_LIB")
    parent = model(native._load(parent_path), persist_decode=4) if parent_path else None
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
            outs = [fn() for _, fn in variants]          # warm-up of every shape and route
            torch.cuda.synchronize()
            t = [[] for _ in variants]
            for r in range(ROUNDS):
                order = list(range(len(variants)))
                order = order[r % len(order):] + order[:r % len(order)]
                for i in order:
                    t[i].append(timed(variants[i][1]))
            med = [statistics.median(x) for x in t]
            cells = "   ".join(f"{name}: {m:7.3f} (spread {max(x) - min(x):5.3f})" for (name, _), x, m in zip(variants, t, med))
            if T <= 32:
                same = all(torch.equal(o[0], outs[0][0]) for o in outs)
                verdict = f"short forms on every variant, same bits: {same}"
                if parent is not None:
                    lo, hi = min(t[2]), max(t[2])
                    verdict += f"; this build's median {'inside' if lo <= med[1] <= hi else 'OUTSIDE'} the parent's rounds [{lo:.3f}, {hi:.3f}]"
            else:
                faster = max(t[1]) < min(t[0])
                verdict = (f"x{med[0] / med[1]:.2f}, {(med[0] - med[1]) * 1e3 / S:5.2f} us per step saved, "
                           f"{'faster beyond the spread' if faster else 'NOT faster beyond the spread'}; same bits as the launch route: {torch.equal(outs[0][0], outs[1][0])}")
            print(f"B = {B} T = {T:3d}   {cells}   {verdict}")
    torch.cuda.synchronize()
    print(f"persistent launches that gave up: {native.persist_timeouts()}")


if __name__ == "__main__":
    main()
