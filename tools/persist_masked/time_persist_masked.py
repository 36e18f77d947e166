"""Option "persist_masked" (include/l2s.h): what the persistent forms buy a masked call.  One l2s_inference_masked at S = 300 on a model with the
option off (the masked launch-per-phase route: the parent's code unchanged) against a model with it on (pdecode.hip's length-masked instantiations),
both at persist_decode = 4, persist_frames = 80, for
  B = 2 [40, 75] padded to 75;  B = 4 [27, 50, 62, 75] padded to 75;  B = 4 [26, 34, 42, 50] padded to 50;  B = 2 [13, 29] padded to 29.
In the same process: the UNMASKED persistent call of two 75-frame clips (what do lengths cost on this route?), and
`PARENT_LIB=<path to a libl2s_hip.so built from the parent commit>`: an unmasked B = 2, T = 29 call of that build interleaved with this build's (has the
default path moved?).  Per shape: ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the REPS
calls; per variant the median of the rounds and the spread (max - min).  A row says "faster beyond the spread" only where option-off's median minus
option-on's exceeds the two spreads added.
-> profiles/persist_masked_times.txt (stdout)

Lives in a sub-directory of tools/ (like persist_long/, masked_lengths/ and early_stop/): the flat tools/ inventory is pinned by tests/test_tools_smoke.py."""
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
SHAPES = [([40, 75], 75), ([27, 50, 62, 75], 75), ([26, 34, 42, 50], 50), ([13, 29], 29)]
BASE = dict(persist_decode=4, persist_frames=80)


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


def rounds(variants):
    """-> per variant: the per-round times, after one warm-up call each"""
    outs = [fn() for _, fn in variants]
    torch.cuda.synchronize()
    t = [[] for _ in variants]
    for r in range(ROUNDS):
        order = list(range(len(variants)))
        order = order[r % len(order):] + order[:r % len(order)]
        for i in order:
            t[i].append(timed(variants[i][1]))
    return t, outs


def cells(variants, t):
    return "   ".join(f"{name}: {statistics.median(x):7.3f} (spread {max(x) - min(x):5.3f})" for (name, _), x in zip(variants, t))


def inputs(lens, T, tag):
    B = len(lens)
    video = synth.synth_video(B, T, tag=tag)
    for b, n in enumerate(lens):
        video[b, :, n:] = 0
    return video.cuda(), synth.synth_speaker_embedding(B, tag=tag).cuda(), synth.synth_gumbel(B * native.min_T(T), tag=tag).cuda()


def main():
    off = model(**BASE)
    on = model(persist_masked=1, **BASE)
    print(f"l2s_inference_masked, S = {S}, persist_decode = 4, persist_frames = 80; persistent forms available on this device: {native.persist_available()}; "
          f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; ms per call: median of the rounds (spread = max - min)")
    for lens, T in SHAPES:
        video, emb, gum = inputs(lens, T, f"pmt{len(lens)}_{T}")
        variants = [("persist_masked = 0", lambda: off.inference(video, emb, gum, S=S, video_lengths=lens)),
                    ("persist_masked = 1", lambda: on.inference(video, emb, gum, S=S, video_lengths=lens))]
        if lens == [40, 75]:
            variants.append(("unmasked T = 75, persistent", lambda: on.inference(video, emb, gum, S=S)))
        t, outs = rounds(variants)
        med = [statistics.median(x) for x in t]
        gain, spread = med[0] - med[1], (max(t[0]) - min(t[0])) + (max(t[1]) - min(t[1]))
        verdict = (f"x{med[0] / med[1]:.2f}, {gain * 1e3 / S:5.2f} us per step saved, {'faster' if gain > spread else 'NOT faster'} beyond the spread "
                   f"({gain:.3f} against {spread:.3f}); same bits as the launch route: {torch.equal(outs[0][0], outs[1][0])}")
        print(f"B = {len(lens)} {str(lens):18s} padded to {T:2d}   {cells(variants, t)}   {verdict}")
    parent_path = os.environ.get("PARENT_LIB")
    if parent_path:
        parent = model(native._load(parent_path), persist_decode=4)
        video, emb, gum = inputs([29, 29], 29, "pmt-parent")
        variants = [("this build", lambda: off.inference(video, emb, gum, S=S)), ("parent build", lambda: parent.inference(video, emb, gum, S=S))]
        t, outs = rounds(variants)
        lo, hi = min(t[1]), max(t[1])
        m = statistics.median(t[0])
        print(f"B = 2 unmasked T = 29 (default path)   {cells(variants, t)}   same bits: {torch.equal(outs[0][0], outs[1][0])}; "
              f"this build's median {'inside' if lo <= m <= hi else 'OUTSIDE'} the parent's rounds [{lo:.3f}, {hi:.3f}]")
    torch.cuda.synchronize()
    print(f"persistent launches that gave up: {native.persist_timeouts()}")


if __name__ == "__main__":
    main()
