"""What an evaluate-shaped ragged group buys (include/l2s.h, l2s_forward_eval_ragged): G = 8 padded batches of unequal B x T and step count, free-running
(evaluate.py's tf_ratio = 1), as
  (a) eight l2s_forward_eval_masked calls back to back - the honour_lengths evaluate route before l2s_forward_eval_ragged existed - from this build and,
      with `PARENT_LIB=<path to a libl2s_hip.so built from the parent commit>`, from that build in the same process;
  (b) ONE l2s_forward_eval_ragged call.
Workloads (those of time_ragged.py): 8 x 16 clips with lengths uniform in [25, 75], each batch padded to its own maximum T_g, and 8 x 32 clips in [26, 50];
S_g = round(2.5 * T_g) (GRID has 188 mel frames per 75 video frames).  Per workload the share sum B_g S_g / (N * Smax) of the decode rows that are real:
the chain decodes every row for Smax steps.
Default path: with PARENT_LIB, l2s_forward_eval_multi at G = 8, B = 32, T = 29, S = 77 from both builds, interleaved: it must not move outside the spread.
ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the REPS calls; per variant the median of the
rounds and the spread.  No ratio is fixed in advance: the tool writes what it measures and says so when (b)'s rounds do not lie wholly under (a)'s.
-> profiles/forward_ragged_times.txt (stdout)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from lip2speech_amd import native, synth

REPS = int(os.environ.get("REPS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 7))
G = 8
WORKLOADS = (("config 4's shape", 16, 25, 75), ("config 5's shape", 32, 26, 50))


def model(library=None):
    sd = synth.synth_state_dict()
    nm = native.NativeModel(library)
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
    t = [[] for _ in variants]
    for r in range(ROUNDS):
        order = list(range(len(variants)))
        order = order[r % len(order):] + order[:r % len(order)]
        for i in order:
            t[i].append(timed(variants[i][1]))
    return t


def report(variants, t):
    med = [statistics.median(x) for x in t]
    for (name, _), x, m in zip(variants, t, med):
        print(f"{name:<58} {m:8.3f} ms  (spread {max(x) - min(x):6.3f}, min {min(x):8.3f}, max {max(x):8.3f})")
    return med


def inside(t, med, i, j):
    return min(t[j]) <= med[i] <= max(t[j]) or min(t[i]) <= med[j] <= max(t[i])


def workload(title, B, lo, hi, this, parent):
    tag = f"ragged-times-{B}"
    # uniform draws, as in time_ragged.py: the batches are to differ in their own maximum
    lens = [[min(hi, lo + int(u * (hi - lo + 1))) for u in synth.uniform01(f"lens:{tag}-{g}", B).astype(float)] for g in range(G)]
    Ts = [max(l) for l in lens]
    Ss = [int(round(2.5 * t)) for t in Ts]
    base = synth.synth_video(B, max(Ts), tag=tag).cuda()      # one set of frames, cut to every batch's own T (what the frames hold does not move a time)
    batches = []
    for g in range(G):
        v = base[:, :, :Ts[g]].clone()
        for b, n in enumerate(lens[g]):
            v[b, :, n:] = 0
        batches.append((v, synth.synth_speaker_embedding(B, tag=f"{tag}-{g}").cuda(), synth.synth_gumbel(B * native.min_T(Ts[g]), tag=f"{tag}-{g}").cuda()))
    real, done = sum(B * s for s in Ss), G * B * max(Ss)
    print(f"\n== {title}: {G} batches x {B} clips, lengths U[{lo}, {hi}], each batch padded to its own maximum T_g = {Ts}, S_g = round(2.5 T_g) = {Ss}; N = {G * B} clips")
    print(f"decode rows: sum B_g S_g = {real} real of N * Smax = {done} decoded ({real / done:.1%})")

    def masked8(nm):
        return lambda: [nm.forward_eval(*bt, s, video_lengths=l) for bt, s, l in zip(batches, Ss, lens)]

    variants = [("(a) this build, 8 x l2s_forward_eval_masked", masked8(this)),
                ("(b) this build, 1 x l2s_forward_eval_ragged", lambda: this.forward_eval_ragged(batches, lens, Ss))]
    if parent is not None:
        variants.append(("(a) parent build, 8 x l2s_forward_eval_masked", masked8(parent)))
    outs = [fn() for _, fn in variants]          # warm-up of every shape and route
    torch.cuda.synchronize()
    same = all(all(torch.equal(x, y) for x, y in zip(a, b)) for a, b in zip(outs[0], outs[1]))
    worst = max(float((a[1] - b[1]).abs().max()) for a, b in zip(outs[0], outs[1]))
    print(f"(b) against (a): all five outputs bit-identical: {same} (max |d mel_post| = {worst:.3e}; the kernel choice depends on the row count at these sizes, DESIGN.md section 8)")
    t = rounds(variants)
    med = report(variants, t)
    print(f"(b) rounds span [{min(t[1]):.3f}, {max(t[1]):.3f}] ms, (a) rounds span [{min(t[0]):.3f}, {max(t[0]):.3f}] ms -> "
          f"{'(b) lies wholly under (a)' if max(t[1]) < min(t[0]) else 'the spans OVERLAP: no gain outside the spread'}; (a) / (b) = {med[0] / med[1]:.2f}; "
          f"per batch {med[0] / G:.3f} -> {med[1] / G:.3f} ms")
    if parent is not None:
        print(f"today's route, 8 x l2s_forward_eval_masked: this build {med[0]:.3f} ms, parent build {med[2]:.3f} ms -> a median "
              f"{'inside' if inside(t, med, 0, 2) else 'OUTSIDE'} the other's spread")


def default_path(this, parent):
    B, T, S = 32, 29, 77
    batches = [(synth.synth_video(B, T, tag=f"fwd-multi-{g}").cuda(), synth.synth_speaker_embedding(B, tag=f"fwd-multi-{g}").cuda(),
                synth.synth_gumbel(B * native.min_T(T), tag=f"fwd-multi-{g}").cuda()) for g in range(G)]
    variants = [("this build, l2s_forward_eval_multi", lambda: this.forward_eval_multi(batches, S)),
                ("parent build, l2s_forward_eval_multi", lambda: parent.forward_eval_multi(batches, S))]
    outs = [fn() for _, fn in variants]
    torch.cuda.synchronize()
    same = all(all(torch.equal(x, y) for x, y in zip(a, b)) for a, b in zip(outs[0], outs[1]))
    print(f"\n== default path: l2s_forward_eval_multi, G = {G}, B = {B}, T = {T}, S = {S}; both builds bit-identical: {same}")
    t = rounds(variants)
    med = report(variants, t)
    print(f"-> a median {'inside' if inside(t, med, 0, 1) else 'OUTSIDE'} the other's spread")


def main():
    this = model()
    parent_path = os.environ.get("PARENT_LIB")
    parent = model(native._load(parent_path)) if parent_path else None
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min"
          + ("" if parent else "; PARENT_LIB not given: this build only, default path not measured"))
    for w in WORKLOADS:
        workload(*w, this, parent)
    if parent is not None:
        default_path(this, parent)


if __name__ == "__main__":
    main()
