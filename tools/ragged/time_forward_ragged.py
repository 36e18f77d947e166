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
`G=` batches per group (8), `CLIPS=` clips per batch and `LENS=lo-hi` the length range (one workload of that shape instead of the two above; the default
path then runs at CLIPS clips per batch too), `ROUNDS=`, `REPS=`.
-> profiles/forward_ragged_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native, synth
from tools import abtime

REPS = int(os.environ.get("REPS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 7))
G = int(os.environ.get("G", 8))
WORKLOADS = (("config 4's shape", 16, 25, 75), ("config 5's shape", 32, 26, 50))
if os.environ.get("CLIPS") or os.environ.get("LENS"):
    WORKLOADS = (("CLIPS / LENS", int(os.environ.get("CLIPS", 16)), *(int(v) for v in os.environ.get("LENS", "25-75").split("-"))),)


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

    variants = [(f"(a) this build, {G} x l2s_forward_eval_masked", masked8(this)),
                ("(b) this build, 1 x l2s_forward_eval_ragged", lambda: this.forward_eval_ragged(batches, lens, Ss))]
    if parent is not None:
        variants.append((f"(a) parent build, {G} x l2s_forward_eval_masked", masked8(parent)))
        variants.append(("(b) parent build, 1 x l2s_forward_eval_ragged", lambda: parent.forward_eval_ragged(batches, lens, Ss)))
    t, outs = abtime.rounds(variants, ROUNDS, REPS)          # the warm-up call covers every shape and route
    same = all(all(torch.equal(x, y) for x, y in zip(a, b)) for a, b in zip(outs[0], outs[1]))
    worst = max(float((a[1] - b[1]).abs().max()) for a, b in zip(outs[0], outs[1]))
    print(f"(b) against (a): all five outputs bit-identical: {same} (max |d mel_post| = {worst:.3e}; the kernel choice depends on the row count at these sizes, DESIGN.md section 8)")
    med = abtime.report(variants, t)
    print(f"(b) rounds span [{min(t[1]):.3f}, {max(t[1]):.3f}] ms, (a) rounds span [{min(t[0]):.3f}, {max(t[0]):.3f}] ms -> "
          f"{'(b) lies wholly under (a)' if abtime.wholly_under(t[1], t[0]) else 'the spans OVERLAP: no gain outside the spread'}; (a) / (b) = {med[0] / med[1]:.2f}; "
          f"per batch {med[0] / G:.3f} -> {med[1] / G:.3f} ms")
    if parent is not None:
        print(f"today's route, {G} x l2s_forward_eval_masked: this build {med[0]:.3f} ms, parent build {med[2]:.3f} ms -> a median "
              f"{'inside' if abtime.median_inside(t[0], t[2]) else 'OUTSIDE'} the other's spread")
        same = all(all(torch.equal(x, y) for x, y in zip(a, b)) for a, b in zip(outs[1], outs[3]))
        print(f"ragged route, 1 x l2s_forward_eval_ragged: both builds bit-identical: {same}; this build {med[1]:.3f} ms, parent build {med[3]:.3f} ms (rounds "
              f"[{min(t[3]):.3f}, {max(t[3]):.3f}]) -> {'inside or below' if abtime.not_above(t[1], t[3]) else 'ABOVE'} the parent's span")


def default_path(this, parent):
    B, T, S = int(os.environ.get("CLIPS", 32)), 29, 77
    batches = [(synth.synth_video(B, T, tag=f"fwd-multi-{g}").cuda(), synth.synth_speaker_embedding(B, tag=f"fwd-multi-{g}").cuda(),
                synth.synth_gumbel(B * native.min_T(T), tag=f"fwd-multi-{g}").cuda()) for g in range(G)]
    variants = [("this build, l2s_forward_eval_multi", lambda: this.forward_eval_multi(batches, S)),
                ("parent build, l2s_forward_eval_multi", lambda: parent.forward_eval_multi(batches, S))]
    t, outs = abtime.rounds(variants, ROUNDS, REPS)
    same = all(all(torch.equal(x, y) for x, y in zip(a, b)) for a, b in zip(outs[0], outs[1]))
    print(f"\n== default path: l2s_forward_eval_multi, G = {G}, B = {B}, T = {T}, S = {S}; both builds bit-identical: {same}")
    abtime.report(variants, t)
    print(f"-> a median {'inside' if abtime.median_inside(t[0], t[1]) else 'OUTSIDE'} the other's spread")


def main():
    this = abtime.synth_model()
    parent = next((abtime.synth_model(lib) for _, lib in abtime.libs_from_env("PARENT_LIB", native._load)), None)
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min"
          + ("" if parent else "; PARENT_LIB not given: this build only, default path not measured"))
    for w in WORKLOADS:
        workload(*w, this, parent)
    if parent is not None:
        default_path(this, parent)


if __name__ == "__main__":
    main()
