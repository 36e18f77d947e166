"""What a ragged group buys (include/l2s.h "ragged groups"): G = 8 padded batches of unequal length, S = 300, as
  (a) eight l2s_inference_masked calls back to back - the honour_lengths route before l2s_inference_ragged existed - from this build and, with
      `PARENT_LIB=<path to a libl2s_hip.so built from the parent commit>`, from that build in the same process;
  (b) ONE l2s_inference_ragged call;
  (c) for orientation only (its results are OTHER results: every clip then depends on its padding): l2s_inference_multi on the batches re-padded to
      a common T, lengths ignored.
Workloads: 8 x 16 clips with lengths uniform in [25, 75], each batch padded to its own maximum (BASELINE.json config 4's shape, N = 128 clips), and
8 x 32 clips in [26, 50] (config 5's shape, N = 256).  Per workload: sum len against sum B_g * T_g (the encoder frames done against the padded
frames), and the front-end / trunk time of (a) and (b) from the launch profile (l2s_profile_*, one profiled call each).
Default path: with PARENT_LIB, the parent's l2s_inference (first batch) and l2s_inference_multi (variant c) next to this build's, interleaved.
ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the REPS calls; per variant the median of
the rounds and the spread.  Acceptance (the criterion of "persist_frames"): the whole span of (b)'s rounds lies under the whole span of (a)'s.
`G=` batches per group (8), `CLIPS=` clips per batch and `LENS=lo-hi` the length range (one workload of that shape instead of the two above), `S=`,
`ROUNDS=`, `REPS=`.
-> profiles/ragged_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native, synth
from tools import abtime

REPS = int(os.environ.get("REPS", 10))
ROUNDS = int(os.environ.get("ROUNDS", 7))
S = int(os.environ.get("S", 300))
G = int(os.environ.get("G", 8))
WORKLOADS = (("config 4's shape", 16, 25, 75), ("config 5's shape", 32, 26, 50))
if os.environ.get("CLIPS") or os.environ.get("LENS"):
    WORKLOADS = (("CLIPS / LENS", int(os.environ.get("CLIPS", 16)), *(int(v) for v in os.environ.get("LENS", "25-75").split("-"))),)


def encoder_ms(fn):
    """(front-end ms, trunk ms) of one profiled call"""
    native.profile_enable(True)
    try:
        native.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = native.profile_read()
    finally:
        native.profile_enable(False)
    fe = sum(ms for name, _, ms in prof if name.startswith("frontend3d_conv"))
    trunk = sum(ms for name, _, ms in prof if name.startswith("shuffle_") or name == "conv_last_gemm")
    return fe, trunk


def workload(title, B, lo, hi, this, parent):
    tag = f"ragged-times-{B}"
    # uniform draws, NOT synth_clip_lengths (which forces one clip of every batch to `hi`): the batches are to differ in their own maximum
    lens = [[min(hi, lo + int(u * (hi - lo + 1))) for u in synth.uniform01(f"lens:{tag}-{g}", B).astype(float)] for g in range(G)]
    Ts = [max(l) for l in lens]
    Tmax = max(Ts)
    base = synth.synth_video(B, Tmax, tag=tag).cuda()      # one set of frames, cut to every batch's own T (what the frames hold does not move a time)
    batches, common = [], []
    for g in range(G):
        v = base[:, :, :Ts[g]].clone()
        for b, n in enumerate(lens[g]):
            v[b, :, n:] = 0
        emb = synth.synth_speaker_embedding(B, tag=f"{tag}-{g}").cuda()
        batches.append((v, emb, synth.synth_gumbel(B * native.min_T(Ts[g]), tag=f"{tag}-{g}").cuda()))
        vc = torch.zeros(B, 3, Tmax, 96, 96, device="cuda")
        vc[:, :, :Ts[g]] = v
        common.append((vc, emb, synth.synth_gumbel(B * native.min_T(Tmax), tag=f"{tag}-c{g}").cuda()))
    real, padded = sum(sum(l) for l in lens), sum(B * t for t in Ts)
    print(f"\n== {title}: {G} batches x {B} clips, lengths U[{lo}, {hi}], each batch padded to its own maximum {Ts}; N = {G * B} clips, S = {S}")
    print(f"encoder frames: sum len = {real} against sum B_g * T_g = {padded} padded frames ({real / padded:.1%}); re-padded to a common T = {Tmax}: {G * B * Tmax}")

    def masked8(nm):
        return lambda: [nm.inference(*bt, S=S, video_lengths=l) for bt, l in zip(batches, lens)]

    variants = [(f"(a) this build, {G} x l2s_inference_masked", masked8(this)),
                ("(b) this build, 1 x l2s_inference_ragged", lambda: this.inference_ragged(batches, lens, S=S)),
                ("(c) this build, l2s_inference_multi, re-padded (other results)", lambda: this.inference_multi(common, S=S)),
                ("    this build, l2s_inference, first batch", lambda: this.inference(*batches[0], S=S))]
    if parent is not None:
        variants += [(f"(a) parent build, {G} x l2s_inference_masked", masked8(parent)),
                     ("(c) parent build, l2s_inference_multi, re-padded", lambda: parent.inference_multi(common, S=S)),
                     ("    parent build, l2s_inference, first batch", lambda: parent.inference(*batches[0], S=S)),
                     ("(b) parent build, 1 x l2s_inference_ragged", lambda: parent.inference_ragged(batches, lens, S=S))]
    t, outs = abtime.rounds(variants, ROUNDS, REPS)          # the warm-up call covers every shape and route
    same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(outs[0], outs[1]))
    worst = max(float((a[0] - b[0]).abs().max()) for a, b in zip(outs[0], outs[1]))
    print(f"(b) against (a): mel_post and lengths bit-identical: {same} (max |d mel_post| = {worst:.3e}; the kernel choice depends on the row count at these sizes, DESIGN.md section 8)")
    med = abtime.report(variants, t, ratio="(a)")
    print(f"acceptance: (b) rounds span [{min(t[1]):.3f}, {max(t[1]):.3f}] ms, (a) rounds span [{min(t[0]):.3f}, {max(t[0]):.3f}] ms -> "
          f"{'(b) lies wholly under (a)' if abtime.wholly_under(t[1], t[0]) else 'the spans OVERLAP'}; (a) / (b) = {med[0] / med[1]:.2f}")
    if parent is not None:
        for mine, theirs, what in ((0, 4, f"{G} x l2s_inference_masked"), (2, 5, "l2s_inference_multi"), (3, 6, "l2s_inference")):
            print(f"default path, {what}: this build {med[mine]:.3f} ms (rounds [{min(t[mine]):.3f}, {max(t[mine]):.3f}]), parent build {med[theirs]:.3f} ms "
                  f"(rounds [{min(t[theirs]):.3f}, {max(t[theirs]):.3f}]) -> a median {'inside' if abtime.median_inside(t[mine], t[theirs]) else 'OUTSIDE'} the other's spread")
        same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(outs[1], outs[7]))
        print(f"ragged route, 1 x l2s_inference_ragged: both builds bit-identical: {same}; this build {med[1]:.3f} ms, parent build {med[7]:.3f} ms (rounds "
              f"[{min(t[7]):.3f}, {max(t[7]):.3f}]) -> {'inside or below' if abtime.not_above(t[1], t[7]) else 'ABOVE'} the parent's span")
    fe_a, tr_a = encoder_ms(variants[0][1])
    fe_b, tr_b = encoder_ms(variants[1][1])
    print(f"launch profile (one call, event brackets around every launch): front-end (a) {fe_a:.3f} ms -> (b) {fe_b:.3f} ms; trunk (a) {tr_a:.3f} ms -> (b) {tr_b:.3f} ms")


def main():
    this = abtime.synth_model()
    parent = next((abtime.synth_model(lib) for _, lib in abtime.libs_from_env("PARENT_LIB", native._load)), None)
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min"
          + ("" if parent else "; PARENT_LIB not given: this build only"))
    for w in WORKLOADS:
        workload(*w, this, parent)


if __name__ == "__main__":
    main()
