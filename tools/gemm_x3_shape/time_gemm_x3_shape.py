"""The split-bf16 GEMM family (gemm_x3.hip) on the 16x16x32 MFMA shape against the parent commit's build (32x32x16), kernel level: the headline path's
launches of that family, each through the operator entries of the diagnostic build with the split-bf16 kernel forced and, where the model brings
weight planes, the LDS-DMA weight form (flags 1 | 8; the per-call derivation of the planes is inside the bracket for both builds alike) -
  Conv1d 256 x 300 rows 512 -> 512, 80 -> 512 and 512 -> 80 with k = 5 (post-net layers 1-3, 0 and 4), the eight MultiHop branch convs at 256 x 29
  rows (k = 1, 3, 7, 11, twice each; the operator entries launch one conv at a time, so the group is timed as its members back to back), the BiLSTM
  input GEMM 7 424 x 4 096 x 1 024 and conv_last 7 424 x 768 x 464 (K an odd multiple of 16).
`PARENT_DIAG_LIB=<path to a libl2s_diag.so built from the parent commit>`: loaded into the same process and timed interleaved with this build's;
without it only this build is timed.  Per shape one untimed round on each build, then ROUNDS interleaved rounds of REPS warm calls each (7 x 10), HIP events around the REPS calls; per shape and
build every round's figure, the median of the rounds and the spread (max - min), then the sum over the shapes.  Last, outside the sum and on this
build alone, 7 424 x 512 on the wide tile against the narrow one (116 tiles against 232, one round of blocks each): the case the tile choice
(x3_wide in gemm_x3.hip) decides by its cost ratio.
`CLIPS=` (256) scales every shape's row count; `ROUNDS=`, `REPS=`.
-> profiles/gemm_x3_shape_times.txt (stdout)

`POST_WINO=1`: instead of the above, the post-net (l2s_postnet, five layers) with layers 1-3 direct (diagnostic option "post_wino" = 0) against their
Winograd F(4,5) form (1: eight K = 512 products of the same family per layer, csrc/post_wino.h) at CLIPS x 300 and CLIPS / 8 x 300 rows, and
`PARENT_LIB=<the parent commit's libl2s_hip.so>` in the same process; same rounds; then the library's event profile per kernel name, five calls averaged.
-> profiles/post_wino_times.txt (stdout)"""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native
from tools import abtime

REPS = int(os.environ.get("REPS", 10))
ROUNDS = int(os.environ.get("ROUNDS", 7))
CLIPS = int(os.environ.get("CLIPS", 256))


def conv_case(name, B, T, Ci, Co, k, flags):
    X = torch.randn(B, T, Ci, device="cuda")
    Wp = (torch.randn(Co, k * Ci, device="cuda") / (k * Ci) ** 0.5)
    out = torch.empty(B, T, Co, device="cuda")

    def run(L):
        native.check(L.l2s_op_conv1d_ex(X.data_ptr(), Wp.data_ptr(), None, None, None, out.data_ptr(), B, T, Ci, Co, k, 1, k // 2, 0, flags, native._stream()), L)
        return out
    return name, [run]


def gemm_case(name, M, N, K, flags):
    A = torch.randn(M, K, device="cuda")
    W = (torch.randn(N, K, device="cuda") / K ** 0.5)
    C = torch.empty(M, N, device="cuda")

    def run(L):
        native.check(L.l2s_op_gemm_ex(A.data_ptr(), W.data_ptr(), None, None, None, C.data_ptr(), M, N, K, 0, flags, native._stream()), L)
        return C
    return name, [run]


def lower(t):
    """the verdict of this tool: this build's median under the parent's by more than the larger of the two spreads (t: parent's rounds, this build's)"""
    spread = max(max(x) - min(x) for x in t)
    return "LOWER by more than the larger spread" if statistics.median(t[0]) - statistics.median(t[1]) > spread else "not lower by more than the larger spread"


def show(name, variants, t):
    print(name)
    med = abtime.report(variants, t, unit="us", ratio="the first" if len(variants) == 2 else None)
    if len(variants) == 2:
        print(f"    this / parent {med[1] / med[0]:5.3f}  {lower(t)}")
    for (bname, _), x in zip(variants, t):
        print(f"    {bname:<12} rounds: " + " ".join(f"{v * 1e3:8.1f}" for v in x))


def event_profile(nm, call):
    """{kernel name: (launches, ms)} per call of `call`, five calls averaged, from the event brackets of the library that owns `nm`"""
    L = nm._L
    call(); torch.cuda.synchronize()
    native.check(L.l2s_profile_reset(), L); native.check(L.l2s_profile_enable(1), L)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    out = {}
    for i in range(L.l2s_profile_count()):
        name, n, ms = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_double()
        native.check(L.l2s_profile_get(i, ctypes.byref(name), ctypes.byref(n), ctypes.byref(ms)), L)
        if n.value:
            out[name.value.decode()] = (n.value // 5, ms.value / 5)
    native.check(L.l2s_profile_enable(0), L); native.check(L.l2s_profile_reset(), L)
    return out


def post_wino():
    parents = abtime.libs_from_env("PARENT_LIB", native._load)[:1]
    direct, wino = abtime.synth_model(native.diag(), post_wino=0), abtime.synth_model(native.diag(), post_wino=1)
    models = [("this build, post_wino 0", direct), ("this build, post_wino 1", wino)] + [(f"parent build ({label})", abtime.synth_model(lib)) for label, lib in parents]
    print(f"l2s_postnet, five layers; {ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min")
    for B in (CLIPS, max(1, CLIPS // 8)):
        torch.manual_seed(1)
        mel = torch.randn(B, 300, 80, device="cuda")
        variants = [(name, (lambda m=m: m.postnet(mel)[0])) for name, m in models]
        t, outs = abtime.rounds(variants, ROUNDS, REPS)
        print(f"\n{B * 300} rows (B = {B}, S = 300)")
        med = abtime.report(variants, t, ratio="post_wino 0")
        print(f"    Winograd - direct: {(med[1] - med[0]) * 1e3:8.1f} us over three layers = {(med[1] - med[0]) * 1e3 / 3:7.1f} us per layer; "
              f"every Winograd round under every direct round: {abtime.wholly_under(t[1], t[0])}")
        print(f"    max |Winograd - direct| = {float((outs[1] - outs[0]).abs().max()):.3e}, max |out| = {float(outs[0].abs().max()):.2f}"
              + (f"; post_wino 0 has the parent's bits: {torch.equal(outs[0], outs[2])}" if parents else ""))
        for name, m in models[:2]:
            pr = event_profile(m, lambda: m.postnet(mel))
            print(f"    event profile, {name}: " + ", ".join(f"{k} {n} x = {ms * 1e3:.0f} us" for k, (n, ms) in sorted(pr.items())))


def main():
    if os.environ.get("POST_WINO", "0") != "0":
        return post_wino()
    torch.manual_seed(0)
    rows = CLIPS * 29
    multihop = ("MultiHop branches, 8 convs 512 -> 512 (k = 1, 3, 7, 11 twice), %d x 29 rows" % CLIPS,
                [conv_case("", CLIPS, 29, 512, 512, k, 9)[1][0] for k in (11, 11, 7, 7, 3, 3, 1, 1)])
    cases = [conv_case(f"Conv1d {CLIPS} x 300 rows 512 -> 512 k = 5 (dma)", CLIPS, 300, 512, 512, 5, 9),
             conv_case(f"Conv1d {CLIPS} x 300 rows  80 -> 512 k = 5 (dma)", CLIPS, 300, 80, 512, 5, 9),
             conv_case(f"Conv1d {CLIPS} x 300 rows 512 ->  80 k = 5 (narrow tile)", CLIPS, 300, 512, 80, 5, 1),
             multihop,
             gemm_case(f"BiLSTM input GEMM {rows} x 4096 x 1024 (dma)", rows, 4096, 1024, 9),
             gemm_case(f"conv_last {rows} x 768 x 464 (dma)", rows, 768, 464, 9)]
    builds = [("parent build", lib) for _, lib in abtime.libs_from_env("PARENT_DIAG_LIB", native._load)][:1] + [("this build", native.diag())]
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; us per call: median of the rounds (spread = max - min)")

    def on_builds(fns):
        return [(bname, lambda L=L: [fn(L) for fn in fns]) for bname, L in builds]

    total = [[0.0] * ROUNDS for _ in builds]
    for name, fns in cases:
        # warm-up of every shape on every build: one untimed round (a single call leaves the first timed round of a shape 7-17 % slow on either
        # build, the clock still settling)
        t, _ = abtime.rounds(on_builds(fns), ROUNDS, REPS, warm=REPS)
        total = [[a + v for a, v in zip(tot, x)] for tot, x in zip(total, t)]
        show(name, on_builds(fns), t)
    show("sum over the six shapes (round by round)", on_builds([]), total)
    # the tile choice's margin case on this build: flags 1 = the wide tile wherever it fits, 1 | 4 = the narrow tile everywhere (in-kernel weight split in both)
    L = builds[-1][1]
    for K in (512, 2560):
        variants = [(form, lambda fn=gemm_case("", rows, 512, K, f)[1][0]: fn(L)) for form, f in (("wide tile", 1), ("narrow tile", 5))]
        print(f"tile choice, this build, {rows} x 512 x {K}:")
        wide, narrow = abtime.report(variants, abtime.rounds(variants, ROUNDS, REPS)[0], unit="us")
        print(f"    wide / narrow {wide / narrow:5.3f}")


if __name__ == "__main__":
    main()
