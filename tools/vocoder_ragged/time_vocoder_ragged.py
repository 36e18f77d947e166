"""What the ragged forms of the device vocoder and metric buy (include/l2s.h `l2s_inverse_mel_ragged`, `l2s_griffin_lim_ragged`, `l2s_estoi_ragged`;
vocoder.hip) - the tail of evaluate.py / demo.py, NOT on the mel-frames/s path.  Log-mels of unequal length in, waveforms and ESTOI scores out, the vocoder at
ITERS + ITERS iterations, three routes over the same clips:
  (a) solo calls back to back: per clip `MelSpec2Audio(backend="hip")(mel[b:b+1, :, :L_b])` and `estoi_device` on its own samples - what a user of
      `demo_clips` pays today, and the definition of the other two routes' results;
  (b) today's padded call per loader batch: `MelSpec2Audio(backend="hip")(mel_batch)` out to the batch's longest clip and `estoi_device` on the padded pairs -
      what `evaluate_net(honour_lengths=True)` does (it computes something else for every clip but the longest: shown for its time only);
  (c) one ragged call for everything: `MelSpec2Audio(backend="hip")(mel, lengths=...)` and `estoi_device(..., lengths=...)`.
Workload one: CLIPS clips of FRAMES mel frames (one GRID batch); workload two: BATCHES such batches.
EXPECTATION, stated before measuring: (c) beats (a) by roughly the launch count (a long clip's solo vocoder is ~ITERS tile launches, and (c) makes one chain of
them for all clips); (c) beats (b) on the many-batch workload by running one chain sized by the real frames instead of one chain per batch.
Then the DEFAULT path: `l2s_griffin_lim` and `l2s_estoi` at DEFAULT_SHAPE from this build and from every library in `ALT_LIBS=name=path[,name=path...]`
(the parent commit's build; `PARENT_LIB=path` adds one named "parent build") in the same process, with a bit comparison: the solo entry points must not have
moved outside the spread.  Route (c) of both workloads is run from every such library too: same bits, and this build's median inside or below its span.
ROUNDS interleaved rounds, the variants rotating inside a round, wall clock around REPS synchronised calls; per variant the median of the rounds and the span.
`CLIPS=`, `BATCHES=`, `FRAMES=lo-hi`, `DEFAULT_SHAPE=NxL`, `ROUNDS=`, `REPS=`, `ITERS=`.
-> profiles/vocoder_ragged_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from lip2speech_amd import metrics, native
from lip2speech_amd.datasets.spectrograms import MelSpec2Audio, MelSpectrogram
from tools import abtime

ROUNDS = int(os.environ.get("ROUNDS", 7))
REPS = int(os.environ.get("REPS", 1))
ITERS = int(os.environ.get("ITERS", 256))
CLIPS = int(os.environ.get("CLIPS", 16))
BATCHES = int(os.environ.get("BATCHES", 8))
F_LO, F_HI = (int(v) for v in os.environ.get("FRAMES", "63-188").split("-"))
DEF_N, DEF_L = (int(v) for v in os.environ.get("DEFAULT_SHAPE", "16x188").split("x"))
FS = 16000


def from_library(lib, fn):
    """fn with `lib` as the library the package's own callers (native.lib()) reach"""
    def call():
        keep, native._lib = native._lib, lib
        try:
            return fn()
        finally:
            native._lib = keep
    return call


def workload(title, n_batches, alts=()):
    rng = np.random.default_rng(n_batches)
    lengths = [[int(v) for v in rng.integers(F_LO, F_HI + 1, CLIPS)] for _ in range(n_batches)]
    for ls in lengths:
        ls[0], ls[-1] = F_HI, F_LO                                   # every batch is padded to the longest clip, as a GRID batch is
    flat = [L for ls in lengths for L in ls]
    n_flat = [256 * (L - 1) for L in flat]
    t = np.arange(256 * (F_HI - 1)) / FS
    clean = np.stack([np.sin(2 * np.pi * (110 + 7 * i) * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t)) + 0.3 * rng.standard_normal(len(t)) for i in range(len(flat))])
    clean_dev = torch.from_numpy(clean.astype(np.float32) * 0.1).cuda()
    for i, n in enumerate(n_flat):
        clean_dev[i, n:] = 0
    mel = MelSpectrogram(backend="torch").cuda()(clean_dev)[:, :, :F_HI].contiguous()
    voc = MelSpec2Audio(max_iters=ITERS, backend="hip").cuda()
    g = torch.Generator(device="cuda")
    solo_mels = [mel[i:i + 1, :, :L].contiguous() for i, L in enumerate(flat)]
    solo_clean = [clean_dev[i:i + 1, :n].contiguous() for i, n in enumerate(n_flat)]
    keep = {}

    def solo_route():
        g.manual_seed(1)
        waves = [voc(m, generator=g) for m in solo_mels]
        keep["a"] = waves
        return torch.cat([metrics.estoi_device(c, w, FS) for c, w in zip(solo_clean, waves)]).cpu().numpy()

    def padded_route():
        g.manual_seed(1)
        out = []
        for k in range(n_batches):
            rows = slice(k * CLIPS, (k + 1) * CLIPS)
            pred = voc(mel[rows], generator=g)
            out.append(metrics.estoi_device(clean_dev[rows, :pred.shape[1]].contiguous(), pred, FS))
        return torch.cat(out).cpu().numpy()

    def ragged_route(key="c"):
        pred = voc(mel, generator=g.manual_seed(1), lengths=flat)
        keep[key] = pred
        return metrics.estoi_device(clean_dev[:, :pred.shape[1]].contiguous(), pred, FS, lengths=n_flat).cpu().numpy()

    variants = [("(a) solo calls back to back", solo_route), ("(b) padded call per batch", padded_route), ("(c) one ragged call", ragged_route)]
    variants += [(f"(c) one ragged call, {nm}", from_library(lib, lambda nm=nm: ragged_route(nm))) for nm, lib in alts]
    tt, (sa, sb, sc, *s_alt) = abtime.rounds(variants, ROUNDS, REPS, clock="host")          # the warm-up call covers the three routes
    print(f"\n== {title}: {n_batches} x {CLIPS} clips of {F_LO}-{F_HI} mel frames ({sum(flat)} frames, {n_batches * CLIPS * F_HI} padded), {ITERS} + {ITERS} iterations")
    same = all(torch.equal(keep["c"][i, :n], keep["a"][i][0]) and not keep["c"][i, n:].any() for i, n in enumerate(n_flat))
    print(f"waveforms of (c) bit-identical to (a): {same}; scores of (c) bit-identical to (a): {np.array_equal(sa, sc)}")
    print(f"mean ESTOI: (a) {sa.mean():.4f}  (b) {sb.mean():.4f}  (c) {sc.mean():.4f}   ((b) scores padded pairs: another quantity for all but the longest clips)")
    med = abtime.report(variants, tt, ratio="the first")
    print(f"(a) / (c) = {med[0] / med[2]:.2f}, whole span of (c) below the whole span of (a): {abtime.wholly_under(tt[2], tt[0])}")
    print(f"(b) / (c) = {med[1] / med[2]:.2f}, whole span of (c) below the whole span of (b): {abtime.wholly_under(tt[2], tt[1])}")
    for (nm, _), s, x in zip(alts, s_alt, tt[3:]):
        print(f"(c) from {nm}: waveforms and scores bit-identical to this build's: {torch.equal(keep[nm], keep['c']) and np.array_equal(s, sc)}; this build's median "
              f"{med[2]:.3f} ms, its rounds span [{min(x):.3f}, {max(x):.3f}] ms -> {'inside or below' if abtime.not_above(tt[2], x) else 'ABOVE'} its span")


def default_path(alts):
    """The solo entry points at DEFAULT_SHAPE, this build against the other builds: the same bits and the same time."""
    N, L = DEF_N, DEF_L
    n = 256 * (L - 1)
    g = torch.Generator(device="cuda")
    power = torch.rand(N, 513, L, device="cuda", generator=g.manual_seed(2)) ** 4 * 3.0
    ang = torch.rand(N, 513, L, 2, device="cuda", generator=g.manual_seed(3))
    clean = torch.randn(N, n, device="cuda", generator=g.manual_seed(4)) * 0.1
    pred = clean + 0.05 * torch.randn(N, n, device="cuda", generator=g.manual_seed(5))
    h, up, down, n_pre, n_out = metrics.resample_poly_plan(n, metrics.FS, FS)
    fir = torch.from_numpy(h.astype(np.float32)).cuda()
    import ctypes
    bands = (ctypes.c_int * 30)(*metrics.band_edges())

    def gl_call(lib):
        ws = torch.empty(int(lib.l2s_griffin_lim_workspace_bytes(N, L)), dtype=torch.uint8, device="cuda")
        wave = torch.empty(N, n, device="cuda")

        def call():
            native.check(lib.l2s_griffin_lim(power.data_ptr(), ang.data_ptr(), N, L, 1024, 256, ITERS, 0.99, wave.data_ptr(), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream().cuda_stream), lib)
            return wave
        return call

    def es_call(lib):
        ws = torch.empty(int(lib.l2s_estoi_workspace_bytes_long(N, n_out)), dtype=torch.uint8, device="cuda")
        score = torch.empty(N, device="cuda")

        def call():
            native.check(lib.l2s_estoi(clean.data_ptr(), pred.data_ptr(), N, n, fir.data_ptr(), fir.numel(), up, down, n_pre, n_out, bands, score.data_ptr(),
                                       ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), lib)
            return score
        return call

    print(f"\n== the default path: l2s_griffin_lim at {N} x {L} ({ITERS} iterations) and l2s_estoi at {N} x {n} samples, this build"
          + (f" against {', '.join(nm for nm, _ in alts)}" if alts else " (ALT_LIBS not given: nothing to compare with)"))
    for what, make in (("l2s_griffin_lim", gl_call), ("l2s_estoi", es_call)):
        variants = [(f"{what}, this build", make(native.lib()))] + [(f"{what}, {nm}", make(lib)) for nm, lib in alts]
        tt, outs = abtime.rounds(variants, ROUNDS, REPS, clock="host")          # outs: each build's own buffer, which every call of it rewrites
        for (nm, _), out in zip(variants[1:], outs[1:]):
            print(f"{nm}: output bit-identical to this build's: {torch.equal(out, outs[0])}")
        med = abtime.report(variants, tt, ratio="the first")
        for (nm, _), x, m in list(zip(variants, tt, med))[1:]:
            print(f"this build's span ({min(tt[0]):.3f} .. {max(tt[0]):.3f} ms) overlaps the span of {nm} ({min(x):.3f} .. {max(x):.3f}): "
                  f"{min(tt[0]) <= max(x) and min(x) <= max(tt[0])}")


def main():
    alts = abtime.libs_from_env("ALT_LIBS", native._load) + [("parent build", lib) for _, lib in abtime.libs_from_env("PARENT_LIB", native._load)]
    print(f"{ROUNDS} interleaved rounds, wall clock around {REPS} synchronised call(s); median of the rounds, span = min .. max")
    workload("one batch", 1, alts)
    workload(f"{BATCHES} batches", BATCHES, alts)
    default_path(alts)


if __name__ == "__main__":
    main()
