"""What the voice tower costs on clips of unequal length (include/l2s.h `l2s_speaker_encoder_packed`) - the speaker embedding of demo.py / evaluate.py,
once per batch, NOT on the mel-frames/s path:
  (a) `l2s_speaker_encoder_fwd` on the clips zero-padded to the longest (B x L_max rows; what every caller ran before, and the default still);
  (b) `l2s_speaker_encoder_packed` on the same clips packed back to back (R = sum L_b rows; the same 3 x L_max step launches);
  (c) with `PARENT_LIB=<path to a build of the parent commit's library>`: (a) and (b) from that build, in the same process - neither path has moved.
Shapes: 16 clips of 16 000 - 48 000 samples (1 - 3 s, evenly spread) padded to 48 000, and 32 clips of 16 640 - 32 000.  Uploads and workspace allocation
are outside the timed region.  ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the REPS calls;
per variant the median of the rounds and the spread.  `SHAPES=Bxlo-hi[,Bxlo-hi...]`: other workloads of B clips of lo - hi samples; `ROUNDS=`, `REPS=`.
-> profiles/speaker_packed_times.txt (stdout)"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native, statespec, synth
from tools import abtime

REPS = int(os.environ.get("REPS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 7))
WORKLOADS = (("16 clips of 1 - 3 s", 16, 16000, 48000), ("32 clips of 1.04 - 2 s", 32, 16640, 32000))
if os.environ.get("SHAPES"):
    WORKLOADS = [(s, int(s.split("x")[0]), *(int(v) for v in s.split("x")[1].split("-"))) for s in os.environ["SHAPES"].split(",")]


def padded_call(nm, audio):
    B, N = audio.shape
    L = nm._L
    ws = torch.empty(int(L.l2s_speaker_workspace_bytes(B, N)), dtype=torch.uint8, device="cuda")
    emb = torch.empty(B, 256, device="cuda")

    def call():
        native.check(L.l2s_speaker_encoder_fwd(nm._h, audio.data_ptr(), B, N, emb.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), L)
        return emb
    return call


def packed_call(nm, buf, off, ns):
    B, L = len(ns), nm._L
    offs, nss = (ctypes.c_int64 * B)(*off), (ctypes.c_int64 * B)(*ns)
    ws = torch.empty(int(L.l2s_speaker_workspace_bytes_packed(nss, B)), dtype=torch.uint8, device="cuda")
    emb = torch.empty(B, 256, device="cuda")

    def call():
        native.check(L.l2s_speaker_encoder_packed(nm._h, buf.data_ptr(), offs, nss, B, emb.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), L)
        return emb
    return call


def workload(title, B, lo, hi, nm, parent):
    ns = [int(round(lo + (hi - lo) * b / (B - 1))) for b in range(B)]
    ns = ns[::2] + ns[1::2][::-1]                      # not sorted: the plan does the ranking
    N = max(ns)
    g = torch.Generator().manual_seed(B)
    audio = 0.1 * torch.randn(B, N, generator=g)
    off, pos = [], 0
    for b, n in enumerate(ns):
        audio[b, n:] = 0
        off.append(pos)
        pos += n
    buf = torch.cat([audio[b, :n] for b, n in enumerate(ns)]).cuda()
    audio = audio.cuda()
    variants = [("(a) l2s_speaker_encoder_fwd, padded", padded_call(nm, audio)), ("(b) l2s_speaker_encoder_packed", packed_call(nm, buf, off, ns))]
    if parent is not None:
        variants.append(("(c) PARENT_LIB: l2s_speaker_encoder_fwd, padded", padded_call(parent, audio)))
        variants.append(("(c) PARENT_LIB: l2s_speaker_encoder_packed", packed_call(parent, buf, off, ns)))
    t, outs = abtime.rounds(variants, ROUNDS, REPS)          # outs: each route's own embedding buffer, which every call of it rewrites
    R, L_max = sum(n // 160 + 1 for n in ns), N // 160 + 1
    print(f"\n== {title}: B = {B}, {min(ns)} - {N} samples; padded rows B x L_max = {B * L_max}, compact rows R = {R} ({R / (B * L_max):.3f}); {3 * L_max} step launches either way")
    full = [b for b, n in enumerate(ns) if n == N]
    print(f"(b) against (a): max |d emb| on the full-length clip(s) {float((outs[0][full] - outs[1][full]).abs().max()):.3e}, on the padded ones "
          f"{float((outs[0] - outs[1]).abs().max()):.3e} (the padded call runs on over the padding)")
    if parent is not None:
        print(f"(c) against (a): embeddings bit-identical: {torch.equal(outs[2], outs[0])}")
    abtime.report(variants, t, unit="us", ratio="(a)")
    if parent is not None:
        print(f"(c) packed against (b): embeddings bit-identical: {torch.equal(outs[3], outs[1])}; this build's median "
              f"{'inside or below' if abtime.not_above(t[1], t[3]) else 'ABOVE'} the span of the parent's rounds")


def main():
    sd = synth.synth_state_dict(statespec.speaker_encoder_spec("speaker_encoder."), seed=99)
    nm = abtime.synth_model(native.lib(), sd)
    parent_name, parent = next(((name, abtime.synth_model(lib, sd)) for name, lib in abtime.libs_from_env("PARENT_LIB", native._load)), (None, None))
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min"
          + (f"; PARENT_LIB = {parent_name}" if parent else "; PARENT_LIB not given: this build only"))
    for w in WORKLOADS:
        workload(*w, nm, parent)


if __name__ == "__main__":
    main()
