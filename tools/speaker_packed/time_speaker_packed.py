"""What the voice tower costs on clips of unequal length (include/l2s.h `l2s_speaker_encoder_packed`) - the speaker embedding of demo.py / evaluate.py,
once per batch, NOT on the mel-frames/s path:
  (a) `l2s_speaker_encoder_fwd` on the clips zero-padded to the longest (B x L_max rows; what every caller ran before, and the default still);
  (b) `l2s_speaker_encoder_packed` on the same clips packed back to back (R = sum L_b rows; the same 3 x L_max step launches);
  (c) with `PARENT_LIB=<path to a build of the parent commit's library>`: (a) from that build, in the same process - the default path has not moved.
Shapes: 16 clips of 16 000 - 48 000 samples (1 - 3 s, evenly spread) padded to 48 000, and 32 clips of 16 640 - 32 000.  Uploads and workspace allocation
are outside the timed region.  ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the REPS calls;
per variant the median of the rounds and the spread.
-> profiles/speaker_packed_times.txt (stdout)

Lives in a sub-directory of tools/ (like ragged/): the flat tools/ inventory is pinned by tests/test_tools_smoke.py."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from lip2speech_amd import native, statespec, synth

REPS = int(os.environ.get("REPS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 7))
WORKLOADS = (("16 clips of 1 - 3 s", 16, 16000, 48000), ("32 clips of 1.04 - 2 s", 32, 16640, 32000))


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


def model(L, sd):
    nm = native.NativeModel(L)
    nm.load({k: v.cuda() for k, v in sd.items()}, list(sd.keys()))
    return nm


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
    outs = [fn().clone() for _, fn in variants]          # warm-up of every route
    torch.cuda.synchronize()
    R, L_max = sum(n // 160 + 1 for n in ns), N // 160 + 1
    print(f"\n== {title}: B = {B}, {min(ns)} - {N} samples; padded rows B x L_max = {B * L_max}, compact rows R = {R} ({R / (B * L_max):.3f}); {3 * L_max} step launches either way")
    full = [b for b, n in enumerate(ns) if n == N]
    print(f"(b) against (a): max |d emb| on the full-length clip(s) {float((outs[0][full] - outs[1][full]).abs().max()):.3e}, on the padded ones "
          f"{float((outs[0] - outs[1]).abs().max()):.3e} (the padded call runs on over the padding)")
    if parent is not None:
        print(f"(c) against (a): embeddings bit-identical: {torch.equal(outs[2], outs[0])}")
    t = rounds(variants)
    med = [statistics.median(x) for x in t]
    for (name, _), x, m in zip(variants, t, med):
        print(f"{name:<52} {m * 1e3:9.1f} us  (spread {(max(x) - min(x)) * 1e3:7.1f}, min {min(x) * 1e3:9.1f}, max {max(x) * 1e3:9.1f})   x{m / med[0]:6.3f} of (a)")


def main():
    sd = synth.synth_state_dict(statespec.speaker_encoder_spec("speaker_encoder."), seed=99)
    parent_path = os.environ.get("PARENT_LIB")
    nm = model(native.lib(), sd)
    parent = model(native._load(parent_path), sd) if parent_path else None
    print(f"{ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min"
          + (f"; PARENT_LIB = {os.path.basename(parent_path)}" if parent else "; PARENT_LIB not given: this build only"))
    for w in WORKLOADS:
        workload(*w, nm, parent)


if __name__ == "__main__":
    main()
