"""Cost of the training step with per-clip video lengths (include/l2s.h "training with per-clip video lengths"; running statistics): one whole step -
encoder, prologue, S-step loop, post-net, 4-term loss and the backward of all of it (training.model_forward_backward) - on B = 8 clips of 25 - 75 frames
zero-padded to 75, S = 188:
    the unmasked step;  the masked step with ALL lengths = T (the same arithmetic: what the masking machinery costs);  the masked step at the true lengths.
`PARENT_LIB=<path to a libl2s_hip.so built from the parent commit>`: that build's unmasked step is timed in the same process, interleaved with this build's
(has the default path moved?  verdict: abtime.median_inside).
The expectation, written down before any measurement: the encoder's trunk works on sum(len_b) / (B T) of the frames, forward and backward, the front-end and the
loop are unchanged, so the step at the true lengths should be cheaper than the unmasked one by about that share of the trunk's time, and the step with all
lengths = T dearer than the unmasked one by the row kernels and the gather / scatter copies only.
ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the REPS calls; per variant the median of the
rounds and the spread (max - min).  `B=`, `S=`, `LO=`, `HI=`, `ROUNDS=`, `REPS=`.
-> profiles/masked_train_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native, synth
from lip2speech_amd.training import model_forward_backward
from tools import abtime

REPS = int(os.environ.get("REPS", 3))
ROUNDS = int(os.environ.get("ROUNDS", 7))
B = int(os.environ.get("B", 8))
S = int(os.environ.get("S", 188))
LO, HI = int(os.environ.get("LO", 25)), int(os.environ.get("HI", 75))


def bound_model(library=None):
    """A model with every encoder / decoder tensor bound and a gradient slot per parameter (what Lip2Speech._train_state does with its flat buffers)."""
    sd = synth.synth_state_dict()
    nm = abtime.synth_model(library, sd)
    buf = ("running_mean", "running_var", "num_batches_tracked", "pos_table")
    bound = {k: v.clone().cuda() for k, v in sd.items() if k.startswith(("encoder.", "decoder.")) and v.is_floating_point()}
    grads = {k: torch.zeros_like(v) for k, v in bound.items() if not k.endswith(buf)}
    nm.train_bind(bound, grads)
    nm.train_set_bn(False)
    return nm, bound, grads


def main():
    lens = [int(v) for v in synth.synth_clip_lengths(B, LO, HI, "masked-train-times")]
    T = max(lens)
    video = synth.synth_padded_video(B, lens, tag="masked-train-times").cuda()
    emb = synth.synth_speaker_embedding(B, tag="masked-train-times").cuda()
    gum = synth.synth_gumbel(B * native.min_T(T), tag="masked-train-times").cuda()
    mels = synth.synth_mels(B, S, tag="masked-train-times").cuda()
    gate = torch.zeros(B, S, device="cuda")
    gate[:, -1] = 1.0
    this, _, grads = bound_model()

    def step(nm, vl):
        return lambda: model_forward_backward(nm, video, emb, gum, mels, gate, video_lengths=vl)["loss"]
    variants = [("this build, unmasked step", step(this, None)),
                ("this build, masked step, all lengths = T", step(this, [T] * B)),
                ("this build, masked step, true lengths", step(this, lens))]
    parent = next((bound_model(lib)[0] for _, lib in abtime.libs_from_env("PARENT_LIB", native._load)), None)
    if parent is not None:
        variants.insert(0, ("parent build, unmasked step", step(parent, None)))
    base = 1 if parent is not None else 0
    print(f"B = {B} clips, lengths {sorted(lens)} zero-padded to T = {T} (real frames: {sum(lens)} of {B * T} = {sum(lens) / (B * T):.2f}), S = {S}; "
          f"{ROUNDS} interleaved rounds x {REPS} warm steps, HIP events; median of the rounds, spread = max - min")
    t, outs = abtime.rounds(variants, ROUNDS, REPS)
    for (name, _), o in zip(variants, outs):
        print(f"  {name:<44} loss terms bit-identical to this build's unmasked step: {torch.equal(o, outs[base])}")
    abtime.report(variants, t, ratio="this build's unmasked step", base=base)
    if parent is not None:
        print(f"default path: this build's unmasked step against the parent build's, abtime.median_inside: "
              f"{'has not moved' if abtime.median_inside(t[1], t[0]) else 'MOVED'}")


if __name__ == "__main__":
    main()
