"""Cost of the mel-length forms of the decoder half of a training step (include/l2s.h "training with per-clip mel lengths"; running statistics): post-net
forward with its tape, the 4-term loss with its gradients, post-net backward - on B = 16 clips of 63 - 188 mel frames padded to S = 188, no dropout:
    unmasked (l2s_train_postnet_fwd, l2s_loss, l2s_train_postnet_bwd);  masked with ALL lengths = S (the same arithmetic: what the row kernels and the
    table uploads cost);  masked at the true lengths.
`PARENT_LIB=<path to a libl2s_hip.so built from the parent commit>`: that build's unmasked calls are timed in the same process, interleaved with this
build's (has the default path moved?  verdict: abtime.median_inside, i.e. agreement within the measured round-to-round spread).
The expectation, written down before any measurement: the loss keeps its two launches (plus the one that carries the table), the post-net gains about ten
short launches (one row kernel in front, one per layer forward, one per dx backward) and one table upload each way - every one of them a pass over at most
B*S*512 floats that writes only pad rows; the GEMMs are unchanged and still cover the pad rows.  So both masked variants should cost the unmasked time plus
launch-bound microseconds, and no figure is promised.
ROUNDS interleaved rounds of REPS warm calls each, the variants rotating inside a round, HIP events around the REPS calls; per variant the median of the
rounds and the spread (max - min).  `B=`, `S=`, `LO=`, `ROUNDS=`, `REPS=`.
-> profiles/masked_mel_times.txt (stdout)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from lip2speech_amd import native, synth
from lip2speech_amd.training import loss_terms
from tools import abtime

REPS = int(os.environ.get("REPS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 7))
B = int(os.environ.get("B", 16))
S = int(os.environ.get("S", 188))
LO = int(os.environ.get("LO", 63))


def bound_model(library=None):
    """A model with every decoder tensor bound and a gradient slot per parameter (what Lip2Speech._train_state does with its flat buffers)."""
    sd = synth.synth_state_dict()
    nm = abtime.synth_model(library, sd)
    buf = ("running_mean", "running_var", "num_batches_tracked", "pos_table")
    bound = {k: v.clone().cuda() for k, v in sd.items() if k.startswith(("encoder.", "decoder.")) and v.is_floating_point()}
    grads = {k: torch.zeros_like(v) for k, v in bound.items() if not k.endswith(buf)}
    nm.train_bind(bound, grads)
    nm.train_set_bn(False)
    return nm


def main():
    mlens = [int(v) for v in synth.synth_clip_lengths(B, LO, S, "masked-mel-times")]
    mlens[0] = S
    m = 4
    g = torch.Generator(device="cuda").manual_seed(7)
    mel0 = synth.synth_mels(B, S, tag="masked-mel-times").cuda().permute(0, 2, 1).contiguous() + 0.1 * torch.randn(B, S, 80, device="cuda", generator=g)
    target = synth.synth_mels(B, S, tag="masked-mel-times").cuda()
    stop = torch.randn(B, S, device="cuda", generator=g)
    dis = torch.softmax(torch.randn(B * m, 501, device="cuda", generator=g), dim=1)
    gate = torch.zeros(B, S, device="cuda")
    for b, n in enumerate(mlens):
        gate[b, n - 1:] = 1.0
    this = bound_model()

    def half(nm, ml):
        def run():
            mel = mel0.clone()      # the masked forward zeroes pad rows in place: every call gets the loop's frames
            mel_post, tape = nm.train_postnet_fwd(mel, None, **({"mel_lengths": ml} if ml is not None else {}))
            loss, gr = loss_terms(mel.permute(0, 2, 1).contiguous(), mel_post, stop, dis, target, gate, **({"mel_lengths": ml} if ml is not None else {}))
            nm.train_postnet_bwd(mel, gr["mel_post"], tape, None, **({"mel_lengths": ml} if ml is not None else {}))
            return loss
        return run
    variants = [("this build, unmasked", half(this, None)),
                ("this build, masked, all lengths = S", half(this, [S] * B)),
                ("this build, masked, true lengths", half(this, mlens))]
    parent = next((bound_model(lib) for _, lib in abtime.libs_from_env("PARENT_LIB", native._load)), None)
    if parent is not None:
        variants.insert(0, ("parent build, unmasked", half(parent, None)))
    base = 1 if parent is not None else 0
    print(f"B = {B} clips, mel lengths {sorted(mlens)} padded to S = {S} (real frames: {sum(mlens)} of {B * S} = {sum(mlens) / (B * S):.2f}); post-net forward + "
          f"loss + post-net backward; {ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min")
    t, outs = abtime.rounds(variants, ROUNDS, REPS)
    for (name, _), o in zip(variants, outs):
        print(f"  {name:<40} loss terms bit-identical to this build's unmasked calls: {torch.equal(o, outs[base])}")
    abtime.report(variants, t, ratio="this build's unmasked calls", base=base)
    if parent is not None:
        print(f"default path: this build's unmasked calls against the parent build's, abtime.median_inside: "
              f"{'has not moved' if abtime.median_inside(t[1], t[0]) else 'MOVED'}")


if __name__ == "__main__":
    main()
