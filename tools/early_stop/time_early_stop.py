"""Time l2s_inference with option "early_stop" on against off (include/l2s.h) on the cases of tests/test_early_stop_gpu.py: one clip of length 183
and two clips of lengths 13 / 220 (persistent decode loop), the 22- / 28- / 29-clip sub-batches of the B = 32 stop golden and the whole batch
(launch-per-phase loop; E = 37 / 238 / 296 / 300), and one grouped chain of 8 such batches.  ROUNDS interleaved rounds of REPS warm calls each,
off and on alternating inside a round, HIP events around the REPS calls; per case the median of the rounds and their spread (max - min).
`DECODE=1` also prints the decode loop's own share from the library's per-kernel event profile (l2s_profile_*; a run of its own: the brackets
serialise the launches).
`ROUNDS=`, `REPS=`.
-> profiles/early_stop_times.txt (stdout)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import early_stop_common as es
from lip2speech_amd import native, synth
from tools import abtime

REPS = int(os.environ.get("REPS", 10))
ROUNDS = int(os.environ.get("ROUNDS", 7))
S = 300


def golden(name):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(ROOT, "tests", "golden", name)).items()}


def model_for(g, persist):
    sd = dict(synth.synth_state_dict())
    sd["decoder.stop_token_layer.linear_layer.weight"] = g["stop_weight"]
    sd["decoder.stop_token_layer.linear_layer.bias"] = g["stop_bias"]
    return abtime.synth_model(state_dict=sd, persist_decode=persist)


def ab(name, nm, fn, E):
    def with_option(v):          # the option is the model's own: every call of a variant sets it first
        def call():
            nm.set_option("early_stop", v)
            return fn()
        return call

    variants = [("    early_stop off", with_option(0)), ("    early_stop on", with_option(1))]
    t, _ = abtime.rounds(variants, ROUNDS, REPS)
    nm.set_option("early_stop", 0)
    print(f"{name:<44} E={E:3d}")
    off, on = abtime.report(variants, t)
    print(f"    on/off {on / off:5.3f}   saved {off - on:7.3f} ms")


def main():
    g32, g2 = golden("stop_lrw_b32.npz"), golden("stop_lrw_b2.npz")
    v32, e32 = synth.synth_video(32, 29, tag="bench"), synth.synth_speaker_embedding(32, tag="bench")
    v2, e2 = synth.synth_video(2, 29, tag="video-lrw2"), synth.synth_speaker_embedding(2, tag="spk-lrw2")
    lens32, lens2 = g32["output_lengths"], g2["output_lengths"]

    def args(video, emb, g, idx):
        return video[idx].cuda(), emb[idx].cuda(), es.gumbel_rows(g["gumbel"], idx).cuda()

    print(f"l2s_inference, S = {S}: option early_stop off / on; {ROUNDS} interleaved rounds x {REPS} warm calls, HIP events; median of the rounds, spread = max - min")
    print(f"persistent forms available: {native.persist_available()}")
    p2, p32, l32 = model_for(g2, 4), model_for(g32, 4), model_for(g32, 0)
    b = lens2.tolist().index(183)
    a = args(v2, e2, g2, [b])
    ab("1 clip, length 183 (persistent)", p2, lambda: p2.inference(*a, S=S), es.end_step(lens2[[b]], S))
    idx = [lens32.tolist().index(13), lens32.tolist().index(220)]
    a2 = args(v32, e32, g32, idx)
    ab("2 clips, lengths 13 / 220 (persistent)", p32, lambda: p32.inference(*a2, S=S), es.end_step(lens32[idx], S))
    ab("2 clips, lengths 13 / 220 (launch route)", l32, lambda: l32.inference(*a2, S=S), es.end_step(lens32[idx], S))
    for max_len, n, E in es.SUB_BATCHES:
        idx = es.rows_upto(lens32, max_len)
        ai = args(v32, e32, g32, idx)
        ab(f"{n} clips, lengths <= {max_len} (launch route)", l32, lambda: l32.inference(*ai, S=S), E)
        if max_len in (27, 228, 300):
            ab(f"group of 8 x {n} clips, lengths <= {max_len}", l32, lambda: l32.inference_multi([ai] * 8, S=S), E)
    if os.environ.get("DECODE", "0") != "0":
        L = native.lib()
        import ctypes
        for max_len, n, E in es.SUB_BATCHES:
            idx = es.rows_upto(lens32, max_len)
            ai = args(v32, e32, g32, idx)
            for v in (0, 1):
                l32.set_option("early_stop", v)
                l32.inference(*ai, S=S)
                torch.cuda.synchronize()
                L.l2s_profile_reset(); L.l2s_profile_enable(1)
                l32.inference(*ai, S=S)
                torch.cuda.synchronize()
                tot = {}
                for i in range(L.l2s_profile_count()):
                    nm_, ln, ms = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_double()
                    L.l2s_profile_get(i, ctypes.byref(nm_), ctypes.byref(ln), ctypes.byref(ms))
                    tot[nm_.value.decode()] = (ln.value, ms.value)
                L.l2s_profile_enable(0)
                step = sum(ms for k, (_, ms) in tot.items() if k.startswith("step_"))
                post = sum(ms for k, (_, ms) in tot.items() if k.startswith("postnet"))
                print(f"  event-bracketed kernels, {n} clips, early_stop={v}: step kernels {step:7.3f} ms in {sum(c for k, (c, _) in tot.items() if k.startswith('step_'))} launches, "
                      f"post-net {post:6.3f} ms")
            l32.set_option("early_stop", 0)


if __name__ == "__main__":
    main()
