#!/usr/bin/env python
"""A fixed small driver for comparing which kernels two builds launch (csrc/skinny.hip skinny_form): a staged prologue and l2s_decode_steps at T = 8,
S = 4 for 16, 112 and 208 rows, each with one and with three launch chains hinted, then one early-stop l2s_inference call of two clips.  Run once per
build under a kernel trace of its own, the program after `--`:
    L2S_LIB=<the build's libl2s_hip.so> rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/lstm_shared_panel/skinny_form_trace.py
    python tools/lstm_shared_panel/skinny_form_trace.py hist DIR        # kernel name -> launches, one line each, sorted by name
-> profiles/skinny_form_kernel_trace.txt (the two histograms must be equal line for line)"""
import glob, os, sqlite3, sys

if len(sys.argv) > 2 and sys.argv[1] == "hist":
    db = sorted(glob.glob(os.path.join(sys.argv[2], "**", "*.db"), recursive=True))[0]
    for name, n in sqlite3.connect(db).execute("select name, count(*) from kernels group by name order by name"):
        print(f"{n:6d}  {name}")
    sys.exit(0)

import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from lip2speech_amd import native, synth

T, S, ROWS = 8, 4, (16, 112, 208)
sd = synth.synth_state_dict()
nm = native.NativeModel()
nm.set_option("persist_decode", 0)      # the launch-per-phase loop
nm.load({k: v.cuda() for k, v in sd.items()}, list(sd.keys()))
gen = torch.Generator().manual_seed(1024)
vis = (0.5 * torch.randn(max(ROWS), T, 1024, generator=gen)).cuda()
emb = synth.synth_speaker_embedding(max(ROWS), tag="trace").cuda()
gum = synth.synth_gumbel(max(ROWS) * native.min_T(T), tag="trace").cuda()
for B in ROWS:
    state, _ = nm.decoder_prologue(vis[:B].contiguous(), emb[:B].contiguous(), gum[:B * native.min_T(T)].contiguous())
    for chains in (1, 3):
        native.set_thread_chains(chains)
        nm.decode_steps(state.clone(), B, T, S, want_attn=True)
native.set_thread_chains(1)
nm.set_option("early_stop", 1)
nm.inference(synth.synth_video(2, T, tag="trace").cuda(), emb[:2].contiguous(), gum[:2 * native.min_T(T)].contiguous(), S=S)
torch.cuda.synchronize()
print("skinny_form_trace: done")
