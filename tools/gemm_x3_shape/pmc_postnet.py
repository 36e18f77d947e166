"""One post-net layer (Conv1d 256 x 300 rows, 512 -> 512, k = 5, split-bf16 wide tile with LDS-DMA weight planes) a few times, for a counter-only
rocprofv3 pass: `L2S_LIB=<libl2s_diag.so of the build to profile> PMC_SCRIPT=tools/gemm_x3_shape/pmc_postnet.py PMC_CLOCK_ONLY=1 bash
tools/pmc_dense_kernels.sh`.  -> the clock rows of profiles/gemm_x3_shape_times.txt"""
import os, sys, torch
os.environ.setdefault("L2S_LIB", "diag")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from lip2speech_amd import native
B, T, C, k = int(os.environ.get("CLIPS", 256)), 300, 512, 5
torch.manual_seed(0)
X = torch.randn(B, T, C, device="cuda")
Wp = torch.randn(C, k * C, device="cuda") / (k * C) ** 0.5
for _ in range(6):
    native.op_conv1d(X, Wp, taps=k, pad=k // 2, x3=True, x3_dma=True)
torch.cuda.synchronize()
print(f"post-net layer at {B} clips done (run under rocprofv3: tools/pmc_dense_kernels.sh)")
