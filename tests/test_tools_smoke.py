"""Every script under tools/ - sub-directories included - that produces a file under profiles/ runs for one small iteration (`-m gpu`); the readers of
rocprofv3 databases and the shell drivers are checked for syntax (their inputs only exist under a profiler)."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
HIP_LIB = os.path.join(ROOT, "lip2speech_amd", "csrc", "libl2s_hip.so")
DIAG_LIB = os.path.join(ROOT, "lip2speech_amd", "csrc", "libl2s_diag.so")
ONCE = {"ROUNDS": "1", "REPS": "1"}

# script (path relative to tools/) -> (argv, env): the smallest setting each script offers.  The tools/<feature>/time_*.py scripts get this build's own
# library as their parent / alt build, so that the "other build" variants and their bit comparisons run too.
RUNS = {
    "attn_l2_probe.py": ([], {"ROWS": "32"}),
    "attn_timeline.py": ([], {"ROWS": "32"}),
    "coresident_probe.py": (["1"], {"PAIRS": "10", "REP": "1"}),
    "flat_timeline.py": ([], {}),
    "fused_unit_timeline.py": ([], {"B": "32"}),
    "gemm_x3_timeline.py": (["1024", "512", "512"], {}),
    "hash_encoder.py": ([], {}),
    "hash_inference.py": ([], {}),
    "hash_stage_routes.py": ([], {}),
    "hash_step_routes.py": ([], {}),
    "hash_train_step.py": ([], {}),
    "kernel_resources.py": ([os.path.join(ROOT, "lip2speech_amd", "csrc", "decoder_kernels.hip")], {}),
    "overlap_stamps.py": (["1"], {"PAIRS": "10", "S": "10", "CHAINS": "2"}),
    "pdecode_timeline.py": ([], {"B": "2", "S": "20"}),
    "pmc_dense.py": ([], {"ROWS": "32"}),
    "prof_decode.py": ([], {"ROWS": "32", "REPS": "1"}),
    "prof_train.py": ([], {}),
    "s2_unit_timeline.py": ([], {"B": "32"}),
    "skinny_timeline.py": ([], {"ROWS": "32"}),
    "steps20_timeline.py": ([], {"K": "3", "REP": "1"}),
    "time_evaluate_net.py": ([], {"N": "2", "ITERS": "4"}),
    "time_frontend.py": ([], {}),
    "time_group.py": ([], {"G": "1", "NT": "1"}),
    "time_latency.py": ([], {"ROWS": "2", "REPS": "1", "S": "20"}),
    "time_trunk.py": ([], {"B": "32"}),
    "time_step_phases.py": (["1"], {}),
    "time_vocoder.py": ([], {"N": "32", "ITERS": "4"}),
    "train_stages.py": ([], {}),
    "early_stop/time_early_stop.py": ([], ONCE),
    "face_align/time_face_align.py": ([], dict(ONCE, SHAPES="2x3x40")),
    "face_tower/time_face_tower.py": ([], {"SIZES": "1", "REPS": "1"}),
    "frame_resize/time_frame_resize.py": ([], dict(ONCE, SHAPES="2x3x40", ALT_LIB=HIP_LIB)),
    "gemm_x3_shape/pmc_postnet.py": ([], {"CLIPS": "2"}),
    "gemm_x3_shape/time_gemm_x3_shape.py": ([], dict(ONCE, CLIPS="2", PARENT_DIAG_LIB=DIAG_LIB)),
    "lstm_shared_panel/skinny_form_trace.py": ([], {}),
    "masked_lengths/time_masked_lengths.py": ([], dict(ONCE, B="2", S="4", PARENT_LIB=HIP_LIB)),
    "mel_targets/time_mel_targets.py": ([], dict(ONCE, SHAPES="2x2048", ALT_LIB=HIP_LIB)),
    # one T at or below 32 frames and one above: the short and the long persistent kernel families both launch
    "persist_long/time_persist_long.py": ([], dict(ONCE, BS="1", TS="9,40", S="4", PARENT_LIB=HIP_LIB)),
    "persist_masked/time_persist_masked.py": ([], dict(ONCE, LENS="9-20,33-40", S="4", PARENT_LIB=HIP_LIB)),
    # two batches of two clips, 7 frames being the shortest legal clip
    "ragged/time_forward_ragged.py": ([], dict(ONCE, G="2", CLIPS="2", LENS="7-9", PARENT_LIB=HIP_LIB)),
    "ragged/time_ragged.py": ([], dict(ONCE, G="2", CLIPS="2", LENS="7-9", S="4", PARENT_LIB=HIP_LIB)),
    "speaker_packed/time_speaker_packed.py": ([], dict(ONCE, SHAPES="2x3200-4800", PARENT_LIB=HIP_LIB)),
}
SYNTAX_ONLY = ["pmc_decode_json.py", "pmc_read.py", "rocprof_concurrency.py", "rocprof_summary.py", "face_tower/per_call.py"]
MODULES = ["abtime.py"]          # imported by the scripts; tests/test_abtime_host.py
COVERED_BY = {      # run, with assertions on what they print, by a test next to the feature's own
    "vocoder_long/time_vocoder_long.py": "tests/test_vocoder_long_gpu.py::test_time_vocoder_long_tool_runs",
    "vocoder_ragged/time_vocoder_ragged.py": "tests/test_vocoder_ragged_gpu.py::test_time_vocoder_ragged_tool_runs",
}
SUBDIR_SHELL = ["face_tower/profile_face_tower.sh", "lstm_shared_panel/measure.sh"]          # the top-level shell drivers are listed in the inventory test


def _tree(*suffixes):
    return sorted(os.path.relpath(f, TOOLS) for s in suffixes for f in glob.glob(os.path.join(TOOLS, "**", "*" + s), recursive=True))


def test_tools_inventory_is_what_the_readme_lists():
    have = _tree(".py", ".sh")
    want = sorted(list(RUNS) + SYNTAX_ONLY + ["ab_bench.sh", "attn_l2_sweep.sh", "gpurun_retry.sh", "pmc_dense_kernels.sh", "pmc_step_kernels.sh", "profile_r5.sh", "profile_r5_chains.sh", "profile_r6.sh"])
    want = sorted(want + MODULES + list(COVERED_BY) + SUBDIR_SHELL)
    assert have == want, (set(have) ^ set(want))
    for f, test in COVERED_BY.items():
        path, name = test.split("::")
        source = open(os.path.join(ROOT, path)).read()
        assert f"def {name}(" in source and os.path.basename(f) in source, f"{test} does not run tools/{f}"
    readme = open(os.path.join(TOOLS, "README.md")).read()
    for f in have + ["membw/membw.hip", "persist/persist_probe.hip"]:
        assert f in readme, f"tools/README.md does not mention {f}"
    for f in have:
        if f.endswith(".sh"):
            subprocess.run(["bash", "-n", os.path.join(TOOLS, f)], check=True)
        else:
            source = open(os.path.join(TOOLS, f)).read()
            compile(source, f, "exec")
            assert "profiles/" in source, f"{f}: name the profiles/ file it produces in its docstring"
            if os.sep in f:      # the per-feature scripts time through tools/abtime.py, not through a copy of it
                assert not any(d in source for d in ("def timed(", "def rounds(", "def report(")), f"tools/{f}: use tools/abtime.py"


@pytest.mark.gpu
@pytest.mark.parametrize("script", sorted(RUNS))
def test_tool_runs_one_iteration(script):
    argv, env = RUNS[script]
    r = subprocess.run([sys.executable, os.path.join(TOOLS, script)] + argv, cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.strip(), "no output"
