"""The one timing harness of the tools/<feature>/time_*.py scripts (imported as `tools.abtime` with the repository root on sys.path; produces no file
under profiles/ itself): interleaved rounds of warm calls, per variant the median of the rounds and the spread, the two verdicts DESIGN.md words its
claims with, the synthetic-weights model and the "another build of the library in this process" environment variables.  tests/test_abtime_host.py
checks the logic without a device."""
import os
import statistics
import time


def timed(fn, reps, clock="events", warm=0):
    """ms per call of `reps` back-to-back calls after `warm` untimed ones.  clock "events": one HIP event pair around the calls, then a synchronise;
    "host": synchronise, perf_counter, the calls, synchronise (for routes with host work inside)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("tools.abtime.timed: no GPU is visible, and a time taken without one would measure nothing")
    if clock not in ("events", "host"):
        raise ValueError(f"clock = {clock!r}: 'events' or 'host'")
    for _ in range(warm):
        fn()
    if warm or clock == "host":
        torch.cuda.synchronize()
    if clock == "host":
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _synchronize():
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def rounds(variants, n_rounds, reps, clock="events", warm=1, timer=timed):
    """variants: [(name, fn)].  `warm` untimed calls of every variant (the last outputs are returned: tools compare them bit for bit), then `n_rounds`
    rounds in which every variant is timed once over `reps` calls (an int, or one per variant), round r starting at variant r % n.
    -> (per variant the list of per-round ms, the warm-up outputs)"""
    n = len(variants)
    reps = [reps] * n if isinstance(reps, int) else list(reps)
    outs = [None] * n
    for _ in range(warm):
        outs = [fn() for _, fn in variants]
    _synchronize()
    times = [[] for _ in variants]
    for r in range(n_rounds):
        for i in list(range(n))[r % n:] + list(range(n))[:r % n]:
            times[i].append(timer(variants[i][1], reps[i], clock))
    return times, outs


def report(variants, times, unit="ms", ratio=None, base=0, extra=lambda name, ms: ""):
    """One line per variant: name, median, spread = max - min, min, max, in `unit` ("ms" or "us"; `times` are ms); with `ratio` (a label such as
    "the first") the median over variant `base`'s; `extra(name, median ms)` may append a column.  -> the medians (ms)"""
    scale, digits = {"ms": (1.0, 3), "us": (1e3, 1)}[unit]
    med = [statistics.median(x) for x in times]
    width = max(len(name) for name, _ in variants)
    for (name, _), x, m in zip(variants, times, med):
        lo, hi = min(x) * scale, max(x) * scale
        print(f"{name:<{width}} {m * scale:10.{digits}f} {unit}  (spread {hi - lo:9.{digits}f}, min {lo:10.{digits}f}, max {hi:10.{digits}f})"
              + (f"   x{m / med[base]:7.4f} of {ratio}" if ratio else "") + extra(name, m))
    return med


def wholly_under(a, b):
    """every round of a below every round of b: the only case a tool calls "faster beyond the spread" """
    return max(a) < min(b)


def median_inside(a, b):
    """the median of one lies inside the other's spread (either way round): "has not moved" """
    ma, mb = statistics.median(a), statistics.median(b)
    return min(b) <= ma <= max(b) or min(a) <= mb <= max(a)


def not_above(a, b):
    """the median of a lies inside the span of b's rounds, or below it: "no slower than" """
    return statistics.median(a) <= max(b)


def synth_model(library=None, state_dict=None, **options):
    """A NativeModel of `library` (default: the package's own) with the options set, loaded with `state_dict` (default: synth.synth_state_dict())."""
    from lip2speech_amd import native, synth
    sd = synth.synth_state_dict() if state_dict is None else state_dict
    nm = native.NativeModel(library)
    for k, v in options.items():
        nm.set_option(k, v)
    nm.load({k: v.cuda() for k, v in sd.items()}, list(sd.keys()))
    return nm


def libs_from_env(name, load=None):
    """Other builds of the library named by environment variable `name`: "path" or "label=path,label=path".  -> [(label, path)], the label of a bare
    path being its file name; with `load` (native._load) the second member is the loaded library."""
    libs = []
    for item in os.environ.get(name, "").split(","):
        if item:
            label, _, path = item.rpartition("=")
            libs.append((label or os.path.basename(path), load(path) if load else path))
    return libs
