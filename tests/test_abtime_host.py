"""tools/abtime.py without a device: the rotation and sample counts of `rounds` under a fake timer, the warm-up outputs, median / spread of `report` on
hand-made lists, the two verdicts on overlapping, touching and disjoint spans, the environment forms of `libs_from_env`, and `timed` refusing to run
without a GPU."""
import pytest
import torch

from tools import abtime


def test_rounds_rotate_and_sample_every_variant():
    calls, order = [], []
    variants = [(name, lambda name=name: calls.append(name) or f"out-{name}") for name in "abc"]

    def fake_timer(fn, reps, clock):
        order.append((fn(), reps, clock))
        return float(len(order))

    times, outs = abtime.rounds(variants, 4, (5, 6, 7), clock="host", timer=fake_timer)
    assert outs == ["out-a", "out-b", "out-c"]                      # one warm-up call each, outputs returned in variant order
    assert calls[:3] == ["a", "b", "c"]
    assert [o[0][-1] for o in order] == list("abc" "bca" "cab" "abc")          # round r starts at variant r % 3
    assert all(o[1:] == ({"a": 5, "b": 6, "c": 7}[o[0][-1]], "host") for o in order)
    assert [len(t) for t in times] == [4, 4, 4]
    assert times == [[1.0, 6.0, 8.0, 10.0], [2.0, 4.0, 9.0, 11.0], [3.0, 5.0, 7.0, 12.0]]


def test_rounds_warm_count_and_scalar_reps():
    calls = []
    variants = [("x", lambda: calls.append("x") or len(calls))]
    times, outs = abtime.rounds(variants, 2, 3, warm=2, timer=lambda fn, reps, clock: reps * 1.0)
    assert calls == ["x", "x"] and outs == [2] and times == [[3.0, 3.0]]
    times, outs = abtime.rounds(variants, 1, 1, warm=0, timer=lambda fn, reps, clock: 0.5)
    assert outs == [None] and times == [[0.5]]


def test_report_median_spread_ratio(capsys):
    variants = [("first", None), ("second one", None)]
    med = abtime.report(variants, [[3.0, 1.0, 2.0], [4.0, 8.0]], ratio="the first", extra=lambda name, m: f"   <{name}:{m}>")
    assert med == [2.0, 6.0]
    a, b = capsys.readouterr().out.splitlines()
    assert a.split() == "first 2.000 ms (spread 2.000, min 1.000, max 3.000) x 1.0000 of the first <first:2.0>".split()
    assert b.split() == "second one 6.000 ms (spread 4.000, min 4.000, max 8.000) x 3.0000 of the first <second one:6.0>".split()
    assert a.index(" ms") == b.index(" ms")
    med = abtime.report(variants, [[0.5], [0.25]], unit="us", ratio="(b)", base=1)
    assert med == [0.5, 0.25]
    a, b = capsys.readouterr().out.splitlines()
    assert a.split() == "first 500.0 us (spread 0.0, min 500.0, max 500.0) x 2.0000 of (b)".split()
    assert abtime.report(variants[:1], [[1.0]]) == [1.0]
    assert " of " not in capsys.readouterr().out          # no ratio column unless asked for


def test_verdicts():
    low, mid, high = [1.0, 2.0, 3.0], [2.5, 4.0, 5.0], [3.5, 6.0, 7.0]
    assert abtime.wholly_under(low, high) and not abtime.wholly_under(high, low)           # disjoint
    assert not abtime.wholly_under(low, mid) and not abtime.wholly_under(mid, low)          # overlapping
    assert not abtime.wholly_under(low, [3.0, 4.0])                                         # touching: max == min is not under
    assert abtime.median_inside(mid, high) and abtime.median_inside(high, mid)              # 4.0 inside [3.5, 7.0]
    assert not abtime.median_inside(low, high) and not abtime.median_inside(high, low)      # disjoint
    assert abtime.median_inside([1.0, 2.0, 2.0], [2.0, 3.0, 3.0])                           # touching: a's median on b's edge
    assert abtime.median_inside([1.0, 1.0, 9.0], [4.0, 5.0, 6.0])                           # either way round: b's median inside a's spread
    assert not abtime.median_inside([1.0, 1.0, 3.5], [3.0, 4.0, 4.0])                       # spans overlap, neither median inside
    assert abtime.not_above(mid, high) and abtime.not_above(low, high) and not abtime.not_above(high, low)      # inside, below, above


def test_libs_from_env(monkeypatch):
    monkeypatch.delenv("SOME_LIB", raising=False)
    assert abtime.libs_from_env("SOME_LIB") == []
    monkeypatch.setenv("SOME_LIB", "")
    assert abtime.libs_from_env("SOME_LIB") == []
    monkeypatch.setenv("SOME_LIB", "/x/y/libl2s_hip.so")
    assert abtime.libs_from_env("SOME_LIB") == [("libl2s_hip.so", "/x/y/libl2s_hip.so")]
    monkeypatch.setenv("SOME_LIB", "a=p,b=/q/r.so")
    assert abtime.libs_from_env("SOME_LIB") == [("a", "p"), ("b", "/q/r.so")]
    assert abtime.libs_from_env("SOME_LIB", load=str.upper) == [("a", "P"), ("b", "/Q/R.SO")]


def test_timed_refuses_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ran = []
    for clock in ("events", "host"):
        with pytest.raises(RuntimeError, match="no GPU"):
            abtime.timed(lambda: ran.append(1), 1, clock=clock, warm=1)
    assert not ran
