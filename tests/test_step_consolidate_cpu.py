"""Step consolidation without a GPU: the two Python models of
step_consolidate_model.py against the reference's own tables
(golden/step_consolidator_vectors.json) and against each other on the seeded
series of step_consolidate_cases.py, and the argument rules of the four
m3gpu_step_* / m3gpu_decode_steps_* entries, which return before any HIP
call."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_consolidate_cases as cases  # noqa: E402
import step_consolidate_model as model  # noqa: E402
from m3_amd import engine  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
M3GPU_ERR_BADARG = -2
SEC = cases.SEC

with open(os.path.join(HERE, "golden", "step_consolidator_vectors.json")) as f:
    GOLDEN = json.load(f)


def golden_series():
    """Per series the stitched (ts, vals) of the fixture's blocks."""
    start = GOLDEN["start_seconds"] * SEC
    block = GOLDEN["block_seconds"] * SEC
    out = []
    for blocks in GOLDEN["series"]:
        ts, vals = [], []
        for b, pts in enumerate(blocks):
            for v, off in pts:
                ts.append(start + b * block + off * SEC)
                vals.append(float(v))
        out.append((ts, vals))
    return out


def golden_grid(table):
    start = GOLDEN["start_seconds"] * SEC
    span = GOLDEN["block_seconds"] * max(len(s) for s in GOLDEN["series"])
    step = table["step_seconds"]
    assert span % step == 0 and span // step == len(table["expected"])
    return start, step * SEC, span // step, GOLDEN["lookback_seconds"] * SEC


def table_bits(table, i):
    return [model.NAN_BITS if row[i] is None else model.bits(float(row[i]))
            for row in table["expected"]]


@pytest.mark.parametrize("table", GOLDEN["tables"], ids=lambda t: t["name"])
def test_models_reproduce_the_reference_tables(table):
    start, step, nsteps, lookback = golden_grid(table)
    for i, (ts, vals) in enumerate(golden_series()):
        want = table_bits(table, i)
        assert model.procedural_steps(ts, vals, start, step, nsteps,
                                      lookback) == want, i
        assert model.closed_form(ts, vals, start, step, nsteps,
                                 lookback) == (want, 0), i


def test_procedural_model_reproduces_test_consolidator():
    start = GOLDEN["start_seconds"] * SEC
    c = model.StepLookbackConsolidator(60 * SEC, 60 * SEC, start)
    takes = 0
    for op in GOLDEN["consolidator_sequence"]:
        if op["op"] == "buffer_step":
            c.buffer_step()
        elif op["op"] == "add_point":
            c.add_point(start + op["offset_seconds"] * SEC, float(op["value"]))
        else:
            got = c.consolidate_and_move_to_next()
            takes += 1
            if op["expected"] is None:
                assert math.isnan(got), takes
            else:
                assert got == op["expected"], takes
    assert takes == 5


@pytest.mark.parametrize("step,lookback", cases.grid_cases())
@pytest.mark.parametrize("nsteps", [1, 7, 33])
def test_closed_form_equals_the_procedure(step, lookback, nsteps):
    batch = cases.make_batch(7 + nsteps, 70, cases.START, step, nsteps,
                             lookback)
    seen_values = 0
    for i, (ts, vals) in enumerate(batch):
        assert all(a < b for a, b in zip(ts, ts[1:])), i
        want = model.procedural_steps(ts, vals, cases.START, step, nsteps,
                                      lookback)
        got, err = model.closed_form(ts, vals, cases.START, step, nsteps,
                                     lookback)
        assert err == 0 and got == want, (i, cases.KINDS[i % 7])
        seen_values += sum(b != model.NAN_BITS for b in got)
    assert seen_values > nsteps


def test_batch_has_the_cases_the_window_rule_can_get_wrong():
    step, lookback, nsteps = 60 * SEC, 25 * SEC, 9
    start = cases.START
    t_last = start + (nsteps - 1) * step
    batch = cases.make_batch(3, 70, start, step, nsteps, lookback)
    kinds = {k: [b for i, b in enumerate(batch) if cases.KINDS[i % 7] == k]
             for k in cases.KINDS}
    assert all(ts == [] for ts, _ in kinds["empty"])
    ts, vals = kinds["boundary"][0]
    for k in (0, nsteps - 1):
        tk = start + k * step
        for base in (tk, tk - lookback):
            assert {base - 1, base, base + 1} <= set(ts)
    assert min(ts) < start - lookback and sum(t > t_last for t in ts) >= 2
    # the point on the window's lower edge counts, the one 1 ns before not
    got, _ = model.closed_form(ts, vals, start, step, nsteps, lookback)
    at = dict(zip(ts, vals))
    assert got[0] == model.bits(at[start])
    only_edge = [(t, v) for t, v in zip(ts, vals) if t <= start - lookback]
    got, _ = model.closed_form(*zip(*only_edge), start, step, nsteps, lookback)
    assert got[0] == model.bits(at[start - lookback])
    only_before = [(t, v) for t, v in zip(ts, vals) if t < start - lookback]
    got, _ = model.closed_form(*zip(*only_before), start, step, nsteps,
                               lookback)
    assert got[0] == model.NAN_BITS
    # NaN as the newest point of a window: the value before it shows
    ts, vals = kinds["boundary_nan"][0]
    at = dict(zip(ts, vals))
    assert math.isnan(at[start]) and not math.isnan(at[start - 1])
    got, _ = model.closed_form(ts, vals, start, step, nsteps, lookback)
    assert got[0] == model.bits(at[start - 1])
    assert all(all(t > t_last for t in ts) for ts, _ in kinds["after"])
    assert all(all(t < start for t in ts) for ts, _ in kinds["before"])
    assert any(any(math.isnan(v) for v in vals) for _, vals in kinds["dense"])


def test_closed_form_error_rules():
    start, step, nsteps, lookback = cases.START, 10 * SEC, 4, 10 * SEC
    t_last = start + 3 * step
    ts = [start, start + step, t_last + 1]
    vals = [1.0, 2.0, 3.0]
    nan_col = [model.NAN_BITS] * nsteps
    # a row error behind a point past t_last is never reached
    got, err = model.closed_form(ts, vals, start, step, nsteps, lookback, 5)
    assert err == 0 and got[:2] == [model.bits(1.0), model.bits(2.0)]
    # without that point it is, and the column is all NaN
    assert model.closed_form(ts[:2], vals[:2], start, step, nsteps, lookback,
                             5) == (nan_col, 5)
    # equal and smaller timestamps among the points read
    assert model.closed_form([start, start], [1.0, 2.0], start, step, nsteps,
                             lookback) == (nan_col, model.OUT_OF_ORDER)
    got, err = model.closed_form([start, start], [1.0, 2.0], start, step,
                                 nsteps, lookback, dedupe=True)
    assert err == 0 and got[0] == model.bits(1.0)
    assert model.closed_form([start + 1, start], [1.0, 2.0], start, step,
                             nsteps, lookback,
                             dedupe=True) == (nan_col, model.OUT_OF_ORDER)
    # past the peeked point nothing is looked at
    got, err = model.closed_form(ts + [start], vals + [9.0], start, step,
                                 nsteps, lookback)
    assert err == 0


def test_new_symbols_exported():
    L = engine.lib()
    for sym in ("m3gpu_step_consolidate_batch_dev",
                "m3gpu_decode_steps_batch_dev",
                "m3gpu_step_consolidate_batch", "m3gpu_decode_steps_batch"):
        assert hasattr(L, sym), sym


I64_MAX = 2 ** 63 - 1
I64_MIN = -2 ** 63
GOOD = dict(nseries=3, rows=4, start=cases.START, step=SEC, nsteps=5,
            lookback=SEC, pitch=3)
BAD = {
    "step_zero": dict(step=0),
    "step_negative": dict(step=-SEC),
    "lookback_negative": dict(lookback=-1),
    "nsteps_zero": dict(nsteps=0),
    "rows_zero": dict(rows=0),  # stride, or nblocks
    "pitch_below_nseries": dict(pitch=2),
    "grid_overflows": dict(start=I64_MAX - 3 * SEC),
    "grid_span_overflows": dict(start=0, step=I64_MAX // 2, nsteps=4),
    "lookback_underflows": dict(start=I64_MIN + 5, lookback=6),
}


def _call(form, a):
    """Every data pointer null and nseries > 0: an entry that got as far as
    a copy or a launch would fault or return a HIP error instead."""
    L = engine.lib()
    grid = [a["start"], a["step"], a["nsteps"], a["lookback"]]
    out = [None, a["pitch"], None]
    if form == "rows_dev":
        return L.m3gpu_step_consolidate_batch_dev(
            None, None, None, None, a["nseries"], a["rows"], *grid, *out, None)
    if form == "rows_host":
        return L.m3gpu_step_consolidate_batch(
            None, None, None, None, a["nseries"], a["rows"], *grid, *out)
    if form == "streams_dev":
        return L.m3gpu_decode_steps_batch_dev(
            None, None, None, a["nseries"], a["rows"], 1, 1, *grid, *out, None)
    return L.m3gpu_decode_steps_batch(
        None, 0, None, None, a["nseries"], a["rows"], 1, 1, *grid, *out)


FORMS = ["rows_dev", "rows_host", "streams_dev", "streams_host"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bad", list(BAD))
def test_badarg_before_any_hip_call(bad, form):
    rc = _call(form, dict(GOOD, **BAD[bad]))
    assert rc == M3GPU_ERR_BADARG
    assert engine.lib().m3gpu_last_error().decode()


@pytest.mark.parametrize("form", FORMS)
def test_good_arguments_with_no_series_are_ok(form):
    assert _call(form, dict(GOOD, nseries=0, pitch=0)) == 0
    # the largest grid that still fits
    assert _call(form, dict(GOOD, nseries=0, pitch=0, start=I64_MAX - 4 * SEC,
                            lookback=I64_MAX)) == 0


def test_step_iter_wrapper():
    from m3_amd.iterators import StepIter
    steps = np.array([[1.0, np.nan], [2.0, 3.0], [np.nan, 4.0]])
    it = StepIter(steps, np.zeros(2, np.int32), start_ns=100, step_ns=10)
    assert it.StepCount() == 3
    seen = []
    while it.Next():
        t, col = it.Current()
        seen.append((t, col.view(np.uint64).tolist()))
    assert [t for t, _ in seen] == [100, 110, 120]
    assert seen[1][1] == steps[1].view(np.uint64).tolist()
    assert it.Err() is None and not it.Next()
    bad = StepIter(steps, np.array([0, 100], np.int32), start_ns=0, step_ns=1)
    assert not bad.Next() and "out_of_order" in str(bad.Err())
