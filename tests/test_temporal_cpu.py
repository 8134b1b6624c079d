"""Temporal functions without a GPU: the two Python models of
temporal_model.py against the reference's own tables
(golden/temporal_vectors.json) and against each other on the seeded series of
temporal_cases.py, what those series contain, and the argument rules of
m3gpu_temporal_batch_dev / m3gpu_temporal_batch, which return before any HIP
call."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import temporal_cases as cases  # noqa: E402
import temporal_model as model  # noqa: E402
from m3_amd import engine  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
M3GPU_ERR_BADARG = -2
SEC = cases.SEC
START = cases.START

with open(os.path.join(HERE, "golden", "temporal_vectors.json")) as f:
    GOLDEN = json.load(f)


def golden_inputs(table):
    """(grid, param, per series (ts, vals)) of one fixture table."""
    step = GOLDEN["step_seconds"] * SEC
    grid = (START, step, GOLDEN["nsteps"], GOLDEN["range_seconds"] * SEC)
    series = []
    for row in table["vals"]:
        ts = [START + i * step + GOLDEN["point_offset_ns"]
              for i in range(len(row))]
        series.append((ts, [math.nan if v is None else float(v)
                            for v in row]))
    return grid, GOLDEN["predict_linear_seconds"], series


def assert_close_to_table(cells, expected, what):
    for k, ((b, _), want) in enumerate(zip(cells, expected)):
        got = model.from_bits(b)
        if want is None:
            assert math.isnan(got), (what, k, got)
        else:
            # compare.EqualsWithNansWithDelta: delta > |expected - actual|
            assert GOLDEN["compare_delta"] > abs(want - got), (what, k, got,
                                                               want)


def test_fixture_has_every_table_and_function():
    assert len(GOLDEN["tables"]) == 45
    assert {t["table"] for t in GOLDEN["tables"]} == {
        "aggregationTestCases", "rateTestCases", "deltaTestCases",
        "increaseTestCases", "temporalFunctionTestCases",
        "linearRegressionTestCases"}
    assert {t["fn"] for t in GOLDEN["tables"]} == set(model.FNS)
    assert engine.TEMPORAL_FNS == model.FN_ID


@pytest.mark.parametrize("table", GOLDEN["tables"], ids=lambda t: t["name"])
def test_models_reproduce_the_reference_tables(table):
    grid, param, series = golden_inputs(table)
    for i, (ts, vals) in enumerate(series):
        proc = model.procedural(table["fn"], ts, vals, *grid, param=param)
        closed, err = model.closed_form(table["fn"], ts, vals, *grid,
                                        param=param)
        assert err == 0
        assert_close_to_table(proc, table["expected"][i], ("procedural", i))
        assert_close_to_table(closed, table["expected"][i], ("closed", i))


def test_hand_checked_cells():
    by_name = {t["name"]: t for t in GOLDEN["tables"]}
    grid, _, series = golden_inputs(by_name["irate"])
    cells, _ = model.closed_form("irate", *series[0], *grid)
    # (683214 - 680986) / 60 s
    assert model.from_bits(cells[2][0]) == (683214.0 - 680986.0) / 60.0
    grid, _, series = golden_inputs(by_name["rate"])
    cells, _ = model.closed_form("rate", *series[1], *grid)
    # 3904 * (120 + 30 + 1e-6) / 120 / 300
    assert abs(model.from_bits(cells[2][0]) -
               3904 * (120 + 30 + 1e-6) / 120 / 300) < 1e-9


def same_cells(a, b):
    """Bit for bit where a value, NaN for NaN, literal flag for flag."""
    if len(a) != len(b):
        return False
    for (ba, la), (bb, lb) in zip(a, b):
        if la != lb:
            return False
        na, nb = math.isnan(model.from_bits(ba)), math.isnan(
            model.from_bits(bb))
        if na != nb or (not na and ba != bb):
            return False
    return True


@pytest.mark.parametrize("step,range_ns", cases.grid_cases())
@pytest.mark.parametrize("nsteps", [1, 9, 33])
def test_closed_form_equals_the_procedure(step, range_ns, nsteps):
    batch = cases.make_batch(11 + nsteps, 2 * len(cases.KINDS), START, step,
                             nsteps, range_ns)
    for i, (ts, vals) in enumerate(batch):
        assert all(a < b for a, b in zip(ts, ts[1:])), i
        many, err = model.closed_form_many(model.FNS, ts, vals, START, step,
                                           nsteps, range_ns, param=37.5)
        assert err == 0
        for fn in model.FNS:
            want = model.procedural(fn, ts, vals, START, step, nsteps,
                                    range_ns, param=37.5)
            assert same_cells(many[fn], want), \
                (fn, i, cases.KINDS[i % len(cases.KINDS)])


def test_batch_is_not_vacuous():
    """For every function at least half of the dense series' cells hold a
    number, and every NaN-returning branch of the processors is taken."""
    step, range_ns = cases.grid_cases()[0]
    nsteps = 33
    batch = cases.make_batch(5, 3 * len(cases.KINDS), START, step, nsteps,
                             range_ns)
    model.HITS.clear()
    for fn in model.FNS:
        numbers = cells = 0
        for i, (ts, vals) in enumerate(batch):
            got = model.procedural(fn, ts, vals, START, step, nsteps,
                                   range_ns, param=37.5)
            if cases.KINDS[i % len(cases.KINDS)] == "dense":
                # the dense spacing: range is four sample intervals
                gaps = np.diff(ts)
                assert range_ns >= 3 * int(np.median(gaps))
                cells += len(got)
                numbers += sum(not math.isnan(model.from_bits(b))
                               for b, _ in got)
        assert cells >= 3 * nsteps and 2 * numbers >= cells, (fn, numbers,
                                                              cells)
    assert model.HITS == model.NAN_BRANCHES, model.NAN_BRANCHES - model.HITS


def test_batch_has_the_cases_integers_cannot_show():
    step, range_ns = cases.grid_cases()[2]
    nsteps = 9
    batch = cases.make_batch(3, len(cases.KINDS), START, step, nsteps,
                             range_ns)
    kind = dict(zip(cases.KINDS, batch))
    # non-integer doubles over a wide exponent range
    vals = [v for v in kind["dense"][1] if not math.isnan(v)]
    exps = [math.frexp(v)[1] for v in vals]
    assert max(exps) - min(exps) > 60
    # (every double from 2^52 up is a whole number)
    assert sum(v != int(v) for v in vals) > len(vals) // 3
    # a monotone counter with resets
    vals = [v for v in kind["counter"][1] if not math.isnan(v)]
    drops = sum(b < a for a, b in zip(vals, vals[1:]))
    assert 0 < drops < len(vals) // 3
    # +0 then -0, and -0 then +0, next to each other
    signs = [math.copysign(1.0, v) for v in kind["zeros"][1]]
    zeros = [v == 0 for v in kind["zeros"][1]]
    pairs = {(a, b) for a, b, za, zb in zip(signs, signs[1:], zeros,
                                            zeros[1:]) if za and zb}
    assert {(1.0, -1.0), (-1.0, 1.0)} <= pairs
    assert math.inf in kind["inf"][1] and -math.inf in kind["inf"][1]
    # points on t_k, on t_k - range and 1 ns either side of both
    ts, vals = kind["boundary"]
    for k in (0, nsteps - 1):
        tk = START + k * step
        for base in (tk, tk - range_ns):
            assert {base - 1, base, base + 1} <= set(ts)
    # both ends are inclusive: the edge points count, their outer
    # neighbours do not
    at = dict(zip(ts, vals))
    inside = [t for t in ts if START - range_ns <= t <= START]
    cells, _ = model.closed_form("count_over_time", ts, vals, START, step,
                                 nsteps, range_ns)
    assert START - range_ns in inside and START in inside
    assert START - range_ns - 1 in at and START + 1 in at
    assert model.from_bits(cells[0][0]) == len(inside)
    cells, _ = model.closed_form("last_over_time", ts, vals, START, step,
                                 nsteps, range_ns)
    assert cells[0][0] == model.bits(at[START])
    cells, _ = model.closed_form("min_over_time", [START - range_ns - 1],
                                 [1.0], START, step, nsteps, range_ns)
    assert cells[0] == (model.NAN_BITS, True)
    cells, _ = model.closed_form("min_over_time", [START - range_ns], [1.0],
                                 START, step, nsteps, range_ns)
    assert cells[0] == (model.bits(1.0), False)
    # NaN runs on a window's first and last point
    ts, vals = kind["boundary_nan"]
    at = dict(zip(ts, vals))
    assert math.isnan(at[START]) and math.isnan(at[START - range_ns])
    ts, vals = kind["nan_runs"]
    wins, _ = model.windows(ts, vals, START, step, nsteps, range_ns)
    assert any(len(w) > 2 and math.isnan(w[0][1]) for w in wins)
    assert any(len(w) > 2 and math.isnan(w[-1][1]) for w in wins)
    # window sizes around the ring depth, 3C included (range < step here)
    for ring in (8, 16):
        ts, vals = cases.make_series(np.random.default_rng(1), START, step,
                                     33, range_ns, "windows", ring)
        wins, _ = model.windows(ts, vals, START, step, 33, range_ns)
        assert set(cases.window_sizes(ring)) <= {len(w) for w in wins}


def test_signed_zero_and_payload_rules():
    grid = (START, 10 * SEC, 1, 10 * SEC)
    ts = [START - 2, START - 1]
    mn = model.closed_form("min_over_time", ts, [0.0, -0.0], *grid)[0][0][0]
    assert mn == model.bits(-0.0)
    mn = model.closed_form("min_over_time", ts, [-0.0, 0.0], *grid)[0][0][0]
    assert mn == model.bits(-0.0)
    mx = model.closed_form("max_over_time", ts, [-0.0, 0.0], *grid)[0][0][0]
    assert mx == model.bits(0.0)
    mx = model.closed_form("max_over_time", ts, [0.0, -0.0], *grid)[0][0][0]
    assert mx == model.bits(0.0)
    payload = 0x7FF80000DEADBEEF
    last = model.closed_form("last_over_time", ts,
                             [1.0, model.from_bits(payload)], *grid)[0][0]
    assert last == (payload, False)


def test_seconds_helpers_differ_in_the_last_bit():
    """Duration.Seconds() is not subSeconds: irate uses the first, rate's
    sampled interval the second."""
    d = 59 * SEC + 999999000
    assert model.duration_seconds(d) == 59.0 + 999999000 / 1e9
    assert model.sub_seconds(d, 0) == float(d) / 1e9
    assert any(model.duration_seconds(x) != model.sub_seconds(x, 0)
               for x in range(d, d + 2000, 7))


def test_closed_form_error_rules():
    start, step, nsteps, range_ns = START, 10 * SEC, 4, 25 * SEC
    t_last = start + 3 * step
    ts = [start, start + step, t_last + 1]
    vals = [1.5, 2.5, 3.5]
    nan_col = [(model.NAN_BITS, True)] * nsteps
    # a row error fails the series even behind a point past t_last
    assert model.closed_form("sum_over_time", ts, vals, start, step, nsteps,
                             range_ns, row_err=5) == (nan_col, 5)
    # equal and smaller timestamps among the points read
    for bad in ([start, start], [start + 1, start],
                [start, start - 1, t_last + 1]):
        assert model.closed_form(
            "sum_over_time", bad, [1.0] * len(bad), start, step, nsteps,
            range_ns) == (nan_col, model.OUT_OF_ORDER)
    # past the first point beyond t_last nothing is looked at
    got, err = model.closed_form("sum_over_time", ts + [start], vals + [9.0],
                                 start, step, nsteps, range_ns)
    assert err == 0 and got[1][0] == model.bits(4.0)


def test_new_symbols_exported():
    L = engine.lib()
    for sym in ("m3gpu_temporal_batch_dev", "m3gpu_temporal_batch",
                "m3gpu_temporal_ring_depth"):
        assert hasattr(L, sym), sym
    assert L.m3gpu_temporal_ring_depth() in (8, 16, 32)
    import m3_amd
    for name in ("TEMPORAL_FNS", "temporal_dev", "temporal",
                 "fetch_temporal_dev"):
        assert hasattr(m3_amd, name), name
    assert len(engine.TEMPORAL_FNS) == 17
    assert engine.TEMPORAL_FNS["rate"] == 8
    assert engine.TEMPORAL_FNS["predict_linear"] == 16


I64_MAX = 2 ** 63 - 1
I64_MIN = -2 ** 63
GOOD = dict(nseries=3, stride=4, start=START, step=SEC, nsteps=5,
            range_ns=SEC, fn=0, pitch=3)
BAD = {
    "step_zero": dict(step=0),
    "step_negative": dict(step=-SEC),
    "range_zero": dict(range_ns=0),
    "range_negative": dict(range_ns=-1),
    "nsteps_zero": dict(nsteps=0),
    "stride_zero": dict(stride=0),
    "pitch_below_nseries": dict(pitch=2),
    "fn_negative": dict(fn=-1),
    "fn_past_the_enum": dict(fn=17),
    "grid_overflows": dict(start=I64_MAX - 3 * SEC),
    "grid_span_overflows": dict(start=0, step=I64_MAX // 2, nsteps=4),
    "range_underflows": dict(start=I64_MIN + 5, range_ns=6),
}
FORMS = ["dev", "host"]


def _call(form, a):
    """Every data pointer null and nseries > 0: an entry that got as far as
    a copy or a launch would fault or return a HIP error instead."""
    L = engine.lib()
    args = [None, None, None, None, a["nseries"], a["stride"], a["start"],
            a["step"], a["nsteps"], a["range_ns"], a["fn"], 0.0, None,
            a["pitch"], None]
    if form == "dev":
        return L.m3gpu_temporal_batch_dev(*args, None)
    return L.m3gpu_temporal_batch(*args)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bad", list(BAD))
def test_badarg_before_any_hip_call(bad, form):
    rc = _call(form, dict(GOOD, **BAD[bad]))
    assert rc == M3GPU_ERR_BADARG
    assert engine.lib().m3gpu_last_error().decode()


@pytest.mark.parametrize("form", FORMS)
def test_good_arguments_with_no_series_are_ok(form):
    assert _call(form, dict(GOOD, nseries=0, pitch=0)) == 0
    for fn in range(17):
        assert _call(form, dict(GOOD, nseries=0, pitch=0, fn=fn)) == 0
    # the largest grid that still fits
    assert _call(form, dict(GOOD, nseries=0, pitch=0, start=I64_MAX - 4 * SEC,
                            range_ns=I64_MAX)) == 0


def test_unknown_function_name_is_an_error():
    with pytest.raises(engine.M3GpuError):
        engine._temporal_fn("quantile_over_time")


def test_step_iter_walks_a_temporal_matrix():
    from m3_amd.iterators import StepIter
    nan = model.GO_NAN
    steps = np.array([[nan, 1.5], [2.0, nan], [0.25, 4.0]])
    it = StepIter(steps, np.zeros(2, np.int32), start_ns=START,
                  step_ns=60 * SEC)
    seen = []
    while it.Next():
        t, col = it.Current()
        seen.append((t, col.view(np.uint64).tolist()))
    assert [t for t, _ in seen] == [START + k * 60 * SEC for k in range(3)]
    assert seen[0][1][0] == model.NAN_BITS
    assert it.Err() is None
    bad = StepIter(steps, np.array([0, 100], np.int32), start_ns=0, step_ns=1)
    assert not bad.Next() and "out_of_order" in str(bad.Err())
