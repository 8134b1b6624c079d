"""The CPU side of the rollup value-domain tests (tests/rollup_value_cases.py,
tests/test_rollup_values_gpu.py).

1. The expected side: what Go returns for tiny cases, derived by hand from
   the reference's aggregation/quantile/cm/stream.go and heap.go, timer.go,
   gauge.go and counter.go, against the oracle.
2. The conditions that keep the GPU test honest: the special bit patterns
   survive encode->decode, every series has the depth its path needs, every
   batch holds every class, and every series under test keeps outputs that
   are compared bit for bit."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollup_value_cases as cases  # noqa: E402
import oracle  # noqa: E402
from test_rollup_plan import plan_py  # noqa: E402

QS = (0.5, 0.95, 0.99)
P0, N0 = 0, cases.NEG_ZERO
T0 = 1427162400 * 10**9


def f64(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def stream(values):
    """(min, max, [q...]) of the oracle's CKMS stream, as bit patterns."""
    v = np.array([bits(x) if isinstance(x, float) else x for x in values],
                 np.uint64).view(np.float64)
    q, mn, mx = oracle.ckms_quantiles(v, QS)
    return bits(mn), bits(mx), [bits(x) for x in q]


# ---------------- 1. hand-derived pins: the CKMS stream ----------------
#
# Common to all: AddBatch (stream.go:85-94) makes the first value the first
# sample and the insert cursor; every later value v goes to bufLess if
# v < cursor.value, else to bufMore (:102-106) - a NaN, and a zero of either
# sign against a zero cursor, go to bufMore. Flush (:129-135) runs insert()
# until both heaps are empty. insert() sorts bufMore descending (:294,
# heap.go:92-121) and consumes it from the END (:298); a value is inserted
# before the cursor while vals[idx] <= cursor.value (:305-313), and after
# the last sample it is pushed back while vals[idx] >= Back().value
# (:324-332); what fails that is dropped with the rest (:337). With at most
# 3 values, Quantile(q) is the sample at int(q*n), clamped (:221-227).

def test_stream_pos_zero_then_neg_zero():
    # sample [+0]; -0 < +0 is false -> bufMore [-0]; -0 <= +0 -> inserted
    # BEFORE the cursor (:313): samples [-0, +0]. n = 2: int(0.5*2) = 1.
    assert stream([P0, N0]) == (N0, P0, [P0, P0, P0])


def test_stream_neg_zero_then_pos_zero():
    # the mirror image: samples [+0, -0]
    assert stream([N0, P0]) == (P0, N0, [N0, N0, N0])


def test_stream_zeros_then_one():
    # [+0, -0a, +0, -0b, 1]: sample [+0]; Push (heap.go:36-54) breaks on
    # parent <= child, so bufMore stays in arrival order [-0a, +0, -0b, 1].
    # SortDesc: n=3 swap -> [1,+0,-0b,-0a], sift: left +0 < 1, right -0b <
    # +0 false -> [+0,1,-0b,-0a]; n=2 swap -> [-0b,1,+0,-0a], no sift; n=1
    # swap -> [1,-0b,+0,-0a]. Consumed from the end: -0a, +0, -0b (each <=
    # the cursor +0, inserted before it in that order), then 1 >= Back().
    # Samples [-0a, +0, -0b, +0, 1], all numRanks 1, delta 0; eps 1e-3 never
    # compresses 5 samples. calcQuantiles (:248-276): ranks ceil(2.5) = 3,
    # 5, 5, thresholds 0; maxRank first exceeds 3 at the 4th sample, so p50
    # is prev = -0b; p95 and p99 are the last sample by the post-loop.
    one = bits(1.0)
    assert stream([P0, N0, P0, N0, 1.0]) == (N0, one, [N0, one, one])


@pytest.mark.parametrize("payload", [cases.NAN_GO, cases.NAN_NEG,
                                     cases.NAN_SIG])
def test_stream_nan_first_blocks_every_insert(payload):
    # sample [NaN]; 1 and 2 are not < NaN -> bufMore. insert(): 1 <= NaN
    # false (:305), cursor runs off the end, 1 >= NaN false (:325): both
    # dropped. One sample: min, max and every quantile are that NaN, with
    # its payload (a copy, never arithmetic).
    assert stream([payload, 1.0, 2.0]) == (payload, payload, [payload] * 3)


def test_stream_nan_second():
    # [1, NaN, 2, 0.5]: sample [1]; NaN -> bufMore [NaN]; 2 -> Push: parent
    # NaN <= 2 is false, so they swap: [2, NaN]; 0.5 < 1 -> bufLess [0.5].
    # insert(): SortDesc swaps once: [NaN, 2]; from the end: 2 <= 1 false,
    # cursor off the end, 2 >= 1 pushed back, NaN >= 2 false: dropped.
    # resetInsertCursor swaps the heaps (:425-429); second insert(): 0.5 <=
    # 1 inserted before. Samples [0.5, 1, 2], n = 3: indices 1, 2, 2.
    assert stream([1.0, cases.NAN_GO, 2.0, 0.5]) == \
        (bits(0.5), bits(2.0), [bits(1.0), bits(2.0), bits(2.0)])


def test_stream_nan_takes_the_rest_of_the_heap_with_it():
    # [+0, -0a, 1.5, -0b, +0, NaN]: the NaN climbs to the root on Push
    # ([NaN,-0a,-0b,1.5,+0]) and SortDesc leaves it LAST
    # ([1.5,-0b,-0a,+0,NaN]), so it is consumed first, fails both compares,
    # and the four values before it are dropped too: the 1.5 is lost.
    assert stream([P0, N0, 1.5, N0, P0, cases.NAN_GO]) == (P0, P0, [P0] * 3)


# ---------------- 1b. hand-derived pins: timer, gauge, counter ----------------

def rollup_one(metric, values, aggs):
    """One bucket through the oracle's rollup: {agg: bit pattern}."""
    v = np.array([bits(x) if isinstance(x, float) else x for x in values],
                 np.uint64).view(np.float64)
    ts = T0 + (1 + np.arange(len(v), dtype=np.int64)) * 10**9
    out, _ = oracle.rollup_batch(ts[None, :], v[None, :],
                                 np.array([len(v)], np.uint32),
                                 cases.METRIC[metric], cases.WINDOW, 1, aggs)
    return dict(zip(aggs, (int(b) for b in out[0, 0].view(np.uint64))))


def test_timer_sums_take_every_value():
    # timer.go:60-66: count, sum and sumSq take the NaN the stream drops
    got = rollup_one("timer", [1.0, cases.NAN_GO, 2.0, 0.5],
                     ["count", "sum", "sumsq", "min", "max", "median"])
    assert got["count"] == bits(4.0)
    assert math.isnan(f64(got["sum"])) and math.isnan(f64(got["sumsq"]))
    assert (got["min"], got["max"], got["median"]) == \
        (bits(0.5), bits(2.0), bits(1.0))


def test_gauge_nan_counts_and_is_last():
    # gauge.go:73-103: last and count take the NaN, the totals skip it
    got = rollup_one("gauge", [4.0, N0, cases.NAN_SIG],
                     ["last", "count", "sum", "min", "max"])
    assert got == dict(last=cases.NAN_SIG, count=bits(3.0), sum=bits(4.0),
                       min=N0, max=bits(4.0))


def test_gauge_zero_ties_keep_the_first():
    # gauge.go:93-98: max < v and min > v are strict, so a tie keeps the
    # earlier value's sign; 0 + -0 = +0 in the sum
    got = rollup_one("gauge", [P0, N0], ["min", "max", "sum", "last"])
    assert got == dict(min=P0, max=P0, sum=P0, last=N0)
    got = rollup_one("gauge", [N0, P0], ["min", "max", "sum", "last"])
    assert got == dict(min=N0, max=N0, sum=P0, last=P0)


I64_MIN = -2.0**63
COUNTER_PINS = [
    # counter.go:63-75 on int64(value), Go's amd64 conversion: truncation
    # toward zero, NaN and out-of-range values give math.MinInt64; sum and
    # sumSq wrap. name, values, {agg: expected double}
    ("fractions", [2.9, -2.9, 0.5], dict(sum=0.0, min=-2.0, max=2.0, sumsq=8.0)),
    # 5 + MinInt64; MinInt64^2 = 2^126 = 0 mod 2^64
    ("nan", [5.0, float("nan")],
     dict(sum=float(5 - 2**63), min=I64_MIN, max=5.0, sumsq=25.0, count=2.0)),
    # two MinInt64 sum to 0 mod 2^64
    ("inf", [5.0, float("inf"), -float("inf")],
     dict(sum=5.0, min=I64_MIN, max=5.0, sumsq=25.0)),
    ("out_of_range_pos", [1e19], dict(sum=I64_MIN, min=I64_MIN, max=I64_MIN)),
    ("out_of_range_neg", [-1e19], dict(sum=I64_MIN, max=I64_MIN)),
    ("two_to_63", [2.0**63, 1.0], dict(sum=float(1 - 2**63), max=1.0)),
    ("minus_two_to_63", [-2.0**63, 1.0], dict(sum=float(1 - 2**63), min=I64_MIN)),
    # 2^53 + 1 rounds to even on the way back to float64 (counter.go:123)
    ("sum_past_2p53", [2.0**53, 1.0], dict(sum=2.0**53, max=2.0**53)),
    ("isum_wrap", [2.0**62, 2.0**62], dict(sum=I64_MIN, sumsq=0.0, max=2.0**62)),
    # 2 * 3037000500^2 - 2^64 = 290948384
    ("isumsq_wrap", [3037000500.0, 3037000500.0],
     dict(sum=6074001000.0, sumsq=290948384.0)),
]


@pytest.mark.parametrize("name,values,want", COUNTER_PINS,
                         ids=[p[0] for p in COUNTER_PINS])
def test_counter_pins(name, values, want):
    assert 2 * 3037000500**2 - 2**64 == 290948384
    got = rollup_one("counter", values, list(want))
    assert got == {a: bits(x) for a, x in want.items()}


# ---------------- 2. the batches the GPU test launches ----------------

@pytest.fixture(scope="module", params=list(cases.PATHS))
def B(request):
    return cases.batch(request.param)


def test_batch_shape_and_placement(B):
    assert len(B.streams) == cases.NSERIES >= 65
    assert {3, 64} <= set(B.where)
    assert sorted(B.where.values()) == sorted(cases.classes_of(B.metric))
    for i in B.where:     # between clean neighbours
        assert i - 1 not in B.where and i + 1 not in B.where
        assert 0 < i < cases.NSERIES - 1


def test_decode_returns_the_generated_bits(B):
    for i in range(cases.NSERIES):
        n = int(B.counts[i])
        assert n == len(B.gen_ts[i])
        assert np.array_equal(B.ts[i, :n], B.gen_ts[i])
        assert np.array_equal(B.vals[i, :n].view(np.uint64),
                              B.gen_vals[i].view(np.uint64)), (i, B.where.get(i))


def _buckets_under_test(B, i):
    d = B.depth
    v = B.vals[i].view(np.uint64)
    return v[:d], v[d + cases.CLEAN_DEPTH:2 * d + cases.CLEAN_DEPTH]


def test_specials_survive_the_codec(B):
    if B.metric == "counter":
        for i, c in B.where.items():
            want = np.asarray(cases.COUNTER_CLASSES[c], np.float64)
            b0, b2 = _buckets_under_test(B, i)
            assert np.array_equal(b0, want.view(np.uint64))
            assert np.array_equal(b2, want[::-1].copy().view(np.uint64))
        return
    for i, c in B.where.items():
        for b in _buckets_under_test(B, i):
            for pattern, least in cases.FLOAT_SPECIALS[c](B.depth).items():
                assert least >= 1
                assert int(np.sum(b == np.uint64(pattern))) >= least, (c, hex(pattern))
        # the clean bucket between them holds none of the order-sensitive
        # values
        mid = B.vals[i, B.depth:B.depth + cases.CLEAN_DEPTH]
        assert np.all(mid > 0) and np.all(np.isfinite(mid))
    for i in set(range(cases.NSERIES)) - set(B.where):
        v = B.vals[i, :int(B.counts[i])]
        assert np.all(v > 0) and np.all(np.isfinite(v))


@pytest.mark.parametrize("parity", ["odd", "even"])
def test_depths_reach_the_path(B, parity):
    aggs = cases.aggs_of(B.path, parity)
    assert len(aggs) % 2 == (1 if parity == "odd" else 0)
    plan = plan_py(aggs, 1e-3)
    timer_q = B.metric == "timer" and plan["nq"] > 0
    extreme = timer_q and plan["extreme_cap"] >= 8
    d = B.depth
    if B.path in ("lane_counter", "lane_gauge", "lane_timer"):
        assert not timer_q
    elif B.path == "lane_staged":
        assert timer_q and not extreme
        assert d <= min(cases.RQCAP_LANE, plan["exact_cap"])
    elif B.path == "lane_extreme":
        assert extreme and d <= plan["extreme_cap"]
    elif B.path == "wave":
        assert timer_q and not extreme
        assert cases.RQCAP_LANE < d <= plan["exact_cap"]
    else:
        assert timer_q and d > plan["exact_cap"] >= cases.RQCAP_LANE
    # the clean series and buckets stay on the first tier
    assert cases.CLEAN_DEPTH <= (plan["extreme_cap"] if extreme
                                 else cases.RQCAP_LANE)


@pytest.mark.parametrize("parity", ["odd", "even"])
def test_bitwise_outputs_remain(B, parity):
    """Where the oracle's arithmetic result is NaN the GPU test only asks
    for a NaN: every series under test must keep a non-NaN arithmetic
    output and a selection output, which are compared bit for bit."""
    aggs = cases.aggs_of(B.path, parity)
    out, _ = cases.expected(B.path, parity)
    arith = [k for k, a in enumerate(aggs) if a in cases.ARITHMETIC]
    sel = [k for k, a in enumerate(aggs) if a in cases.SELECTION]
    assert sorted(arith + sel) == list(range(len(aggs)))
    assert arith and sel
    for i in B.where:
        assert np.any(~np.isnan(out[i][:, arith])), B.where[i]
        # and in the buckets under test themselves, for all but the classes
        # whose sum is a NaN by construction
        if not B.where[i].startswith(("nan", "inf_both")) or B.metric != "timer":
            assert np.any(~np.isnan(out[i][[0, 2]][:, arith])), B.where[i]
