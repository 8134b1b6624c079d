"""Value-domain cases for the fused decode->rollup, one batch per code path
(no GPU use): the seven paths of tests/test_rollup_error_paths.py::PATHS with
their window, depths and cadences, 3 buckets, 66 series.

A series under test holds one value class in bucket 0, six clean values in
bucket 1 and the class again (another draw) in bucket 2, so that whatever a
tier keeps for a bucket has to be gone after the close. The classes sit at
series 3, 6, 9, ... and the last of them at 64 (the first lane of the second
wave); every other series is a clean 18-point one, so each series under test
lies between clean neighbours.

Everything is encoded with int_optimized=False: the int-optimized codec folds
-0.0 to +0.0 ("Known reference-faithful quirks"). The expected
side is the oracle's rollup of the CPU-DECODED points of the same streams."""
import functools

import numpy as np

import oracle

WINDOW = 60 * 10**9
NBUCKETS = 3
NSERIES = 66
START = (1427162462 * 10**9 // WINDOW) * WINDOW
MS = 10**6
CLEAN_DEPTH, CLEAN_CAD = 6, 10000
RQCAP_LANE = 16

METRIC = dict(counter=oracle.METRIC_COUNTER, gauge=oracle.METRIC_GAUGE,
              timer=oracle.METRIC_TIMER)

# path -> (metric, aggs for the odd naggs, extra agg for the even naggs,
#          points in buckets 0 and 2 of a series under test, their cadence ms)
PATHS = {
    "lane_counter": ("counter", ["sum", "min", "max", "mean", "count", "sumsq",
                                 "stdev"], "last", 6, 10000),
    "lane_gauge": ("gauge", ["last", "min", "max", "mean", "count", "sum",
                             "sumsq"], "stdev", 6, 10000),
    "lane_timer": ("timer", ["sum", "min", "stdev", "max", "mean", "count",
                             "sumsq"], "last", 6, 10000),
    "lane_staged": ("timer", ["sum", "max", "median", "min", "sumsq", "stdev",
                              "count"], "mean", 6, 10000),
    "lane_extreme": ("timer", ["sum", "max", "p99", "min", "sumsq", "stdev",
                               "count"], "mean", 6, 10000),
    "wave": ("timer", ["median", "p95", "p99", "sum", "min", "max", "sumsq"],
             "count", 30, 2000),
    "ckms": ("timer", ["median", "p95", "p99", "sum", "min", "max", "sumsq"],
             "count", 600, 100),
}
SELECTION = {"last", "min", "max", "count", "median", "p10", "p20", "p25",
             "p30", "p40", "p50", "p60", "p70", "p75", "p80", "p90", "p95",
             "p99", "p999", "p9999"}
ARITHMETIC = {"sum", "sumsq", "mean", "stdev"}

NAN_GO = 0x7FF8000000000001      # Go's math.NaN()
NAN_NEG = 0xFFF8000000000000     # x86's invalid-operation NaN
NAN_SIG = 0x7FF0000000000001     # signalling
NEG_ZERO = 0x8000000000000000
MIN_NORMAL = 2.2250738585072014e-308
MIN_SUBNORMAL = 5e-324


def aggs_of(path, naggs_parity):
    _, odd, extra, _, _ = PATHS[path]
    return odd + [extra] if naggs_parity == "even" else list(odd)


def _bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def _clean_f64(rng, n):
    """Positive, non-zero, four decimals: the suite's comfortable values."""
    return np.round(rng.random(n) * 1e4, 4) + 1.0


def _clean_int(rng, n):
    return rng.integers(-500, 500, n).astype(np.float64)


def _cycle(pattern, n):
    return np.resize(np.asarray(pattern, np.float64), n)


def _with(rng, n, specials):
    """Clean values with {position: bit pattern} put in."""
    v = _clean_f64(rng, n).view(np.uint64)
    for pos, bits in specials.items():
        v[pos] = bits
    return v.view(np.float64)


def _zeros_only(rng, n):
    v = np.zeros(n, np.float64)
    neg = rng.random(n) < 0.5
    neg[0], neg[1] = False, True          # both signs in every bucket
    v[neg] = -0.0
    return v


def _nan_all(rng, n):
    return np.resize(np.array([NAN_GO, NAN_NEG, NAN_SIG], np.uint64),
                     n).view(np.float64).copy()


def _mantissa(rng, n):
    return (rng.random(n) - 0.5) * 2e4    # all 53 bits in use, both signs


P_ZERO = float.fromhex("0x0p0")
N_ZERO = -P_ZERO
# gauge and timer classes: name -> f(rng, n) -> the n values of one bucket
FLOAT_CLASSES = {
    "zeros_pos_first": lambda rng, n: _with(rng, n, {0: 0, 1: NEG_ZERO}),
    "zeros_neg_first": lambda rng, n: _with(rng, n, {0: NEG_ZERO, 1: 0}),
    "zeros_among": lambda rng, n: _cycle(
        [-1.5, P_ZERO, 2.5, N_ZERO, -3.25, P_ZERO, N_ZERO, 7.0], n),
    "zeros_only": _zeros_only,
    "nan_first": lambda rng, n: _with(rng, n, {0: NAN_GO}),
    "nan_middle": lambda rng, n: _with(rng, n, {n // 2: NAN_NEG}),
    "nan_last_go": lambda rng, n: _with(rng, n, {n - 1: NAN_GO}),
    "nan_last_neg": lambda rng, n: _with(rng, n, {n - 1: NAN_NEG}),
    "nan_last_sig": lambda rng, n: _with(rng, n, {n - 1: NAN_SIG}),
    "nan_all": _nan_all,
    "inf_pos": lambda rng, n: _with(rng, n, {n // 3: 0x7FF0000000000000}),
    "inf_both": lambda rng, n: _with(rng, n, {1: 0x7FF0000000000000,
                                              n - 2: 0xFFF0000000000000}),
    "mag_1e200": lambda rng, n: _cycle([1e200, -1e200, 3.5, -1e200, 1e200,
                                        1e-200], n),
    # all six orders of (1e16, 1, -1e16): the sum depends on the order
    "mag_order": lambda rng, n: _cycle(
        [1e16, 1, -1e16, 1, 1e16, -1e16, -1e16, 1e16, 1,
         1e16, -1e16, 1, 1, -1e16, 1e16, -1e16, 1, 1e16], n),
    "mag_mantissa": _mantissa,
    "mag_subnormal": lambda rng, n: _cycle(
        [MIN_SUBNORMAL, MIN_NORMAL, -MIN_SUBNORMAL, 3 * MIN_SUBNORMAL,
         -MIN_NORMAL, 1.5 * MIN_NORMAL], n),
    # last in the list: the class that sits at series 64
    "nan_twice": lambda rng, n: _with(rng, n, {n // 3: NAN_GO,
                                               (2 * n) // 3: NAN_SIG}),
}
# the bit patterns each class must still hold after encode->decode, per
# bucket under test: name -> f(n) -> {bit pattern: least count}
FLOAT_SPECIALS = {
    "zeros_pos_first": lambda n: {0: 1, NEG_ZERO: 1},
    "zeros_neg_first": lambda n: {0: 1, NEG_ZERO: 1},
    "zeros_among": lambda n: {0: n // 4, NEG_ZERO: n // 4},
    "zeros_only": lambda n: {0: 1, NEG_ZERO: 1},
    "nan_first": lambda n: {NAN_GO: 1},
    "nan_middle": lambda n: {NAN_NEG: 1},
    "nan_last_go": lambda n: {NAN_GO: 1},
    "nan_last_neg": lambda n: {NAN_NEG: 1},
    "nan_last_sig": lambda n: {NAN_SIG: 1},
    "nan_all": lambda n: {NAN_GO: n // 3, NAN_NEG: n // 3, NAN_SIG: n // 3},
    "inf_pos": lambda n: {0x7FF0000000000000: 1},
    "inf_both": lambda n: {0x7FF0000000000000: 1, 0xFFF0000000000000: 1},
    "mag_1e200": lambda n: {_bits(1e200): n // 6 * 2,
                            _bits(-1e200): n // 6 * 2},
    "mag_order": lambda n: {_bits(1e16): n // 3, _bits(-1e16): n // 3},
    "mag_mantissa": lambda n: {},
    "mag_subnormal": lambda n: {1: n // 6, 0x0010000000000000: n // 6,
                                0x8000000000000001: n // 6},
    "nan_twice": lambda n: {NAN_GO: 1, NAN_SIG: 1},
}

_NAN = float("nan")
_INF = float("inf")
# counter classes: the six values of one bucket (the counter path's depth)
COUNTER_CLASSES = {
    "fractions": [2.9, -2.9, 0.5, -0.5, 1000.999, -7.25],
    "nan": [5.0, _NAN, -3.0, 11.0, _NAN, 2.0],
    "inf": [5.0, _INF, -3.0, -_INF, 11.0, 2.0],
    "out_of_range": [1e19, -1e19, 2.0**63, -2.0**63, 4.0, -9.0],
    # isum 2^54 + 2^52 + 11 is not a double: the conversion has to round
    "sum_past_2p53": [2.0**53, 1.0, 2.0**53, 3.0, 2.0**52, 7.0],
    # 2^62 twice is 2^63: isum wraps to INT64_MIN and goes on from there
    "isum_wrap": [2.0**62, 2.0**62, 5.0, 2.0**62, -3.0, 2.0**61],
    # 3037000500^2 = 9.2234e18 is just past 2^63: isumsq wraps at the 2nd
    "isumsq_wrap": [3037000500.0, 3037000499.0, -3037000500.0, 12345.0,
                    -1.0, 3037000000.0],
}


def classes_of(metric):
    return list(COUNTER_CLASSES if metric == "counter" else FLOAT_CLASSES)


def placement(metric):
    """{series index: class name}: 3, 6, 9, ... and the last class at 64."""
    names = classes_of(metric)
    where = {3 + 3 * k: c for k, c in enumerate(names[:-1])}
    assert max(where) < 63
    where[64] = names[-1]
    return where


def _bucket_ts(b, n, cad_ms):
    return START + b * WINDOW + np.arange(n, dtype=np.int64) * cad_ms * MS


class Batch:
    """One path's batch. gen_*: what was generated; ts/vals/counts: what the
    CPU decoder returns for the streams, zero-padded rows."""


@functools.lru_cache(maxsize=None)
def batch(path):
    metric, _, _, depth, cad = PATHS[path]
    rng = np.random.default_rng(20261021)
    where = placement(metric)
    clean = _clean_int if metric == "counter" else _clean_f64
    clean_ts = np.concatenate([_bucket_ts(b, CLEAN_DEPTH, CLEAN_CAD)
                               for b in range(NBUCKETS)])
    test_ts = np.concatenate([_bucket_ts(0, depth, cad),
                              _bucket_ts(1, CLEAN_DEPTH, CLEAN_CAD),
                              _bucket_ts(2, depth, cad)])
    units = None if cad % 1000 == 0 else np.full(len(test_ts), 2, np.uint8)
    B = Batch()
    B.path, B.metric, B.depth, B.where = path, metric, depth, where
    B.gen_ts, B.gen_vals, B.streams = [], [], []
    for i in range(NSERIES):
        if i in where:
            if metric == "counter":
                assert depth == 6
                cls = np.asarray(COUNTER_CLASSES[where[i]], np.float64)
                b0, b2 = cls, cls[::-1].copy()
            else:
                f = FLOAT_CLASSES[where[i]]
                b0, b2 = f(rng, depth), f(rng, depth)
            ts = test_ts
            vals = np.concatenate([b0, clean(rng, CLEAN_DEPTH), b2])
            u = units
        else:
            ts, vals, u = clean_ts, clean(rng, len(clean_ts)), None
        B.gen_ts.append(ts)
        B.gen_vals.append(vals)
        B.streams.append(oracle.encode_series(ts, vals, units=u, start_ns=START,
                                              int_optimized=False))
    width = len(test_ts)
    B.ts = np.zeros((NSERIES, width), np.int64)
    B.vals = np.zeros((NSERIES, width), np.float64)
    B.counts = np.zeros(NSERIES, np.uint32)
    for i, s in enumerate(B.streams):
        d = oracle.decode_series(s, int_optimized=False)
        n = len(d["ts"])
        B.ts[i, :n], B.vals[i, :n], B.counts[i] = d["ts"], d["vals"], n
    for a in (B.ts, B.vals, B.counts):
        a.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def expected(path, naggs_parity):
    """The oracle's rollup of the decoded points: (out, window_ts),
    computed once per parameter and shared read-only."""
    B = batch(path)
    out, wts = oracle.rollup_batch(B.ts, B.vals, B.counts, METRIC[B.metric],
                                   WINDOW, NBUCKETS,
                                   aggs_of(path, naggs_parity))
    out.setflags(write=False)
    wts.setflags(write=False)
    return out, wts
