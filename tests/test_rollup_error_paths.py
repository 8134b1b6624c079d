"""The error paths and the empty-bucket paths of the fused decode->rollup on
every tier (k_rollup_lane in its five instantiations, k_rollup_batch,
k_rollup_ckms): an unsorted point, a point past the last bucket, a stream that
ends inside a bucket, gaps and an early end.

65 series (one full wave plus one lane), window 60 s, 4 buckets. The series
under test sits at index 3 and at index 64; every other series is a clean
24-point one. The outputs are prefilled with a sentinel: a failed series must
have written exactly the buckets it closed before the fault, bit-equal to the
oracle's rollup of the points before the fault, and nothing else.

Four buckets cannot hold an interior gap of two empty buckets AND trailing
empty buckets in one series, so the no-fault case comes as two: `gap`
(buckets 0 and 3 hold points) and `tail` (buckets 0 and 1 do)."""
import ctypes
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

WINDOW = 60 * 10**9
NBUCKETS = 4
NSERIES = 65
UNDER_TEST = (3, 64)
START = (1427162462 * 10**9 // WINDOW) * WINDOW
SENTINEL = 0x7FF8DEADBEEF5A5A      # a NaN payload no rollup produces
SENTINEL32 = 0x5A5A5A5A
UNSORTED, CAPACITY = 7, 6          # M3GPU_SERIES_UNSORTED / _CAPACITY
MS = 10**6

# code path that ends up handling the series under test ->
#   (metric, aggs for naggs=3, extra agg for naggs=4, points in bucket 0,
#    cadence of bucket 0 in ms)
PATHS = {
    "lane_counter": ("counter", ["sum", "min", "max"], "count", 6, 10000),
    "lane_gauge": ("gauge", ["last", "min", "max"], "sum", 6, 10000),
    "lane_timer": ("timer", ["sum", "min", "stdev"], "max", 6, 10000),
    "lane_staged": ("timer", ["sum", "max", "median"], "min", 6, 10000),
    "lane_extreme": ("timer", ["sum", "max", "p99"], "min", 6, 10000),
    # bucket 0 deeper than RQCAP_LANE = 16: the lane tier overflows there
    # before it has written anything
    "wave": ("timer", ["median", "p95", "p99"], "sum", 30, 2000),
    # bucket 0 deeper than the set's exact_cap too (checked in the test)
    "ckms": ("timer", ["median", "p95", "p99"], "sum", 600, 100),
}
FAULTS = ["before_base", "earlier_bucket", "past_last_bucket", "truncated",
          "gap", "tail"]
METRIC = dict(counter=oracle.METRIC_COUNTER, gauge=oracle.METRIC_GAUGE,
              timer=oracle.METRIC_TIMER)


def _aggs(path, naggs):
    _, aggs3, extra, _, _ = PATHS[path]
    return aggs3 + [extra] if naggs == 4 else aggs3


def _values(rng, metric, n):
    if metric == "counter":
        return rng.integers(-500, 500, n).astype(np.float64)
    return np.round(rng.random(n) * 1e4, 4)


def _bucket(b, n, cad_ms):
    return START + b * WINDOW + np.arange(n, dtype=np.int64) * cad_ms * MS


@functools.lru_cache(maxsize=None)
def _clean(metric):
    """The 64 clean neighbours' points, 6 per bucket in all 4 buckets.
    Generated once per metric, shared, read-only."""
    rng = np.random.default_rng(211)
    ts = np.tile(np.concatenate([_bucket(b, 6, 10000) for b in range(NBUCKETS)]),
                 (NSERIES, 1))
    vals = _values(rng, metric, NSERIES * 24).reshape(NSERIES, 24)
    streams = tuple(oracle.encode_series(ts[i], vals[i], start_ns=START)
                    for i in range(NSERIES))
    ts.setflags(write=False)
    vals.setflags(write=False)
    return ts, vals, streams


@functools.lru_cache(maxsize=None)
def _clean_rollup(metric, aggs):
    ts, vals, _ = _clean(metric)
    return oracle.rollup_batch(ts, vals, np.full(NSERIES, 24, np.uint32),
                               METRIC[metric], WINDOW, NBUCKETS, list(aggs))


@functools.lru_cache(maxsize=None)
def _faulty(path, fault):
    """(stream, ts, vals, open_bucket): the stream of the series under test,
    the points before the fault, and the bucket open when it strikes (None
    for the two no-fault cases, where ts/vals are the whole series)."""
    metric, _, _, depth, cad = PATHS[path]
    rng = np.random.default_rng(223)
    if fault == "gap":
        ts = np.concatenate([_bucket(0, depth, cad), _bucket(3, 6, 10000)])
    elif fault == "tail":
        ts = np.concatenate([_bucket(0, depth, cad), _bucket(1, 6, 10000)])
    else:   # bucket 0 closed, bucket 1 open with 3 (truncated: 6) points
        ts = np.concatenate([_bucket(0, depth, cad),
                             _bucket(1, 6 if fault == "truncated" else 3, 10000)])
    bad = {"before_base": START - 10 * 10**9,
           "earlier_bucket": START + 5 * 10**9,
           "past_last_bucket": START + NBUCKETS * WINDOW + 5 * 10**9}.get(fault)
    good = len(ts)
    if bad is not None:   # the bad point, then two more that must not count
        ts = np.concatenate([ts, [bad], _bucket(2, 2, 10000)])
    vals = _values(rng, metric, len(ts))
    units = None if cad % 1000 == 0 else np.full(len(ts), 2, np.uint8)
    stream = oracle.encode_series(ts, vals, units=units, start_ns=START)
    if fault == "truncated":
        # cut inside the 3rd..4th point of bucket 1: a point takes more than
        # a byte here, so at least one and at most three of them decode
        raw, _ = oracle.encode_series(ts[:depth + 3], vals[:depth + 3],
                                      units=None if units is None else units[:depth + 3],
                                      start_ns=START, raw=True)
        head, _ = oracle.encode_series(ts[:depth + 1], vals[:depth + 1],
                                       units=None if units is None else units[:depth + 1],
                                       start_ns=START, raw=True)
        assert len(head) < len(raw) - 1 < len(stream)
        stream = stream[:len(raw) - 1]
        good = depth + 1
    open_bucket = None if fault in ("gap", "tail") else 1
    return stream, ts[:good], vals[:good], open_bucket


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    t.cuda.set_device("cuda:0")
    return t


@pytest.fixture(scope="module")
def engine():
    from m3_amd import engine as e
    return e


def exact_cap(engine, aggs):
    L = engine.lib()
    L.m3gpu_ckms_exact_cap.restype = ctypes.c_int
    L.m3gpu_ckms_exact_cap.argtypes = [ctypes.POINTER(ctypes.c_int32),
                                       ctypes.c_int, ctypes.c_double]
    a = np.asarray([engine.M3GPU_AGG[x] for x in aggs], dtype=np.int32)
    return L.m3gpu_ckms_exact_cap(
        a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(a), 1e-3)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("naggs", [3, 4])
@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_rollup_fault(torch, engine, path, fault, naggs):
    metric, _, _, depth, _ = PATHS[path]
    aggs = _aggs(path, naggs)
    if path == "ckms":
        assert depth > exact_cap(engine, aggs) >= 30
    elif path == "wave":
        assert 16 < depth <= exact_cap(engine, aggs)
    _, _, clean_streams = _clean(metric)
    c_out, c_wts = _clean_rollup(metric, tuple(aggs))
    stream, f_ts, f_vals, open_bucket = _faulty(path, fault)
    streams = list(clean_streams)
    for i in UNDER_TEST:
        streams[i] = stream
    blob, offsets, lens = engine.pack_streams(streams)

    want_err = 0
    if fault in ("before_base", "earlier_bucket"):
        want_err = UNSORTED
    elif fault == "past_last_bucket":
        want_err = CAPACITY
    elif fault == "truncated":   # the decoder's own code for these bytes
        sb, so, sl = engine.pack_streams([stream])
        want_err = int(engine.decode_batch(sb, so, sl, depth + 8,
                                           check_errors=False)[3][0])
        assert want_err != 0
    f_out, f_wts = oracle.rollup_batch(
        f_ts[None, :], f_vals[None, :], np.array([len(f_ts)], np.uint32),
        METRIC[metric], WINDOW, NBUCKETS, aggs)

    dev = "cuda:0"
    d_blob = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(dev)
    out = torch.full((NSERIES, NBUCKETS, naggs), SENTINEL, dtype=torch.int64,
                     device=dev).view(torch.float64)
    wts = torch.full((NSERIES, NBUCKETS), SENTINEL, dtype=torch.int64, device=dev)
    errs = torch.full((NSERIES,), SENTINEL32, dtype=torch.int32, device=dev)
    engine.rollup_batch_dev(d_blob, d_off, d_lens, METRIC[metric], WINDOW,
                            NBUCKETS, aggs, out, wts, errs)
    torch.cuda.synchronize()
    g, gw, ge = _u64(out.cpu().numpy()), wts.cpu().numpy(), errs.cpu().numpy()

    want_errs = np.zeros(NSERIES, np.int32)
    want_errs[list(UNDER_TEST)] = want_err
    assert list(ge) == list(want_errs)
    for i in range(NSERIES):
        if i in UNDER_TEST:
            done = NBUCKETS if open_bucket is None else open_bucket
            assert np.array_equal(g[i, :done], _u64(f_out[0, :done])), i
            assert np.array_equal(gw[i, :done], f_wts[0, :done]), i
            assert np.all(g[i, done:] == np.uint64(SENTINEL)), i
            assert np.all(gw[i, done:] == SENTINEL), i
        else:
            assert np.array_equal(g[i], _u64(c_out[i])), i
            assert np.array_equal(gw[i], c_wts[i]), i
