"""Decode/rollup parity at the ring, tile and wave boundaries of the
series-per-lane kernels (k_decode_batch, k_rollup_lane).

Each lane buffers its stream in a 4-word LDS ring that is topped up every
few points by a burst of exec-masked loads, issued at the start of a span of
points and committed to the ring at its end; a lane may read only the words
of its own stream. The shapes below sit where that can go wrong: streams of 0 to
12 words, tiles that end exactly at / one before / one after a multiple of
8 points, waves with 1, 63, 64 and 65 live lanes, and waves that mix streams
which drain the ring inside a tile with streams that never do. Everything is
compared bit-exactly against the oracle; streams are oracle-encoded.

The generators are checked on the CPU (test_generated_cases_*): the oracle
alone must decode every case, and the encoded lengths are pinned so that a
generator change cannot silently move a case off its boundary.
"""
import functools
import re

import numpy as np
import pytest

import oracle

T0 = 1427162400 * 10**9  # minute-aligned
CADENCE = 10 * 10**9
SENTINEL = 0x5A5A5A5A5A5A5A5A
EOF = 1       # M3GPU_SERIES_EOF
CAPACITY = 6  # M3GPU_SERIES_CAPACITY


# ----------------------------- generators -----------------------------

def _sparse(seed, n):
    """Small one-decimal gauges on a regular cadence: ~2-3 bits/pt ts+value
    in int-optimized mode, the ring is never drained inside a tile."""
    rng = np.random.default_rng(seed)
    ts = T0 + np.arange(n, dtype=np.int64) * CADENCE
    vals = rng.integers(0, 200, n).astype(np.float64) / 10.0
    return ts, vals


def _dense(seed, n):
    """Random finite f64 bit patterns: ~66 bits/pt, more than a word per
    point, so an 8-point tile consumes about twice what the ring holds."""
    rng = np.random.default_rng(seed)
    ts = T0 + np.arange(n, dtype=np.int64) * CADENCE
    bits = rng.integers(0, 2**63, n, dtype=np.uint64)
    expo = rng.integers(1, 2046, n).astype(np.uint64) << np.uint64(52)
    vals = (bits & np.uint64(0x800FFFFFFFFFFFFF)) | expo
    return ts, vals.view(np.float64)


KINDS = {"sparse": _sparse, "dense": _dense}


@functools.lru_cache(maxsize=None)
def _series(kind, n, intopt=True, seed=None):
    """(ts, vals, stream): the stream is oracle-encoded, and (ts, vals) is
    what the ORACLE decodes from it — the reference for every comparison
    (the int-optimized codec is not lossless on integral doubles above
    2^53, which the dense kind contains). Generated once, shared, never
    modified (the arrays are read-only)."""
    in_ts, in_vals = KINDS[kind](100 + n if seed is None else seed, n)
    stream = oracle.encode_series(in_ts, in_vals, start_ns=T0,
                                  int_optimized=intopt)
    d = oracle.decode_series(stream, int_optimized=intopt)
    ts, vals = d["ts"].copy(), d["vals"].copy()
    assert len(ts) == n and np.array_equal(ts, in_ts)
    ts.setflags(write=False)
    vals.setflags(write=False)
    return ts, vals, stream


def _words(stream):
    return (len(stream) + 7) // 8


def _alternating(nseries, npts, intopt=True):
    """dense, sparse, dense, ... with per-series seeds."""
    return [_series("dense" if i % 2 == 0 else "sparse", npts, intopt,
                    seed=1000 + i) for i in range(nseries)]


# stream-length cases: (kind, npts) -> encoded length in 8-byte words,
# int-optimized. Pinned: both sides of 4, 5, 8 and 9 words are covered by
# both kinds together, and 2/3 words by the sparse kind.
LENGTH_CASES = {
    ("sparse", 1): 2, ("sparse", 2): 2, ("sparse", 3): 3, ("sparse", 4): 3,
    ("sparse", 5): 3, ("sparse", 7): 3, ("sparse", 8): 3, ("sparse", 9): 3,
    ("sparse", 10): 4, ("sparse", 14): 5, ("sparse", 33): 8, ("sparse", 38): 9,
    ("dense", 1): 3, ("dense", 2): 4, ("dense", 3): 5, ("dense", 4): 6,
    ("dense", 5): 7, ("dense", 7): 10, ("dense", 8): 11, ("dense", 9): 12,
}
TRUNC_BYTES = 40          # dense 9-point stream cut inside its 4th point
TRUNC_POINTS = 3          # complete points in the first TRUNC_BYTES bytes


def _length_batch():
    """The stream-length batch: every LENGTH_CASES stream, then a
    zero-length stream, a 1-word stub (8 bytes: not even a full first
    timestamp + value), a stream truncated mid-way, and two whole streams
    after them as neighbours. Returns (streams, expected) with expected[i] =
    (ts, vals, count, err)."""
    streams, exp = [], []
    for (kind, n) in LENGTH_CASES:
        ts, vals, s = _series(kind, n)
        streams.append(s)
        exp.append((ts, vals, n, 0))
    ts9, v9, s9 = _series("dense", 9)
    streams.append(b"")
    exp.append((ts9, v9, 0, EOF))
    streams.append(s9[:8])
    exp.append((ts9, v9, 0, EOF))
    streams.append(s9[:TRUNC_BYTES])
    exp.append((ts9, v9, TRUNC_POINTS, EOF))
    for kind in ("sparse", "dense"):
        ts, vals, s = _series(kind, 9)
        streams.append(s)
        exp.append((ts, vals, 9, 0))
    return streams, exp


def _oracle_error(stream, intopt=True):
    """Oracle's per-series error code for a stream it rejects, else 0."""
    try:
        oracle.decode_series(stream, int_optimized=intopt)
    except RuntimeError as e:
        return -int(re.search(r"(-?\d+)$", str(e)).group(1))
    return 0


# -------------------------- CPU-side case checks --------------------------

def test_generated_cases_lengths_are_pinned():
    got = {k: _words(_series(*k)[2]) for k in LENGTH_CASES}
    assert got == LENGTH_CASES
    words = set(got.values())
    for boundary in (4, 5, 8, 9):
        assert boundary in words
        assert any(w < boundary for w in words)
        assert any(w > boundary for w in words)
    # dense really drains a 4-word ring inside one tile, sparse never does
    assert _words(_series("dense", 40)[2]) > 40
    assert _words(_series("sparse", 40)[2]) <= 10


def test_generated_cases_decode_on_the_oracle():
    streams, exp = _length_batch()
    for s, (ts, vals, count, err) in zip(streams, exp):
        assert _oracle_error(s) == err
        if err == 0:
            d = oracle.decode_series(s)
            assert len(d["ts"]) == count
            assert np.array_equal(d["ts"], ts)
            assert np.array_equal(d["vals"].view(np.uint64), vals.view(np.uint64))
    # the truncation point: TRUNC_POINTS whole points fit, one more does not
    ts9, v9, _ = _series("dense", 9)

    def raw_bits(k):
        b, pos = oracle.encode_series(ts9[:k], v9[:k], start_ns=T0, raw=True)
        return (len(b) - 1) * 8 + pos
    assert raw_bits(TRUNC_POINTS) <= TRUNC_BYTES * 8 < raw_bits(TRUNC_POINTS + 1)
    for intopt in (True, False):
        assert len(_alternating(64, 40, intopt)) == 64  # each decodes (see _series)


# ------------------------------ GPU plumbing ------------------------------

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


def _pack_tight(streams):
    """8-byte-aligned, zero-padded to 8 bytes and nothing more (the C ABI's
    minimum): the blob ends with the last stream's last word, and a
    zero-length stream owns no byte at all."""
    lens = np.array([len(s) for s in streams], dtype=np.uint32)
    padded = (lens.astype(np.uint64) + 7) & ~np.uint64(7)
    offsets = np.zeros(len(streams) + 1, dtype=np.uint64)
    np.cumsum(padded, out=offsets[1:])
    blob = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for i, s in enumerate(streams):
        o = int(offsets[i])
        blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    return blob, offsets, lens


def _dev_streams(torch, streams):
    blob, offsets, lens = _pack_tight(streams)
    return (torch.from_numpy(blob).to("cuda:0"),
            torch.from_numpy(offsets[:-1].astype(np.int64)).to("cuda:0"),
            torch.from_numpy(lens.astype(np.int32)).to("cuda:0"))


def _gpu_decode(torch, engine, streams, stride, intopt=True, reverse=False):
    d_blob, d_off, d_lens = _dev_streams(torch, streams)
    n = len(streams)
    out_ts = torch.full((n, stride), SENTINEL, dtype=torch.int64, device="cuda:0")
    out_vals = torch.full((n, stride), SENTINEL, dtype=torch.int64,
                          device="cuda:0").view(torch.float64)
    out_counts = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out_errs = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    perm = None
    if reverse:
        perm = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda:0")
    engine.decode_batch_dev(d_blob, d_off, d_lens, out_ts, out_vals,
                            out_counts, out_errs, int_optimized=intopt,
                            d_perm=perm)
    torch.cuda.synchronize()
    return (out_ts.cpu().numpy(), out_vals.cpu().numpy().view(np.uint64),
            out_counts.cpu().numpy(), out_errs.cpu().numpy())


def _check(got, exp):
    """exp[i] = (ts, vals, count, err). Leading `count` points bit-equal,
    everything past them untouched."""
    g_ts, g_vals, g_counts, g_errs = got
    assert list(g_errs) == [e[3] for e in exp]
    assert list(g_counts) == [e[2] for e in exp]
    for i, (ts, vals, count, _) in enumerate(exp):
        assert np.array_equal(g_ts[i, :count], ts[:count]), i
        assert np.array_equal(g_vals[i, :count],
                              vals[:count].view(np.uint64)), i
        assert np.all(g_ts[i, count:] == SENTINEL), i
        assert np.all(g_vals[i, count:] == np.uint64(SENTINEL)), i


# -------------------------------- GPU tests --------------------------------

@pytest.mark.gpu
def test_stream_lengths_in_words(torch, engine):
    """0, 1 and 2..12-word streams side by side in one wave: the short ones
    end inside the first top-up, the rest on both sides of the 4-word ring
    and of the second (5, 8, 9 words) top-up. The zero-length, stub and
    truncated streams report EOF and leave their neighbours alone."""
    streams, exp = _length_batch()
    _check(_gpu_decode(torch, engine, streams, 40), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("npts", [1, 7, 8, 9, 15, 16, 17, 33])
def test_tile_boundary_capacity_exactly_met(torch, engine, npts):
    series = _alternating(65, npts)
    exp = [(ts, vals, npts, 0) for ts, vals, _ in series]
    got = _gpu_decode(torch, engine, [s for _, _, s in series], npts)
    _check(got, exp)


@pytest.mark.gpu
def test_tile_boundary_capacity_one_short(torch, engine):
    """stride == npts - 1 with npts one past a tile: every series flags
    CAPACITY, and the points that fit are right."""
    npts = 17
    series = _alternating(65, npts)
    exp = [(ts, vals, npts - 1, CAPACITY) for ts, vals, _ in series]
    got = _gpu_decode(torch, engine, [s for _, _, s in series], npts - 1)
    _check(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("nseries", [1, 63, 64, 65, 257])
def test_wave_and_block_boundary(torch, engine, nseries):
    """Partially filled waves: idle lanes sit through every top-up burst
    and must not load anything. With nseries == 1 the blob is one tightly
    packed stream, so there is nowhere valid for a stray load to go."""
    npts = 17
    series = _alternating(nseries, npts)
    exp = [(ts, vals, npts, 0) for ts, vals, _ in series]
    got = _gpu_decode(torch, engine, [s for _, _, s in series], npts)
    _check(got, exp)


@pytest.mark.gpu
def test_wave_of_empty_streams(torch, engine):
    """A whole wave without a single word (no lane may load anything) next
    to a wave with data."""
    ts, vals, s = _series("dense", 9)
    streams = [b""] * 64 + [s]
    exp = [(ts, vals, 0, EOF)] * 64 + [(ts, vals, 9, 0)]
    _check(_gpu_decode(torch, engine, streams, 16), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("intopt", [True, False])
@pytest.mark.parametrize("reverse", [False, True])
def test_mixed_density_in_one_wave(torch, engine, intopt, reverse):
    """Lanes that drain the ring mid-tile (dense) beside lanes that never
    do (sparse), in natural and in reversed schedule order."""
    series = _alternating(64, 40, intopt)
    exp = [(ts, vals, 40, 0) for ts, vals, _ in series]
    got = _gpu_decode(torch, engine, [s for _, _, s in series], 40,
                      intopt=intopt, reverse=reverse)
    _check(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("metric,agg", [("gauge", "last"), ("timer", "p99")])
def test_rollup_lane_small(torch, engine, metric, agg):
    """65 series x 33 points through the fused series-per-lane rollup."""
    nseries, npts = 65, 33
    series = _alternating(nseries, npts)
    ts = np.stack([t for t, _, _ in series])
    vals = np.stack([v for _, v, _ in series])
    counts = np.full(nseries, npts, np.uint32)
    window = 60 * 10**9
    nbuckets = int((ts[0, -1] - T0) // window) + 1
    mt = dict(gauge=oracle.METRIC_GAUGE, timer=oracle.METRIC_TIMER)[metric]
    o_out, o_wts = oracle.rollup_batch(ts, vals, counts, mt, window, nbuckets,
                                       [agg])
    d_blob, d_off, d_lens = _dev_streams(torch, [s for _, _, s in series])
    out = torch.empty((nseries, nbuckets, 1), dtype=torch.float64, device="cuda:0")
    wts = torch.empty((nseries, nbuckets), dtype=torch.int64, device="cuda:0")
    errs = torch.empty(nseries, dtype=torch.int32, device="cuda:0")
    engine.rollup_batch_dev(d_blob, d_off, d_lens, mt, window, nbuckets, [agg],
                            out, wts, errs)
    torch.cuda.synchronize()
    assert np.all(errs.cpu().numpy() == 0)
    assert np.array_equal(wts.cpu().numpy(), o_wts)
    assert np.array_equal(out.cpu().numpy().view(np.uint64),
                          o_out.view(np.uint64))
