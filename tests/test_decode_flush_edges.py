"""Decode parity at the edges of k_decode_batch's output flush.

A wave stages 8 points per lane in an LDS tile and writes it out transposed.
With 16-byte-aligned outputs and an even stride a lane stores a PAIR of
points, 16 bytes per array (lane l: row (l>>2)+16j, points 2*(l&3) and
2*(l&3)+1); otherwise it stores one point, 8 bytes per array (row (l>>3)+8j,
point l&7). A tile in which every row is full takes an unconditional path,
any other tile a masked one, where a pair stores 16 bytes when both of its
points exist, 8 when only the first does, and nothing otherwise.

The shapes below sit where that can go wrong: rows that end inside a pair,
at and around a tile boundary, waves with 1, 63, 64 and 65 live lanes, even
and odd strides, strides smaller than a series, output bases that are only
8-byte aligned, and a reversed schedule permutation. Every output element is
pre-filled with a sentinel; the decoded points must equal the oracle's bit
for bit and every other element - past a row's count, in the guard row after
the last series, in front of the first - must still hold the sentinel.
Streams are oracle-encoded.
"""
import functools

import numpy as np
import pytest

import oracle

T0 = 1427162400 * 10**9  # minute-aligned
CADENCE = 10 * 10**9
SENTINEL = 0x5A5A5A5A5A5A5A5A
CAPACITY = 6  # M3GPU_SERIES_CAPACITY

# one of each per 8 lanes, so every wave mixes them and no tile but a 1-lane
# wave's is full in every row; the odd counts end inside a pair
MIXED_COUNTS = (1, 2, 7, 8, 9, 15, 16, 17)


# ----------------------------- generators -----------------------------

def _sparse(seed, n):
    """Small one-decimal gauges on a regular cadence: a few bits per point."""
    rng = np.random.default_rng(seed)
    ts = T0 + np.arange(n, dtype=np.int64) * CADENCE
    vals = rng.integers(0, 200, n).astype(np.float64) / 10.0
    return ts, vals


def _dense(seed, n):
    """Random finite f64 bit patterns: more than a word per point."""
    rng = np.random.default_rng(seed)
    ts = T0 + np.arange(n, dtype=np.int64) * CADENCE
    bits = rng.integers(0, 2**63, n, dtype=np.uint64)
    expo = rng.integers(1, 2046, n).astype(np.uint64) << np.uint64(52)
    vals = (bits & np.uint64(0x800FFFFFFFFFFFFF)) | expo
    return ts, vals.view(np.float64)


GENERATORS = {"sparse": _sparse, "dense": _dense}


@functools.lru_cache(maxsize=None)
def _series(kind, n, seed):
    """(ts, vals, stream): the stream is oracle-encoded and (ts, vals) is
    what the ORACLE decodes from it, the reference of every comparison.
    Generated once, shared, read-only."""
    in_ts, in_vals = GENERATORS[kind](seed, n)
    stream = oracle.encode_series(in_ts, in_vals, start_ns=T0,
                                  int_optimized=True)
    d = oracle.decode_series(stream, int_optimized=True)
    ts, vals = d["ts"].copy(), d["vals"].copy()
    ts.setflags(write=False)
    vals.setflags(write=False)
    return ts, vals, stream


def _kind_of(kinds, i):
    return ("dense", "sparse")[i % 2] if kinds == "mixed" else kinds


@functools.lru_cache(maxsize=None)
def _batch(nseries, counts, kinds):
    """nseries series, series i with counts[i % len(counts)] points."""
    return tuple(_series(_kind_of(kinds, i), counts[i % len(counts)], 7000 + i)
                 for i in range(nseries))


# every (nseries, counts, kinds) the GPU tests below use
BATCHES = (
    [(65, MIXED_COUNTS, k) for k in ("mixed", "sparse", "dense")]
    + [(n, MIXED_COUNTS, "mixed") for n in (1, 63, 64, 257)]
    + [(64, (c,), "mixed") for c in (8, 16, 17, 24)]
)


def _expected(batch, stride):
    """[(ts, vals, count, err)]: a series longer than the stride keeps its
    first `stride` points and reports CAPACITY."""
    return [(ts, vals, min(len(ts), stride),
             CAPACITY if len(ts) > stride else 0) for ts, vals, _ in batch]


# ----------------------------- CPU-side check -----------------------------

def test_generated_cases_decode_on_the_oracle():
    """The oracle alone decodes every generated stream to the intended
    number of points, and the mixed batches really mix: every count of
    MIXED_COUNTS occurs among any 8 neighbours, in both stream kinds."""
    for nseries, counts, kinds in BATCHES:
        batch = _batch(nseries, counts, kinds)
        assert len(batch) == nseries
        for i, (ts, vals, stream) in enumerate(batch):
            want = counts[i % len(counts)]
            d = oracle.decode_series(stream, int_optimized=True)
            assert len(d["ts"]) == want == len(ts) == len(vals)
            assert np.array_equal(d["ts"],
                                  T0 + np.arange(want, dtype=np.int64) * CADENCE)
            assert np.array_equal(d["vals"].view(np.uint64),
                                  vals.view(np.uint64))
    assert set(MIXED_COUNTS) == {1, 2, 7, 8, 9, 15, 16, 17}
    # a pair whose second point is past the count: odd counts
    assert any(c % 2 for c in MIXED_COUNTS)
    # dense streams take more than a word per point, sparse ones far less
    assert len(_series("dense", 17, 7000)[2]) > 17 * 8
    assert len(_series("sparse", 17, 7001)[2]) < 17 * 4
    # strides below some counts: the expectation itself
    exp = _expected(_batch(65, MIXED_COUNTS, "mixed"), 9)
    assert [e[2] for e in exp[:8]] == [1, 2, 7, 8, 9, 9, 9, 9]
    assert [e[3] for e in exp[:8]] == [0, 0, 0, 0, 0] + [CAPACITY] * 3


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


def _dev_streams(torch, streams):
    lens = np.array([len(s) for s in streams], dtype=np.uint32)
    padded = (lens.astype(np.uint64) + 7) & ~np.uint64(7)
    offsets = np.zeros(len(streams) + 1, dtype=np.uint64)
    np.cumsum(padded, out=offsets[1:])
    blob = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for i, s in enumerate(streams):
        o = int(offsets[i])
        blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    return (torch.from_numpy(blob).to("cuda:0"),
            torch.from_numpy(offsets[:-1].astype(np.int64)).to("cuda:0"),
            torch.from_numpy(lens.astype(np.int32)).to("cuda:0"))


def _run_and_check(torch, engine, batch, stride, misalign=False,
                   reverse=False):
    """Decode `batch` into sentinel-filled [n, stride] outputs that are
    followed by a guard row, and compare everything. With `misalign` the
    outputs start one element into their allocation, so their base is 8- but
    not 16-byte aligned; the element in front is a guard too."""
    n = len(batch)
    exp = _expected(batch, stride)
    d_blob, d_off, d_lens = _dev_streams(torch, [s for _, _, s in batch])
    lead = 1 if misalign else 0
    total = lead + (n + 1) * stride
    flat_ts = torch.full((total,), SENTINEL, dtype=torch.int64, device="cuda:0")
    flat_vals = torch.full((total,), SENTINEL, dtype=torch.int64,
                           device="cuda:0").view(torch.float64)
    rows_ts = flat_ts[lead:].view(n + 1, stride)
    rows_vals = flat_vals[lead:].view(n + 1, stride)
    out_ts, out_vals = rows_ts[:n], rows_vals[:n]
    assert out_ts.is_contiguous() and out_vals.is_contiguous()
    for t in (out_ts, out_vals):
        assert t.data_ptr() % 16 == (8 if misalign else 0)
    out_counts = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out_errs = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    perm = None
    if reverse:
        perm = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda:0")
    engine.decode_batch_dev(d_blob, d_off, d_lens, out_ts, out_vals,
                            out_counts, out_errs, int_optimized=True,
                            d_perm=perm)
    torch.cuda.synchronize()
    g_ts = flat_ts.cpu().numpy()
    g_vals = flat_vals.view(torch.int64).cpu().numpy().view(np.uint64)
    assert list(out_errs.cpu().numpy()) == [e[3] for e in exp]
    assert list(out_counts.cpu().numpy()) == [e[2] for e in exp]
    sent = np.uint64(SENTINEL)
    # in front of the first row
    assert np.all(g_ts[:lead] == SENTINEL) and np.all(g_vals[:lead] == sent)
    r_ts = g_ts[lead:].reshape(n + 1, stride)
    r_vals = g_vals[lead:].reshape(n + 1, stride)
    for i, (ts, vals, count, _) in enumerate(exp):
        assert np.array_equal(r_ts[i, :count], ts[:count]), i
        assert np.array_equal(r_vals[i, :count],
                              vals[:count].view(np.uint64)), i
        assert np.all(r_ts[i, count:] == SENTINEL), i
        assert np.all(r_vals[i, count:] == sent), i
    # the guard row after the last series
    assert np.all(r_ts[n] == SENTINEL) and np.all(r_vals[n] == sent)


# -------------------------------- GPU tests --------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("stride", [17, 18])
def test_mixed_counts_in_one_wave(torch, engine, stride, misalign, reverse):
    """Counts 1, 2, 7, 8, 9, 15, 16 and 17 side by side, dense and sparse
    lanes alternating, 65 series: every tile runs the masked path, and the
    odd counts end on a pair's first point. Stride 18 with an aligned base
    stores 16 bytes per lane; stride 17 or the offset base stores 8."""
    _run_and_check(torch, engine, _batch(65, MIXED_COUNTS, "mixed"), stride,
                   misalign=misalign, reverse=reverse)


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("kinds", ["sparse", "dense"])
def test_stream_kinds(torch, engine, kinds, misalign):
    _run_and_check(torch, engine, _batch(65, MIXED_COUNTS, kinds), 18,
                   misalign=misalign)


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("npts,stride", [(8, 8), (16, 16), (16, 17),
                                         (17, 18), (24, 24), (24, 26)])
def test_all_rows_equal(torch, engine, npts, stride, misalign):
    """Every lane of the wave holds the same count: whole tiles take the
    unconditional path (16-byte stores where stride and base allow, 8-byte
    ones otherwise), and 17 points add one masked tile of a single point."""
    _run_and_check(torch, engine, _batch(64, (npts,), "mixed"), stride,
                   misalign=misalign)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("nseries", [1, 63, 64, 65, 257])
def test_wave_and_block_boundary(torch, engine, nseries, reverse):
    """Partially filled waves and more than one block: rows of idle lanes
    must not be written, wherever the flush's row shuffle lands on them."""
    _run_and_check(torch, engine, _batch(nseries, MIXED_COUNTS, "mixed"), 18,
                   reverse=reverse)


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("stride", [2, 8, 9, 16])
def test_stride_smaller_than_some_counts(torch, engine, stride, misalign):
    """Series longer than the stride report CAPACITY, keep their first
    `stride` points and write nothing past them - the next row's first
    elements, or the guard row's."""
    _run_and_check(torch, engine, _batch(65, MIXED_COUNTS, "mixed"), stride,
                   misalign=misalign)
