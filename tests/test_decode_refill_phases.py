"""Decode parity where k_decode_batch's input schedule can go wrong.

A wave tops its lanes' 4-word LDS rings up in bursts whose spacing it picks
per tile from what the tile before consumed: one burst per 8-point tile
while every lane stays within its ring, four otherwise, and a lane that runs
dry between two bursts loads in the parser's own chain. Which of these runs
must never show in the outputs. The streams here span the regimes - below 2
bytes a point, and above 8, 12 and 16 - and switch between them inside a
tile and from tile to tile, differently in neighbouring lanes, so one wave
holds lanes that predict right, lanes that over-provide and lanes that run
dry. Rows end inside a tile next to lanes that are still dense, markers
(annotation, time-unit change) sit inside a dense tile, and dense streams
are cut around word boundaries at three depths of the look-ahead.

Streams are oracle-encoded; the expectation is oracle.decode_series, bit for
bit. Every output element is pre-filled with a sentinel and a guard row
follows the last series, as in test_decode_flush_edges.py. 40 points are 5
tiles.
"""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_full_cases as cases  # noqa: E402

T0 = 1427162400 * 10**9  # minute-aligned
CADENCE = 10 * 10**9
SENTINEL = 0x5A5A5A5A5A5A5A5A
OK, EOF, CAPACITY = cases.OK, cases.EOF, cases.CAPACITY
NPTS = 40
TILE = 8


# ----------------------------- generators -----------------------------

def _random_f64(rng, n):
    """Random finite f64 bit patterns."""
    bits = rng.integers(0, 2**63, n, dtype=np.uint64)
    expo = rng.integers(1, 2046, n).astype(np.uint64) << np.uint64(52)
    return ((bits & np.uint64(0x800FFFFFFFFFFFFF)) | expo).view(np.float64)


def _masked(seed, mask, max_step_s=2**25):
    """One series, point j dense where mask[j]: a dense point comes an
    irregular number of seconds (below max_step_s) after its predecessor and
    holds a random f64; a sparse point comes one cadence after it and holds
    a small one-decimal gauge."""
    rng = np.random.default_rng(seed)
    mask = np.asarray(mask, bool)
    n = len(mask)
    step = np.where(mask, rng.integers(1, max_step_s, n) * 10**9, CADENCE)
    ts = T0 + np.cumsum(step.astype(np.int64))
    gauge = rng.integers(0, 200, n).astype(np.float64) / 10.0
    vals = np.where(mask, _random_f64(rng, n), gauge)
    return ts, vals, None


def _sparse(seed, n):
    return _masked(seed, np.zeros(n, bool))


def _irregular(seed, n):
    return _masked(seed, np.ones(n, bool))


def _dense(seed, n):
    """Regular cadence, random f64: more than a word a point."""
    rng = np.random.default_rng(seed)
    ts = T0 + np.arange(1, n + 1, dtype=np.int64) * CADENCE
    return ts, _random_f64(rng, n), None


def _nanos(seed, n):
    """Nanosecond unit, irregular steps of up to 2^40 ns, random f64: more
    than four words per two points."""
    rng = np.random.default_rng(seed)
    ts = T0 + np.cumsum(rng.integers(1, 2**40, n, dtype=np.int64))
    return ts, _random_f64(rng, n), np.full(n, 4, np.uint8)


def _tile_mask(k, dense_first, n=NPTS):
    """Sparse for k points of every tile, dense for the other 8 - k."""
    j = np.arange(n) % TILE
    return (j < TILE - k) if dense_first else (j >= k)


def _tiles_mask(dense_tiles, n=NPTS):
    return np.isin(np.arange(n) // TILE, dense_tiles)


@functools.lru_cache(maxsize=None)
def _series(kind, seed, n=NPTS):
    """(in_ts, in_vals, ts, vals, stream): the stream is oracle-encoded and
    (ts, vals) is what the ORACLE decodes from it, the reference of every
    comparison. Generated once, shared, read-only."""
    if kind[0] == "switch":
        in_ts, in_vals, units = _masked(seed, _tile_mask(kind[1], kind[2], n))
    elif kind[0] == "tiles":
        in_ts, in_vals, units = _masked(seed, _tiles_mask(kind[1], n))
    else:
        gen = {"sparse": _sparse, "dense": _dense, "irregular": _irregular,
               "nanos": _nanos}[kind[0]]
        in_ts, in_vals, units = gen(seed, n)
    stream = oracle.encode_series(in_ts, in_vals, units=units, start_ns=T0,
                                  int_optimized=True)
    d = oracle.decode_series(stream, int_optimized=True)
    out = (in_ts, in_vals, d["ts"].copy(), d["vals"].copy())
    for a in out:
        a.setflags(write=False)
    return out + (stream,)


REGIMES = (("sparse",), ("dense",), ("irregular",), ("nanos",))
DENSE_KINDS = (("dense",), ("irregular",), ("nanos",))

# density switches: k sparse points per tile, both orders; neighbouring lanes
# differ in k. Then 3 sparse tiles + 2 dense ones, and the reverse.
SWITCH_KINDS = tuple(("switch", k, first) for first in (False, True)
                     for k in range(1, 8)) + (
    ("tiles", (3, 4)), ("tiles", (0, 1)))


@functools.lru_cache(maxsize=None)
def _switch_batch(nseries=130):
    return tuple(_series(SWITCH_KINDS[i % len(SWITCH_KINDS)], 3100 + i)[2:]
                 for i in range(nseries))


@functools.lru_cache(maxsize=None)
def _count_batch(nseries):
    """Counts 33, 37 and 40 side by side; the 40-point lanes around a short
    row are dense of all three kinds, the short rows dense and sparse."""
    counts = (33, 40, 37, 40, 40, 33, 40, 37)
    kinds = DENSE_KINDS + (("sparse",),)
    return tuple(_series(kinds[(i + i // 8) % 4], 5000 + i,
                         counts[i % len(counts)])[2:]
                 for i in range(nseries))


def _expected(batch, stride):
    return [(ts, vals, min(len(ts), stride),
             CAPACITY if len(ts) > stride else OK) for ts, vals, _ in batch]


# ----------------------------- CPU-side check -----------------------------

def _bytes_per_point(kind, seeds=range(100, 108)):
    return np.mean([len(_series(kind, s)[4]) for s in seeds]) / NPTS


def test_generated_cases_decode_on_the_oracle():
    """The oracle alone decodes every generated stream to the intended
    points, and the generators span the regimes."""
    every = [(k, s) for k in REGIMES for s in range(100, 108)]
    every += [(SWITCH_KINDS[i % len(SWITCH_KINDS)], 3100 + i)
              for i in range(130)]
    for kind, seed in every:
        in_ts, in_vals, ts, vals, stream = _series(kind, seed)
        assert len(ts) == NPTS
        assert np.array_equal(ts, in_ts), (kind, seed)
        # The int-optimised codec snaps doubles that are integers to within
        # an ulp, and codes a gauge that follows doubles as a difference
        # against them: in the switching series a value need not come back
        # to the last bit, so only the pure regimes are compared with the
        # input. The GPU is compared with the oracle's decode of every
        # point, whatever it is.
        if kind in REGIMES:
            assert np.array_equal(vals.view(np.uint64),
                                  in_vals.view(np.uint64)), (kind, seed)
        assert np.isfinite(vals).all()
    for ts, vals, stream in _count_batch(257):
        assert len(ts) in (33, 37, 40) and len(vals) == len(ts)
    bpp = {k[0]: _bytes_per_point(k) for k in REGIMES}
    print("bytes per point:", bpp)
    assert bpp["sparse"] < 2
    assert bpp["dense"] > 8
    assert bpp["irregular"] > 12
    assert bpp["nanos"] > 16  # > 4 words per 2-point span
    # the switching series really switch inside every tile
    for k in range(1, 8):
        for first in (False, True):
            m = _tile_mask(k, first).reshape(-1, TILE)
            assert (m.sum(axis=1) == TILE - k).all()
            assert m[0, 0] == first
    assert _tiles_mask((3, 4)).reshape(-1, TILE).all(axis=1).tolist() == \
        [False, False, False, True, True]
    # and cost in between the two regimes, more the fewer sparse points
    sw = [_bytes_per_point(("switch", k, False)) for k in range(1, 8)]
    assert all(a > b for a, b in zip(sw, sw[1:]))
    assert bpp["sparse"] < sw[-1] and sw[0] < bpp["irregular"]


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
    blob = np.zeros(max(int(offsets[-1]), 8), dtype=np.uint8)
    for i, s in enumerate(streams):
        o = int(offsets[i])
        blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    return (torch.from_numpy(blob).to("cuda:0"),
            torch.from_numpy(offsets[:-1].astype(np.int64)).to("cuda:0"),
            torch.from_numpy(lens.astype(np.int32)).to("cuda:0"))


def _decode(torch, engine, streams, stride, reverse=False):
    """Decode into sentinel-filled [n, stride] outputs followed by a guard
    row. Returns (rows_ts [n+1, stride], rows_vals as uint64, counts,
    errs)."""
    n = len(streams)
    d_blob, d_off, d_lens = _dev_streams(torch, streams)
    flat_ts = torch.full(((n + 1) * stride,), SENTINEL, dtype=torch.int64,
                         device="cuda:0")
    flat_vals = torch.full(((n + 1) * stride,), SENTINEL, dtype=torch.int64,
                           device="cuda:0").view(torch.float64)
    out_ts = flat_ts.view(n + 1, stride)[:n]
    out_vals = flat_vals.view(n + 1, stride)[:n]
    out_counts = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out_errs = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    perm = None
    if reverse:
        perm = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda:0")
    engine.decode_batch_dev(d_blob, d_off, d_lens, out_ts, out_vals,
                            out_counts, out_errs, int_optimized=True,
                            d_perm=perm)
    torch.cuda.synchronize()
    r_ts = flat_ts.cpu().numpy().reshape(n + 1, stride)
    r_vals = flat_vals.view(torch.int64).cpu().numpy().view(np.uint64) \
        .reshape(n + 1, stride)
    return r_ts, r_vals, out_counts.cpu().numpy(), out_errs.cpu().numpy()


def _check_rows(r_ts, r_vals, exp):
    """exp: [(ts, vals, count)]: the first `count` elements of row i equal
    the reference's, the rest of it and the guard row hold the sentinel."""
    sent = np.uint64(SENTINEL)
    n = len(exp)
    for i, (ts, vals, count) in enumerate(exp):
        assert np.array_equal(r_ts[i, :count], ts[:count]), i
        assert np.array_equal(r_vals[i, :count],
                              vals[:count].view(np.uint64)), i
        assert np.all(r_ts[i, count:] == SENTINEL), i
        assert np.all(r_vals[i, count:] == sent), i
    assert np.all(r_ts[n] == SENTINEL) and np.all(r_vals[n] == sent)


def _run_and_check(torch, engine, batch, stride, reverse=False):
    exp = _expected(batch, stride)
    r_ts, r_vals, counts, errs = _decode(torch, engine,
                                         [s for _, _, s in batch], stride,
                                         reverse=reverse)
    assert list(errs) == [e[3] for e in exp]
    assert list(counts) == [e[2] for e in exp]
    _check_rows(r_ts, r_vals, [e[:3] for e in exp])


# -------------------------------- GPU tests --------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", [k[0] for k in REGIMES])
def test_each_regime(torch, engine, kind):
    """65 series of one regime: a whole wave and one lane of the next."""
    batch = tuple(_series((kind,), 100 + i % 8)[2:] for i in range(65))
    _run_and_check(torch, engine, batch, NPTS)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_density_switches_against_the_prediction(torch, engine, reverse):
    """Sparse for k points of every tile and dense for the other 8 - k, every
    k in 1..7 and both orders, k differing from lane to lane; next to them
    series that are sparse for 3 tiles and then dense for 2, and dense for 2
    and then sparse for 3. 130 series, three waves."""
    _run_and_check(torch, engine, _switch_batch(), NPTS, reverse=reverse)


@pytest.mark.gpu
@pytest.mark.parametrize("nseries", [1, 63, 64, 65, 257])
def test_rows_ending_mid_tile_next_to_dense_lanes(torch, engine, nseries):
    """Counts 33, 37 and 40 side by side, stride 40 (16-byte flush)."""
    _run_and_check(torch, engine, _count_batch(nseries), 40)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("stride", [40, 41])
def test_wide_and_narrow_flush(torch, engine, stride, reverse):
    """Stride 41 takes the 8-byte flush; a reversed schedule permutation."""
    _run_and_check(torch, engine, _count_batch(65), stride, reverse=reverse)


@pytest.mark.gpu
def test_capacity_inside_a_dense_tile(torch, engine):
    """Stride 36 under 40-point series: the 37- and 40-point rows report
    CAPACITY in the middle of the last tile and keep 36 points."""
    batch = _count_batch(65)
    _run_and_check(torch, engine, batch, 36)
    assert {len(b[0]) for b in batch} == {33, 37, 40}


# ------------------------- markers inside a tile -------------------------

MARKED = (3, 6, 27, 30)  # points 3 and 6 of tiles 0 and 3


@functools.lru_cache(maxsize=None)
def _marked_cases(nseries=65):
    """Dense series (irregular seconds, random f64) whose points 3 and 6 of
    the first and of the fourth tile each carry an annotation and change the
    time unit, that is between points 2 and 3 and between 5 and 6 of the
    tile; every other lane is the same series without markers."""
    out = []
    for i in range(nseries):
        # steps below 2^20 s: their differences fit the 32-bit bucket of
        # the millisecond unit too
        ts, vals, _ = _masked(6000 + i, np.ones(NPTS, bool), 2**20)
        if i % 2:
            out.append(cases.Case(oracle.encode_series(
                ts, vals, start_ns=T0, int_optimized=True), True))
            continue
        rng = np.random.default_rng(6500 + i)
        units = np.ones(NPTS, np.uint8)
        anns = [b""] * NPTS
        cur = 1
        for p in MARKED:
            cur = int(rng.choice([u for u in (1, 2, 3, 4) if u != cur]))
            units[p:] = cur
            anns[p] = bytes(rng.integers(0, 256, int(rng.integers(1, 13)),
                                         dtype=np.uint8).tobytes())
        out.append(cases.Case(oracle.encode_series(
            ts, vals, units=units, annotations=anns, start_ns=T0,
            int_optimized=True), True))
    return tuple(out)


def test_marked_cases_on_the_oracle():
    batch = _marked_cases()
    for i, c in enumerate(batch):
        assert len(c) == NPTS
        assert len(c.stream) > 12 * NPTS
        in_ts, in_vals, _ = _masked(6000 + i, np.ones(NPTS, bool), 2**20)
        assert np.array_equal(c.ts, in_ts)
        assert np.array_equal(c.vals.view(np.uint64), in_vals.view(np.uint64))
        if i % 2 == 0:
            assert [p for p, _ in c.events] == list(MARKED)
            changes = np.nonzero(np.diff(c.units.astype(int)))[0] + 1
            assert changes.tolist() == list(MARKED)
        else:
            assert not c.events and (c.units == 1).all()


@pytest.mark.gpu
def test_markers_inside_a_dense_tile(torch, engine):
    """Through decode_batch_dev, and through the full-decode entry compared
    as test_decode_full_gpu.py compares it: units, block start, annotation
    regions, sentinels."""
    import test_decode_full_gpu as full
    batch = _marked_cases()
    plain = tuple((c.ts, c.vals, c.stream) for c in batch)
    _run_and_check(torch, engine, plain, NPTS)
    _run_and_check(torch, engine, plain, NPTS + 1)
    for stride in (NPTS, NPTS + 1):
        o = full.run_full(torch, engine, batch, stride)
        full.check(engine, o, batch)


# ------------------------------- truncation -------------------------------

# word boundaries of the cut stream: inside the first ring fill (4 words),
# inside the look-ahead a dense lane wants for one tile (words 4..15), and
# beyond everything a first phase could have fetched
CUT_BOUNDARIES = (16, 48, 320)
CUT_LENGTHS = tuple(b + d for b in CUT_BOUNDARIES for d in range(-8, 9))


@functools.lru_cache(maxsize=None)
def _cut_streams():
    ts, vals, stream = _series(("irregular",), 7777)[2:]
    assert len(stream) > max(CUT_LENGTHS) + 64
    return ts, vals, tuple(stream[:n] for n in CUT_LENGTHS)


def test_cut_streams_fail_on_the_oracle():
    """Every cut is a truncated stream for the oracle too: it stops with an
    error after fewer than 40 points."""
    ts, vals, cuts = _cut_streams()
    assert len(cuts) == 51
    for cut in cuts:
        k, err = cases.oracle_partial(cut)
        assert err != OK and k < NPTS


@pytest.mark.gpu
def test_truncated_dense_stream(torch, engine):
    """One wave per cut, the cut stream at a lane that moves from wave to
    wave, its 63 neighbours all sparse in one launch and all dense in the
    other."""
    ts, vals, cuts = _cut_streams()
    counts_by_neighbours = []
    for kind in (("sparse",), ("irregular",)):
        streams, exp, where = [], [], []
        for w, cut in enumerate(cuts):
            lane = (w * 5) % 64
            for l in range(64):
                if l == lane:
                    where.append(len(streams))
                    streams.append(cut)
                    exp.append(None)
                else:
                    n_ts, n_vals, n_stream = _series(kind, 100 + l % 8)[2:]
                    streams.append(n_stream)
                    exp.append((n_ts, n_vals, NPTS))
        r_ts, r_vals, counts, errs = _decode(torch, engine, streams, NPTS)
        for i in where:
            assert errs[i] != OK, i
            assert 0 <= counts[i] < NPTS, i
            # a bit-exact prefix of the untruncated decode, nothing behind it
            exp[i] = (ts, vals, int(counts[i]))
        assert all(errs[i] == OK for i in range(len(streams))
                   if i not in set(where))
        assert [int(counts[i]) for i in range(len(streams))] == \
            [e[2] for e in exp]
        _check_rows(r_ts, r_vals, exp)
        counts_by_neighbours.append([int(counts[i]) for i in where])
    print("counts per cut length:",
          dict(zip(CUT_LENGTHS, counts_by_neighbours[0])))
    assert counts_by_neighbours[0] == counts_by_neighbours[1]
