"""Decode parity around the depth and the refill of k_decode_batch's ring.

k_decode_batch reads each lane's stream through an 8-word LDS ring that is
topped up in bursts of up to 8 words, loaded 16 bytes at a time where the
address is 16-byte aligned and 8 bytes in front of and behind such pairs. The
cases here sit where that depth and those loads can go wrong, not where the
workload is: streams of 0 to 17 words, so that a lane's ring is never full,
filled exactly once, or wrapped exactly once, with every length next to every
other in one wave; lanes that pull fewer than 8, about 8 and more than 8
words in one 8-point tile, and lanes that alternate calm and busy tiles, so
the wave changes its top-up span while rings are half full; the same batch at
three alignments of the streams, which must not show in the outputs; dense
streams cut around the byte boundaries of words 7, 8 and 9; and partial
waves and blocks, with and without a schedule permutation, through both
instantiations of the kernel.

Streams are oracle-encoded; the expectation is the oracle's decode, bit for
bit, for ts, vals, counts and error codes. Outputs are sentinel-filled and a
guard row follows the last series, as in test_decode_refill_phases.py, whose
generators this module shares. 40 points are 5 tiles.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_full_cases as cases  # noqa: E402
import test_decode_refill_phases as ph  # noqa: E402

OK, EOF, CAPACITY = cases.OK, cases.EOF, cases.CAPACITY
NPTS = ph.NPTS
TILE = ph.TILE
SENTINEL = ph.SENTINEL
RING_WORDS = 8

WORD_LENGTHS = (0, 1, 3, 7, 8, 9, 15, 16, 17)
# one byte before, at, and one byte after the end of words 7, 8 and 9
CUT_BYTES = tuple(8 * w + d for w in (7, 8, 9) for d in (-1, 0, 1))


# ------------------------------- reference -------------------------------

def _oracle_read(stream, cap=64):
    """(ts, vals, count, err) as the oracle reads `stream`, also where it
    stops with an error: the points before the error stay."""
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    ts = np.full(cap, -1, np.int64)
    vals = np.zeros(cap, np.float64)
    units = np.zeros(cap, np.uint8)
    P = ctypes.POINTER
    r = oracle.lib().oracle_decode_series(
        buf.ctypes.data_as(P(ctypes.c_uint8)), len(buf), 1, 1,
        ts.ctypes.data_as(P(ctypes.c_int64)),
        vals.ctypes.data_as(P(ctypes.c_double)),
        units.ctypes.data_as(P(ctypes.c_uint8)), None, None, 0, cap)
    if r >= 0:
        return ts[:r], vals[:r], int(r), OK
    k = int(np.count_nonzero(ts != -1))
    assert np.all(ts[:k] != -1)
    return ts[:k], vals[:k], k, int(-r)


def _ref(stream):
    """(ts, vals, stream) with the oracle's count and error."""
    ts, vals, k, err = _oracle_read(stream)
    for a in (ts, vals):
        a.setflags(write=False)
    return ts, vals, bytes(stream), err


@functools.lru_cache(maxsize=None)
def _length_batch(nseries=130):
    """Dense streams (more than a word a point) cut to WORD_LENGTHS words,
    lane i and lane i + 1 at different lengths, from four different series;
    every 10th lane keeps its whole stream."""
    out = []
    for i in range(nseries):
        kind = ph.DENSE_KINDS[(i // 3) % 3]
        stream = ph._series(kind, 100 + i % 8)[4]
        if i % 10 == 9:
            out.append(_ref(stream))
        else:
            nw = WORD_LENGTHS[i % len(WORD_LENGTHS)]
            assert len(stream) > 8 * nw
            out.append(_ref(stream[:8 * nw]))
    return tuple(out)


# tiles 0, 2, 4 busy and 1, 3 calm, and the reverse
ALTERNATING = (("tiles", (0, 2, 4)), ("tiles", (1, 3)))
CONSUMPTION_KINDS = ph.REGIMES + ph.SWITCH_KINDS + ALTERNATING


@functools.lru_cache(maxsize=None)
def _consumption_batch(nseries=130):
    return tuple(
        _ref(ph._series(CONSUMPTION_KINDS[i % len(CONSUMPTION_KINDS)],
                        4200 + i)[4]) for i in range(nseries))


@functools.lru_cache(maxsize=None)
def _cut_batch():
    """One wave per dense kind: the nine cuts of one stream at lanes spread
    over the wave, whole dense streams in the other lanes."""
    out, where = [], []
    for w, kind in enumerate(ph.DENSE_KINDS):
        victim = ph._series(kind, 7000 + w)[4]
        assert len(victim) > max(CUT_BYTES) + 8
        at = {(7 * c + 3 * w) % 64: n for c, n in enumerate(CUT_BYTES)}
        assert len(at) == len(CUT_BYTES)
        for l in range(64):
            if l in at:
                where.append(len(out))
                out.append(_ref(victim[:at[l]]))
            else:
                out.append(_ref(ph._series(kind, 100 + l % 8)[4]))
    return tuple(out), tuple(where)


def _expected(batch, stride):
    exp = []
    for ts, vals, _, err in batch:
        if len(ts) > stride:
            exp.append((ts, vals, stride, CAPACITY))
        else:
            exp.append((ts, vals, len(ts), err))
    return exp


# ----------------------------- CPU-side checks -----------------------------

def test_length_batch_on_the_oracle():
    batch = _length_batch()
    lens = [len(s) for _, _, s, _ in batch]
    assert {n // 8 for n in lens if n <= 8 * 17} >= set(WORD_LENGTHS)
    for i, (ts, vals, stream, err) in enumerate(batch):
        if i % 10 == 9:
            assert err == OK and len(ts) == NPTS
        else:
            assert err == EOF and len(ts) < NPTS, (i, err)
    # a stream shorter than the reader's three-word look-ahead yields no
    # point or one; neighbours differ in length
    assert all(len(batch[i][0]) <= 1 for i in range(0, 9) if lens[i] <= 8)
    assert all(lens[i] != lens[i + 1] for i in range(len(lens) - 1))


def test_consumption_batch_on_the_oracle():
    """Lanes below, around and above one ring (8 words) per 8-point tile,
    and the alternating series alternate."""
    batch = _consumption_batch()
    per_tile = np.array([len(s) / (NPTS / TILE) / 8.0
                         for _, _, s, _ in batch])
    print("words per tile, min / median / max:", per_tile.min(),
          np.median(per_tile), per_tile.max())
    assert (per_tile < RING_WORDS - 2).any()
    assert ((per_tile > RING_WORDS - 1.5) & (per_tile < RING_WORDS + 1.5)).any()
    assert (per_tile > 2 * RING_WORDS).any()
    for ts, vals, s, err in batch:
        assert err == OK and len(ts) == NPTS
    assert ph._tiles_mask((0, 2, 4)).reshape(-1, TILE).all(axis=1).tolist() \
        == [True, False, True, False, True]
    assert ph._tiles_mask((1, 3)).reshape(-1, TILE).all(axis=1).tolist() \
        == [False, True, False, True, False]
    # a busy tile of the alternating series alone overruns the ring
    assert ph._bytes_per_point(("irregular",)) * TILE > 8 * RING_WORDS


def test_cut_batch_on_the_oracle():
    batch, where = _cut_batch()
    assert len(where) == 3 * len(CUT_BYTES)
    for i, (ts, vals, s, err) in enumerate(batch):
        if i in where:
            assert err == EOF and len(ts) < NPTS
        else:
            assert err == OK and len(ts) == NPTS


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


def _offsets(streams, packing):
    """Byte offsets of the streams in the blob and the blob's size. line:
    every stream on a 64-byte boundary (engine.pack_streams); odd8: every
    stream at an offset = 8 (mod 16); mixed: neighbouring lanes at 0, 8, 16,
    ... 56 (mod 64) by turns; tight: 8-byte padding only."""
    offs, o = [], 0
    for i, s in enumerate(streams):
        if packing == "line":
            o = (o + 63) & ~63
        elif packing == "odd8":
            o = ((o + 15) & ~15) + 8
        elif packing == "mixed":
            o = ((o + 63) & ~63) + 8 * ((5 * i) % 8)
        else:
            assert packing == "tight"
        offs.append(o)
        o += (len(s) + 7) & ~7
    return offs, max(o, 8)


def _dev_streams(torch, streams, packing):
    offs, size = _offsets(streams, packing)
    blob = np.zeros(size, dtype=np.uint8)
    for o, s in zip(offs, streams):
        blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    lens = np.array([len(s) for s in streams], dtype=np.int32)
    d_blob = torch.from_numpy(blob).to("cuda:0")
    assert d_blob.data_ptr() % 64 == 0
    return (d_blob, torch.from_numpy(np.array(offs, np.int64)).to("cuda:0"),
            torch.from_numpy(lens).to("cuda:0"))


def _decode(torch, engine, streams, stride, packing="tight", reverse=False):
    """Rows [n + 1, stride] of ts and of vals (as uint64), counts, errs."""
    n = len(streams)
    d_blob, d_off, d_lens = _dev_streams(torch, streams, packing)
    flat_ts = torch.full(((n + 1) * stride,), SENTINEL, dtype=torch.int64,
                         device="cuda:0")
    flat_vals = torch.full(((n + 1) * stride,), SENTINEL, dtype=torch.int64,
                           device="cuda:0").view(torch.float64)
    out_counts = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out_errs = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    perm = None
    if reverse:
        perm = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda:0")
    engine.decode_batch_dev(d_blob, d_off, d_lens,
                            flat_ts.view(n + 1, stride)[:n],
                            flat_vals.view(n + 1, stride)[:n],
                            out_counts, out_errs, int_optimized=True,
                            d_perm=perm)
    torch.cuda.synchronize()
    r_ts = flat_ts.cpu().numpy().reshape(n + 1, stride)
    r_vals = flat_vals.view(torch.int64).cpu().numpy().view(np.uint64) \
        .reshape(n + 1, stride)
    return r_ts, r_vals, out_counts.cpu().numpy(), out_errs.cpu().numpy()


def _run_and_check(torch, engine, batch, stride, packing="tight",
                   reverse=False):
    exp = _expected(batch, stride)
    got = _decode(torch, engine, [s for _, _, s, _ in batch], stride,
                  packing=packing, reverse=reverse)
    r_ts, r_vals, counts, errs = got
    assert errs.tolist() == [e[3] for e in exp]
    assert counts.tolist() == [e[2] for e in exp]
    ph._check_rows(r_ts, r_vals, [e[:3] for e in exp])
    return got


# -------------------------------- GPU tests --------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_stream_lengths_around_the_ring(torch, engine, reverse):
    """0, 1, 3, 7, 8, 9, 15, 16 and 17 words side by side in three waves:
    EOF with the oracle's count on the cut lanes, whole streams between."""
    _run_and_check(torch, engine, _length_batch(), NPTS, reverse=reverse)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_words_per_tile_below_at_and_above_the_ring(torch, engine, reverse):
    _run_and_check(torch, engine, _consumption_batch(), NPTS, reverse=reverse)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lengths", "consumption"])
def test_alignment_of_the_streams_does_not_show(torch, engine, which):
    """64-byte aligned streams, every stream at 8 (mod 16), and mixed
    alignments within a wave: each equals the oracle, hence each other;
    the raw arrays, sentinels included, are compared as well."""
    batch = _length_batch() if which == "lengths" else _consumption_batch()
    outs = [_run_and_check(torch, engine, batch, NPTS, packing=p)
            for p in ("line", "odd8", "mixed")]
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)


def test_packings_are_what_they_say():
    streams = [s for _, _, s, _ in _length_batch()]
    line, _ = _offsets(streams, "line")
    odd8, _ = _offsets(streams, "odd8")
    mixed, _ = _offsets(streams, "mixed")
    assert all(o % 64 == 0 for o in line)
    assert all(o % 16 == 8 for o in odd8)
    assert {o % 64 for o in mixed[:64]} == set(range(0, 64, 8))
    from m3_amd import engine as e
    blob, offs, lens = e.pack_streams(streams)
    assert offs[:-1].tolist() == line
    for offs_ in (line, odd8, mixed):
        ends = [o + ((len(s) + 7) & ~7) for o, s in zip(offs_, streams)]
        assert all(e <= o for e, o in zip(ends, offs_[1:]))


@pytest.mark.gpu
def test_dense_streams_cut_at_words_7_8_9(torch, engine):
    """EOF and the oracle's count on the cut series only."""
    batch, where = _cut_batch()
    r_ts, r_vals, counts, errs = _run_and_check(torch, engine, batch, NPTS)
    assert [i for i in range(len(batch)) if errs[i] != OK] == list(where)
    assert all(errs[i] == EOF for i in where)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("nseries", [1, 63, 65, 257])
def test_partial_wave_and_block(torch, engine, nseries, reverse):
    batch = (_consumption_batch(130) + _length_batch(130))[:nseries]
    _run_and_check(torch, engine, batch, NPTS, reverse=reverse)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [36, 37])
def test_row_ending_inside_a_tile_next_to_dense_lanes(torch, engine, stride):
    """40-point series under a stride of 36 (16-byte flush) and 37 (8-byte
    flush): CAPACITY in the middle of the last tile, next to lanes that ended
    earlier with EOF."""
    batch = (_consumption_batch() + _length_batch())[100:165]
    exp = _expected(batch, stride)
    assert {e[3] for e in exp} == {CAPACITY, EOF}
    _run_and_check(torch, engine, batch, stride)


@pytest.mark.gpu
def test_full_decode_with_units(torch, engine):
    """k_decode_batch<true>: the consumption batch through
    decode_batch_full_dev, units, block start and sentinels compared as
    test_decode_full_gpu.py compares them."""
    import test_decode_full_gpu as full
    batch = tuple(cases.Case(s, True) for _, _, s, _ in _consumption_batch(65))
    for stride in (NPTS, NPTS + 1):
        o = full.run_full(torch, engine, batch, stride)
        full.check(engine, o, batch)
