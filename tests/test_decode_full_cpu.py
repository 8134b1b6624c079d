"""Full decode (m3gpu_decode_batch_full*, m3gpu_merge_batch_units_dev): the
parts that need no GPU. The generators of test_decode_full_gpu.py and
test_merge_units_gpu.py hold what those tests assume of them, on the oracle
alone; the iterators report per-point units; the argument checks return
before any HIP call."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_full_cases as cases  # noqa: E402
import oracle  # noqa: E402
from m3_amd import engine  # noqa: E402
from m3_amd.iterators import BatchIterators, SliceReaderIterator  # noqa: E402

M3GPU_ERR_BADARG = -2


# ------------------------- generator premises -------------------------

@pytest.mark.parametrize("int_optimized", [True, False])
def test_generated_streams_decode_to_the_intended_counts(int_optimized):
    for nseries, counts in cases.BATCHES:
        b = cases.batch(nseries, counts, int_optimized)
        assert len(b) == nseries
        for i, c in enumerate(b):
            assert len(c) == counts[i % len(counts)] == len(c.units)
            in_ts, _, in_units, in_anns, start = cases.gen_inputs(
                9000 + i, len(c))
            # steps are multiples of the unit in force: nothing is rounded
            assert np.array_equal(c.ts, in_ts)
            assert np.array_equal(c.units, in_units)
            assert c.start == start


def test_batch_holds_the_unit_changes_it_is_meant_to():
    b = cases.batch(257, cases.MIXED_COUNTS)
    # before point 0: the first unit is not initialTimeUnit(start, Second)
    initial = [1 if c.start % 10**9 == 0 else 0 for c in b]
    assert any(c.units[0] != u0 and u0 == 1 for c, u0 in zip(b, initial))
    assert any(u0 == 0 for u0 in initial)
    for p in (1, 7, 8):
        assert any(len(c) > p and c.units[p] != c.units[p - 1] for c in b), p
    assert any(len(c) > 1 and c.units[-1] != c.units[-2] for c in b)
    # a change inside a tile and away from its edges as well
    assert any(len(c) > 4 and c.units[4] != c.units[3] for c in b)
    assert {int(u) for c in b for u in c.units} == {1, 2, 3, 4}
    changes = sum(int(np.count_nonzero(np.diff(c.units))) for c in b)
    assert changes > 257
    # about a fifth of the points annotated
    npts = sum(len(c) for c in b)
    nann = sum(len(c.events) for c in b)
    assert 0.1 * npts < nann < 0.3 * npts
    # the all-equal batches keep changes too
    assert any(np.count_nonzero(np.diff(c.units))
               for c in cases.batch(64, (8,)))


@pytest.mark.parametrize("int_optimized", [True, False])
def test_oracle_round_trip_of_generated_streams(int_optimized):
    """oracle decode -> oracle encode reproduces every stream: what the GPU
    round trip is asked to do, the reference does."""
    for nseries, counts in cases.BATCHES:
        for c in cases.batch(nseries, counts, int_optimized):
            assert c.reencode() == c.stream


def test_oracle_round_trip_of_golden_full_streams():
    fs, gold = cases.golden_full_streams()
    assert len(gold) == 4
    for case, c in zip(fs["cases"], gold):
        assert c.reencode() == c.stream == bytes(case["stream_bytes"])
        assert c.start == fs["start_ns"]
        assert list(c.units) == [p["unit"] for p in case["points"]]


def test_oracle_round_trip_of_production_samples():
    for c in cases.production_samples():
        assert len(c) in (719, 720)
        assert c.reencode() == c.stream


def test_expected_start_is_the_first_64_bits():
    for c in cases.batch(65, cases.MIXED_COUNTS):
        assert c.start == int.from_bytes(c.stream[:8], "big", signed=True)
        assert c.start < c.ts[0]
    # an empty stream has no first 64 bits; the oracle fails it with EOF
    assert cases.oracle_partial(b"") == (0, cases.EOF)


def test_cut_streams_fail_with_eof_after_a_prefix():
    """The GPU error test cuts 17-point streams at 60% of their bytes: the
    oracle then decodes a proper prefix of at least one point and fails EOF."""
    for i in range(16):
        c = cases.series(9500 + i, 17, True)
        cut = c.stream[:len(c.stream) * 6 // 10]
        n, err = cases.oracle_partial(cut)
        assert err == cases.EOF and 1 <= n < 17, (i, n, err)


@pytest.mark.parametrize("R", [1, 2, 4])
def test_merge_model_agrees_with_the_oracle(R):
    ts, vals, units, counts = cases.merge_inputs(R)
    o_ts, o_vals, o_counts, o_errs = oracle.merge_batch(ts, vals, counts)
    model = cases.merge_model(ts, vals, units, counts)
    assert np.all(o_errs == 0)
    ties = 0
    for i, (m_ts, m_vals, m_units) in enumerate(model):
        n = int(o_counts[i])
        assert n == len(m_ts)
        assert o_ts[i, :n].tolist() == m_ts
        assert o_vals[i, :n].tolist() == m_vals
        # the value names the replica (100 * (r + 1) + t): so does the unit
        assert [int(v // 100) for v in m_vals] == m_units
        ties += sum(1 for t in m_ts
                    if sum(t in ts[r, i, :counts[r, i]] for r in range(R)) > 1)
    assert (counts == 0).any() and (counts == ts.shape[2]).any()
    if R > 1:
        assert ties > 100


# ----------------------------- iterators -----------------------------

def test_iterators_report_per_point_units():
    ts = np.arange(10, 16, dtype=np.int64).reshape(2, 3)
    vals = np.arange(6, dtype=np.float64).reshape(2, 3)
    units = np.array([[1, 2, 2], [4, 4, 3]], np.uint8)
    counts = np.array([3, 2], np.uint32)
    it = SliceReaderIterator(ts[0], vals[0], 3, unit=7, units=units[0])
    got = []
    while it.Next():
        got.append(it.Current())
    assert got == [(10, 0.0, 1), (11, 1.0, 2), (12, 2.0, 2)]
    assert all(type(u) is int for _, _, u in got)
    b = BatchIterators(ts, vals, counts, unit=7, units=units)
    assert [[it.Current()[2] for _ in iter(it.Next, False)] for it in b] == \
        [[1, 2, 2], [4, 4]]
    # without units= nothing changes: the constructor's unit
    it = SliceReaderIterator(ts[0], vals[0], 3, unit=7)
    assert [it.Current()[2] for _ in iter(it.Next, False)] == [7, 7, 7]
    b = BatchIterators(ts, vals, counts, unit=2)
    assert [[it.Current()[2] for _ in iter(it.Next, False)] for it in b] == \
        [[2, 2, 2], [2, 2]]


# --------------------------- argument checks ---------------------------

needs_lib = pytest.mark.skipif(not engine.engine_available(),
                               reason="libm3gpu.so not built")


@needs_lib
def test_new_symbols_exported():
    L = engine.lib()
    for sym in ("m3gpu_decode_batch_full_dev", "m3gpu_decode_batch_full",
                "m3gpu_merge_batch_units_dev"):
        assert hasattr(L, sym), sym
    for name in ("decode_batch_full_dev", "decode_batch_full",
                 "merge_batch_units_dev"):
        assert callable(getattr(engine, name))


@needs_lib
@pytest.mark.parametrize("ann,ann_stride", [
    (4096, 18),   # ann_stride % 4 != 0
    (4096, 12),   # ann_stride < 16
    (4096, 0),    # regions, ann_stride 0
    (None, 16),   # no regions, ann_stride != 0
    (4098, 16),   # regions not 4-byte aligned
])
def test_full_dev_badarg(ann, ann_stride):
    """Rejected before anything dereferences a pointer or launches."""
    L = engine.lib()
    fake = ctypes.c_void_p(4096)
    rc = L.m3gpu_decode_batch_full_dev(
        fake, fake, fake, None, 1, 1, 1, fake, fake, fake, fake, 8,
        fake, fake, None if ann is None else ctypes.c_void_p(ann), ann_stride,
        None)
    assert rc == M3GPU_ERR_BADARG
    assert "ann" in L.m3gpu_last_error().decode()


@needs_lib
def test_full_host_badarg():
    blob, offsets, lens = engine.pack_streams([b"\0" * 16])
    L = engine.lib()
    out = np.zeros(64, np.uint8)
    P = ctypes.POINTER
    p8 = out.ctypes.data_as(P(ctypes.c_uint8))
    rc = L.m3gpu_decode_batch_full(
        blob.ctypes.data_as(P(ctypes.c_uint8)), len(blob),
        offsets.ctypes.data_as(P(ctypes.c_uint64)),
        lens.ctypes.data_as(P(ctypes.c_uint32)), 1, 1, 1,
        None, None, None, None, 8, None, None, p8, 12)
    assert rc == M3GPU_ERR_BADARG
    with pytest.raises(engine.M3GpuError, match="ann_stride"):
        engine.decode_batch_full(blob, offsets, lens, 8, ann_stride=18)


@needs_lib
@pytest.mark.parametrize("R,units,out_units", [
    (0, 4096, 4096), (5, 4096, 4096), (2, None, 4096), (2, 4096, None)])
def test_merge_units_badarg(R, units, out_units):
    L = engine.lib()
    fake = ctypes.c_void_p(4096)
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    rc = L.m3gpu_merge_batch_units_dev(
        fake, fake, vp(units), fake, R, 1, 8, fake, fake, vp(out_units), fake,
        fake, 8, None)
    assert rc == M3GPU_ERR_BADARG
