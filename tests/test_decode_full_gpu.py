"""Full decode on the GPU (m3gpu_decode_batch_full*): each point's time unit,
the block start and the annotation regions, bit for bit against the oracle
and the reference's golden vectors, and decode -> encode on the device
reproducing every stream.

The units leave the kernel from registers: a lane packs the 8 unit bytes of a
tile and stores its own row at the flush, 8 bytes at once where the row has 8
points and the address is 8-byte aligned, byte by byte otherwise. The shapes
sit where that can go wrong: rows that end inside a tile, at and around its
edge, odd strides, unit arrays at odd addresses, strides below a count, waves
with 1, 63, 64 and 65 lanes, a reversed schedule. Every output is pre-filled
with a sentinel and whatever the decode does not own must still hold it.
Streams and expectations come from decode_full_cases.py (checked on the CPU
by test_decode_full_cpu.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_full_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
USENT = 0xA5
UGUARD = 16  # guard bytes in front of the unit rows
OK, EOF, CAPACITY = cases.OK, cases.EOF, cases.CAPACITY


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    t.cuda.set_device(DEV)
    return t


@pytest.fixture(scope="module")
def engine():
    from m3_amd import engine as e
    return e


def dev_streams(torch, streams):
    lens = np.array([len(s) for s in streams], dtype=np.uint32)
    padded = (lens.astype(np.uint64) + 7) & ~np.uint64(7)
    offsets = np.zeros(len(streams) + 1, dtype=np.uint64)
    np.cumsum(padded, out=offsets[1:])
    blob = np.zeros(max(int(offsets[-1]), 8), dtype=np.uint8)
    for i, s in enumerate(streams):
        o = int(offsets[i])
        blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    return (torch.from_numpy(blob).to(DEV),
            torch.from_numpy(offsets[:-1].astype(np.int64)).to(DEV),
            torch.from_numpy(lens.astype(np.int32)).to(DEV))


def ann_stride_for(engine, batch):
    return max(engine.ann_region_size(c.events) for c in batch)


class Out:
    """Sentinel-filled outputs for n series: ts/vals rows with a guard row
    behind and, with ts_lead, a guard element in front (base then 8- but not
    16-byte aligned); unit rows units_off bytes past an 8-byte boundary with
    UGUARD + units_off guard bytes in front and a guard row behind;
    start_ns and the regions with a guard element / row behind."""

    def __init__(self, torch, n, stride, ann_stride, ts_lead=0, units_off=0):
        self.n, self.stride, self.ann_stride = n, stride, ann_stride
        self.ts_lead, self.u_lead = ts_lead, UGUARD + units_off
        total = ts_lead + (n + 1) * stride
        self.flat_ts = torch.full((total,), SENTINEL, dtype=torch.int64,
                                  device=DEV)
        self.flat_vals = torch.full((total,), SENTINEL, dtype=torch.int64,
                                    device=DEV).view(torch.float64)
        self.ts = self.flat_ts[ts_lead:].view(n + 1, stride)[:n]
        self.vals = self.flat_vals[ts_lead:].view(n + 1, stride)[:n]
        self.flat_units = torch.full((self.u_lead + (n + 1) * stride,), USENT,
                                     dtype=torch.uint8, device=DEV)
        self.units = self.flat_units[self.u_lead:].view(n + 1, stride)[:n]
        assert self.units.data_ptr() % 8 == units_off
        assert self.ts.data_ptr() % 16 == 8 * ts_lead
        self.flat_start = torch.full((n + 1,), SENTINEL, dtype=torch.int64,
                                     device=DEV)
        self.start = self.flat_start[:n]
        self.flat_ann = torch.full((n + 1, max(ann_stride, 1)), USENT,
                                   dtype=torch.uint8, device=DEV)
        self.ann = self.flat_ann[:n] if ann_stride else None
        self.counts = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        self.errs = torch.full((n,), -1, dtype=torch.int32, device=DEV)

    def host(self):
        n, stride = self.n, self.stride
        h = lambda t: t.cpu().numpy()
        self.h_ts = h(self.flat_ts)
        self.h_vals = h(self.flat_vals.view(self.flat_ts.dtype)).view(np.uint64)
        self.h_units = h(self.flat_units)
        self.h_start = h(self.flat_start)
        self.h_ann = h(self.flat_ann)
        self.h_counts, self.h_errs = h(self.counts), h(self.errs)
        self.r_ts = self.h_ts[self.ts_lead:].reshape(n + 1, stride)
        self.r_vals = self.h_vals[self.ts_lead:].reshape(n + 1, stride)
        self.r_units = self.h_units[self.u_lead:].reshape(n + 1, stride)
        return self


def run_full(torch, engine, batch, stride, ts_lead=0, units_off=0,
             reverse=False, want=("units", "start", "ann"), ann_stride=None):
    n = len(batch)
    io = batch[0].int_optimized
    if ann_stride is None:
        ann_stride = ann_stride_for(engine, batch)
    d_blob, d_off, d_lens = dev_streams(torch, [c.stream for c in batch])
    o = Out(torch, n, stride, ann_stride, ts_lead, units_off)
    perm = None
    if reverse:
        perm = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=DEV)
    engine.decode_batch_full_dev(
        d_blob, d_off, d_lens, o.ts, o.vals, o.counts, o.errs,
        out_units=o.units if "units" in want else None,
        out_start_ns=o.start if "start" in want else None,
        out_ann=o.ann if "ann" in want else None,
        int_optimized=io, default_unit=1, d_perm=perm)
    torch.cuda.synchronize()
    return o.host()


def check(engine, o, batch, want=("units", "start", "ann"), expected=None):
    """Everything the decode owns equals the oracle's, everything else still
    holds its sentinel. expected: [(count, err)] where it is not simply the
    capacity rule."""
    n, stride = o.n, o.stride
    sent = np.uint64(SENTINEL)
    if expected is None:
        expected = [(min(len(c), stride), CAPACITY if len(c) > stride else OK)
                    for c in batch]
    assert o.h_errs.tolist() == [e for _, e in expected]
    assert o.h_counts.tolist() == [k for k, _ in expected]
    assert np.all(o.h_ts[:o.ts_lead] == SENTINEL)
    assert np.all(o.h_vals[:o.ts_lead] == sent)
    assert np.all(o.h_units[:o.u_lead] == USENT)
    for i, (c, (k, _)) in enumerate(zip(batch, expected)):
        assert np.array_equal(o.r_ts[i, :k], c.ts[:k]), i
        assert np.array_equal(o.r_vals[i, :k], c.vals[:k].view(np.uint64)), i
        assert np.all(o.r_ts[i, k:] == SENTINEL), i
        assert np.all(o.r_vals[i, k:] == sent), i
        if "units" in want:
            assert np.array_equal(o.r_units[i, :k], c.units[:k]), i
            assert np.all(o.r_units[i, k:] == USENT), i
        if "start" in want:
            assert o.h_start[i] == (c.start if len(c.stream) >= 8 else 0), i
        if "ann" in want:
            region = o.h_ann[i]
            got = engine.parse_ann_region(region)
            # the point that hit the capacity was parsed, its annotation
            # with it: only events of stored points are compared
            assert [e for e in got if e[0] < k] == \
                [e for e in c.events if e[0] < k], i
            used = np.zeros(o.ann_stride, bool)
            used[:4 + 12 * len(got)] = True
            for (_, b), j in zip(got, range(len(got))):
                off = int(region[4 + 12 * j + 4: 4 + 12 * j + 8]
                          .view(np.uint32)[0])
                used[off:off + len(b)] = True
            assert np.all(region[~used] == USENT), i
    assert np.all(o.r_ts[n] == SENTINEL) and np.all(o.r_vals[n] == sent)
    if "units" not in want:
        assert np.all(o.h_units == USENT)
    assert np.all(o.r_units[n] == USENT)
    if "start" not in want:
        assert np.all(o.h_start == SENTINEL)
    assert o.h_start[n] == SENTINEL
    if "ann" not in want:
        assert np.all(o.h_ann == USENT)
    assert np.all(o.h_ann[n] == USENT)


# ------------------------------ layout edges ------------------------------

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("units_off", [0, 1, 3])
@pytest.mark.parametrize("ts_lead", [0, 1])
@pytest.mark.parametrize("stride", [17, 18])
def test_mixed_counts_in_one_wave(torch, engine, stride, ts_lead, units_off,
                                  reverse):
    """Counts 1, 2, 7, 8, 9, 15, 16 and 17 side by side in 65 series. With
    stride 17 a row's unit bytes start at every residue mod 8, whatever the
    base; with stride 18 and an aligned base every fourth row takes the
    8-byte store."""
    batch = cases.batch(65, cases.MIXED_COUNTS)
    o = run_full(torch, engine, batch, stride, ts_lead, units_off, reverse)
    check(engine, o, batch)


# -------------------------- wave and block edges --------------------------

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("nseries", [1, 63, 64, 65, 257])
def test_wave_and_block_boundary(torch, engine, nseries, reverse):
    batch = cases.batch(nseries, cases.MIXED_COUNTS)
    check(engine, run_full(torch, engine, batch, 18, reverse=reverse), batch)


@pytest.mark.parametrize("units_off", [0, 3])
@pytest.mark.parametrize("npts,stride", [(8, 8), (16, 16), (17, 18), (17, 24),
                                         (24, 24)])
def test_all_rows_equal(torch, engine, npts, stride, units_off):
    """Every lane holds the same count: whole tiles take the unconditional
    flush; with a stride that is a multiple of 8 and an aligned base every
    full tile of units is one 8-byte store."""
    batch = cases.batch(64, (npts,))
    check(engine, run_full(torch, engine, batch, stride, units_off=units_off),
          batch)


# -------------------------------- capacity --------------------------------

@pytest.mark.parametrize("units_off", [0, 1])
@pytest.mark.parametrize("stride", [2, 8, 9, 16])
def test_stride_smaller_than_some_counts(torch, engine, stride, units_off):
    """Units are kept for exactly the first `stride` points of a series that
    reports CAPACITY; the next row's first bytes are its own."""
    batch = cases.batch(65, cases.MIXED_COUNTS)
    o = run_full(torch, engine, batch, stride, units_off=units_off)
    assert CAPACITY in o.h_errs.tolist()
    check(engine, o, batch)


# ----------------------------- optional outputs -----------------------------

@pytest.mark.parametrize("want", [("units",), ("start",), ("ann",), ()])
def test_optional_outputs(torch, engine, want):
    batch = cases.batch(65, cases.MIXED_COUNTS)
    o = run_full(torch, engine, batch, 18, want=want)
    check(engine, o, batch, want=want)
    if want:
        return
    # all absent: the plain decode's outputs, byte for byte
    d_blob, d_off, d_lens = dev_streams(torch, [c.stream for c in batch])
    p = Out(torch, 65, 18, 0)
    engine.decode_batch_dev(d_blob, d_off, d_lens, p.ts, p.vals, p.counts,
                            p.errs, int_optimized=True)
    torch.cuda.synchronize()
    p.host()
    assert np.array_equal(o.h_ts, p.h_ts)
    assert np.array_equal(o.h_vals, p.h_vals)
    assert np.array_equal(o.h_counts, p.h_counts)
    assert np.array_equal(o.h_errs, p.h_errs)


# ---------------------------------- golden ----------------------------------

def test_golden_full_streams(torch, engine):
    fs, gold = cases.golden_full_streams()
    o = run_full(torch, engine, gold, 9)
    check(engine, o, gold)
    for i, case in enumerate(fs["cases"]):
        pts = case["points"]
        k = len(pts)
        assert o.h_counts[i] == k and o.h_errs[i] == OK, case["name"]
        assert o.r_ts[i, :k].tolist() == [
            fs["base_ns"] + p.get("dt_s", 0) * 10**9 + p.get("dt_ns", 0)
            for p in pts], case["name"]
        assert o.r_vals[i, :k].view(np.float64).tolist() == \
            [p["value"] for p in pts], case["name"]
        assert o.r_units[i, :k].tolist() == [p["unit"] for p in pts], \
            case["name"]
        assert o.h_start[i] == fs["start_ns"], case["name"]
        per_point = [None] * k
        for p, b in engine.parse_ann_region(o.h_ann[i]):
            per_point[p] = list(b)
        assert per_point == case.get("decoded_annotations", [None] * k), \
            case["name"]


# ------------------------- round trip on the device -------------------------

def round_trip(torch, engine, batch, stride):
    """decode_batch_full_dev, then encode_batch_full_dev on the decode's own
    output tensors: the input streams, byte for byte."""
    n = len(batch)
    io = batch[0].int_optimized
    ann_stride = ann_stride_for(engine, batch)
    d_blob, d_off, d_lens = dev_streams(torch, [c.stream for c in batch])
    o = Out(torch, n, stride, ann_stride)
    engine.decode_batch_full_dev(
        d_blob, d_off, d_lens, o.ts, o.vals, o.counts, o.errs,
        out_units=o.units, out_start_ns=o.start, out_ann=o.ann,
        int_optimized=io, default_unit=1)
    out_stride = engine.full_out_stride(stride, True, ann_stride,
                                        ann_stride // 12)
    r_out = torch.zeros((n, out_stride), dtype=torch.uint8, device=DEV)
    r_lens = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    r_errs = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    engine.encode_batch_full_dev(
        o.ts, o.vals, o.counts, r_out, r_lens, r_errs, d_units=o.units,
        d_start_ns=o.start, d_ann=o.ann, int_optimized=io, default_unit=1)
    torch.cuda.synchronize()
    assert np.all(o.errs.cpu().numpy() == OK)
    assert o.counts.cpu().numpy().tolist() == [len(c) for c in batch]
    assert np.all(r_errs.cpu().numpy() == OK)
    rows, lens = r_out.cpu().numpy(), r_lens.cpu().numpy()
    for i, c in enumerate(batch):
        assert lens[i] == len(c.stream), i
        assert bytes(rows[i, :lens[i]]) == c.stream, i


@pytest.mark.parametrize("int_optimized", [True, False])
def test_round_trip_generated(torch, engine, int_optimized):
    round_trip(torch, engine,
               cases.batch(257, cases.MIXED_COUNTS, int_optimized), 17)


def test_round_trip_golden(torch, engine):
    round_trip(torch, engine, cases.golden_full_streams()[1], 9)


def test_round_trip_production(torch, engine):
    round_trip(torch, engine, cases.production_samples(), 720)


# ---------------------------------- errors ----------------------------------

def test_cut_and_empty_streams(torch, engine):
    """A stream cut mid-way reports EOF and keeps the units of the points in
    front of the cut; an empty stream, and one shorter than 8 bytes, have no
    block start. Whole streams between them are unaffected."""
    whole = [cases.series(9500 + i, 17, True) for i in range(16)]
    batch, expected = [], []
    for i, c in enumerate(whole):
        cut = c.stream[:len(c.stream) * 6 // 10]
        k, err = cases.oracle_partial(cut)
        assert err == EOF and 1 <= k < 17
        # the oracle's view of the whole stream; the bytes are the cut ones
        shadow = cases.Case(c.stream, True)
        shadow.stream = cut
        batch += [shadow, c]
        expected += [(k, EOF), (17, OK)]
    for stub in (b"", whole[1].stream[:5]):
        shadow = cases.Case(whole[0].stream, True)
        shadow.stream = stub
        batch.append(shadow)
        expected.append((0, EOF))
    ann_stride = ann_stride_for(engine, whole)
    o = run_full(torch, engine, batch, 18, units_off=1, ann_stride=ann_stride)
    check(engine, o, batch, expected=expected)
    assert o.h_start[o.n - 2:o.n].tolist() == [0, 0]


def test_badarg_returns_before_any_launch(torch, engine):
    batch = cases.batch(1, cases.MIXED_COUNTS)
    d_blob, d_off, d_lens = dev_streams(torch, [c.stream for c in batch])
    for ann_stride in (18, 12):
        o = Out(torch, 1, 8, ann_stride)
        with pytest.raises(engine.M3GpuError, match="ann_stride"):
            engine.decode_batch_full_dev(
                d_blob, d_off, d_lens, o.ts, o.vals, o.counts, o.errs,
                out_units=o.units, out_start_ns=o.start, out_ann=o.ann)
        torch.cuda.synchronize()
        o.host()
        assert np.all(o.h_ts == SENTINEL) and np.all(o.h_units == USENT)
        assert np.all(o.h_start == SENTINEL) and np.all(o.h_ann == USENT)
        assert o.h_counts.tolist() == [-1] and o.h_errs.tolist() == [-1]


# --------------------------------- host form ---------------------------------

def test_host_form_equals_device_form(torch, engine):
    batch = cases.batch(65, cases.MIXED_COUNTS)
    stride = 17
    ann_stride = ann_stride_for(engine, batch)
    o = run_full(torch, engine, batch, stride)
    blob, offsets, lens = engine.pack_streams([c.stream for c in batch])
    h = engine.decode_batch_full(blob, offsets, lens, stride,
                                 ann_stride=ann_stride)
    assert np.array_equal(h["counts"], o.h_counts.astype(np.uint32))
    assert np.array_equal(h["errs"], o.h_errs)
    assert np.array_equal(h["start_ns"], o.h_start[:65])
    for i, k in enumerate(o.h_counts):
        assert np.array_equal(h["ts"][i, :k], o.r_ts[i, :k]), i
        assert np.array_equal(h["vals"][i, :k].view(np.uint64),
                              o.r_vals[i, :k]), i
        assert np.array_equal(h["units"][i, :k], o.r_units[i, :k]), i
        assert not h["units"][i, k:].any(), i
        assert engine.parse_ann_region(h["ann"][i]) == \
            engine.parse_ann_region(o.h_ann[i]), i
    # the optional outputs can be left out here too
    h = engine.decode_batch_full(blob, offsets, lens, stride, units=False,
                                 start_ns=False)
    assert h["units"] is None and h["start_ns"] is None and h["ann"] is None
    assert np.array_equal(h["counts"], o.h_counts.astype(np.uint32))
