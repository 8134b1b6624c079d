"""Full encode on the GPU (m3gpu_encode_batch_full*): per-point time units,
annotations and an explicit block start, byte-exact against the reference's
golden vectors and against the oracle, one series at a time."""
import json
import os
import re

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
START = 1427162400 * 10**9   # whole seconds
BASE = 1427162462 * 10**9
DEV = "cuda:0"

OK, DOD_OVERFLOW, NO_SCHEME, ANNOTATION, CAPACITY = 0, 2, 3, 5, 6
ANN_LENS = [1, 3, 4, 5, 8, 12, 31, 32, 33, 40, 64, 65, 67, 129, 300]


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


# ------------------------------ helpers ------------------------------

class Series:
    """One series' inputs. events: [(point, bytes)] (b"" = a len-0 event)."""

    def __init__(self, ts, vals, units=None, events=(), start=None):
        self.ts = np.asarray(ts, np.int64)
        self.vals = np.asarray(vals, np.float64)
        self.units = None if units is None else np.asarray(units, np.uint8)
        self.events = list(events)
        self.start = start

    def expected(self, int_optimized):
        """(stream bytes, series error) from the oracle."""
        anns = None
        if self.events:
            anns = [b""] * len(self.ts)
            for p, b in self.events:
                anns[p] = b
        if len(self.ts) == 0:
            return b"", OK
        try:
            return oracle.encode_series(
                self.ts, self.vals, units=self.units, annotations=anns,
                start_ns=self.start, int_optimized=int_optimized), OK
        except RuntimeError as e:
            return b"", -int(re.search(r"-?\d+$", str(e)).group())


def pack(engine, series, width, with_units, with_start, with_ann,
         ann_stride=None):
    n = len(series)
    ts = np.zeros((n, width), np.int64)
    vals = np.zeros((n, width), np.float64)
    counts = np.zeros(n, np.int32)
    units = np.ones((n, width), np.uint8) if with_units else None
    starts = np.zeros(n, np.int64) if with_start else None
    for i, s in enumerate(series):
        k = len(s.ts)
        ts[i, :k], vals[i, :k], counts[i] = s.ts, s.vals, k
        if with_units and s.units is not None:
            units[i, :k] = s.units
        if with_start:
            starts[i] = s.start if s.start is not None else (s.ts[0] if k else 0)
    ann = None
    if with_ann:
        if ann_stride is None:
            ann_stride = max(engine.ann_region_size(s.events) for s in series)
        ann = np.stack([engine.build_ann_region(s.events, ann_stride)
                        for s in series])
    return ts, vals, counts, units, starts, ann


def gpu_encode_full(torch, engine, ts, vals, counts, units=None, starts=None,
                    ann=None, int_optimized=True, default_unit=1,
                    out_stride=None):
    n, width = ts.shape
    if out_stride is None:
        out_stride = engine.full_out_stride(
            width, units is not None, 0 if ann is None else ann.shape[1],
            0 if ann is None else ann.shape[1] // 12)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    d_out = torch.zeros((n, out_stride), dtype=torch.uint8, device=DEV)
    d_lens = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_errs = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    engine.encode_batch_full_dev(
        dev(ts), dev(vals), dev(counts), d_out, d_lens, d_errs,
        d_units=dev(units), d_start_ns=dev(starts), d_ann=dev(ann),
        int_optimized=int_optimized, default_unit=default_unit)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_lens.cpu().numpy(), d_errs.cpu().numpy()


def check_against_oracle(series, rows, lens, errs, int_optimized=True):
    for i, s in enumerate(series):
        exp, exp_err = s.expected(int_optimized)
        assert errs[i] == exp_err, (i, errs[i], exp_err)
        assert lens[i] == len(exp), (i, lens[i], len(exp))
        assert bytes(rows[i, :lens[i]]) == exp, i


def rand_points(rng, n, t0=BASE):
    ts = t0 + np.cumsum(rng.integers(1, 60, n)) * 10**9
    vals = np.round(rng.random(n) * 1000, int(rng.integers(0, 3)))
    return ts, vals


def payload(rng, n):
    """n binary bytes that hold 0x00 and 0xff."""
    b = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    b[0] = 0x00
    b[-1] = 0xff
    if n > 2:
        b[n // 2] = 0x00
    return bytes(b)


# --------------------- 1. reference golden vectors ---------------------

def test_golden_full_streams(torch, engine):
    """Every full_streams case of the reference's own vectors: block start
    before the first point, per-point units, annotations."""
    with open(os.path.join(GOLDEN, "encoder_vectors.json")) as f:
        fs = json.load(f)["full_streams"]
    series = []
    for case in fs["cases"]:
        ts, vals, units, events = [], [], [], []
        for p, ptd in enumerate(case["points"]):
            ts.append(fs["base_ns"] + ptd.get("dt_s", 0) * 10**9
                      + ptd.get("dt_ns", 0))
            vals.append(ptd["value"])
            units.append(ptd["unit"])
            if "annotation" in ptd:
                events.append((p, bytes(ptd["annotation"])))
        series.append(Series(ts, vals, units, events, fs["start_ns"]))
    width = max(len(s.ts) for s in series)
    args = pack(engine, series, width, True, True, True)
    rows, lens, errs = gpu_encode_full(torch, engine, *args,
                                       int_optimized=False)
    for i, case in enumerate(fs["cases"]):
        assert errs[i] == OK, case["name"]
        assert list(rows[i, :lens[i]]) == case["stream_bytes"], case["name"]


# ------------------------ 2. degenerate = bulk ------------------------

@pytest.mark.parametrize("default_unit", [1, 2])
@pytest.mark.parametrize("int_optimized", [False, True])
def test_all_null_equals_bulk(torch, engine, default_unit, int_optimized):
    rng = np.random.default_rng(5)
    counts_from = [0, 1, 7, 8, 9, 17]
    series = [Series(*rand_points(rng, counts_from[i % 6])) for i in range(70)]
    ts, vals, counts, _, _, _ = pack(engine, series, 17, False, False, False)
    out_stride = (24 * 17 + 32 + 7) & ~7
    rows, lens, errs = gpu_encode_full(
        torch, engine, ts, vals, counts, int_optimized=int_optimized,
        default_unit=default_unit, out_stride=out_stride)
    b_out = torch.zeros((70, out_stride), dtype=torch.uint8, device=DEV)
    b_lens = torch.full((70,), -1, dtype=torch.int32, device=DEV)
    b_errs = torch.full((70,), -1, dtype=torch.int32, device=DEV)
    engine.encode_batch_dev(
        torch.from_numpy(ts).to(DEV), torch.from_numpy(vals).to(DEV),
        torch.from_numpy(counts).to(DEV), b_out, b_lens, b_errs,
        int_optimized=int_optimized, unit=default_unit)
    torch.cuda.synchronize()
    assert np.array_equal(errs, b_errs.cpu().numpy())
    assert np.all(errs == OK)
    assert np.array_equal(lens, b_lens.cpu().numpy())
    assert np.array_equal(lens == 0, counts == 0)
    assert np.array_equal(rows, b_out.cpu().numpy())


# --------------------------- 3. annotations ---------------------------

def annotation_series():
    """70 series x up to 17 points; annotated and plain lanes share waves."""
    rng = np.random.default_rng(11)
    counts_from = [17, 9, 8, 16, 12, 17, 10]
    A, B = payload(rng, 6), payload(rng, 9)
    series = []
    for i in range(70):
        n = counts_from[i % 7]
        ts, vals = rand_points(rng, n)
        if i == 0:
            ev = [(0, b"\x00")]                       # point 0, one zero byte
        elif i == 1:
            ev = [(7, payload(rng, 5)), (8, payload(rng, 7))]  # tile edge
        elif i == 2:
            ev = [(3, A), (4, A), (5, A)]             # written once
        elif i == 3:
            ev = [(2, A), (3, B), (4, A)]             # written three times
        elif i == 4:
            ev = [(1, A), (5, b""), (6, A), (7, B)]   # len 0: nothing; A: same
        elif i == 5:
            ev = [(0, b"\xff"), (n - 1, payload(rng, 33))]
        elif 6 <= i < 6 + len(ANN_LENS):
            ev = [((i * 5) % n, payload(rng, ANN_LENS[i - 6]))
                  if ANN_LENS[i - 6] > 1 else ((i * 5) % n, b"\xff")]
        elif i % 2 == 0:
            ev = []                                   # plain lane
        else:
            pts = sorted(rng.choice(n, size=int(rng.integers(1, 5)),
                                    replace=False).tolist())
            ev = [(p, payload(rng, int(rng.choice(ANN_LENS[1:11]))))
                  for p in pts]
        series.append(Series(ts, vals, None, ev, START))
    return series


@pytest.fixture(scope="module")
def ann_case(torch, engine):
    series = annotation_series()
    args = pack(engine, series, 17, False, True, True)
    rows, lens, errs = gpu_encode_full(torch, engine, *args)
    return series, args, rows, lens, errs


def test_annotations(ann_case):
    series, _, rows, lens, errs = ann_case
    assert np.all(errs == OK)
    check_against_oracle(series, rows, lens, errs)
    # the dedupe cases hold what they are meant to: A once, and A twice + B
    exp_a, _ = series[2].expected(True)
    exp_aba, _ = series[3].expected(True)
    a = series[2].events[0][1]
    assert oracle.decode_series(exp_a, with_annotations=True)[
        "annotations"].count(a) == 1
    assert oracle.decode_series(exp_aba, with_annotations=True)[
        "annotations"].count(a) == 2


# ------------------------------ 4. units ------------------------------

def unit_series():
    rng = np.random.default_rng(17)
    series = []
    # s -> ms -> us -> ns -> s ..., changes at points 3, 7, 8, 9, 12, 16
    ts, vals = rand_points(rng, 17)
    units = np.ones(17, np.uint8)
    cur, change_at = 1, {3, 7, 8, 9, 12, 16}
    for p in range(17):
        if p in change_at:
            cur = cur % 4 + 1
        units[p] = cur
        ts[p:] += [0, 0, 7 * 10**6, 13 * 10**3, 11][cur]
    series.append(Series(ts, vals, units))
    # plain neighbour
    series.append(Series(*rand_points(rng, 17), np.ones(17, np.uint8)))
    # start not a multiple of the default unit: unit None, marker at point 0
    ts, vals = rand_points(rng, 9)
    series.append(Series(ts, vals, np.ones(9, np.uint8), start=BASE + 500))
    # annotation and unit change on the same point
    ts, vals = rand_points(rng, 12)
    units = np.ones(12, np.uint8)
    units[8:] = 2
    series.append(Series(ts, vals, units, [(8, payload(rng, 12))]))
    # change to unit 5 (valid, no scheme), then stay there
    ts, vals = rand_points(rng, 8)
    units = np.ones(8, np.uint8)
    units[3:] = 5
    series.append(Series(ts, vals, units))
    series.append(Series(*rand_points(rng, 8), np.full(8, 2, np.uint8)))
    # unit 0 on a point
    ts, vals = rand_points(rng, 9)
    units = np.ones(9, np.uint8)
    units[2] = 0
    series.append(Series(ts, vals, units))
    series.append(Series(*rand_points(rng, 1), np.full(1, 4, np.uint8)))
    # delta-of-delta beyond 32 bits at unit s
    ts, vals = rand_points(rng, 10)
    ts[5:] += 2**32 * 10**9
    series.append(Series(ts, vals, np.ones(10, np.uint8)))
    series.append(Series(*rand_points(rng, 17), np.full(17, 3, np.uint8)))
    return series


def test_units(torch, engine):
    series = unit_series()
    args = pack(engine, series, 17, True, True, True)
    rows, lens, errs = gpu_encode_full(torch, engine, *args)
    check_against_oracle(series, rows, lens, errs)
    assert errs.tolist() == [OK, OK, OK, OK, NO_SCHEME, OK, NO_SCHEME, OK,
                             DOD_OVERFLOW, OK]
    # the unaligned start did put a time-unit marker in front of point 0
    dec = oracle.decode_series(bytes(rows[2, :lens[2]]))
    assert dec["ts"][0] == series[2].ts[0] and dec["units"][0] == 1


# -------------------------- 5. explicit start --------------------------

def test_explicit_start(torch, engine):
    rng = np.random.default_rng(23)
    series = []
    for i, n in enumerate([1, 8, 9, 17, 7, 16]):
        ts, vals = rand_points(rng, n)
        start = START - 10 * 10**9 * i + (0 if i % 2 == 0 else 123 + i)
        assert start < ts[0]
        series.append(Series(ts, vals, start=start))
    args = pack(engine, series, 17, False, True, False)
    rows, lens, errs = gpu_encode_full(torch, engine, *args)
    assert np.all(errs == OK)
    check_against_oracle(series, rows, lens, errs)
    for i, s in enumerate(series):  # the first 64 bits are the start
        assert int.from_bytes(bytes(rows[i, :8]), "big") == s.start


# ----------------- 6. round trip through the GPU decoder -----------------

def test_round_trip_through_decoder(torch, engine, ann_case):
    series, args, rows, lens, errs = ann_case
    n = len(series)
    streams = [bytes(rows[i, :lens[i]]) for i in range(n)]
    blob, offsets, slens = engine.pack_streams(streams)
    ann_stride = args[5].shape[1]
    d_ts = torch.zeros((n, 17), dtype=torch.int64, device=DEV)
    d_vals = torch.zeros((n, 17), dtype=torch.float64, device=DEV)
    d_counts = torch.empty(n, dtype=torch.int32, device=DEV)
    d_errs = torch.empty(n, dtype=torch.int32, device=DEV)
    d_ann = torch.zeros((n, ann_stride), dtype=torch.uint8, device=DEV)
    engine.decode_batch_dev_ann(
        torch.from_numpy(blob).to(DEV),
        torch.from_numpy(offsets.astype(np.int64)).to(DEV),
        torch.from_numpy(slens.astype(np.int32)).to(DEV),
        d_ts, d_vals, d_counts, d_errs, d_ann)
    torch.cuda.synchronize()
    assert np.all(d_errs.cpu().numpy() == 0)
    assert np.array_equal(d_counts.cpu().numpy(), args[2])
    out_stride = rows.shape[1]
    r_out = torch.zeros((n, out_stride), dtype=torch.uint8, device=DEV)
    r_lens = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    r_errs = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    engine.encode_batch_full_dev(
        d_ts, d_vals, d_counts, r_out, r_lens, r_errs,
        d_start_ns=torch.from_numpy(args[4]).to(DEV), d_ann=d_ann)
    torch.cuda.synchronize()
    assert np.all(r_errs.cpu().numpy() == OK)
    assert np.array_equal(r_lens.cpu().numpy(), lens)
    assert np.array_equal(r_out.cpu().numpy(), rows)


# --------------------- 7. bad input stays contained ---------------------

def test_bad_regions_are_contained(torch, engine):
    """Each malformed region fails its own series with ANNOTATION before a
    byte of it is used; every other series encodes as the oracle does."""
    rng = np.random.default_rng(29)
    series = [Series(*rand_points(rng, [17, 9, 8, 12][i % 4]), None,
                     [(i % 8, payload(rng, 10 + i))], START)
              for i in range(70)]
    ts, vals, counts, _, starts, ann = pack(engine, series, 17, False, True,
                                            True, ann_stride=128)
    words = ann.view(np.uint32)           # [70, 32]
    bad = {}
    words[3, 0] = (128 - 4) // 12 + 1     # n_events too large for ann_stride
    bad[3] = "n_events"
    words[10, 0] = 0xffffffff
    bad[10] = "n_events huge"
    words[20, 2], words[20, 3] = 120, 9   # off + len = 129 > 128
    bad[20] = "off+len"
    words[21, 2], words[21, 3] = 0xfffffff0, 0x20  # off + len wraps
    bad[21] = "off+len wrap"
    ev2 = engine.build_ann_region([(4, b"abc"), (5, b"def")], 128).view(np.uint32)
    ann[40] = ev2.view(np.uint8)
    words[40, 4] = 4                      # second event's point == first's
    bad[40] = "equal points"
    ann[41] = ev2.view(np.uint8)
    words[41, 4] = 2                      # decreasing points
    bad[41] = "decreasing points"
    words[64, 1] = counts[64]             # point == count
    bad[64] = "point >= count"
    words[69, 1] = 0x80000000
    bad[69] = "point huge"
    rows, lens, errs = gpu_encode_full(torch, engine, ts, vals, counts,
                                       starts=starts, ann=ann)
    for i, s in enumerate(series):
        if i in bad:
            assert errs[i] == ANNOTATION, (i, bad[i], errs[i])
            assert lens[i] == 0, (i, bad[i])
        else:
            exp, _ = s.expected(True)
            assert errs[i] == OK, i
            assert bytes(rows[i, :lens[i]]) == exp, i


def test_annotation_overflows_out_stride(torch, engine):
    """out_stride fits the points but not series 33's annotation: CAPACITY
    there, the oracle's bytes everywhere else."""
    rng = np.random.default_rng(31)
    series = [Series(*rand_points(rng, 17), None, [], START) for _ in range(70)]
    series[33].events = [(9, payload(rng, 600))]
    series[34].events = [(9, payload(rng, 40))]
    out_stride = (24 * 17 + 32 + 7) & ~7  # 440: the bulk bound
    args = pack(engine, series, 17, False, True, True)
    rows, lens, errs = gpu_encode_full(torch, engine, *args,
                                       out_stride=out_stride)
    for i, s in enumerate(series):
        if i == 33:
            assert errs[i] == CAPACITY and lens[i] == 0
            continue
        exp, _ = s.expected(True)
        assert errs[i] == OK, i
        assert bytes(rows[i, :lens[i]]) == exp, i


# ----------------------------- 8. host form -----------------------------

def test_host_form_equals_dev(engine, ann_case):
    series, args, rows, lens, errs = ann_case
    ts, vals, counts, units, starts, ann = args
    h_rows, h_lens, h_errs = engine.encode_batch_full(
        ts, vals, counts, units=units, start_ns=starts, ann=ann,
        out_stride=rows.shape[1])
    assert np.array_equal(h_errs, errs)
    assert np.array_equal(h_lens, lens.astype(np.uint32))
    assert np.array_equal(h_rows, rows)


# -------------------- 9. lossless commit log bootstrap --------------------

def commitlog_entries(t_lo, t_hi):
    """12 series, points t_lo..t_hi-1 of 21: per-series units 1..4, series 5
    changing unit at t = 10, annotations at t = 0, 7, 14 on every third."""
    rng = np.random.default_rng(37)
    nseries, npts = 12, 21
    per = []
    for i in range(nseries):
        unit = i % 4 + 1
        ts = BASE + np.cumsum(rng.integers(1, 60, npts)) * 10**9
        vals = np.round(rng.random(npts) * 1000, 2)
        units = np.full(npts, unit, np.uint8)
        if i == 5:
            units[10:] = 3
        anns = [b""] * npts
        if i % 3 == 0:
            for t in (0, 7, 14):
                anns[t] = b"ann\x00\xff" + bytes([t, i])
        per.append((ts, vals, units, anns))
    entries = []
    for t in range(t_lo, t_hi):
        for i in range(nseries):
            ts, vals, units, anns = per[i]
            entries.append((i, f"full.{i:03d}".encode(), i % 4, int(ts[t]),
                            float(vals[t]), int(units[t]), anns[t] or None,
                            None))
    return per, entries


def check_bootstrap(torch, per, result, lossless):
    meta, d_bytes, d_lens, d_errs = result
    torch.cuda.synchronize()
    assert len(meta) == len(per)
    assert np.all(d_errs.cpu().numpy() == 0)
    rows, lens = d_bytes.cpu().numpy(), d_lens.cpu().numpy()
    for i, (ts, vals, units, anns) in enumerate(per):
        assert meta[i]["id"] == f"full.{i:03d}".encode()
        if lossless:
            exp = oracle.encode_series(ts, vals, units=units, annotations=anns)
        else:
            exp = oracle.encode_series(ts, vals)
        assert bytes(rows[i, :lens[i]]) == exp, (i, lossless)
    return rows, lens


def test_commitlog_bootstrap_lossless(torch, engine, tmp_path):
    from oracle import commitlog_writer as clw
    per, entries = commitlog_entries(0, 21)
    path = tmp_path / "commitlog-0-0.db"
    clw.write_commitlog(str(path), entries)
    check_bootstrap(torch, per, engine.commitlog_bootstrap_dev(
        torch, str(path), lossless=True), True)
    rows, lens = check_bootstrap(
        torch, per, engine.commitlog_bootstrap_dev(torch, str(path)), False)
    # the default is today's call: the bulk encoder at the default unit
    ts = np.stack([p[0] for p in per])
    vals = np.stack([p[1] for p in per])
    o_rows, o_lens = oracle.encode_batch(ts, vals, np.full(12, 21, np.uint32),
                                         int_optimized=True)
    assert np.array_equal(lens.astype(np.uint32), o_lens)


def test_commitlog_bootstrap_dir_lossless(torch, engine, tmp_path):
    from oracle import commitlog_writer as clw
    per, first = commitlog_entries(0, 9)
    _, second = commitlog_entries(9, 21)
    clw.write_commitlog(str(tmp_path / "commitlog-0-1.db"), second, index=2)
    clw.write_commitlog(str(tmp_path / "commitlog-0-0.db"), first, index=1)
    check_bootstrap(torch, per, engine.commitlog_bootstrap_dir_dev(
        torch, str(tmp_path), lossless=True), True)
    check_bootstrap(torch, per, engine.commitlog_bootstrap_dir_dev(
        torch, str(tmp_path)), False)
