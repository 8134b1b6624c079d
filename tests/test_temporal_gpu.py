"""Batched temporal functions on the GPU: k_temporal_rows
(m3gpu_temporal_batch_dev) against the closed-form model of temporal_model.py
on the seeded series of temporal_cases.py, the reference's tables of
golden/temporal_vectors.json, and the fetch and host forms. Where the model
holds a number the cell's uint64 must equal it (signed zeros count); where it
holds a NaN the cell is a NaN; where the reference returned math.NaN()
itself the cell is NAN_BITS exactly; last_over_time hands an input NaN on
bit for bit. Outputs sit in sentinel-filled buffers with out_pitch = nseries
+ 3 and a guard row behind: only the nsteps x nseries cells and errs may
change."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import temporal_cases as cases  # noqa: E402
import temporal_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
HERE = os.path.dirname(os.path.abspath(__file__))
SEC = cases.SEC
START = cases.START
EOF = 1
PARAM = 37.5  # predict_linear's seconds
NSERIES = [1, 63, 64, 65, 257]
NSTEPS = [1, 7, 8, 9, 33]  # the step tile is 8: 7, 8, 9 straddle it
GRIDS = cases.grid_cases()
PAYLOAD_NAN = 0x7FF80000DEADBEEF

with open(os.path.join(HERE, "golden", "temporal_vectors.json")) as f:
    GOLDEN = json.load(f)


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
    assert hasattr(e.lib(), "m3gpu_temporal_batch_dev")
    return e


def ring_depth():
    from m3_amd import engine as e
    return e.lib().m3gpu_temporal_ring_depth()


class Guarded:
    """The matrix and errs in sentinel-filled buffers."""

    def __init__(self, torch, nsteps, nseries):
        self.nsteps, self.nseries = nsteps, nseries
        self.pitch = nseries + 3
        self.flat = torch.full(((nsteps + 1) * self.pitch,), SENTINEL,
                               dtype=torch.int64, device=DEV)
        self.out = self.flat.view(torch.float64).view(
            nsteps + 1, self.pitch)[:nsteps]
        self.eflat = torch.full((nseries + 1,), -77, dtype=torch.int32,
                                device=DEV)
        self.errs = self.eflat[:nseries]

    def host(self):
        """(uint64 [nsteps, nseries], errs) after checking every guard."""
        m = self.flat.cpu().numpy().view(np.uint64).reshape(
            self.nsteps + 1, self.pitch)
        assert np.all(m[:, self.nseries:] == SENTINEL), "pitch padding written"
        assert np.all(m[self.nsteps] == SENTINEL), "guard row written"
        e = self.eflat.cpu().numpy()
        assert e[self.nseries] == -77
        return m[:self.nsteps, :self.nseries].copy(), e[:self.nseries].copy()


def _assert_cells(got, exp_cells, exp_errs, what, exact_nan=False):
    """exp_cells: per series a list of (bits, literal)."""
    g, e = got
    want = np.array([[b for b, _ in col] for col in exp_cells],
                    dtype=np.uint64).T.reshape(g.shape)
    literal = np.array([[lit for _, lit in col] for col in exp_cells],
                       dtype=bool).T.reshape(g.shape)
    want_nan = np.isnan(want.view(np.float64))
    got_nan = np.isnan(g.view(np.float64))
    ok = np.where(want_nan, got_nan, g == want)
    ok &= ~literal | (g == model.NAN_BITS)
    if exact_nan:
        ok &= g == want
    bad_e = np.nonzero(e != np.asarray(exp_errs, dtype=np.int32))[0]
    assert not len(bad_e), (what, bad_e[:10], e[bad_e[:10]])
    bad = np.argwhere(~ok)
    assert not len(bad), (what, len(bad), bad[:5].tolist(),
                          [(hex(g[k, i]), hex(want[k, i]), literal[k, i])
                           for k, i in bad[:5]])


# ------------------------------ the rows ------------------------------

def _rows_batch(seed, nseries, step, nsteps, range_ns):
    """Rows [nseries, stride] from the seeded series, counts from 0 to
    stride, plus crafted rows when there is room: out of order in front of
    and behind the first point past t_last, and NaNs with a payload."""
    series = [list(map(list, s)) for s in cases.make_batch(
        seed, nseries, START, step, nsteps, range_ns, ring_depth())]
    t_last = START + (nsteps - 1) * step
    if nseries >= 63:
        series[14] = [[START, START], [1.5, 2.5]]            # equal: error
        series[15] = [[START - 5, START - 6], [1.5, 2.5]]    # smaller: error
        # non-increasing only behind the first point past t_last: not seen
        series[16] = [[START - 1, START, t_last + 1, START], [1.5, 2.5, 3.5,
                                                              4.5]]
        # equal timestamps behind a clean start
        series[17] = [[START - 1, START, START], [1.5, 2.5, 3.5]]
        nan = model.from_bits(PAYLOAD_NAN)
        series[18] = [[START - 2, START - 1, START], [0.75, nan, nan]]
    stride = max(2, max(len(ts) for ts, _ in series))
    ts = np.full((nseries, stride), -1, dtype=np.int64)
    vals = np.full((nseries, stride), 12345.0)
    counts = np.zeros(nseries, dtype=np.int32)
    for i, (t, v) in enumerate(series):
        ts[i, :len(t)] = t
        vals[i, :len(t)] = v
        counts[i] = len(t)
    return series, ts, vals, counts


@functools.lru_cache(maxsize=None)
def _case(seed, nseries, grid_i, nsteps, err_every=0):
    """The rows of one case and what every function gives for them: computed
    once, shared, never changed."""
    step, range_ns = GRIDS[grid_i]
    series, ts, vals, counts = _rows_batch(seed, nseries, step, nsteps,
                                           range_ns)
    row_errs = np.zeros(nseries, dtype=np.int32)
    if err_every:
        row_errs[::err_every] = 3
    cells = {fn: [] for fn in model.FNS}
    errs = []
    for i, (t, v) in enumerate(series):
        many, err = model.closed_form_many(
            model.FNS, t, v, START, step, nsteps, range_ns, param=PARAM,
            row_err=int(row_errs[i]))
        for fn in model.FNS:
            cells[fn].append(many[fn])
        errs.append(err)
    for a in (ts, vals, counts, row_errs):
        a.setflags(write=False)
    return series, ts, vals, counts, row_errs, cells, errs


def _upload(torch, ts, vals, counts, shift=0):
    n, stride = ts.shape

    def moved(a):
        flat = torch.empty(a.size + shift, dtype=torch.from_numpy(a).dtype,
                           device=DEV)
        flat[shift:] = torch.from_numpy(a.reshape(-1)).to(DEV)
        return flat[shift:].view(n, stride)

    d_ts, d_vals = moved(np.array(ts)), moved(np.array(vals))
    assert (d_ts.data_ptr() % 16 == 0) == (shift % 2 == 0)
    return d_ts, d_vals, torch.from_numpy(np.array(counts)).to(DEV)


def _run(torch, engine, dev, grid, fn, d_errs=None, param=PARAM):
    start, step, nsteps, range_ns = grid
    g = Guarded(torch, nsteps, dev[2].numel())
    engine.temporal_dev(dev[0], dev[1], dev[2], start, step, nsteps,
                        range_ns, fn, g.out, g.errs, d_errs=d_errs,
                        param=param)
    torch.cuda.synchronize()
    return g.host()


@pytest.mark.parametrize("nsteps", NSTEPS)
@pytest.mark.parametrize("nseries", NSERIES)
def test_kernel_equals_model(torch, engine, nseries, nsteps):
    """Every function over the same rows; the grid (range >, == and < step)
    goes round with the shape."""
    grid_i = (NSERIES.index(nseries) + NSTEPS.index(nsteps)) % len(GRIDS)
    step, range_ns = GRIDS[grid_i]
    series, ts, vals, counts, _, cells, errs = _case(
        nseries * 100 + nsteps, nseries, grid_i, nsteps)
    assert counts.min() == 0 or nseries == 1
    assert counts.max() == ts.shape[1] or nseries == 1
    if nseries >= 63:
        assert errs[14] == errs[15] == errs[17] == model.OUT_OF_ORDER
        assert errs[16] == 0
    dev = _upload(torch, ts, vals, counts)
    for fn in model.FNS:
        got = _run(torch, engine, dev, (START, step, nsteps, range_ns), fn)
        _assert_cells(got, cells[fn], errs, fn,
                      exact_nan=fn == "last_over_time")
        if nseries >= 63 and fn == "last_over_time":
            assert got[0][0, 18] == PAYLOAD_NAN
        if nseries >= 63:
            # a failed series next to clean ones
            assert np.all(got[0][:, 14] == model.NAN_BITS)
            assert got[1][13] == 0 and got[1][16] == 0


def test_windows_cross_the_ring(torch, engine):
    """Windows of 0, 1, 2, C-1, C, C+1 and 3C points for the ring depth C
    that was built: 3C reaches from LDS into global memory."""
    ring = ring_depth()
    step, range_ns = GRIDS[2]  # range < step: a window is one cluster
    nsteps, nseries = 33, 70
    rng = np.random.default_rng(9)
    series = [cases.make_series(rng, START, step, nsteps, range_ns, "windows",
                                ring) for _ in range(nseries)]
    wins, _ = model.windows(*series[0], START, step, nsteps, range_ns)
    assert set(cases.window_sizes(ring)) <= {len(w) for w in wins}
    stride = max(len(t) for t, _ in series)
    ts = np.full((nseries, stride), -1, dtype=np.int64)
    vals = np.full((nseries, stride), 12345.0)
    counts = np.zeros(nseries, dtype=np.int32)
    for i, (t, v) in enumerate(series):
        ts[i, :len(t)], vals[i, :len(t)], counts[i] = t, v, len(t)
    dev = _upload(torch, ts, vals, counts)
    exp = [model.closed_form_many(model.FNS, t, v, START, step, nsteps,
                                  range_ns, param=PARAM)[0]
           for t, v in series]
    for fn in model.FNS:
        got = _run(torch, engine, dev, (START, step, nsteps, range_ns), fn)
        _assert_cells(got, [e[fn] for e in exp], [0] * nseries, fn,
                      exact_nan=fn == "last_over_time")


@pytest.mark.parametrize("form", ["rows_plus_8", "odd_stride"])
@pytest.mark.parametrize("with_errs", [False, True])
def test_load_forms_and_row_errors(torch, engine, form, with_errs):
    """Rows 8 bytes off a 16-byte boundary, or an odd stride, take single
    loads. A row error fails its series wherever its points lie, and its
    neighbours are untouched."""
    nseries, nsteps, grid_i = 130, 9, 0
    step, range_ns = GRIDS[grid_i]
    series, ts, vals, counts, row_errs, cells, errs = _case(
        5, nseries, grid_i, nsteps, err_every=2 if with_errs else 0)
    if form == "odd_stride":
        pad = (ts.shape[1] | 1) + 2 - ts.shape[1]
        ts = np.pad(ts, ((0, 0), (0, pad)), constant_values=-1)
        vals = np.pad(vals, ((0, 0), (0, pad)), constant_values=7.0)
        assert ts.shape[1] % 2 == 1
    if with_errs:
        t_last = START + (nsteps - 1) * step
        even = range(0, nseries, 2)
        assert all(errs[i] == 3 for i in even)
        # with and without points past the last step
        assert any(any(x > t_last for x in series[i][0]) for i in even)
        assert any(all(x <= t_last for x in series[i][0]) for i in even)
        assert sum(errs[i] == 0 for i in range(1, nseries, 2)) > 50
    dev = _upload(torch, ts, vals, counts,
                  shift=1 if form == "rows_plus_8" else 0)
    d_errs = torch.from_numpy(np.array(row_errs)).to(DEV) if with_errs \
        else None
    for fn in model.FNS:
        got = _run(torch, engine, dev, (START, step, nsteps, range_ns), fn,
                   d_errs=d_errs)
        _assert_cells(got, cells[fn], errs, fn,
                      exact_nan=fn == "last_over_time")


def test_host_form_equals_device_form(torch, engine):
    nseries, nsteps, grid_i = 65, 9, 0
    step, range_ns = GRIDS[grid_i]
    _, ts, vals, counts, row_errs, cells, errs = _case(7, nseries, grid_i,
                                                       nsteps, err_every=5)
    dev = _upload(torch, ts, vals, counts)
    d_errs = torch.from_numpy(np.array(row_errs)).to(DEV)
    for fn in ("rate", "stddev_over_time", "predict_linear", "changes"):
        got = _run(torch, engine, dev, (START, step, nsteps, range_ns), fn,
                   d_errs=d_errs)
        steps, out_errs = engine.temporal(ts, vals, counts, START, step,
                                          nsteps, range_ns, fn,
                                          errs=row_errs, param=PARAM)
        assert steps.shape == (nsteps, nseries)
        assert np.array_equal(steps.view(np.uint64), got[0]), fn
        assert np.array_equal(out_errs, got[1])
        _assert_cells((steps.view(np.uint64), out_errs), cells[fn], errs, fn)


# ----------------------------- golden fixture -----------------------------

@pytest.mark.parametrize("table", GOLDEN["tables"], ids=lambda t: t["name"])
def test_golden_tables(torch, engine, table):
    step = GOLDEN["step_seconds"] * SEC
    nsteps = GOLDEN["nsteps"]
    grid = (START, step, nsteps, GOLDEN["range_seconds"] * SEC)
    param = GOLDEN["predict_linear_seconds"]
    n = len(table["vals"][0])
    ts = np.array([[START + i * step + GOLDEN["point_offset_ns"]
                    for i in range(n)]] * 2, dtype=np.int64)
    vals = np.array([[math.nan if v is None else float(v) for v in row]
                     for row in table["vals"]])
    counts = np.full(2, n, dtype=np.int32)
    got, errs = _run(torch, engine, _upload(torch, ts, vals, counts), grid,
                     table["fn"], param=param)
    assert errs.tolist() == [0, 0]
    exp = [model.closed_form(table["fn"], ts[i].tolist(), vals[i].tolist(),
                             *grid, param=param)[0] for i in range(2)]
    _assert_cells((got, errs), exp, [0, 0], table["name"])
    for i in range(2):
        for k, want in enumerate(table["expected"][i]):
            cell = float(got[k, i:i + 1].view(np.float64)[0])
            if want is None:
                assert math.isnan(cell), (i, k, cell)
            else:
                assert GOLDEN["compare_delta"] > abs(want - cell), (i, k,
                                                                    cell)


# --------------------------- fetch_temporal_dev ---------------------------

def _encode(ts, vals):
    import oracle
    if not len(ts):
        return b""
    ts = np.asarray(ts, dtype=np.int64)
    stream = oracle.encode_series(
        ts, np.asarray(vals, dtype=np.float64),
        units=np.full(len(ts), 4, dtype=np.uint8), start_ns=int(ts[0]),
        int_optimized=True)
    d = oracle.decode_series(stream, int_optimized=True)
    assert d["ts"].tolist() == ts.tolist()
    return stream


def _dev_streams(torch, engine, streams):
    blob, offsets, lens = engine.pack_streams(streams)
    return (torch.from_numpy(blob).to(DEV),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV),
            torch.from_numpy(lens.astype(np.int32)).to(DEV))


def _model_over_rows(rows, grid, fn):
    """The closed form over what fetch_series_dev yields."""
    ts = rows["ts"].cpu().numpy()
    vals = rows["vals"].cpu().numpy()
    counts = rows["counts"].cpu().numpy()
    errs = rows["errs"].cpu().numpy()
    cells, out_errs = [], []
    for i in range(len(counts)):
        c, e = model.closed_form(fn, ts[i, :counts[i]].tolist(),
                                 vals[i, :counts[i]].tolist(), *grid,
                                 param=PARAM, row_err=int(errs[i]))
        cells.append(c)
        out_errs.append(e)
    return cells, out_errs


def test_fetch_temporal_three_replicas(torch, engine):
    nseries, nblocks, nsteps, R = 65, 2, 17, 3
    step, range_ns = GRIDS[0]
    grid = (START, step, nsteps, range_ns)
    rng = np.random.default_rng(42)
    lo = START - range_ns - 2 * step
    mid = START + (nsteps // 2) * step + 1
    streams = {}
    for i in range(nseries):
        ts, vals = cases.make_series(rng, START, step, nsteps, range_ns,
                                     "counter" if i % 2 else "dense")
        for r in range(R):
            keep = [(t, v) for t, v in zip(ts, vals) if rng.random() < 0.7]
            for b in range(nblocks):
                part = [(t, v) for t, v in keep if (t >= mid) == bool(b)]
                if not part:  # no absent blocks here: see the next test
                    part = [(mid if b else lo, 0.5)]
                streams[(r, b, i)] = _encode(*zip(*part))
    order = [streams[(r, b, i)] for r in range(R) for b in range(nblocks)
             for i in range(nseries)]
    dev = _dev_streams(torch, engine, order)
    stride = 8 * nsteps + 16
    rows = engine.fetch_series_dev(torch, *dev, R, nblocks, stride)
    for fn in ("rate", "avg_over_time", "deriv"):
        out = engine.fetch_temporal_dev(torch, *dev, R, nblocks, stride,
                                        *grid, fn, param=PARAM)
        torch.cuda.synchronize()
        assert out["steps"].shape == (nsteps, nseries)
        cells, errs = _model_over_rows(rows, grid, fn)
        got = (out["steps"].cpu().numpy().view(np.uint64),
               out["errs"].cpu().numpy())
        _assert_cells(got, cells, errs, fn)
        assert not any(errs)
        assert np.sum(~np.isnan(out["steps"].cpu().numpy())) > \
            nsteps * nseries // 2


def test_fetch_temporal_one_replica_one_block(torch, engine):
    """1 x 1 skips the merge. A truncated stream fails its series, a
    zero-length one is an absent block: no points and no error."""
    nseries, nsteps = 66, 9
    step, range_ns = GRIDS[0]
    grid = (START, step, nsteps, range_ns)
    rng = np.random.default_rng(43)
    streams = []
    for i in range(nseries):
        ts, vals = cases.make_series(rng, START, step, nsteps, range_ns,
                                     "dense")
        streams.append(_encode(ts, vals))
    streams[3] = streams[3][:-3]
    dev = _dev_streams(torch, engine, streams)
    stride = 8 * nsteps + 17
    rows = engine.fetch_series_dev(torch, *dev, 1, 1, stride)
    for fn in ("increase", "max_over_time"):
        out = engine.fetch_temporal_dev(torch, *dev, 1, 1, stride, *grid, fn)
        torch.cuda.synchronize()
        cells, errs = _model_over_rows(rows, grid, fn)
        assert errs[3] == EOF and sum(map(bool, errs)) == 1
        got = (out["steps"].cpu().numpy().view(np.uint64),
               out["errs"].cpu().numpy())
        _assert_cells(got, cells, errs, fn)
    streams[5] = b""
    dev = _dev_streams(torch, engine, streams)
    out = engine.fetch_temporal_dev(torch, *dev, 1, 1, stride, *grid,
                                    "sum_over_time")
    torch.cuda.synchronize()
    errs = out["errs"].cpu().numpy()
    steps = out["steps"].cpu().numpy().view(np.uint64)
    assert errs[5] == 0 and np.all(steps[:, 5] == model.NAN_BITS)
    assert errs[3] == EOF and errs[4] == 0
    assert np.any(steps[:, 4] != model.NAN_BITS)
