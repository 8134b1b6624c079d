"""Batched StepIter on the GPU: k_step_rows (m3gpu_step_consolidate_batch_dev)
and k_step_fused (m3gpu_decode_steps_batch_dev) against the closed-form model
of step_consolidate_model.py, the reference's tables of
golden/step_consolidator_vectors.json, and each other. Outputs are compared as
uint64 and sit in sentinel-filled buffers with out_pitch = nseries + 3 and a
guard row behind: only the nsteps x nseries cells and errs may change."""
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_full_cases as full_cases  # noqa: E402
import series_iter_model as iter_model  # noqa: E402
import step_consolidate_cases as cases  # noqa: E402
import step_consolidate_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
HERE = os.path.dirname(os.path.abspath(__file__))
SEC = cases.SEC
START = cases.START
EOF = 1
NSERIES = [1, 63, 64, 65, 257]
NSTEPS = [1, 7, 8, 9, 33]  # the step tile is 8: 7, 8, 9 straddle it
GRIDS = cases.grid_cases()


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
    assert hasattr(e.lib(), "m3gpu_step_consolidate_batch_dev")
    assert hasattr(e.lib(), "m3gpu_decode_steps_batch_dev")
    return e


class Guarded:
    """The step matrix and errs in sentinel-filled buffers."""

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


def _assert_matrix(got, exp):
    """exp: per series (step bits, err)."""
    g, e = got
    want = np.array([b for b, _ in exp], dtype=np.uint64).T
    want_e = np.array([x for _, x in exp], dtype=np.int32)
    bad = [i for i in range(len(exp))
           if e[i] != want_e[i] or not np.array_equal(g[:, i], want[:, i])]
    assert not bad, (len(bad), bad[:10], int(e[bad[0]]), int(want_e[bad[0]]),
                     [hex(x) for x in g[:, bad[0]].tolist()],
                     [hex(x) for x in want[:, bad[0]].tolist()])


# ----------------------------- rows kernel -----------------------------

def _rows_batch(seed, nseries, step, nsteps, lookback):
    """Rows [nseries, stride] from the seeded series, counts from 0 to
    stride, plus three crafted out-of-order rows when there is room."""
    series = [list(map(list, s)) for s in
              cases.make_batch(seed, nseries, START, step, nsteps, lookback)]
    t_last = START + (nsteps - 1) * step
    if nseries >= 63:
        series[10] = [[START, START], [1.0, 2.0]]            # equal: error
        series[11] = [[START - 5, START - 6], [1.0, 2.0]]    # smaller: error
        # non-increasing only behind the peeked point: never looked at
        series[12] = [[START, t_last + 1, START], [1.0, 2.0, 3.0]]
    stride = max(2, max(len(ts) for ts, _ in series))
    ts = np.full((nseries, stride), -1, dtype=np.int64)
    vals = np.full((nseries, stride), 12345.0)
    counts = np.zeros(nseries, dtype=np.int32)
    for i, (t, v) in enumerate(series):
        ts[i, :len(t)] = t
        vals[i, :len(t)] = v
        counts[i] = len(t)
    return series, ts, vals, counts


def _run_rows(torch, engine, ts, vals, counts, errs, grid, shift=0):
    start, step, nsteps, lookback = grid
    n, stride = ts.shape

    def moved(a):
        flat = torch.empty(a.size + shift, dtype=torch.from_numpy(a).dtype,
                           device=DEV)
        flat[shift:] = torch.from_numpy(a.reshape(-1)).to(DEV)
        return flat[shift:].view(n, stride)

    d_ts, d_vals = moved(ts), moved(vals)
    assert (d_ts.data_ptr() % 16 == 0) == (shift % 2 == 0)
    g = Guarded(torch, nsteps, n)
    engine.step_consolidate_dev(
        d_ts, d_vals, torch.from_numpy(counts).to(DEV), start, step, nsteps,
        lookback, g.out, g.errs,
        d_errs=None if errs is None else torch.from_numpy(errs).to(DEV))
    torch.cuda.synchronize()
    return g.host()


@pytest.mark.parametrize("nsteps", NSTEPS)
@pytest.mark.parametrize("nseries", NSERIES)
def test_rows_kernel_equals_model(torch, engine, nseries, nsteps):
    step, lookback = GRIDS[(nseries + nsteps) % len(GRIDS)]
    series, ts, vals, counts = _rows_batch(nseries * 100 + nsteps, nseries,
                                           step, nsteps, lookback)
    assert counts.min() == 0 or nseries == 1
    assert counts.max() == ts.shape[1] or nseries == 1
    exp = [model.closed_form(t, v, START, step, nsteps, lookback)
           for t, v in series]
    if nseries >= 63:
        assert exp[10][1] == exp[11][1] == model.OUT_OF_ORDER
        assert exp[12][1] == 0
    got = _run_rows(torch, engine, ts, vals, counts, None,
                    (START, step, nsteps, lookback))
    _assert_matrix(got, exp)


@pytest.mark.parametrize("form", ["rows_plus_8", "odd_stride"])
@pytest.mark.parametrize("with_errs", [False, True])
def test_rows_kernel_alignment_and_row_errors(torch, engine, form, with_errs):
    """Rows 8 bytes off a 16-byte boundary, or an odd stride, take single
    loads. A row error shows exactly when the row has no point past the last
    step."""
    nseries, nsteps = 130, 9
    step, lookback = GRIDS[2]
    series, ts, vals, counts = _rows_batch(5, nseries, step, nsteps, lookback)
    if form == "odd_stride":
        stride = ts.shape[1] | 1
        pad = stride + 2 - ts.shape[1]
        ts = np.pad(ts, ((0, 0), (0, pad)), constant_values=-1)
        vals = np.pad(vals, ((0, 0), (0, pad)), constant_values=7.0)
        assert ts.shape[1] % 2 == 1
    errs = None
    row_errs = np.zeros(nseries, dtype=np.int32)
    if with_errs:
        row_errs[::2] = 3
        errs = row_errs
    exp = [model.closed_form(t, v, START, step, nsteps, lookback,
                             row_err=int(row_errs[i]))
           for i, (t, v) in enumerate(series)]
    if with_errs:
        t_last = START + (nsteps - 1) * step
        even = [i for i in range(0, nseries, 2) if i != 10]  # 10: equal ts
        peeked = [any(x > t_last for x in series[i][0]) for i in even]
        surfaced = [exp[i][1] == 3 for i in even]
        assert any(peeked) and not all(peeked)
        assert all(s != p for s, p in zip(surfaced, peeked))
    got = _run_rows(torch, engine, ts, vals, counts, errs,
                    (START, step, nsteps, lookback),
                    shift=1 if form == "rows_plus_8" else 0)
    _assert_matrix(got, exp)


def test_rows_host_form(engine):
    nseries, nsteps = 5, 9
    step, lookback = GRIDS[0]
    series, ts, vals, counts = _rows_batch(11, nseries, step, nsteps, lookback)
    errs = np.array([0, 4, 0, 0, 4], dtype=np.int32)
    exp = [model.closed_form(t, v, START, step, nsteps, lookback,
                             row_err=int(errs[i]))
           for i, (t, v) in enumerate(series)]
    steps, out_errs = engine.step_consolidate(ts, vals, counts, START, step,
                                              nsteps, lookback, errs=errs)
    assert steps.shape == (nsteps, nseries)
    _assert_matrix((steps.view(np.uint64), out_errs), exp)


# ----------------------------- fused kernel -----------------------------

def _encode(ts, vals, int_optimized, start_ns=None):
    import oracle
    if not len(ts):
        return b""
    ts = np.asarray(ts, dtype=np.int64)
    stream = oracle.encode_series(
        ts, np.asarray(vals, dtype=np.float64),
        units=np.full(len(ts), 4, dtype=np.uint8),
        start_ns=int(ts[0]) if start_ns is None else start_ns,
        int_optimized=int_optimized)
    d = oracle.decode_series(stream, int_optimized=int_optimized)
    assert d["ts"].tolist() == ts.tolist()
    assert d["vals"].view(np.uint64).tolist() == \
        np.asarray(vals, dtype=np.float64).view(np.uint64).tolist()
    return stream


def _split(ts, vals, nblocks, lo, hi):
    """The points cut into nblocks time ranges of [lo, hi)."""
    edges = [lo + (hi - lo) * b // nblocks for b in range(1, nblocks)]
    out = [([], []) for _ in range(nblocks)]
    for t, v in zip(ts, vals):
        b = sum(t >= e for e in edges)
        out[b][0].append(t)
        out[b][1].append(v)
    return out


FUSED_KINDS = ["dense", "fewer_blocks", "leading_empty", "long", "short",
               "eof_surfaces", "eof_hidden", "equal_inside", "smaller_inside",
               "smaller_across", "equal_across", "units_and_annotations",
               "empty", "boundary", "boundary_nan"]


@functools.lru_cache(maxsize=None)
def _fused_batch(nseries, nblocks, nsteps, grid_i, int_optimized):
    """Per series nblocks blocks (stream, ts, vals, err): the stream, the
    points the model is given for it and the error behind them. Series i is
    of kind FUSED_KINDS[i % 15]."""
    step, lookback = GRIDS[grid_i]
    rng = np.random.default_rng(1000 * nseries + 10 * nsteps + nblocks)
    t_last = START + (nsteps - 1) * step
    lo, hi = START - lookback - 2 * step, t_last + 4 * step
    batch = []
    for i in range(nseries):
        kind = FUSED_KINDS[i % len(FUSED_KINDS)]
        blocks = None
        if kind in ("boundary", "boundary_nan", "empty"):
            ts, vals = cases.make_series(rng, START, step, nsteps, lookback,
                                         kind)
        elif kind == "units_and_annotations":
            c = full_cases.series(9000 + i, 17, int_optimized)
            assert len(set(c.units.tolist())) > 1 or c.events
            assert all(a < b for a, b in zip(c.ts, c.ts[1:]))
            blocks = [(c.stream, c.ts.tolist(), c.vals.tolist(), 0)]
            blocks += [(b"", [], [], 0)] * (nblocks - 1)
        elif kind == "long":
            ts = sorted(set((lo + rng.integers(0, hi - lo, size=40 * nsteps +
                                               200)).tolist()))
            vals = rng.integers(0, 9, size=len(ts)).astype(float).tolist()
        elif kind == "short":
            ts, vals = [START + int(rng.integers(0, step))], [4.5]
        elif kind in ("eof_surfaces", "eof_hidden"):
            # six points ending on the last step; "hidden" has 40 more past
            # it, in front of where its last stream is cut short
            ts = sorted({t_last - j * (step // 3) for j in range(6)})
            if kind == "eof_hidden":
                ts += [t_last + 1 + 1000 * j for j in range(40)]
            vals = [float(j % 7) for j in range(len(ts))]
        else:
            ts, vals = cases.make_series(rng, START, step, nsteps, lookback,
                                         "dense")
        if blocks is None:
            parts = _split(ts, vals, nblocks, lo, hi)
            if kind == "fewer_blocks":
                parts = _split(ts, vals, 1, lo, hi) + \
                    [([], [])] * (nblocks - 1)
            elif kind == "leading_empty" and nblocks > 1:
                parts = [([], [])] + _split(ts, vals, nblocks - 1, lo, hi)
            elif kind in ("equal_inside", "smaller_inside", "smaller_across",
                          "equal_across"):
                b0 = min(b for b in range(nblocks) if parts[b][0])
                b_ts, b_vals = parts[b0]
                if kind.endswith("inside"):
                    j = len(b_ts) // 2
                    b_ts.insert(j + 1, b_ts[j] - (kind == "smaller_inside"))
                    b_vals.insert(j + 1, 77.0)
                elif b0 + 1 < nblocks:
                    t = b_ts[-1] - (kind == "smaller_across")
                    parts[b0 + 1] = ([t] + parts[b0 + 1][0],
                                     [88.0] + parts[b0 + 1][1])
            blocks = []
            for b_ts, b_vals in parts:
                stream = _encode(b_ts, b_vals, int_optimized)
                blocks.append((stream, list(b_ts), list(b_vals), 0))
            if kind in ("eof_surfaces", "eof_hidden"):
                last = max(b for b in range(nblocks) if blocks[b][1])
                stream, b_ts, b_vals, _ = blocks[last]
                blocks[last] = (stream[:-3], b_ts, b_vals, EOF)
        batch.append(blocks)
    return batch


def _fused_expected(batch, grid):
    start, step, nsteps, lookback = grid
    exp = []
    for blocks in batch:
        ts, vals, err = model.stitch_blocks(
            [(b[1], b[2], b[3]) for b in blocks])
        exp.append(model.closed_form(ts, vals, start, step, nsteps, lookback,
                                     row_err=err, dedupe=True))
    return exp


def _upload_streams(torch, engine, batch, nblocks):
    """Streams in the order b*nseries + i."""
    streams = [batch[i][b][0] for b in range(nblocks)
               for i in range(len(batch))]
    blob, offsets, lens = engine.pack_streams(streams)
    if not len(blob):
        blob = np.zeros(8, dtype=np.uint8)
    return (torch.from_numpy(blob).to(DEV),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV),
            torch.from_numpy(lens.astype(np.int32)).to(DEV),
            max(2, max(len(b[1]) for bl in batch for b in bl) + 2))


def _run_fused(torch, engine, dev, nseries, nblocks, grid, int_optimized):
    start, step, nsteps, lookback = grid
    g = Guarded(torch, nsteps, nseries)
    engine.decode_steps_dev(dev[0], dev[1], dev[2], nblocks, start, step,
                            nsteps, lookback, g.out, g.errs,
                            int_optimized=int_optimized)
    torch.cuda.synchronize()
    return g.host()


def _run_composed(torch, engine, dev, nseries, nblocks, grid, int_optimized):
    """decode -> series merge (one replica, no range) -> rows kernel, with
    the decode errors of absent blocks (zero-length streams) cleared."""
    start, step, nsteps, lookback = grid
    d_blob, d_offsets, d_lens, stride = dev
    stride = (stride + 1) & ~1
    nrows = nseries * nblocks
    r_ts = torch.empty((nrows, stride), dtype=torch.int64, device=DEV)
    r_vals = torch.empty((nrows, stride), dtype=torch.float64, device=DEV)
    r_counts = torch.empty(nrows, dtype=torch.int32, device=DEV)
    r_errs = torch.empty(nrows, dtype=torch.int32, device=DEV)
    engine.decode_batch_dev(d_blob, d_offsets, d_lens, r_ts, r_vals, r_counts,
                            r_errs, int_optimized=int_optimized)
    r_errs.masked_fill_(d_lens == 0, 0)
    out_stride = nblocks * stride
    m_ts = torch.empty((nseries, out_stride), dtype=torch.int64, device=DEV)
    m_vals = torch.empty((nseries, out_stride), dtype=torch.float64,
                         device=DEV)
    m_counts = torch.empty(nseries, dtype=torch.int32, device=DEV)
    m_errs = torch.empty(nseries, dtype=torch.int32, device=DEV)
    engine.series_merge_dev(r_ts, r_vals, r_counts, 1, nblocks, m_ts, m_vals,
                            m_counts, m_errs, d_errs=r_errs)
    g = Guarded(torch, nsteps, nseries)
    engine.step_consolidate_dev(m_ts, m_vals, m_counts, start, step, nsteps,
                                lookback, g.out, g.errs, d_errs=m_errs)
    torch.cuda.synchronize()
    return g.host()


@pytest.mark.parametrize("nsteps", NSTEPS)
@pytest.mark.parametrize("nseries", NSERIES)
def test_fused_kernel_equals_model_and_composed_path(torch, engine, nseries,
                                                     nsteps):
    k = NSERIES.index(nseries) + NSTEPS.index(nsteps)
    nblocks = 3 if k % 2 else 1
    int_optimized = (k // 2) % 2 == 0
    grid_i = k % len(GRIDS)
    grid = (START, GRIDS[grid_i][0], nsteps, GRIDS[grid_i][1])
    batch = _fused_batch(nseries, nblocks, nsteps, grid_i, int_optimized)
    exp = _fused_expected(batch, grid)
    dev = _upload_streams(torch, engine, batch, nblocks)
    fused = _run_fused(torch, engine, dev, nseries, nblocks, grid,
                       int_optimized)
    _assert_matrix(fused, exp)
    composed = _run_composed(torch, engine, dev, nseries, nblocks, grid,
                             int_optimized)
    assert np.array_equal(fused[0], composed[0])
    assert np.array_equal(fused[1], composed[1])


@pytest.mark.parametrize("int_optimized", [True, False])
@pytest.mark.parametrize("nblocks", [1, 3])
def test_fused_kernel_crafted_series(torch, engine, nblocks, int_optimized):
    """Each crafted kind gives what its name says, next to untouched
    neighbours (every series is compared with the model)."""
    nseries, nsteps, grid_i = 65, 9, 2
    grid = (START, GRIDS[grid_i][0], nsteps, GRIDS[grid_i][1])
    batch = _fused_batch(nseries, nblocks, nsteps, grid_i, int_optimized)
    exp = _fused_expected(batch, grid)
    dev = _upload_streams(torch, engine, batch, nblocks)
    got = _run_fused(torch, engine, dev, nseries, nblocks, grid,
                     int_optimized)
    _assert_matrix(got, exp)
    composed = _run_composed(torch, engine, dev, nseries, nblocks, grid,
                             int_optimized)
    assert np.array_equal(got[0], composed[0])
    assert np.array_equal(got[1], composed[1])
    kind = {k: FUSED_KINDS.index(k) for k in FUSED_KINDS}
    nan_col = np.full(nsteps, model.NAN_BITS, dtype=np.uint64)
    i = kind["eof_surfaces"]
    assert got[1][i] == EOF and np.array_equal(got[0][:, i], nan_col)
    i = kind["eof_hidden"]
    assert got[1][i] == 0 and np.any(got[0][:, i] != model.NAN_BITS)
    i = kind["equal_inside"]
    assert got[1][i] == 0 and np.any(got[0][:, i] != model.NAN_BITS)
    i = kind["smaller_inside"]
    assert got[1][i] == model.OUT_OF_ORDER
    assert np.array_equal(got[0][:, i], nan_col)
    if nblocks > 1:
        i = kind["smaller_across"]
        assert got[1][i] == model.OUT_OF_ORDER
        assert np.array_equal(got[0][:, i], nan_col)
        assert got[1][kind["equal_across"]] == 0
        assert not batch[kind["leading_empty"]][0][0]
        assert not batch[kind["fewer_blocks"]][nblocks - 1][0]
    i = kind["units_and_annotations"]
    assert got[1][i] == 0 and np.any(got[0][:, i] != model.NAN_BITS)
    lens = sorted(sum(len(b[1]) for b in bl) for bl in batch)
    assert lens[-1] > 10 * max(1, lens[len(lens) // 2])


# ----------------------------- golden fixture -----------------------------

with open(os.path.join(HERE, "golden", "step_consolidator_vectors.json")) as f:
    GOLDEN = json.load(f)


@pytest.mark.parametrize("table", GOLDEN["tables"], ids=lambda t: t["name"])
def test_golden_tables(torch, engine, table):
    """The fixture's blocks, oracle-encoded, empty blocks as zero-length
    streams, nblocks = 5, through the fused entry and through decode ->
    series merge -> rows entry: the reference's tables."""
    import oracle
    start = GOLDEN["start_seconds"] * SEC
    block = GOLDEN["block_seconds"] * SEC
    nblocks = 5
    batch = []
    for blocks in GOLDEN["series"]:
        row = []
        for b in range(nblocks):
            pts = blocks[b] if b < len(blocks) else []
            ts = [start + b * block + off * SEC for _, off in pts]
            vals = [float(v) for v, _ in pts]
            stream = oracle.encode_series(
                ts, vals, start_ns=start + b * block) if pts else b""
            row.append((stream, ts, vals, 0))
        batch.append(row)
    step = table["step_seconds"] * SEC
    nsteps = len(table["expected"])
    assert nsteps * step == nblocks * block
    grid = (start, step, nsteps, GOLDEN["lookback_seconds"] * SEC)
    exp = [([model.NAN_BITS if r[i] is None else model.bits(float(r[i]))
             for r in table["expected"]], 0) for i in range(3)]
    dev = _upload_streams(torch, engine, batch, nblocks)
    _assert_matrix(_run_fused(torch, engine, dev, 3, nblocks, grid, True), exp)
    _assert_matrix(_run_composed(torch, engine, dev, 3, nblocks, grid, True),
                   exp)


# ----------------------------- fetch_steps_dev -----------------------------

def test_fetch_steps_three_replicas(torch, engine):
    """nreplicas = 3: the model run on what the Python SeriesIterator model
    yields for the decoded replicas."""
    nseries, nblocks, nsteps, R = 65, 2, 17, 3
    step, lookback = GRIDS[0]
    rng = np.random.default_rng(42)
    t_last = START + (nsteps - 1) * step
    lo, hi = START - lookback - step, t_last + 3 * step
    streams = {}
    exp = []
    for i in range(nseries):
        ts, _ = cases.make_series(rng, START, step, nsteps, lookback, "dense")
        replicas = []
        for r in range(R):
            keep = [t for t in ts if rng.random() < 0.7]
            vals = [float(rng.integers(0, 5)) for _ in keep]
            parts = _split(keep, vals, nblocks, lo, hi)
            blocks = []
            for b, (b_ts, b_vals) in enumerate(parts):
                streams[(r, b, i)] = _encode(b_ts, b_vals, True)
                blocks.append((b_ts, b_vals, [4] * len(b_ts), 0))
            replicas.append(blocks)
        m_ts, m_vals, _, m_err = iter_model.series_iterate(replicas)
        exp.append(model.closed_form(m_ts, m_vals, START, step, nsteps,
                                     lookback, row_err=m_err))
    order = [streams[(r, b, i)] for r in range(R) for b in range(nblocks)
             for i in range(nseries)]
    blob, offsets, lens = engine.pack_streams(order)
    out = engine.fetch_steps_dev(
        torch, torch.from_numpy(blob).to(DEV),
        torch.from_numpy(offsets.astype(np.int64)).to(DEV),
        torch.from_numpy(lens.astype(np.int32)).to(DEV), R, nblocks,
        4 * nsteps + 4, START, step, nsteps, lookback)
    torch.cuda.synchronize()
    assert out["steps"].shape == (nsteps, nseries)
    got = (out["steps"].cpu().numpy().view(np.uint64),
           out["errs"].cpu().numpy())
    _assert_matrix(got, exp)
    assert sum(int(np.sum(g != model.NAN_BITS)) for g in got[0]) > nseries


def test_fetch_steps_one_replica_is_the_fused_entry(torch, engine):
    nseries, nblocks, nsteps, grid_i = 65, 3, 9, 2
    grid = (START, GRIDS[grid_i][0], nsteps, GRIDS[grid_i][1])
    batch = _fused_batch(nseries, nblocks, nsteps, grid_i, True)
    dev = _upload_streams(torch, engine, batch, nblocks)
    fused = _run_fused(torch, engine, dev, nseries, nblocks, grid, True)
    out = engine.fetch_steps_dev(torch, dev[0], dev[1], dev[2], 1, nblocks,
                                 dev[3], *grid)
    torch.cuda.synchronize()
    assert np.array_equal(out["steps"].cpu().numpy().view(np.uint64), fused[0])
    assert np.array_equal(out["errs"].cpu().numpy(), fused[1])
    assert np.any(fused[1] != 0) and np.any(fused[1] == 0)


def test_streams_host_form(engine):
    nseries, nblocks, nsteps, grid_i = 15, 3, 9, 2
    grid = (START, GRIDS[grid_i][0], nsteps, GRIDS[grid_i][1])
    batch = _fused_batch(nseries, nblocks, nsteps, grid_i, True)
    exp = _fused_expected(batch, grid)
    streams = [batch[i][b][0] for b in range(nblocks) for i in range(nseries)]
    blob, offsets, lens = engine.pack_streams(streams)
    pitch = nseries + 3
    out = np.full((nsteps, pitch), -5.0)
    errs = np.full(nseries, -77, dtype=np.int32)
    P = ctypes.POINTER
    rc = engine.lib().m3gpu_decode_steps_batch(
        blob.ctypes.data_as(P(ctypes.c_uint8)), len(blob),
        offsets.ctypes.data_as(P(ctypes.c_uint64)),
        lens.ctypes.data_as(P(ctypes.c_uint32)), nseries, nblocks, 1, 1,
        grid[0], grid[1], grid[2], grid[3],
        out.ctypes.data_as(P(ctypes.c_double)), pitch,
        errs.ctypes.data_as(P(ctypes.c_int32)))
    assert rc == 0
    assert np.all(out[:, nseries:] == -5.0)
    _assert_matrix((np.ascontiguousarray(out[:, :nseries]).view(np.uint64),
                    errs), exp)
