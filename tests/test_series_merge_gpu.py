"""Batched SeriesIterator on the GPU (m3gpu_series_merge_batch_dev,
k_series_merge): the kernel against the Python model of series_iter_model.py
on the generated batches of series_merge_cases.py (what they contain is
checked in test_series_iter_cpu.py). Every output sits in sentinel-filled
buffers with a guard row behind, the units at an odd address with three guard
bytes in front, and nothing past a series' count may change."""
import base64
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import series_iter_model as model  # noqa: E402
import series_merge_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
USENT = 0xA5
CAPACITY = 6
HERE = os.path.dirname(os.path.abspath(__file__))


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
    assert hasattr(e.lib(), "m3gpu_series_merge_batch_dev")
    return e


_dev_cache = {}


def _inputs(torch, bt):
    """The batch's rows on the device, uploaded once per (R, B)."""
    key = (bt.R, bt.B)
    if key not in _dev_cache:
        S = bt.stride
        _dev_cache[key] = (
            torch.from_numpy(bt.ts.reshape(-1, S).copy()).to(DEV),
            torch.from_numpy(bt.vals.reshape(-1, S).copy()).to(DEV),
            torch.from_numpy(bt.units.reshape(-1, S).copy()).to(DEV),
            torch.from_numpy(bt.counts.reshape(-1).astype(np.int32)).to(DEV),
            torch.from_numpy(bt.errs.reshape(-1).copy()).to(DEV))
    return _dev_cache[key]


def _even_out_stride(exp):
    return (max(len(e[0]) for e in exp) + 3) & ~1


def _run(torch, engine, bt, start, end, strategy, out_stride, shift=0,
         inputs=None):
    """Merge the batch into guarded buffers; `shift` moves the ts and vals
    rows by that many elements off the allocation's (16-byte aligned) base.
    Returns host arrays: ts, val bits, units (with guard rows), counts, errs,
    and the unit guard bytes."""
    d_ts, d_vals, d_units, d_counts, d_errs = inputs or _inputs(torch, bt)
    N = bt.nseries
    rows = (N + 1) * out_stride
    f_ts = torch.full((shift + rows,), SENTINEL, dtype=torch.int64, device=DEV)
    f_vals = torch.full((shift + rows,), SENTINEL, dtype=torch.int64,
                        device=DEV)
    f_units = torch.full((3 + rows,), USENT, dtype=torch.uint8, device=DEV)
    o_ts = f_ts[shift:].view(N + 1, out_stride)
    o_vals = f_vals[shift:].view(torch.float64).view(N + 1, out_stride)
    o_units = f_units[3:].view(N + 1, out_stride)
    o_counts = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    o_errs = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    assert (o_ts.data_ptr() % 16 == 0) == (shift % 2 == 0)
    assert o_units.data_ptr() % 2 == 1
    engine.series_merge_dev(d_ts, d_vals, d_counts, bt.R, bt.B, o_ts[:N],
                            o_vals[:N], o_counts, o_errs, d_units=d_units,
                            out_units=o_units[:N], d_errs=d_errs,
                            start_ns=start, end_ns=end, strategy=strategy)
    torch.cuda.synchronize()
    h_ts = f_ts.cpu().numpy()
    h_vals = f_vals.cpu().numpy()
    h_units = f_units.cpu().numpy()
    assert np.all(h_ts[:shift] == SENTINEL) and np.all(h_vals[:shift] == SENTINEL)
    assert np.all(h_units[:3] == USENT)
    return (h_ts[shift:].reshape(N + 1, out_stride),
            h_vals[shift:].reshape(N + 1, out_stride).view(np.uint64),
            h_units[3:].reshape(N + 1, out_stride),
            o_counts.cpu().numpy(), o_errs.cpu().numpy())


def _capped(exp, out_stride):
    """The model's row under an out_stride: CAPACITY when a further point
    was due, with the stored prefix."""
    ts, vals, units, err = exp
    if len(ts) > out_stride:
        return ts[:out_stride], vals[:out_stride], units[:out_stride], CAPACITY
    return exp


def _check(got, exp, out_stride):
    g_ts, g_vals, g_units, g_counts, g_errs = got
    N = len(exp)
    bad = []
    for i in range(N):
        m_ts, m_vals, m_units, m_err = _capped(exp[i], out_stride)
        n = len(m_ts)
        ok = (g_counts[i] == n and g_errs[i] == m_err and
              g_ts[i, :n].tolist() == m_ts and
              g_vals[i, :n].tolist() == cases.bits(m_vals) and
              g_units[i, :n].tolist() == m_units and
              np.all(g_ts[i, n:] == SENTINEL) and
              np.all(g_vals[i, n:] == SENTINEL) and
              np.all(g_units[i, n:] == USENT))
        if not ok:
            bad.append(i)
    assert not bad, (len(bad), bad[:10], int(g_counts[bad[0]]),
                     int(g_errs[bad[0]]), g_ts[bad[0]].tolist(),
                     _capped(exp[bad[0]], out_stride))
    assert np.all(g_ts[N] == SENTINEL) and np.all(g_vals[N] == SENTINEL)
    assert np.all(g_units[N] == USENT)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("strategy", [0, 1, 2, 3])
def test_kernel_equals_model(torch, engine, strategy, R, B):
    bt = cases.make_batch(R, B)
    exp = cases.expected(R, B, 0, 0, strategy)
    out_stride = _even_out_stride(exp)
    _check(_run(torch, engine, bt, 0, 0, strategy, out_stride), exp,
           out_stride)


def _keys(exp):
    """Expectations in a form == can compare (NaN values as bits)."""
    return [(ts, cases.bits(vals), units, err) for ts, vals, units, err in exp]


S = cases.SEC
FILTERS = {
    # 5 s is a point of many series (kept), 8 s too (dropped)
    "on_points": (cases.FILTER_START, cases.FILTER_END),
    "no_start": (0, cases.FILTER_END),          # filter off
    "no_end": (cases.FILTER_START, 0),          # filter off
    "before_all_data": (cases.BASE - 100 * S, cases.BASE - 50 * S),
    "across_blocks": (cases.BASE + 7 * S, cases.BASE + 33 * S),
}


@pytest.mark.parametrize("R,B", [(2, 1), (4, 3)])
@pytest.mark.parametrize("name", list(FILTERS))
def test_filter(torch, engine, name, R, B):
    start, end = FILTERS[name]
    bt = cases.make_batch(R, B)
    exp = cases.expected(R, B, start, end, 0)
    off = cases.expected(R, B, 0, 0, 0)
    i = bt.names["filter"]
    if name == "on_points":
        # start on a point keeps it, end on a point drops it, and replica 1
        # is dropped at its 9 while replica 0 goes on: its 6 is never seen
        assert exp[i][0] == cases._t(5, 6, 7) and exp[i][3] == 0
        assert _keys(exp) != _keys(off)
    elif name in ("no_start", "no_end"):
        assert _keys(exp) == _keys(off)
    elif name == "before_all_data":
        assert all(len(e[0]) == 0 for e in exp)
    out_stride = _even_out_stride(off)
    _check(_run(torch, engine, bt, start, end, 0, out_stride), exp,
           out_stride)


@pytest.mark.parametrize("strategy", [0, 3])
def test_filter_with_a_value_strategy(torch, engine, strategy):
    start, end = FILTERS["across_blocks"]
    bt = cases.make_batch(3, 3)
    exp = cases.expected(3, 3, start, end, strategy)
    out_stride = _even_out_stride(exp)
    _check(_run(torch, engine, bt, start, end, strategy, out_stride), exp,
           out_stride)


def test_errors_stay_in_their_series(torch, engine):
    """Every crafted error series gives the model's prefix and code, and the
    series on both sides of each are what the model says (all of them are
    compared)."""
    R, B = 2, 3
    bt = cases.make_batch(R, B)
    exp = cases.expected(R, B)
    out_stride = _even_out_stride(exp)
    got = _run(torch, engine, bt, 0, 0, 0, out_stride)
    _check(got, exp, out_stride)
    want = {"inblock_decrease": model.OUT_OF_ORDER,
            "crossblock_decrease": model.OUT_OF_ORDER,
            "row_err_mid": 1, "row_err_empty_mid": 1, "err_at_push": 1}
    for name, code in want.items():
        i = bt.names[name]
        assert got[4][i] == code == exp[i][3], name
        assert got[3][i] == len(exp[i][0]), name
    assert got[3][bt.names["err_at_push"]] == 0


def test_capacity_keeps_the_prefix(torch, engine):
    R, B = 2, 3
    bt = cases.make_batch(R, B)
    exp = cases.expected(R, B)
    out_stride = 5
    assert sum(len(e[0]) > out_stride for e in exp) > 100
    assert any(len(e[0]) <= out_stride and e[3] == 0 for e in exp)
    got = _run(torch, engine, bt, 0, 0, 0, out_stride)
    _check(got, exp, out_stride)
    assert np.sum(got[4] == CAPACITY) > 100


@pytest.mark.parametrize("form", ["odd_stride", "base_plus_8", "both"])
def test_flush_forms(torch, engine, form):
    """The 8-byte flush: an odd out_stride, or rows 8 bytes off a 16-byte
    boundary (test_kernel_equals_model runs the 16-byte one)."""
    R, B = 3, 3
    bt = cases.make_batch(R, B)
    exp = cases.expected(R, B, 0, 0, 1)
    out_stride = _even_out_stride(exp) + (form != "base_plus_8")
    shift = 0 if form == "odd_stride" else 1
    _check(_run(torch, engine, bt, 0, 0, 1, out_stride, shift), exp,
           out_stride)


@pytest.mark.parametrize("form", ["rows_plus_8", "units_odd", "stride_14"])
def test_input_alignment_forms(torch, engine, form):
    """The kernel loads four points at once where the input rows allow it
    (stride a multiple of 4, 16-byte aligned ts and vals, 4-byte aligned
    units; the other tests' inputs do). Rows 8 bytes off take single loads,
    units at an odd address single unit loads, and a stride of 14 two points
    per load."""
    R, B = 3, 3
    bt = cases.make_batch(R, B)
    d_ts, d_vals, d_units, d_counts, d_errs = _inputs(torch, bt)

    def moved(t, by):
        flat = torch.empty(t.numel() + by, dtype=t.dtype, device=DEV)
        flat[by:] = t.reshape(-1)
        return flat[by:].view(t.shape)

    if form == "rows_plus_8":
        d_ts, d_vals = moved(d_ts, 1), moved(d_vals, 1)
        assert d_ts.data_ptr() % 16 == 8 and d_vals.data_ptr() % 16 == 8
    elif form == "units_odd":
        d_units = moved(d_units, 1)
        assert d_units.data_ptr() % 2 == 1
    else:
        def widened(t):
            w = torch.zeros((t.shape[0], 14), dtype=t.dtype, device=DEV)
            w[:, :bt.stride] = t
            return w
        d_ts, d_vals, d_units = widened(d_ts), widened(d_vals), widened(d_units)
    exp = cases.expected(R, B, 0, 0, 2)
    out_stride = _even_out_stride(exp)
    _check(_run(torch, engine, bt, 0, 0, 2, out_stride,
                inputs=(d_ts, d_vals, d_units, d_counts, d_errs)), exp,
           out_stride)


@pytest.mark.parametrize("R", [2, 4])
def test_equals_the_replica_merge_on_strictly_increasing_rows(torch, engine, R):
    """B=1, no filter, LAST_PUSHED, strictly increasing rows: byte for byte
    m3gpu_merge_batch_units_dev, guard rows included."""
    rng = np.random.default_rng(900 + R)
    N, stride = cases.NSERIES, 16
    ts = np.zeros((R, N, stride), dtype=np.int64)
    vals = np.zeros((R, N, stride), dtype=np.float64)
    units = np.zeros((R, N, stride), dtype=np.uint8)
    counts = np.zeros((R, N), dtype=np.int32)
    for r in range(R):
        for i in range(N):
            c = int(rng.integers(0, stride + 1))
            slots = np.sort(rng.choice(24, size=c, replace=False))
            ts[r, i, :c] = cases.BASE + slots * cases.SEC
            vals[r, i, :c] = rng.integers(0, 4, size=c)
            units[r, i, :c] = 1 + r
            counts[r, i] = c
    d = lambda a: torch.from_numpy(a.reshape(R * N, -1)).to(DEV)
    d_ts, d_vals, d_units = d(ts), d(vals), d(units)
    d_counts = torch.from_numpy(counts.reshape(-1)).to(DEV)
    out_stride = 24

    def outputs():
        return (torch.full((N + 1, out_stride), SENTINEL, dtype=torch.int64,
                           device=DEV),
                torch.full((N + 1, out_stride), SENTINEL, dtype=torch.int64,
                           device=DEV).view(torch.float64),
                torch.full((N + 1, out_stride), USENT, dtype=torch.uint8,
                           device=DEV),
                torch.full((N,), -1, dtype=torch.int32, device=DEV),
                torch.full((N,), -1, dtype=torch.int32, device=DEV))

    a = outputs()
    engine.series_merge_dev(d_ts, d_vals, d_counts, R, 1, a[0][:N], a[1][:N],
                            a[3], a[4], d_units=d_units, out_units=a[2][:N])
    b = outputs()
    engine.merge_batch_units_dev(d_ts, d_vals, d_units, d_counts, R, b[0][:N],
                                 b[1][:N], b[2][:N], b[3], b[4])
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert int(a[3].max()) > stride and int(a[4].abs().sum()) == 0


@pytest.fixture(scope="module")
def production():
    """The 10 production streams and the oracle's decode of each."""
    import oracle
    with open(os.path.join(HERE, "golden", "production_streams.json")) as f:
        streams = [base64.b64decode(s) for s in json.load(f)["samples"]]
    return streams, [oracle.decode_series(s, int_optimized=True)
                     for s in streams]


@pytest.mark.parametrize("ranged", [False, True])
def test_fetch_series_end_to_end(torch, engine, production, ranged):
    """decode + merge of three identical replicas of each stream: the whole
    range is the oracle's decode of one, [ts[100], ts[600]) its points
    100..599, bit-exact."""
    streams, decoded = production
    R = 3

    def fetch(group, start, end):
        blob, offsets, lens = engine.pack_streams(group * R)
        out = engine.fetch_series_dev(
            torch, torch.from_numpy(blob).to(DEV),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV),
            torch.from_numpy(lens.astype(np.int32)).to(DEV), R, 1, 720,
            start_ns=start, end_ns=end, with_units=True)
        torch.cuda.synchronize()
        assert out["ts"].shape == (len(group), 720)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def check(out, k, d, lo, hi):
        ts = np.asarray(d["ts"])[lo:hi]
        n = len(ts)
        assert out["errs"][k] == 0
        assert out["counts"][k] == n
        assert np.array_equal(out["ts"][k, :n], ts)
        assert np.array_equal(
            out["vals"][k, :n].view(np.uint64),
            np.asarray(d["vals"], dtype=np.float64)[lo:hi].view(np.uint64))
        assert np.array_equal(out["units"][k, :n],
                              np.asarray(d["units"])[lo:hi])

    if not ranged:
        out = fetch(streams, 0, 0)
        for i, d in enumerate(decoded):
            check(out, i, d, 0, None)
    else:
        # the range is one per call and the streams' clocks differ
        for s, d in zip(streams, decoded):
            out = fetch([s], int(d["ts"][100]), int(d["ts"][600]))
            check(out, 0, d, 100, 600)


def test_host_form(engine):
    """m3gpu_series_merge_batch on three series of the generated batch."""
    R, B = 2, 3
    bt = cases.make_batch(R, B)
    pick = [bt.names["crossblock_dup"], bt.names["row_err_mid"],
            bt.names["count17"]]
    exp = [cases.expected(R, B, 0, 0, 2)[i] for i in pick]
    out_stride = 20
    ts, vals, units, counts, errs = engine.series_merge(
        bt.ts[:, :, pick], bt.vals[:, :, pick], bt.counts[:, :, pick], R, B,
        out_stride, units=bt.units[:, :, pick], errs=bt.errs[:, :, pick],
        strategy=2)
    for k, (m_ts, m_vals, m_units, m_err) in enumerate(exp):
        n = len(m_ts)
        assert counts[k] == n and errs[k] == m_err, k
        assert ts[k, :n].tolist() == m_ts, k
        assert vals[k, :n].view(np.uint64).tolist() == cases.bits(m_vals), k
        assert units[k, :n].tolist() == m_units, k
        assert np.all(units[k, n:] == 0), k
