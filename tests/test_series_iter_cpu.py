"""Batched SeriesIterator (m3gpu_series_merge_batch*), the part that needs no
GPU: the Python model of series_iter_model.py against the reference's own
test tables and against the oracle's MultiReaderIterator, what
test_series_merge_gpu.py assumes of its generated batches, the argument
rules of the C entries, and the iterator wrappers."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import series_iter_model as model  # noqa: E402
import series_merge_cases as cases  # noqa: E402

import oracle  # noqa: E402
from m3_amd import engine, iterators  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
M3GPU_ERR_BADARG = -2

with open(os.path.join(HERE, "golden", "series_iterator_vectors.json")) as f:
    GOLDEN = json.load(f)["cases"]


@pytest.fixture(autouse=True, scope="module")
def _feature_present():
    """The model and the generated batches describe entries that must exist:
    without them nothing here passes."""
    L = engine.lib()
    assert hasattr(L, "m3gpu_series_merge_batch_dev")
    assert hasattr(L, "m3gpu_series_merge_batch")
    assert hasattr(iterators, "SeriesIterator")


# ------------------------------ the model ------------------------------

@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_model_reproduces_the_reference_tables(case):
    replicas = [[(b["ts"], b["vals"], b["units"], b["err"]) for b in rep]
                for rep in case["replicas"]]
    ts, vals, units, err = model.series_iterate(
        replicas, case["start"], case["end"], case["strategy"])
    exp = case["expected"]
    assert ts == exp["ts"]
    assert vals == exp["vals"]
    assert units == exp["units"]
    assert err == exp["err"]


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_model_equals_the_oracle_on_strictly_increasing_replicas(R):
    """B=1, no filter, LAST_PUSHED: the one case where the two-level
    iterator and the oracle's single-level MultiReaderIterator agree."""
    rng = np.random.default_rng(500 + R)
    nseries, stride = 97, 16
    ts = np.zeros((R, nseries, stride), dtype=np.int64)
    vals = np.zeros((R, nseries, stride), dtype=np.float64)
    counts = np.zeros((R, nseries), dtype=np.uint32)
    for r in range(R):
        for i in range(nseries):
            c = int(rng.integers(0, stride + 1))
            slots = np.sort(rng.choice(40, size=c, replace=False))
            ts[r, i, :c] = cases.BASE + slots * cases.SEC
            vals[r, i, :c] = rng.integers(0, 4, size=c)
            counts[r, i] = c
    o_ts, o_vals, o_counts, o_errs = oracle.merge_batch(ts, vals, counts)
    for i in range(nseries):
        replicas = []
        for r in range(R):
            c = int(counts[r, i])
            replicas.append([(ts[r, i, :c].tolist(), vals[r, i, :c].tolist(),
                              [1 + r] * c, 0)])
        m_ts, m_vals, _, m_err = model.series_iterate(replicas)
        n = int(o_counts[i])
        assert m_err == int(o_errs[i]) == 0
        assert m_ts == o_ts[i, :n].tolist(), i
        assert m_vals == o_vals[i, :n].tolist(), i


# ------------- what the GPU test assumes of its generated batch -------------

def _series_points(bt, i):
    """[(r, b, [ts], [vals])] of series i."""
    out = []
    for r in range(bt.R):
        for b in range(bt.B):
            c = int(bt.counts[r, b, i])
            out.append((r, b, bt.ts[r, b, i, :c].tolist(),
                        bt.vals[r, b, i, :c].tolist()))
    return out


def test_batch_has_the_merged_counts_around_the_tile():
    exp = cases.expected(4, 3)
    got = {len(e[0]) for e in exp if e[3] == 0}
    assert set(cases.COUNTS_WANTED) <= got
    # the smaller shapes hold every count their capacity allows
    for R, B in ((1, 1), (2, 1), (1, 3)):
        got = {len(e[0]) for e in cases.expected(R, B) if e[3] == 0}
        want = {k for k in cases.COUNTS_WANTED if k <= R * B * cases.STRIDE}
        assert want <= got, (R, B)


def test_batch_has_cross_replica_ties_with_equal_and_unequal_values():
    bt = cases.make_batch(4, 3)
    equal = unequal = 0
    for i in range(bt.nseries):
        seen = {}
        for r, _, ts, vals in _series_points(bt, i):
            for t, v in zip(ts, vals):
                for r2, v2 in seen.get(t, []):
                    if r2 != r:
                        if v2 == v:
                            equal += 1
                        else:
                            unequal += 1
                seen.setdefault(t, []).append((r, v))
    assert equal > 100 and unequal > 100


@pytest.mark.parametrize("strategy", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 3])
def test_batch_tells_sorted_removal_from_slot_removal(strategy, B):
    """Trap 5: some series has two replicas run out in one step while two go
    on to a later tie, and a model that removes them in `values` order gives
    another output for it."""
    bt = cases.make_batch(4, B)
    right = cases.expected(4, B, 0, 0, strategy)
    wrong = cases.expected(4, B, 0, 0, strategy, "slot")
    name = {1: "trap_highest", 2: "trap_lowest", 3: "trap_frequency"}[strategy]
    i = bt.names[name]
    # replicas 0 and 1 end at the first timestamp; 2 and 3 tie again later
    first = bt.ts[0, 0, i, 0]
    totals = [int(bt.counts[r, :, i].sum()) for r in range(4)]
    assert totals == [1, 1, 2, 2]
    assert all(bt.ts[r, 0, i, 0] == first for r in range(4))
    assert bt.ts[2, B - 1, i, bt.counts[2, B - 1, i] - 1] == \
        bt.ts[3, B - 1, i, bt.counts[3, B - 1, i] - 1] > first
    assert right[i][3] == 0 and len(right[i][0]) == 2
    assert right[i] != wrong[i]
    assert right[i][2] != wrong[i][2]   # it shows in the winner's unit


def test_batch_has_block_boundary_and_in_block_cases():
    bt = cases.make_batch(4, 3)
    cross_dup = cross_dec = in_dup = neg_zero_tie = nans = 0
    for i in range(bt.nseries):
        pts = _series_points(bt, i)
        by_rb = {(r, b): ts for r, b, ts, _ in pts}
        for r in range(bt.R):
            for b in range(1, bt.B):
                prev, cur = by_rb[(r, b - 1)], by_rb[(r, b)]
                if prev and cur:
                    cross_dup += cur[0] == prev[-1]
                    cross_dec += cur[0] < prev[-1]
        for _, _, ts, vals in pts:
            in_dup += any(a == b for a, b in zip(ts, ts[1:]))
            nans += sum(1 for v in vals if v != v)
        zeros = {}
        for r, _, ts, vals in pts:
            for t, v in zip(ts, vals):
                if v == 0.0:
                    zeros.setdefault(t, set()).add(
                        (r, bool(np.signbit(v))))
        for members in zeros.values():
            signs = {s for _, s in members}
            if len({r for r, _ in members}) > 1 and signs == {True, False}:
                neg_zero_tie += 1
    assert cross_dup >= 3 and cross_dec >= 1
    assert in_dup >= 10
    assert neg_zero_tie >= 1
    assert nans >= 10
    # the crafted ones behave as meant
    exp = cases.expected(4, 3)
    assert len(exp[bt.names["crossblock_dup"]][0]) == 3
    assert exp[bt.names["crossblock_dup"]][3] == 0
    assert exp[bt.names["crossblock_decrease"]][3] == model.OUT_OF_ORDER
    assert exp[bt.names["inblock_decrease"]][3] == model.OUT_OF_ORDER
    assert exp[bt.names["inblock_dup"]][1] == [0.0, 1.0, 3.0]
    assert exp[bt.names["err_at_push"]] == ([], [], [], 1)
    assert exp[bt.names["row_err_mid"]][3] == 1
    assert len(exp[bt.names["row_err_mid"]][0]) == 3
    assert exp[bt.names["row_err_empty_mid"]][3] == 1
    assert len(exp[bt.names["row_err_empty_mid"]][0]) == 2


def test_batch_filter_series_drops_rather_than_skips():
    bt = cases.make_batch(2, 1)
    i = bt.names["filter"]
    exp = cases.expected(2, 1, cases.FILTER_START, cases.FILTER_END)[i]
    # 5 is on start and stays, 8 is on end and goes; replica 1 is dropped at
    # its 9, so its 6 behind it (a decrease) is never looked at
    assert exp[0] == cases._t(5, 6, 7) and exp[3] == 0
    assert exp[2] == [2, 1, 1]
    # with only one bound given nothing is filtered, and the 6 is reached
    for start, end in ((0, cases.FILTER_END), (cases.FILTER_START, 0)):
        e = cases.expected(2, 1, start, end)[i]
        assert e == cases.expected(2, 1)[i]
        assert e[3] == model.OUT_OF_ORDER


# --------------------------- argument checks ---------------------------

def test_new_symbols_exported():
    L = engine.lib()
    for sym in ("m3gpu_series_merge_batch_dev", "m3gpu_series_merge_batch"):
        assert hasattr(L, sym), sym
    for name in ("series_merge_dev", "series_merge", "fetch_series_dev"):
        assert callable(getattr(engine, name))
    assert engine.SERIES_ERRORS[100] == "out_of_order"


GOOD = dict(R=2, B=1, stride=8, out_stride=8, strategy=0, units=False,
            out_units=False)


@pytest.mark.parametrize("bad", [
    dict(R=0), dict(R=5),
    dict(B=0), dict(stride=0), dict(out_stride=0),
    dict(strategy=-1), dict(strategy=4),
    dict(units=True), dict(out_units=True),
], ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
@pytest.mark.parametrize("form", ["dev", "host"])
def test_badarg_before_any_hip_call(bad, form):
    """Null data pointers and nseries > 0: an entry that got as far as a
    copy or a launch would fault or return a HIP error instead."""
    a = dict(GOOD, **bad)
    L = engine.lib()
    fake = ctypes.c_void_p(4096)
    args = [None, None, fake if a["units"] else None, None, None,
            a["R"], a["B"], 3, a["stride"], 0, 0, a["strategy"],
            None, None, fake if a["out_units"] else None, None, None,
            a["out_stride"]]
    if form == "dev":
        rc = L.m3gpu_series_merge_batch_dev(*args, None)
    else:
        P = ctypes.POINTER
        args[2] = ctypes.cast(args[2], P(ctypes.c_uint8)) if args[2] else None
        args[14] = ctypes.cast(args[14], P(ctypes.c_uint8)) if args[14] else None
        rc = L.m3gpu_series_merge_batch(*args)
    assert rc == M3GPU_ERR_BADARG
    assert L.m3gpu_last_error().decode()


def test_good_arguments_with_no_series_are_ok():
    rc = engine.lib().m3gpu_series_merge_batch_dev(
        None, None, None, None, None, 2, 1, 0, 8, 0, 0, 0,
        None, None, None, None, None, 8, None)
    assert rc == 0


# ------------------------------ wrappers ------------------------------

def test_series_iterator_wrapper():
    ts = np.array([[10, 20, 30, 0], [5, 0, 0, 0]], dtype=np.int64)
    vals = np.array([[1., 2., 3., 0.], [9., 0., 0., 0.]])
    units = np.array([[1, 2, 3, 0], [4, 0, 0, 0]], dtype=np.uint8)
    batch = iterators.BatchSeriesIterators(
        ts, vals, [3, 1], errs=[0, 100], start_ns=5, end_ns=40, units=units)
    assert len(batch) == 2
    it = batch.iterator(0)
    with pytest.raises(RuntimeError):
        it.Current()
    got = []
    while it.Next():
        got.append(it.Current())
    assert got == [(10, 1.0, 1), (20, 2.0, 2), (30, 3.0, 3)]
    assert not it.Next() and it.Err() is None
    assert (it.Start(), it.End()) == (5, 40)
    it.Close()
    assert not it.Next()
    # the emitted prefix of a failed series, then its error
    bad = list(batch)[1]
    assert bad.Next() and bad.Current() == (5, 9.0, 4)
    assert not bad.Next() and bad.Err() == "out_of_order"
    # without unit rows Current() reports the constructor's unit
    plain = iterators.SeriesIterator(ts[0], vals[0], 3, unit=2)
    assert plain.Next() and plain.Current() == (10, 1.0, 2)
    assert (plain.Start(), plain.End()) == (0, 0)
