"""Inputs shared by test_series_iter_cpu.py and test_series_merge_gpu.py: one
generated batch per (R, B) in the row layout m3gpu_series_merge_batch_dev
takes, and its expectation from series_iter_model. test_series_iter_cpu.py
checks what the GPU test assumes the batch contains."""
import functools
import math

import numpy as np

import series_iter_model as model

NSERIES = 321   # a full block, a full wave and one lane
STRIDE = 12
GRID = 20       # timestamp slots per block
SEC = 10 ** 9
BASE = 1_600_000_000 * SEC
NAN = float("nan")
COUNTS_WANTED = (0, 1, 7, 8, 9, 15, 16, 17)

# the crafted filter series below is built around this range
FILTER_START = BASE + 5 * SEC
FILTER_END = BASE + 8 * SEC


def _t(*secs):
    return [BASE + int(s * SEC) for s in secs]


def _empty(B):
    return [([], [], 0) for _ in range(B)]


def _crafted(R, B):
    """[(name, series)]; a series is [replica][block] = (ts, vals, err)."""
    out = []

    def rep(*blocks):
        blocks = list(blocks) + [([], [], 0)] * (B - len(blocks))
        return blocks[:B]

    def series(*reps):
        reps = list(reps)[:R]
        while len(reps) < R:
            reps.append(_empty(B))
        return reps

    # merged counts: k distinct points, block by block, dealt over replicas
    for k in COUNTS_WANTED:
        if k > R * B * STRIDE:
            continue
        chunk = max(1, math.ceil(k / B))
        s = [[([], [], 0) for _ in range(B)] for _ in range(R)]
        for p in range(k):
            ts, vals, _ = s[p % R][p // chunk]
            ts.append(BASE + p * SEC)
            vals.append(float(p % 4))
        out.append((f"count{k}", s))

    # filter: r0 has a point below start, one on start, one on end; r1 is
    # dropped at 9 and never reaches its 6, which would be out of order
    out.append(("filter", series(
        rep((_t(3, 5, 6, 7, 8, 10), [0., 1., 2., 3., 0., 1.], 0)),
        rep((_t(5, 9, 6), [2., 3., 1.], 0)))))
    # in-block duplicate (first wins) and in-block decrease
    out.append(("inblock_dup", series(
        rep((_t(1, 2, 2, 3), [0., 1., 2., 3.], 0)))))
    out.append(("inblock_decrease", series(
        rep((_t(1, 4, 3, 5), [0., 1., 2., 3.], 0)),
        rep((_t(1, 2), [1., 1.], 0)))))
    # -0.0 / 0.0 tie and NaNs
    out.append(("signed_zero", series(
        rep((_t(1, 2), [-0.0, 1.], 0)), rep((_t(1, 2), [0.0, 2.], 0)),
        rep((_t(1, 2), [1.0, 2.], 0)), rep((_t(1), [3.0], 0)))))
    out.append(("nan", series(
        rep((_t(1, 2, 3), [NAN, 1., NAN], 0)), rep((_t(1, 2, 3), [2., NAN, NAN], 0)),
        rep((_t(1, 2, 3), [NAN, NAN, 0.], 0)), rep((_t(1, 3), [1., NAN], 0)))))
    # row errors: code 1 behind a row's points, and a replica whose first
    # row is empty with an error (the series then emits nothing)
    out.append(("row_err_mid", series(
        rep((_t(1, 2, 3), [0., 1., 2.], 1), (_t(21, 22), [0., 1.], 0)),
        rep((_t(1, 2, 3, 4, 5), [3., 3., 3., 3., 3.], 0)))))
    out.append(("err_at_push", series(
        rep((_t(1, 2, 3), [0., 1., 2.], 0)),
        rep(([], [], 1), (_t(21, 22), [0., 1.], 0)))))
    if R == 1:
        out.append(("err_at_push_r1", series(rep(([], [], 1)))))
    if B >= 2:
        out.append(("crossblock_dup", series(
            rep((_t(1, 2), [0., 1.], 0), (_t(2, 3), [2., 3.], 0)))))
        out.append(("crossblock_decrease", series(
            rep((_t(1, 5), [0., 1.], 0), (_t(3, 6), [2., 3.], 0)))))
        out.append(("row_err_empty_mid", series(
            rep((_t(1, 2), [0., 1.], 0), ([], [], 1), (_t(41,), [2.], 0)),
            rep((_t(1, 2, 3), [3., 3., 3.], 0)))))
    if R == 4:
        # replicas 0 and 1 run out in the step at t=1, where the sort puts 1
        # in front of 0; 2 and 3 go on to a tie at t=2 that only their
        # order in `values` decides (equal keys, stable sort)
        late = (B - 1) * GRID + 2
        for name, va, vb, vc, vd in (("trap_highest", 3., 1., 2., 2.),
                                     ("trap_lowest", 1., 3., 2., 2.),
                                     ("trap_frequency", 2., 7., 2., 9.)):
            more = rep((_t(1), [vc], 0))
            more[B - 1] = (more[B - 1][0] + _t(late), more[B - 1][1] + [5.], 0)
            more_d = rep((_t(1), [vd], 0))
            more_d[B - 1] = (more_d[B - 1][0] + _t(late),
                             more_d[B - 1][1] + [5.], 0)
            out.append((name, series(rep((_t(1), [va], 0)),
                                     rep((_t(1), [vb], 0)), more, more_d)))
    return out


def _random_series(rng, R, B):
    s = []
    for r in range(R):
        blocks = []
        for b in range(B):
            c = 0 if rng.random() < 0.1 else int(rng.integers(1, STRIDE + 1))
            slots = np.sort(rng.choice(GRID, size=c, replace=False))
            ts = [BASE + (b * GRID + int(x)) * SEC for x in slots]
            vals = [float(v) for v in rng.integers(0, 4, size=c)]
            for j in range(c):
                u = rng.random()
                if u < 0.03:
                    vals[j] = -0.0
                elif u < 0.05:
                    vals[j] = NAN
            if c >= 2 and rng.random() < 0.15:   # in-block duplicate
                j = int(rng.integers(1, c))
                ts[j] = ts[j - 1]
            if c >= 3 and rng.random() < 0.008:  # in-block decrease
                j = int(rng.integers(2, c))
                ts[j] = ts[j - 2]
                if ts[j - 1] == ts[j]:
                    ts[j] -= SEC
            err = 1 if rng.random() < 0.006 else 0
            blocks.append((ts, vals, err))
        for b in range(1, B):
            prev, cur = blocks[b - 1][0], blocks[b][0]
            if prev and cur:
                u = rng.random()
                if u < 0.08:
                    cur[0] = prev[-1]          # duplicate across the boundary
                elif u < 0.09:
                    cur[0] = prev[-1] - SEC    # decrease across the boundary
        s.append(blocks)
    return s


class Batch:
    pass


@functools.lru_cache(maxsize=None)
def make_batch(R, B, seed=11):
    rng = np.random.default_rng(seed * 100 + R * 10 + B)
    crafted = _crafted(R, B)
    series = [s for _, s in crafted]
    while len(series) < NSERIES:
        series.append(_random_series(rng, R, B))
    assert len(series) == NSERIES
    bt = Batch()
    bt.R, bt.B, bt.nseries, bt.stride = R, B, NSERIES, STRIDE
    bt.names = {name: i for i, (name, _) in enumerate(crafted)}
    bt.ts = np.zeros((R, B, NSERIES, STRIDE), dtype=np.int64)
    bt.vals = np.zeros((R, B, NSERIES, STRIDE), dtype=np.float64)
    bt.units = np.zeros((R, B, NSERIES, STRIDE), dtype=np.uint8)
    bt.counts = np.zeros((R, B, NSERIES), dtype=np.uint32)
    bt.errs = np.zeros((R, B, NSERIES), dtype=np.int32)
    for i, s in enumerate(series):
        for r in range(R):
            for b in range(B):
                ts, vals, err = s[r][b]
                c = len(ts)
                bt.ts[r, b, i, :c] = ts
                bt.vals[r, b, i, :c] = vals
                bt.units[r, b, i, :c] = 1 + r   # the unit names the replica
                bt.counts[r, b, i] = c
                bt.errs[r, b, i] = err
    for a in (bt.ts, bt.vals, bt.units, bt.counts, bt.errs):
        a.setflags(write=False)
    return bt


def model_input(bt, i):
    """Series i of a batch as series_iter_model.series_iterate takes it."""
    reps = []
    for r in range(bt.R):
        blocks = []
        for b in range(bt.B):
            c = int(bt.counts[r, b, i])
            blocks.append((bt.ts[r, b, i, :c].tolist(),
                           bt.vals[r, b, i, :c].tolist(),
                           bt.units[r, b, i, :c].tolist(),
                           int(bt.errs[r, b, i])))
        reps.append(blocks)
    return reps


@functools.lru_cache(maxsize=None)
def expected(R, B, start=0, end=0, strategy=0, removal="sorted"):
    """[(ts, vals, units, err)] per series of make_batch(R, B)."""
    bt = make_batch(R, B)
    return [model.series_iterate(model_input(bt, i), start, end, strategy,
                                 removal)
            for i in range(bt.nseries)]


def bits(vals):
    return np.asarray(vals, dtype=np.float64).view(np.uint64).tolist()
