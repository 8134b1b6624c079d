"""Seeded series for the step-consolidation tests (CPU and GPU): increasing
timestamps around a step grid, with the points the window rule can get
wrong. What they contain is asserted in test_step_consolidate_cpu.py."""
import numpy as np

SEC = 10 ** 9
START = 1427162400 * SEC  # the golden fixture's hour-aligned start


def grid_cases():
    """(step_ns, lookback_ns): step < L, step == L, step > L and L == 0."""
    return [(20 * SEC, 50 * SEC), (30 * SEC, 30 * SEC), (60 * SEC, 25 * SEC),
            (15 * SEC, 0)]


def boundary_times(start, step, nsteps, lookback):
    """Points exactly at t_k, t_k - L and 1 ns either side of both, before
    start - L, and past t_last (the first of which is the peeked point)."""
    t_last = start + (nsteps - 1) * step
    out = {start - lookback - 7 * SEC, start - lookback - 1, t_last + 1,
           t_last + 3 * SEC}
    for k in {0, 1, nsteps // 2, nsteps - 1}:
        tk = start + k * step
        for base in (tk, tk - lookback):
            out.update((base - 1, base, base + 1))
    return sorted(out)


def make_series(rng, start, step, nsteps, lookback, kind):
    """(ts list, vals list) with increasing ts. Kinds: "empty"; "boundary"
    (every boundary time); "boundary_nan" (the same with NaN on the points
    at t_k: the newest point of a window is NaN and TakeLast walks back);
    "dense", "sparse", "before", "after" random draws."""
    t_last = start + (nsteps - 1) * step
    if kind == "empty":
        return [], []
    if kind in ("boundary", "boundary_nan"):
        ts = boundary_times(start, step, nsteps, lookback)
        vals = [float(i + 1) for i in range(len(ts))]
        if kind == "boundary_nan":
            for i, t in enumerate(ts):
                if t >= start and (t - start) % step == 0:
                    vals[i] = float("nan")
        return ts, vals
    span = (nsteps + 3) * step + lookback
    lo = start - lookback - 2 * step
    if kind == "dense":
        n = int(rng.integers(nsteps, 4 * nsteps + 2))
    elif kind == "sparse":
        n = int(rng.integers(1, max(2, nsteps // 3)))
    elif kind == "before":
        n, span = int(rng.integers(1, 6)), step
    else:  # "after": every point past t_last
        n, lo = int(rng.integers(1, 6)), t_last + 1
    raw = np.unique(lo + rng.integers(0, span, size=n))
    # some points snapped onto the grid and onto the window's lower edge
    snap = rng.random(len(raw))
    ts = []
    for t, s in zip(raw.tolist(), snap.tolist()):
        k = max(0, min(nsteps - 1, (t - start) // step))
        if kind in ("before", "after"):
            pass
        elif s < 0.15:
            t = start + k * step
        elif s < 0.3:
            t = start + k * step - lookback
        ts.append(int(t))
    ts = sorted(set(ts))
    vals = rng.integers(-50, 50, size=len(ts)).astype(np.float64)
    vals[rng.random(len(ts)) < 0.2] = np.nan
    return ts, vals.tolist()


KINDS = ["empty", "boundary", "boundary_nan", "dense", "sparse", "before",
         "after"]


def make_batch(seed, nseries, start, step, nsteps, lookback):
    """nseries series cycling through KINDS; returns a list of (ts, vals)."""
    rng = np.random.default_rng(seed)
    return [make_series(rng, start, step, nsteps, lookback,
                        KINDS[i % len(KINDS)]) for i in range(nseries)]
