"""Seeded series for the temporal-function tests (CPU and GPU): what the
integer values of step_consolidate_cases.py cannot show. Increasing
timestamps around a step grid with non-integer doubles over a wide exponent
range, monotone counters with resets, +-0.0 in both orders, +-Inf, NaN runs
at a window's first and last point, points exactly on t_k and t_k - range and
1 ns either side of both, and windows of chosen point counts around the
kernel's ring depth. What they contain is asserted in test_temporal_cpu.py."""
import math

import numpy as np

import step_consolidate_cases as step_cases

SEC = step_cases.SEC
START = step_cases.START


def grid_cases():
    """(step_ns, range_ns): range > step (5x overlap), range == step and
    range < step."""
    return [(60 * SEC, 300 * SEC), (30 * SEC, 30 * SEC), (60 * SEC, 25 * SEC)]


def wide_doubles(rng, n):
    """Non-integer doubles, both signs, binary exponents -60..60."""
    m = rng.uniform(1.0, 2.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    return np.ldexp(m, rng.integers(-60, 61, size=n))


def dense_times(rng, start, step, nsteps, range_ns, per_window=4):
    """A point about every range/per_window from two steps before the first
    window to two steps past the last step, jittered, some snapped onto the
    grid and onto a window's lower edge."""
    dt = max(3, range_ns // per_window)
    lo = start - range_ns - 2 * step
    hi = start + (nsteps + 1) * step
    ts = []
    t = lo
    while t <= hi:
        j = int(rng.integers(-(dt // 3), dt // 3 + 1))
        s = rng.random()
        x = t + j
        k = max(0, min(nsteps - 1, (x - start) // step))
        if s < 0.1:
            x = start + k * step
        elif s < 0.2:
            x = start + k * step - range_ns
        ts.append(int(x))
        t += dt
    return sorted(set(ts))


def window_sizes(ring):
    """Point counts per window of the "windows" kind: around the kernel's
    ring depth C, and 3C, where a window reaches from LDS into global
    memory."""
    return [0, 1, 2, ring - 1, ring, ring + 1, 3 * ring]


def make_series(rng, start, step, nsteps, range_ns, kind, ring=16):
    """(ts list, vals list) with strictly increasing ts."""
    t_last = start + (nsteps - 1) * step
    if kind == "empty":
        return [], []
    if kind in ("boundary", "boundary_nan"):
        ts = step_cases.boundary_times(start, step, nsteps, range_ns)
        vals = (wide_doubles(rng, len(ts))).tolist()
        if kind == "boundary_nan":
            # NaN exactly on t_k (a window's last point) and on t_k - range
            # (its first)
            for i, t in enumerate(ts):
                if (t - start) % step == 0 or \
                        (t - start + range_ns) % step == 0:
                    vals[i] = math.nan
        return ts, vals
    if kind == "windows":
        # step k gets sizes[k % 7] points in (t_k - w, t_k], w below both the
        # range and the step: with range < step, W_k holds exactly those
        sizes = window_sizes(ring)
        w = min(range_ns, step) - 2
        ts = []
        for k in range(-1, nsteps + 1):
            n = sizes[(k + 1) % len(sizes)]
            tk = start + k * step
            ts.extend(tk - j * (w // (n + 1)) for j in range(n))
        ts = sorted(set(ts))
        vals = wide_doubles(rng, len(ts))
        vals[rng.random(len(ts)) < 0.05] = np.nan
        return ts, vals.tolist()
    if kind == "sparse":
        n = int(rng.integers(1, max(2, nsteps // 2 + 1)))
        span = (nsteps + 2) * step + range_ns
        ts = sorted(set((start - range_ns - step +
                         rng.integers(0, span, size=n)).tolist()))
        return ts, wide_doubles(rng, len(ts)).tolist()
    if kind == "after":
        ts = [t_last + 1 + 7 * j for j in range(int(rng.integers(1, 5)))]
        return ts, wide_doubles(rng, len(ts)).tolist()
    ts = dense_times(rng, start, step, nsteps, range_ns)
    n = len(ts)
    if kind == "dense":
        vals = wide_doubles(rng, n)
        vals[rng.random(n) < 0.05] = np.nan
    elif kind == "counter":
        # a monotone counter with non-integer increments that resets
        vals = np.empty(n)
        c = float(rng.uniform(0, 50))
        for i in range(n):
            if rng.random() < 0.15:
                c = float(rng.uniform(0, 3))
            c += float(rng.uniform(0.1, 9.7))
            vals[i] = c
        vals[rng.random(n) < 0.05] = np.nan
    elif kind == "zeros":
        # +0 before -0 and -0 before +0, with a few other values between
        pattern = [0.0, -0.0, -0.0, 0.0, 0.0, 0.0, -0.0, 1.5, -0.0, 0.0, -2.5]
        vals = np.array([pattern[i % len(pattern)] for i in range(n)])
    elif kind == "inf":
        vals = wide_doubles(rng, n)
        pick = rng.random(n)
        vals[pick < 0.15] = np.inf
        vals[pick > 0.85] = -np.inf
    elif kind == "nan_runs":
        # runs of two NaNs every six points: windows start and end on them
        vals = wide_doubles(rng, n)
        vals[[i for i in range(n) if i % 6 < 2]] = np.nan
    elif kind == "lonely":
        # one value in five: windows with a single non-NaN point, in front
        # of, between and behind NaNs
        vals = np.full(n, np.nan)
        idx = list(range(int(rng.integers(0, 5)), n, 5))
        vals[idx] = wide_doubles(rng, len(idx))
    elif kind == "all_nan":
        vals = np.full(n, np.nan)
    else:
        raise ValueError(kind)
    return ts, vals.tolist()


KINDS = ["dense", "counter", "boundary", "boundary_nan", "zeros", "inf",
         "nan_runs", "lonely", "all_nan", "windows", "sparse", "empty",
         "after"]


def make_batch(seed, nseries, start, step, nsteps, range_ns, ring=16):
    """nseries series cycling through KINDS; a list of (ts, vals)."""
    rng = np.random.default_rng(seed)
    return [make_series(rng, start, step, nsteps, range_ns,
                        KINDS[i % len(KINDS)], ring) for i in range(nseries)]
