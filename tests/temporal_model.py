"""Plain-Python restatements of the reference's temporal functions: test
infrastructure for test_temporal_cpu.py and test_temporal_gpu.py, written
from the reference sources (src/query/functions/temporal):

  - base.go:255-306, :432-482      the per-series step loop and getIndices
  - aggregation.go:151-251         avg, count, min, max, sum, stddev, stdvar,
                                   last over time; sumAndCount
  - rate.go:150-298                standardRateFunc, irateFunc, findNonNanIdx
  - functions.go:89-118            functionNode.process (resets, changes)
  - linear_regression.go:127-191   linearRegressionNode.process, subSeconds,
                                   linearRegression

Two levels. `procedural` is the reference's procedure: getIndices with its
carried `init`, and each processor restated line by line over the sub-slice
it is handed. `closed_form` is what the kernel is specified to compute
(m3gpu.h): the window as a set, W_k = the points with t_k - range <= ts <=
t_k, each function written from that description on its own, plus the error
rules. On increasing timestamps without an error the two agree bit for bit,
which test_temporal_cpu.py checks.

A cell is (bits, literal): the value's uint64 pattern, and whether the
reference returned math.NaN() itself there (the cell must then hold NAN_BITS
exactly) as opposed to a NaN that arithmetic produced (any NaN will do: Go on
amd64 hands math.NaN() through NaN/0, sqrt(NaN) and NaN*d + NaN unchanged,
but the rule leaves sign and payload of arithmetic NaNs to the hardware).
"""
import bisect
import math
import struct

NAN_BITS = 0x7FF8000000000001
OUT_OF_ORDER = 100  # M3GPU_SERIES_OUT_OF_ORDER
SECOND = 10 ** 9

# include/m3gpu.h M3GPU_TEMPORAL_*
FNS = ["sum_over_time", "count_over_time", "avg_over_time", "min_over_time",
       "max_over_time", "last_over_time", "stddev_over_time",
       "stdvar_over_time", "rate", "increase", "delta", "irate", "idelta",
       "resets", "changes", "deriv", "predict_linear"]
FN_ID = {name: i for i, name in enumerate(FNS)}


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


GO_NAN = from_bits(NAN_BITS)
LITERAL = object()  # a processor returned math.NaN() itself

# Every NaN-returning branch of the processors below, by name; HITS collects
# the ones the procedural model has taken, so that a test can tell a batch
# that reaches them all from one that does not.
NAN_BRANCHES = {
    "sum_and_count:none", "avg:none", "count:none", "min:none", "max:none",
    "last:empty", "last:nan_value", "stdvar:count<2", "stddev:count<2",
    "rate:len<2", "rate:first==last", "irate:len<2", "irate:last<1",
    "irate:no_previous", "function:empty", "function:all_nans",
    "regression:len<2", "regression:one_value", "predict_linear:one_value",
    "regression:no_value"}
HITS = set()


def _lit(tag):
    assert tag in NAN_BRANCHES, tag
    HITS.add(tag)
    return LITERAL


def _nan(tag):
    """A NaN that the reference gets by arithmetic."""
    assert tag in NAN_BRANCHES, tag
    HITS.add(tag)
    return math.nan


def _div(a, b):
    """Go's float64 division: no exception on a zero divisor."""
    if b == 0.0:
        if a == 0.0 or math.isnan(a):
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def go_min(x, y):  # math.Min
    if math.isinf(x) and x < 0 or math.isinf(y) and y < 0:
        return -math.inf
    if math.isnan(x) or math.isnan(y):
        return math.nan
    if x == 0 and x == y:
        return x if math.copysign(1.0, x) < 0 else y
    return x if x < y else y


def go_max(x, y):  # math.Max
    if math.isinf(x) and x > 0 or math.isinf(y) and y > 0:
        return math.inf
    if math.isnan(x) or math.isnan(y):
        return math.nan
    if x == 0 and x == y:
        return y if math.copysign(1.0, x) < 0 else x
    return x if x > y else y


def _trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def duration_seconds(d):  # time.Duration.Seconds()
    sec = _trunc_div(d, SECOND)
    nsec = d - sec * SECOND
    return float(sec) + float(nsec) / 1e9


def sub_seconds(a, b):  # linear_regression.go:140-142
    return float(a - b) / 1e9


# ---------------- the reference's processors, line by line ----------------
# dps is a list of (timestamp, value); each returns a float or LITERAL.

def sum_and_count(values):  # aggregation.go:236-251
    s, count = 0.0, 0.0
    for v in values:
        if not math.isnan(v):
            s += v
            count += 1
    if count == 0:
        return _lit("sum_and_count:none"), 0.0
    return s, count


def p_avg(dps, lo, hi, rng, param):
    s, count = sum_and_count([v for _, v in dps])
    if s is LITERAL:
        return _nan("avg:none")  # math.NaN() / 0: arithmetic
    return s / count


def p_count(dps, lo, hi, rng, param):
    _, count = sum_and_count([v for _, v in dps])
    return _lit("count:none") if count == 0 else count


def p_sum(dps, lo, hi, rng, param):
    s, _ = sum_and_count([v for _, v in dps])
    return s


def p_min(dps, lo, hi, rng, param):
    seen, m = False, math.inf
    for _, v in dps:
        if not math.isnan(v):
            seen = True
            m = go_min(m, v)
    return m if seen else _lit("min:none")


def p_max(dps, lo, hi, rng, param):
    seen, m = False, -math.inf
    for _, v in dps:
        if not math.isnan(v):
            seen = True
            m = go_max(m, v)
    return m if seen else _lit("max:none")


def p_stdvar(dps, lo, hi, rng, param):
    aux = count = mean = 0.0
    for _, v in dps:
        if not math.isnan(v):
            count += 1
            delta = v - mean
            mean += delta / count
            aux += delta * (v - mean)
    if count < 2:
        return _lit("stdvar:count<2")
    return aux / count


def p_stddev(dps, lo, hi, rng, param):
    var = p_stdvar(dps, lo, hi, rng, param)
    if var is LITERAL:
        return _nan("stddev:count<2")  # math.Sqrt(math.NaN()): arithmetic
    return math.sqrt(var) if var >= 0 else math.nan


def p_last(dps, lo, hi, rng, param):
    if len(dps) == 0:
        return _lit("last:empty")
    if math.isnan(dps[-1][1]):
        HITS.add("last:nan_value")
    return dps[-1][1]


def standard_rate(dps, is_rate, is_counter, range_start, range_end, window):
    if len(dps) < 2:
        return _lit("rate:len<2")
    correction = 0.0
    first_val = last_value = 0.0
    first_idx = last_idx = 0
    first_ts = last_ts = 0
    found_first = False
    for i, (t, v) in enumerate(dps):
        if math.isnan(v):
            continue
        if not found_first:
            first_val, first_ts, first_idx = v, t, i
            found_first = True
        if is_counter and v < last_value:
            correction += last_value
        last_value, last_ts, last_idx = v, t, i
    if first_idx == last_idx:
        return _lit("rate:first==last")
    duration_to_start = sub_seconds(first_ts, range_start)
    duration_to_end = sub_seconds(range_end, last_ts)
    sampled_interval = sub_seconds(last_ts, first_ts)
    average_between = _div(sampled_interval, float(last_idx - first_idx))
    result = last_value - first_val + correction
    if is_counter and result > 0 and first_val >= 0:
        duration_to_zero = sampled_interval * _div(first_val, result)
        if duration_to_zero < duration_to_start:
            duration_to_start = duration_to_zero
    threshold = average_between * 1.1
    extrapolate_to = sampled_interval
    if duration_to_start < threshold:
        extrapolate_to += duration_to_start
    else:
        extrapolate_to += average_between / 2
    if duration_to_end < threshold:
        extrapolate_to += duration_to_end
    else:
        extrapolate_to += average_between / 2
    result = result * _div(extrapolate_to, sampled_interval)
    if is_rate:
        result = _div(result, duration_seconds(window))
    return result


def find_non_nan_idx(dps, start):  # rate.go:290-298
    for i in range(start, -1, -1):
        if not math.isnan(dps[i][1]):
            return i
    return -1


def irate(dps, is_rate):
    n = len(dps)
    if n < 2:
        return _lit("irate:len<2")
    index_last = find_non_nan_idx(dps, n - 1)
    if index_last < 1:
        return _lit("irate:last<1")
    non_nan = find_non_nan_idx(dps, index_last - 1)
    if non_nan == -1:
        return _lit("irate:no_previous")
    prev_t, prev_v = dps[non_nan]
    last_t, last_v = dps[index_last]
    if is_rate and last_v < prev_v:
        result = last_v
    else:
        result = last_v - prev_v
    if is_rate:
        interval = last_t - prev_t
        if interval == 0:
            return LITERAL
        result = _div(result, duration_seconds(interval))
    return result


def function_node(dps, comparison):  # functions.go:89-118
    if len(dps) == 0:
        return _lit("function:empty")
    all_nans = True
    result = 0.0
    prev = dps[0][1]
    for _, cur in dps[1:]:
        if math.isnan(cur):
            continue
        all_nans = False
        if not math.isnan(prev):
            if comparison(cur, prev):
                result += 1
        prev = cur
    return _lit("function:all_nans") if all_nans else result


def linear_regression(dps, intercept_time, is_deriv):
    """(slope, intercept), or LITERAL for the pair of math.NaN()."""
    n = 0.0
    sum_dt = sum_vals = sum_dt_vals = sum_dt_sq = 0.0
    value_count = 0
    for t, v in dps:
        if math.isnan(v):
            continue
        if value_count == 0 and is_deriv:
            intercept_time = t
        value_count += 1
        dt = sub_seconds(t, intercept_time)
        n += 1.0
        sum_vals += v
        sum_dt += dt
        sum_dt_vals += dt * v
        sum_dt_sq += dt * dt
    if value_count == 1:
        return _lit("regression:one_value")
    if value_count == 0:
        HITS.add("regression:no_value")  # falls through to 0/0
    cov_xy = sum_dt_vals - _div(sum_dt * sum_vals, n)
    var_x = sum_dt_sq - _div(sum_dt * sum_dt, n)
    slope = _div(cov_xy, var_x)
    intercept = _div(sum_vals, n) - _div(slope * sum_dt, n)
    return slope, intercept


def p_regression(dps, hi, is_deriv, param):
    if len(dps) < 2:
        return _lit("regression:len<2")
    res = linear_regression(dps, hi, is_deriv)
    if res is LITERAL:
        # deriv returns the slope, math.NaN() itself; predict_linear
        # computes NaN*d + NaN
        return LITERAL if is_deriv else _nan("predict_linear:one_value")
    slope, intercept = res
    return slope if is_deriv else slope * param + intercept


PROCESSORS = {
    "sum_over_time": p_sum, "count_over_time": p_count,
    "avg_over_time": p_avg, "min_over_time": p_min, "max_over_time": p_max,
    "last_over_time": p_last, "stddev_over_time": p_stddev,
    "stdvar_over_time": p_stdvar,
    "rate": lambda d, lo, hi, w, p: standard_rate(d, True, True, lo, hi, w),
    "increase": lambda d, lo, hi, w, p: standard_rate(d, False, True, lo, hi,
                                                      w),
    "delta": lambda d, lo, hi, w, p: standard_rate(d, False, False, lo, hi,
                                                   w),
    "irate": lambda d, lo, hi, w, p: irate(d, True),
    "idelta": lambda d, lo, hi, w, p: irate(d, False),
    "resets": lambda d, lo, hi, w, p: function_node(d, lambda a, b: a < b),
    "changes": lambda d, lo, hi, w, p: function_node(d, lambda a, b: a != b),
    "deriv": lambda d, lo, hi, w, p: p_regression(d, hi, True, p),
    "predict_linear": lambda d, lo, hi, w, p: p_regression(d, hi, False, p),
}


def _cell(res):
    if res is LITERAL:
        return NAN_BITS, True
    return bits(res), False


def get_indices(dps, l_bound, r_bound, init):  # base.go:432-482
    if init >= len(dps) or init < 0:
        return -1, -1, False
    l, r = init, -1
    left_bound = False
    for i, (t, _) in enumerate(dps[init:]):
        if not left_bound:
            if t < l_bound:
                continue
            left_bound = True
            l = i
        if t <= r_bound:
            continue
        r = i
        break
    if r == -1:
        r = len(dps)
    else:
        r = r + init
    if left_bound:
        l = l + init
    else:
        return l, r, False
    return l, r, True


def procedural(fn, ts, vals, start, step, nsteps, range_ns, param=0.0):
    """One series through singleProcess's loop (base.go:382-420): a list of
    (bits, literal) cells."""
    process = PROCESSORS[fn]
    dps = list(zip(ts, vals))
    init = 0
    end = start
    lo = end - range_ns
    out = []
    for _ in range(nsteps):
        l, r, ok = get_indices(dps, lo, end, init)
        if not ok:
            res = process([], lo, end, range_ns, param)
        else:
            init = l
            res = process(dps[l:r], lo, end, range_ns, param)
        out.append(_cell(res))
        lo += step
        end += step
    return out


# ------------------------------ closed form ------------------------------

def _f_window(fn, w, tk, range_ns, param):
    """f(W) from the function's description in m3gpu.h; w is the window's
    (ts, value) list in row order."""
    good = [(i, t, v) for i, (t, v) in enumerate(w) if not math.isnan(v)]
    if fn in ("sum_over_time", "count_over_time", "avg_over_time"):
        if not good:
            return math.nan if fn == "avg_over_time" else LITERAL
        s = 0.0
        for _, _, v in good:
            s += v
        n = float(len(good))
        return {"sum_over_time": s, "count_over_time": n}.get(fn, s / n)
    if fn in ("min_over_time", "max_over_time"):
        if not good:
            return LITERAL
        pick = go_min if fn == "min_over_time" else go_max
        m = math.inf if fn == "min_over_time" else -math.inf
        for _, _, v in good:
            m = pick(m, v)
        return m
    if fn == "last_over_time":
        return w[-1][1] if w else LITERAL
    if fn in ("stdvar_over_time", "stddev_over_time"):
        if len(good) < 2:
            return LITERAL if fn == "stdvar_over_time" else math.nan
        aux = mean = 0.0
        for n, (_, _, v) in enumerate(good, 1):
            delta = v - mean
            mean += delta / float(n)
            aux += delta * (v - mean)
        var = aux / float(len(good))
        if fn == "stdvar_over_time":
            return var
        return math.sqrt(var) if var >= 0 else math.nan
    if fn in ("rate", "increase", "delta"):
        if len(w) < 2 or len(good) < 2:
            return LITERAL
        counter = fn != "delta"
        (i0, t0, v0), (i1, t1, v1) = good[0], good[-1]
        correction, last = 0.0, 0.0
        for _, _, v in good:
            if counter and v < last:
                correction += last
            last = v
        to_start = float(t0 - (tk - range_ns)) / 1e9
        to_end = float(tk - t1) / 1e9
        sampled = float(t1 - t0) / 1e9
        gap = _div(sampled, float(i1 - i0))
        result = v1 - v0 + correction
        if counter and result > 0 and v0 >= 0:
            to_zero = sampled * _div(v0, result)
            if to_zero < to_start:
                to_start = to_zero
        total = sampled
        total += to_start if to_start < gap * 1.1 else gap / 2
        total += to_end if to_end < gap * 1.1 else gap / 2
        result = result * _div(total, sampled)
        if fn == "rate":
            result = _div(result, duration_seconds(range_ns))
        return result
    if fn in ("irate", "idelta"):
        if len(w) < 2 or len(good) < 2:
            return LITERAL
        (_, t0, v0), (_, t1, v1) = good[-2], good[-1]
        if fn == "idelta":
            return v1 - v0
        if t1 == t0:
            return LITERAL
        return _div(v1 if v1 < v0 else v1 - v0, duration_seconds(t1 - t0))
    if fn in ("resets", "changes"):
        if not w or all(math.isnan(v) for _, v in w[1:]):
            return LITERAL
        seq = [v for _, _, v in good]
        pairs = zip(seq, seq[1:])
        if fn == "resets":
            return float(sum(b < a for a, b in pairs))
        return float(sum(b != a for a, b in pairs))
    assert fn in ("deriv", "predict_linear")
    if len(w) < 2:
        return LITERAL
    if len(good) == 1:
        return LITERAL if fn == "deriv" else math.nan
    t_ref = good[0][1] if fn == "deriv" and good else tk
    n = sx = sy = sxy = sxx = 0.0
    for _, t, v in good:
        x = float(t - t_ref) / 1e9
        n += 1.0
        sy += v
        sx += x
        sxy += x * v
        sxx += x * x
    slope = _div(sxy - _div(sx * sy, n), sxx - _div(sx * sx, n))
    if fn == "deriv":
        return slope
    return slope * param + (_div(sy, n) - _div(slope * sx, n))


def windows(ts, vals, start, step, nsteps, range_ns, row_err=0):
    """(W_0 .. W_{nsteps-1}, err): the windows of one series as lists of
    (ts, value), or None with the error that fails it. row_err fails the
    series wherever its points lie; a point at or before its predecessor,
    among those up to and including the first past t_last, is
    OUT_OF_ORDER."""
    t_last = start + (nsteps - 1) * step
    if row_err:
        return None, row_err
    read = []
    prev = None
    for t, v in zip(ts, vals):
        if prev is not None and t <= prev:
            return None, OUT_OF_ORDER
        prev = t
        if t > t_last:
            break
        read.append((t, v))
    times = [t for t, _ in read]  # increasing: the set is a slice
    out = []
    for k in range(nsteps):
        tk = start + k * step
        out.append(read[bisect.bisect_left(times, tk - range_ns):
                        bisect.bisect_right(times, tk)])
    return out, 0


def closed_form_many(fns, ts, vals, start, step, nsteps, range_ns, param=0.0,
                     row_err=0):
    """closed_form for several functions over the same windows: a dict fn ->
    cells, and err."""
    wins, err = windows(ts, vals, start, step, nsteps, range_ns, row_err)
    if err:
        return {fn: [(NAN_BITS, True)] * nsteps for fn in fns}, err
    return {fn: [_cell(_f_window(fn, w, start + k * step, range_ns, param))
                 for k, w in enumerate(wins)] for fn in fns}, 0


def closed_form(fn, ts, vals, start, step, nsteps, range_ns, param=0.0,
                row_err=0):
    """What the kernel computes for one series (m3gpu.h): (cells, err) with
    cells a list of (bits, literal); a failed series' column is all
    NAN_BITS."""
    cells, err = closed_form_many([fn], ts, vals, start, step, nsteps,
                                  range_ns, param, row_err)
    return cells[fn], err
