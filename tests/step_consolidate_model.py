"""Plain-Python restatements of the reference's step consolidation: test
infrastructure for test_step_consolidate_cpu.py and
test_step_consolidate_gpu.py, written from the reference sources
(src/query/storage/m3):

  - consolidators/step_consolidator.go:30-136  StepLookbackConsolidator,
                                               removeStale
  - consolidators/types.go:207-216             TakeLast
  - encoded_step_iterator_generic.go:63-119    nextForStep
  - encoded_step_iterator_generic.go:163-189   nextSequential's per-series loop

Two levels. `procedural_steps` is the reference's procedure step by step
over one series' points in iterator order. `closed_form` is what the kernels
are specified to compute (m3gpu.h), with the points-read, error and
all-NaN-column rules; on increasing timestamps without an error the two
agree, which test_step_consolidate_cpu.py checks.

Values travel as uint64 bit patterns where they are compared: a step without
a value holds NAN_BITS (Go's math.NaN()).
"""
import math
import struct

NAN_BITS = 0x7FF8000000000001
OUT_OF_ORDER = 100  # M3GPU_SERIES_OUT_OF_ORDER


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


GO_NAN = from_bits(NAN_BITS)


def take_last(dps):  # types.go:207-216
    for _, v in reversed(dps):
        if not math.isnan(v):
            return v
    return GO_NAN


def remove_stale(earliest, dps):  # step_consolidator.go:30-41
    for i, (t, _) in enumerate(dps):
        if not t < earliest:
            return dps[i:]
    return []


class StepLookbackConsolidator:
    """step_consolidator.go:47-136 with fn = TakeLast; datapoints are
    (timestamp, value) pairs."""

    def __init__(self, lookback, step, start, fn=take_last):
        self.step = step
        self.earliest = start - lookback  # :70
        self.datapoints = []
        self.unconsumed = []
        self.fn = fn

    def add_point(self, t, v):  # :80-87
        if t < self.earliest:
            return
        self.datapoints.append((t, v))

    def buffer_step(self):  # :90-108
        self.earliest += self.step
        val = self.fn(self.datapoints)
        self.datapoints = list(remove_stale(self.earliest, self.datapoints))
        self.unconsumed.append(val)

    def buffer_step_count(self):  # :111-113
        return len(self.unconsumed)

    def consolidate_and_move_to_next(self):  # :117-136
        if not self.unconsumed:
            return self.fn([])
        return self.unconsumed.pop(0)


class _Peek:
    def __init__(self):
        self.started = False
        self.finished = False
        self.point = None


def next_for_step(peek, it, collector, step_time):
    """encoded_step_iterator_generic.go:63-119. `it` is a Python iterator
    over (timestamp, value); its exhaustion is iter.Next() == false."""
    if peek.finished:
        return
    if peek.started:
        t, v = peek.point
        if t > step_time:
            return
        collector.add_point(t, v)
        peek.started = False
        if t == step_time:
            return
    for t, v in it:
        if not t > step_time:
            peek.started = False
            collector.add_point(t, v)
        else:
            peek.point = (t, v)
            peek.started = True
            return
    peek.finished = True


def procedural_steps(ts, vals, start, step, nsteps, lookback):
    """One series through nextSequential's loop (:171-179) and the
    encodedStepIter.update() reads: the value bits of every step."""
    collector = StepLookbackConsolidator(lookback, step, start)
    peek = _Peek()
    it = iter(list(zip(ts, vals)))
    for k in range(nsteps):
        next_for_step(peek, it, collector, start + k * step)
        collector.buffer_step()
    assert collector.buffer_step_count() == nsteps
    return [bits(collector.consolidate_and_move_to_next())
            for _ in range(nsteps)]


def closed_form(ts, vals, start, step, nsteps, lookback, row_err=0,
                dedupe=False):
    """What the kernels compute for one series (m3gpu.h): (step value bits,
    err). Points are read up to and including the first with ts > t_last; a
    point at or before its predecessor is OUT_OF_ORDER (dedupe=True, the
    fused entry's streams: an equal one is skipped instead); row_err comes
    after the points; any error that is reached makes the column all NaN."""
    t_last = start + (nsteps - 1) * step
    read = []
    err = 0
    stopped = False
    prev = None
    for t, v in zip(ts, vals):
        if prev is not None and t <= prev:
            if dedupe and t == prev:
                continue
            err = OUT_OF_ORDER
            break
        prev = t
        if t > t_last:
            stopped = True
            break
        read.append((t, v))
    if not stopped and not err:
        err = row_err
    if err:
        return [NAN_BITS] * nsteps, err
    out = []
    for k in range(nsteps):
        tk = start + k * step
        val = NAN_BITS
        for t, v in reversed(read):
            if t > tk or math.isnan(v):
                continue
            if t >= tk - lookback:
                val = bits(v)
            break
        out.append(val)
    return out, 0


def stitch_blocks(blocks):
    """The one-replica SeriesIterator over a series' blocks, each (ts, vals,
    err): the points in order with what ends them, as (ts, vals, err) for
    closed_form(dedupe=True) -- a block's error comes after its points and
    ends the series there."""
    ts, vals = [], []
    for b_ts, b_vals, b_err in blocks:
        ts.extend(b_ts)
        vals.extend(b_vals)
        if b_err:
            return ts, vals, b_err
    return ts, vals, 0
