"""Reference-shaped iteration over decoded batches.

The GPU engine returns decoded batches as SoA arrays; callers ported from
the reference often want the `encoding.ReaderIterator` shape
(dbnode/encoding/types.go:197-203: Next/Current/Err/Close) or, for a query,
the `encoding.SeriesIterator` shape (types.go: Next/Current/Err/Start/End/
Close). These wrappers give those shapes over rows the GPU already computed —
host logic only, no compute, see INTEGRATION.md §3 for the Go-side equivalent:

  - SliceReaderIterator / BatchIterators walk DECODED rows (one stream
    each); they merge nothing;
  - SeriesIterator / BatchSeriesIterators walk MERGED rows, the output of
    m3gpu_series_merge_batch_dev (engine.series_merge_dev /
    fetch_series_dev): the replica merge, the block stitching, the range
    filter and the equal-timestamp strategy all happened on the GPU, and the
    wrapper only steps through the result;
  - StepIter walks the step x series matrix of
    m3gpu_step_consolidate_batch_dev / m3gpu_decode_steps_batch_dev in the
    `block.StepIter` shape.

ReaderIterator semantics mirrored:
  - Next() advances and reports whether a point is available
    (iterator.go:81-100: first Next positions on the first point);
  - Current() returns (timestamp_ns, value, unit) for the current point
    and is only valid after a true Next() (types.go:200). The unit is the
    point's own when the iterator was built with the `units` rows of
    m3gpu_decode_batch_full_dev, the constructor's `unit` otherwise;
    CurrentAnnotation()
    gives the sticky annotation the reference returns as Current()'s third
    value (iterator.go:226-231) when the iterator was built with the
    annotation-set events of m3gpu_decode_batch_dev_ann;
  - Err() returns the sticky per-series error (the engine's
    M3GPU_SERIES_* code mapped to a string, or None);
  - Close() releases references (pooling is the caller's concern here).
"""
import numpy as np

from .engine import SERIES_ERRORS


class SliceReaderIterator:
    """`encoding.ReaderIterator` over one decoded series row."""

    def __init__(self, ts, vals, count, err=0, unit=1, ann_events=None,
                 units=None):
        self._ts = ts
        self._vals = vals
        self._n = int(count)
        self._err = int(err)
        self._unit = unit
        # optional per-point units (one row of decode_batch_full_dev's
        # out_units): what Current() reports instead of `unit`
        self._units = units
        self._i = -1
        # annotation-set events [(point_idx, bytes)] in stream order
        # (engine.parse_ann_region); carried forward like PrevAnt
        self._ann_events = ann_events or []
        self._ann_j = 0
        self._ann = None

    def Next(self):
        if self._err != 0:
            return False
        if self._i + 1 >= self._n:
            return False
        self._i += 1
        while (self._ann_j < len(self._ann_events) and
               self._ann_events[self._ann_j][0] <= self._i):
            self._ann = self._ann_events[self._ann_j][1]
            self._ann_j += 1
        return True

    def Current(self):
        if self._i < 0 or self._i >= self._n:
            raise RuntimeError("Current() before a successful Next()")
        unit = self._unit if self._units is None else int(self._units[self._i])
        return int(self._ts[self._i]), float(self._vals[self._i]), unit

    def CurrentAnnotation(self):
        """The reference Current()'s third return (sticky PrevAnt,
        iterator.go:226-231): bytes or None."""
        if self._i < 0 or self._i >= self._n:
            raise RuntimeError("CurrentAnnotation() before a successful Next()")
        return self._ann

    def Err(self):
        if self._err == 0:
            return None
        return SERIES_ERRORS.get(self._err, f"error {self._err}")

    def Close(self):
        self._ts = self._vals = self._units = None
        self._n = 0


class BatchIterators:
    """Per-series ReaderIterators over a decoded batch (SoA rows).

    Accepts numpy arrays or torch CPU tensors of shape [nseries, stride]
    plus per-series counts/errs, e.g. the (moved-to-host) outputs of
    `decode_batch_dev` or `fileset_ingest_dev`."""

    def __init__(self, ts, vals, counts, errs=None, unit=1, ann_regions=None,
                 units=None):
        self._ts = np.asarray(ts)
        self._vals = np.asarray(vals)
        self._counts = np.asarray(counts)
        self._errs = np.asarray(errs) if errs is not None else None
        self._unit = unit
        # optional [nseries, ann_stride] uint8 regions from
        # m3gpu_decode_batch_dev_ann
        self._ann = np.asarray(ann_regions) if ann_regions is not None else None
        # optional [nseries, stride] uint8 per-point units from
        # m3gpu_decode_batch_full_dev
        self._units = np.asarray(units) if units is not None else None

    def __len__(self):
        return len(self._counts)

    def iterator(self, i):
        err = int(self._errs[i]) if self._errs is not None else 0
        events = None
        if self._ann is not None:
            from .engine import parse_ann_region
            events = parse_ann_region(self._ann[i])
        units = self._units[i] if self._units is not None else None
        return SliceReaderIterator(self._ts[i], self._vals[i],
                                   self._counts[i], err, self._unit, events,
                                   units)

    def __iter__(self):
        for i in range(len(self)):
            yield self.iterator(i)


class SeriesIterator:
    """`encoding.SeriesIterator` over one merged row of
    m3gpu_series_merge_batch_dev. The series' error is sticky as in the
    reference (series_iterator.go:74-91), but the points the merge emitted
    before it stay readable: Next() turns false behind the last of them and
    Err() then names the error. Annotations are not carried through the
    merge, so there is no FirstAnnotation()."""

    def __init__(self, ts, vals, count, err=0, start_ns=0, end_ns=0, unit=1,
                 units=None):
        self._ts = ts
        self._vals = vals
        self._units = units
        self._n = int(count)
        self._err = int(err)
        self._start = int(start_ns)
        self._end = int(end_ns)
        self._unit = unit
        self._i = -1
        self._closed = False

    def Next(self):
        if self._closed or self._i + 1 >= self._n:
            self._i = self._n
            return False
        self._i += 1
        return True

    def Current(self):
        if self._i < 0 or self._i >= self._n:
            raise RuntimeError("Current() before a successful Next()")
        unit = self._unit if self._units is None else int(self._units[self._i])
        return int(self._ts[self._i]), float(self._vals[self._i]), unit

    def Err(self):
        if self._err == 0:
            return None
        return SERIES_ERRORS.get(self._err, f"error {self._err}")

    def Start(self):
        """StartInclusive of the query range (0: unfiltered)."""
        return self._start

    def End(self):
        """EndExclusive of the query range (0: unfiltered)."""
        return self._end

    def Close(self):
        self._closed = True
        self._ts = self._vals = self._units = None
        self._n = 0


class BatchSeriesIterators:
    """Per-series SeriesIterators over a merged batch: numpy arrays or torch
    CPU tensors [nseries, out_stride] plus counts/errs, e.g. the
    (moved-to-host) outputs of engine.series_merge_dev or fetch_series_dev,
    with the range the merge was given."""

    def __init__(self, ts, vals, counts, errs=None, start_ns=0, end_ns=0,
                 unit=1, units=None):
        self._ts = np.asarray(ts)
        self._vals = np.asarray(vals)
        self._counts = np.asarray(counts)
        self._errs = np.asarray(errs) if errs is not None else None
        self._units = np.asarray(units) if units is not None else None
        self._start = start_ns
        self._end = end_ns
        self._unit = unit

    def __len__(self):
        return len(self._counts)

    def iterator(self, i):
        err = int(self._errs[i]) if self._errs is not None else 0
        units = self._units[i] if self._units is not None else None
        return SeriesIterator(self._ts[i], self._vals[i], self._counts[i],
                              err, self._start, self._end, self._unit, units)

    def __iter__(self):
        for i in range(len(self)):
            yield self.iterator(i)


class StepIter:
    """`block.StepIter` (query/block/types.go: Next/Current/StepCount/Err)
    over the step x series matrix of m3gpu_step_consolidate_batch_dev or
    m3gpu_decode_steps_batch_dev (engine.step_consolidate_dev,
    decode_steps_dev, fetch_steps_dev), moved to the host: the consolidation
    happened on the GPU and the wrapper only steps through the rows.
    Current() returns (step time in ns, the step's column: one float64 per
    series, a view). As in the reference (encoded_step_iterator_generic.go:
    156-158,191-194) one series' error fails the block: Next() is false from
    the start and Err() names the first failed series. The matrix keeps the
    other series' columns; series_errors=False walks them, the failed
    series' columns being all NaN.
    The matrix of m3gpu_temporal_batch_dev (engine.temporal_dev, temporal,
    fetch_temporal_dev) has the same shape, NaN pattern and errs, and is
    walked unchanged: Current() is then the temporal function's column for
    that step, what the temporal node's builder hands on (temporal/base.go:
    289-306)."""

    def __init__(self, steps, errs, start_ns, step_ns, series_errors=True):
        self._steps = np.asarray(steps)
        self._start = int(start_ns)
        self._step = int(step_ns)
        self._k = -1
        self._err = None
        errs = np.asarray(errs)
        bad = np.nonzero(errs)[0]
        if series_errors and len(bad):
            code = int(errs[bad[0]])
            self._err = (f"series {int(bad[0])}: "
                         f"{SERIES_ERRORS.get(code, f'error {code}')}")

    def StepCount(self):
        return self._steps.shape[0]

    def Next(self):
        if self._err is not None or self._k + 1 >= self.StepCount():
            self._k = self.StepCount()
            return False
        self._k += 1
        return True

    def Current(self):
        if self._k < 0 or self._k >= self.StepCount():
            raise RuntimeError("Current() before a successful Next()")
        return self._start + self._k * self._step, self._steps[self._k]

    def Err(self):
        return self._err

    def Close(self):
        self._steps = self._steps[:0]
