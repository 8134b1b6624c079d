"""Plain-Python restatement of the reference's SeriesIterator over lists:
test infrastructure for test_series_iter_cpu.py and test_series_merge_gpu.py,
written from the reference sources (src/dbnode/encoding):

  - series_iterator.go:74-215   seriesIterator Next/Reset/moveToNext
  - iterators.go:60-262         current, push, tryAddEarliest,
                                moveIteratorToFilterNext, moveToValidNext
  - multi_reader_iterator.go:62-155  the per-replica iterator

Two levels. Each replica is a MultiReaderIterator over a slice of slices with
ONE reader per slice (a block); the seriesIterator merges the replicas.

series_iterate(replicas, start, end, strategy) takes, per replica, a list of
blocks (ts, vals, units, err) and returns (ts, vals, units, err).
"""

OUT_OF_ORDER = 100  # errOutOfOrderIterator
LAST_PUSHED, HIGHEST_VALUE, LOWEST_VALUE, HIGHEST_FREQUENCY = 0, 1, 2, 3
TIME_MAX = 2 ** 63 - 1  # iterators.go:33


class _Replica:
    """multiReaderIterator with one reader per slice. `i` is the position in
    block `b` while the block's reader is in the inner `iters` (has=True)."""

    def __init__(self, blocks):
        self.blocks = blocks
        self.b = -1
        self.i = 0
        self.has = False   # inner iters.len() > 0
        self.more = True   # slicesIter != nil
        self.err = 0
        self.first = True
        self._move_to_next()  # ResetSliceOfSlices, :186-187

    def current(self):
        ts, vals, units, _ = self.blocks[self.b]
        return ts[self.i], vals[self.i], units[self.i]

    def _has_next(self):  # :78-92
        return not self.err and (self.has or self.more)

    def next(self):  # :62-72
        if not self.first:
            if not self._has_next():
                return False
            self._move_to_next()
        self.first = False
        return self._has_next()

    def _move_to_next(self):  # :94-134
        if self.has:
            # moveIteratorsToNext (:136-155) over the one reader: the inner
            # moveToValidNext advances it, validateNext (iterators.go:229-236)
            # rejects a smaller timestamp, an equal one is deduped
            ts, _, _, err = self.blocks[self.b]
            while True:
                prev = ts[self.i]
                if self.i + 1 >= len(ts):
                    # the reader's Next() is false: its error, if any, shows
                    # now (iterators.go:172-176), else it is removed
                    self.has = False
                    if err:
                        self.err = err
                    break
                self.i += 1
                if ts[self.i] < prev:
                    self.has = False
                    self.err = OUT_OF_ORDER
                    break
                if ts[self.i] != prev:
                    break
        if self.has or self.err:  # :98-101
            return
        while True:
            if self.b + 1 >= len(self.blocks):  # :104-109
                self.more = False
                return
            self.b += 1
            ts, _, _, err = self.blocks[self.b]
            if len(ts):
                # pushed into a reset `iters` (earliestAt = max): taken as it
                # is, nothing is compared across the boundary (:118-120)
                self.i = 0
                self.has = True
                return
            if err and not self.err:  # :121-126
                self.err = err
            if self.err:  # :130
                return


def _less(strategy, earliest):
    """The `less` of current()'s sort.Slice calls (iterators.go:63-95) over
    the replicas' current values, by index into `earliest`."""
    vals = [rep.current()[1] for rep in earliest]
    if strategy == HIGHEST_VALUE:
        return lambda a, b: vals[a] < vals[b]
    if strategy == LOWEST_VALUE:
        return lambda a, b: vals[a] > vals[b]
    # map[float64]int: keys compare with ==, so -0.0 and 0.0 are one key and
    # a NaN is never found again (frequency 0)
    freq = [sum(1 for w in vals if w == v) for v in vals]
    return lambda a, b: freq[a] < freq[b]


def _sort_earliest(strategy, earliest):
    """sort.Slice at n <= 4: both of Go's implementations (the pre-1.19
    quickSort, which insertion-sorts below 12 elements and shell-passes only
    from 7 on, and pdqsort, which insertion-sorts up to 12) are this loop."""
    idx = list(range(len(earliest)))
    less = _less(strategy, earliest)
    for i in range(1, len(idx)):
        j = i
        while j > 0 and less(idx[j], idx[j - 1]):
            idx[j], idx[j - 1] = idx[j - 1], idx[j]
            j -= 1
    earliest[:] = [earliest[k] for k in idx]


def series_iterate(replicas, start=0, end=0, strategy=LAST_PUSHED,
                   removal="sorted"):
    """removal="slot" is a deliberately WRONG variant for the tests: replicas
    that run out in one step leave `values` in `values` order instead of the
    order current()'s sort left in `earliest`."""
    st = dict(values=[], earliest=[], at=TIME_MAX, err=0)
    filtering = start != 0 and end != 0  # series_iterator.go:145

    def reset():  # iterators.go:242-256
        st["values"] = []
        st["earliest"] = []
        st["at"] = TIME_MAX

    def try_add_earliest(rep):  # iterators.go:125-138
        t = rep.current()[0]
        if t == st["at"]:
            st["earliest"].append(rep)
        elif t < st["at"]:
            st["earliest"] = [rep]
            st["at"] = t

    def filter_next(rep):  # iterators.go:140-158
        nxt = True
        while nxt:
            t = rep.current()[0]
            if t < start:
                nxt = rep.next()
                continue
            if t >= end:
                nxt = False
                break
            break
        return nxt

    def push(rep):  # iterators.go:115-123
        if filtering and not filter_next(rep):
            return False
        st["values"].append(rep)
        try_add_earliest(rep)
        return True

    def move_to_valid_next():  # iterators.go:160-227
        prev_at = st["at"]
        walk = list(st["earliest"])
        if removal == "slot":
            walk = [v for v in st["values"] if any(v is e for e in walk)]
        for rep in walk:
            nxt = rep.next()
            if nxt and filtering:
                nxt = filter_next(rep)
            if rep.err:
                reset()
                return False, rep.err
            if nxt:
                continue
            values = st["values"]
            idx = next(k for k, v in enumerate(values) if v is rep)
            values[idx] = values[-1]
            values.pop()
        st["earliest"] = []
        if not st["values"]:
            reset()
            return False, 0
        st["at"] = TIME_MAX
        for rep in st["values"]:
            try_add_earliest(rep)
        if filtering and not (start <= st["at"] < end):
            return move_to_valid_next()
        if st["at"] < prev_at:  # validateNext :229-236
            reset()
            return False, OUT_OF_ORDER
        return True, 0

    # Reset, series_iterator.go:159-169
    for blocks in replicas:
        rep = _Replica(blocks)
        if not rep.next() or not push(rep):
            if rep.err:
                st["err"] = rep.err

    out_ts, out_vals, out_units = [], [], []
    first = True
    while True:  # Next, series_iterator.go:74-83
        if not first:
            if st["err"] or not st["values"]:
                break
            while True:  # moveToNext :196-215
                prev = st["at"]
                nxt, err = move_to_valid_next()
                if err:
                    st["err"] = err
                    break
                if not nxt or st["at"] != prev:
                    break
        first = False
        if st["err"] or not st["values"]:
            break
        # Current -> iterators.current(), iterators.go:60-109
        if strategy != LAST_PUSHED:
            _sort_earliest(strategy, st["earliest"])
        t, v, u = st["earliest"][-1].current()
        out_ts.append(t)
        out_vals.append(v)
        out_units.append(u)
    return out_ts, out_vals, out_units, st["err"]
