"""Generated streams shared by test_decode_full_cpu.py, test_decode_full_gpu.py
and test_merge_units_gpu.py: series with per-point time units, annotations and
a block start in front of the first point, oracle-encoded, and what the ORACLE
decodes from them, which is the reference of every comparison. Generated once,
cached, read-only. No GPU here."""
import ctypes
import functools
import json
import os

import numpy as np

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
START = 1427162400 * 10**9  # whole seconds: initialTimeUnit(START, s) = s
UNIT_NS = {1: 10**9, 2: 10**6, 3: 10**3, 4: 1}
MIXED_COUNTS = (1, 2, 7, 8, 9, 15, 16, 17)
OK, EOF, CAPACITY = 0, 1, 6


class Case:
    """One stream and the oracle's reading of it."""

    def __init__(self, stream, int_optimized, default_unit=1):
        self.stream = bytes(stream)
        self.int_optimized = int_optimized
        self.default_unit = default_unit
        d = oracle.decode_series(self.stream, int_optimized=int_optimized,
                                 default_unit=default_unit,
                                 with_annotations=True)
        self.ts, self.vals, self.units = d["ts"], d["vals"], d["units"]
        for a in (self.ts, self.vals, self.units):
            a.setflags(write=False)
        # annotation-set events [(point, bytes)], the region's content
        self.events = [(p, a) for p, a in enumerate(d["annotations"])
                       if a is not None]
        self.start = int.from_bytes(self.stream[:8], "big", signed=True)

    def __len__(self):
        return len(self.ts)

    def reencode(self):
        """oracle decode -> oracle encode of this stream."""
        anns = [b""] * len(self)
        for p, a in self.events:
            anns[p] = a
        return oracle.encode_series(self.ts, self.vals, units=self.units,
                                    annotations=anns, start_ns=self.start,
                                    int_optimized=self.int_optimized)


def gen_inputs(seed, n):
    """(ts, vals, units, annotations, start) of one series of n points.
    Units are piecewise constant over {1,2,3,4}: a change is drawn at points
    0, 1, 7, 8 and the last with probability 1/2 each and at every other
    point with probability 1/8. Each step is a multiple of the unit in force,
    so no delta loses precision. About one point in five is annotated. One
    series in four starts off the second, where the stream begins without a
    unit and point 0 carries a marker whatever its unit."""
    rng = np.random.default_rng(seed)
    start = START - int(rng.integers(0, 100)) * 10**9
    if seed % 4 == 3:
        start += int(rng.integers(1, 10**9))
    units = np.empty(n, np.uint8)
    ts = np.empty(n, np.int64)
    cur, t = 1, START + int(rng.integers(1, 60)) * 10**9
    for p in range(n):
        edge = p in (0, 1, 7, 8, n - 1)
        if rng.random() < (0.5 if edge else 0.125):
            cur = int(rng.choice([u for u in (1, 2, 3, 4) if u != cur]))
        units[p] = cur
        t += int(rng.integers(1, 60)) * 10**9 \
            + int(rng.integers(0, 1000)) * UNIT_NS[cur]
        ts[p] = t
    kind = seed % 3
    if kind == 0:      # small decimals: int mode when int_optimized
        vals = np.round(rng.random(n) * 1000, int(rng.integers(0, 3)))
    elif kind == 1:    # random doubles: float mode
        vals = rng.standard_normal(n) * 1e6
    else:              # repeats
        vals = np.repeat(np.round(rng.random((n + 2) // 3) * 50, 1), 3)[:n]
    anns = [bytes(rng.integers(0, 256, int(rng.integers(1, 13)),
                               dtype=np.uint8).tobytes())
            if rng.random() < 0.2 else b"" for _ in range(n)]
    return ts, vals, units, anns, start


@functools.lru_cache(maxsize=None)
def series(seed, n, int_optimized):
    ts, vals, units, anns, start = gen_inputs(seed, n)
    stream = oracle.encode_series(ts, vals, units=units, annotations=anns,
                                  start_ns=start, int_optimized=int_optimized)
    return Case(stream, int_optimized)


@functools.lru_cache(maxsize=None)
def batch(nseries, counts, int_optimized=True):
    """nseries cases, case i with counts[i % len(counts)] points."""
    return tuple(series(9000 + i, counts[i % len(counts)], int_optimized)
                 for i in range(nseries))


# every (nseries, counts) the GPU decode tests use
BATCHES = ([(n, MIXED_COUNTS) for n in (1, 63, 64, 65, 257)]
           + [(64, (c,)) for c in (8, 16, 17, 24)])


@functools.lru_cache(maxsize=None)
def golden_full_streams():
    """The reference's own full_streams vectors: int_optimized=False,
    default unit Second."""
    with open(os.path.join(GOLDEN, "encoder_vectors.json")) as f:
        fs = json.load(f)["full_streams"]
    return fs, tuple(Case(bytes(c["stream_bytes"]), False)
                     for c in fs["cases"])


@functools.lru_cache(maxsize=None)
def production_samples():
    import base64
    with open(os.path.join(GOLDEN, "production_streams.json")) as f:
        ps = json.load(f)
    return tuple(Case(base64.b64decode(b), True) for b in ps["samples"])


def oracle_partial(stream, int_optimized=True, default_unit=1, cap=64):
    """(points decoded before the stream's error, -error) for a stream the
    oracle fails on: oracle.decode_series raises and drops the prefix, so the
    C entry is called directly over sentinel-filled outputs."""
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    ts = np.full(cap, -1, np.int64)
    vals = np.zeros(cap, np.float64)
    units = np.zeros(cap, np.uint8)
    P = ctypes.POINTER
    r = oracle.lib().oracle_decode_series(
        buf.ctypes.data_as(P(ctypes.c_uint8)), len(buf),
        1 if int_optimized else 0, default_unit,
        ts.ctypes.data_as(P(ctypes.c_int64)),
        vals.ctypes.data_as(P(ctypes.c_double)),
        units.ctypes.data_as(P(ctypes.c_uint8)), None, None, 0, cap)
    assert r < 0, "stream decodes"
    return int(np.count_nonzero(ts != -1)), int(-r)


# ------------------------------- merge -------------------------------

def merge_inputs(R, nseries=130, stride=12, seed=31):
    """Ragged replicas (some empty) on a small timestamp grid, so equal
    timestamps across replicas are the rule. units[r] is r + 1 everywhere:
    an output unit names the replica its point came from."""
    rng = np.random.default_rng(seed + R)
    ts = np.zeros((R, nseries, stride), np.int64)
    vals = np.zeros((R, nseries, stride), np.float64)
    units = np.zeros((R, nseries, stride), np.uint8)
    counts = np.zeros((R, nseries), np.uint32)
    for r in range(R):
        for i in range(nseries):
            n = int(rng.integers(0, stride + 1))
            t = np.sort(rng.choice(np.arange(1, 20), size=n, replace=False))
            ts[r, i, :n] = START + t * 10**9
            vals[r, i, :n] = 100.0 * (r + 1) + t
            units[r, i, :n] = r + 1
            counts[r, i] = n
    return ts, vals, units, counts


def merge_model(ts, vals, units, counts):
    """The winner rule of MultiReaderIterator (iterators.go, IterateLastPushed)
    restated with units. The `values` order starts as replica order (replicas
    with points only); the earliest timestamp wins, the LAST holder in
    `values` order among equals; a timestamp equal to the previous one is
    dropped; every replica at the earliest advances, and one that runs out is
    replaced by the tail of `values`, which is then looked at again.
    Returns per series (ts, vals, units) lists."""
    R, nseries, _ = ts.shape
    out = []
    for i in range(nseries):
        cur = [0] * R
        order = [r for r in range(R) if counts[r, i] > 0]
        o_ts, o_vals, o_units = [], [], []
        while order:
            earliest, winner = None, None
            for r in order:
                t = int(ts[r, i, cur[r]])
                if earliest is None or t <= earliest:
                    earliest, winner = t, r
            if not o_ts or earliest != o_ts[-1]:
                assert not o_ts or earliest > o_ts[-1]
                o_ts.append(earliest)
                o_vals.append(float(vals[winner, i, cur[winner]]))
                o_units.append(int(units[winner, i, cur[winner]]))
            k = 0
            while k < len(order):
                r = order[k]
                if int(ts[r, i, cur[r]]) == earliest:
                    cur[r] += 1
                    if cur[r] >= counts[r, i]:
                        order[k] = order[-1]
                        order.pop()
                        continue
                k += 1
        out.append((o_ts, o_vals, o_units))
    return out
