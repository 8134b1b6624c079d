"""The value domain of the fused decode->rollup on every tier: signed zeros,
NaN payloads, infinities, magnitudes whose square overflows, subnormals, and
for counters every float64 the int64 cast has to survive
(tests/rollup_value_cases.py builds the batches, tests/test_rollup_values_cpu.py
pins the expected side and the batches' own conditions).

One launch per (path, naggs parity). Outputs and errs are prefilled with a
sentinel. Expected is the oracle's rollup of the CPU-decoded points.
Selection outputs (last, min, max, count, every quantile) and the window
timestamps compare bit for bit. Arithmetic outputs (sum, sumsq, mean, stdev)
compare bit for bit too, except where the oracle's result is a NaN: the GPU's
must then be a NaN, and its sign and payload are the hardware's (x86 gives
0xFFF8... for inf - inf; DESIGN.md section 4 notes what gfx950 was seen to
give, and the test prints the patterns it meets)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollup_value_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF8DEADBEEF5A5A      # a NaN payload no rollup produces
SENTINEL32 = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    t.cuda.set_device("cuda:0")
    return t


@pytest.fixture(scope="module")
def engine():
    from m3_amd import engine as e
    return e


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("parity", ["odd", "even"])
@pytest.mark.parametrize("path", list(cases.PATHS))
def test_rollup_values(torch, engine, path, parity):
    B = cases.batch(path)
    aggs = cases.aggs_of(path, parity)
    want, want_wts = cases.expected(path, parity)
    blob, offsets, lens = engine.pack_streams(B.streams)

    dev = "cuda:0"
    d_blob = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(dev)
    shape = (cases.NSERIES, cases.NBUCKETS, len(aggs))
    out = torch.full(shape, SENTINEL, dtype=torch.int64,
                     device=dev).view(torch.float64)
    wts = torch.full(shape[:2], SENTINEL, dtype=torch.int64, device=dev)
    errs = torch.full(shape[:1], SENTINEL32, dtype=torch.int32, device=dev)
    engine.rollup_batch_dev(d_blob, d_off, d_lens, cases.METRIC[B.metric],
                            cases.WINDOW, cases.NBUCKETS, aggs, out, wts, errs,
                            int_optimized=False)
    torch.cuda.synchronize()
    got, got_wts, got_errs = out.cpu().numpy(), wts.cpu().numpy(), errs.cpu().numpy()

    g, w = _u64(got), _u64(want)
    arith = np.array([a in cases.ARITHMETIC for a in aggs])
    bad, nan_bits = [], {}
    for i in range(cases.NSERIES):
        cls = B.where.get(i, "clean")
        if got_errs[i] != 0:
            bad.append((i, cls, "err", int(got_errs[i])))
            continue
        if not np.array_equal(got_wts[i], want_wts[i]):
            bad.append((i, cls, "window_ts"))
        # the one exception: an arithmetic output the oracle gives as NaN
        loose = arith[None, :] & np.isnan(want[i])
        if i not in B.where:
            assert not loose.any()     # clean neighbours: all bits, always
        for b, k in zip(*np.nonzero(loose)):
            nan_bits.setdefault(cls, set()).add(hex(g[i, b, k]))
            if not np.isnan(got[i, b, k]) or g[i, b, k] == np.uint64(SENTINEL):
                bad.append((i, cls, int(b), aggs[k], hex(g[i, b, k]), "NaN"))
        for b, k in zip(*np.nonzero(~loose & (g[i] != w[i]))):
            bad.append((i, cls, int(b), aggs[k], hex(g[i, b, k]),
                        hex(w[i, b, k])))
    print("arithmetic NaN bit patterns seen:",
          {c: sorted(v) for c, v in nan_bits.items()})
    assert not bad, "\n".join(str(x) for x in bad[:80])
