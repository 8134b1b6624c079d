"""Host-side unit tests for bench.py's sharding/config logic (the N>1 code
path the driver launches via torch.distributed.run — SURVEY.md §8e)."""
import importlib.util
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def test_shard_range_partitions_exactly():
    for n in (1, 7, 64, 1_000_000, 8_000_001):
        for world in (1, 2, 3, 8):
            got = [bench.shard_range(n, world, r) for r in range(world)]
            # contiguous, disjoint, covering
            assert got[0][0] == 0 and got[-1][1] == n
            for (a, b), (c, d) in zip(got, got[1:]):
                assert b == c and a <= b
            sizes = [hi - lo for lo, hi in got]
            # balanced within 1
            assert max(sizes) - min(sizes) <= 1


def test_plain_run_is_lean_by_default():
    args = bench.parse_args(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert (args.steps, args.warmup) == (4, 2)
    assert args.full is False and args.dump_outputs is None
    args = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert args.full is True and args.dump_outputs == "d"


def test_sample_series_is_fixed_and_follows_row_order():
    import numpy as np
    import torch
    n = 1000
    s1, r1 = bench.sample_series(torch, n, 64, "cpu")
    s2, r2 = bench.sample_series(torch, n, 64, "cpu")
    assert np.array_equal(s1, s2) and np.array_equal(s1, np.unique(s1))
    assert len(s1) == n and np.array_equal(r1.numpy(), s1)
    # the budget bounds the sample
    s3, _ = bench.sample_series(torch, n, bench.DUMP_BUDGET_BYTES // 10, "cpu")
    assert len(s3) == 10
    # output row i holds series order[i]: rows must point back at the sample
    order = torch.from_numpy(np.random.default_rng(1).permutation(n)).to(torch.int32)
    s4, r4 = bench.sample_series(torch, n, bench.DUMP_BUDGET_BYTES // 10, "cpu",
                                 order)
    assert np.array_equal(s4, s3)
    assert np.array_equal(order[r4].numpy(), s4)


def test_dump_outputs_writes_exact_float_arrays(tmp_path):
    import numpy as np
    import torch
    ns = np.array([[1427162462 * 10**9 + 7, 1427162472 * 10**9]], np.int64)
    bench.dump_outputs(str(tmp_path / "d"), np.array([3]),
                       dict(bench.split_ns("ts", torch.from_numpy(ns)),
                            vals=np.array([[0.1, 2.0]]),
                            counts=np.array([2], np.int32)))
    got = {f: np.load(tmp_path / "d" / f) for f in
           ("ts_sec.npy", "ts_nsec.npy", "vals.npy", "counts.npy", "series.npy")}
    assert got["ts_sec.npy"].dtype == np.float64
    assert got["counts.npy"].dtype == np.float32
    back = got["ts_sec.npy"].astype(np.int64) * 10**9 + got["ts_nsec.npy"].astype(np.int64)
    assert np.array_equal(back, ns)
    assert np.array_equal(got["vals.npy"], [[0.1, 2.0]])
    assert got["series.npy"].tolist() == [3.0]


def test_shard_range_matches_reference_shard_model():
    """Contiguous equal ranges — the bench owns placement, mirroring the
    reference's shard-hash distribution (aggregator/sharding/hash.go:89)
    minus the hashing."""
    lo, hi = bench.shard_range(10, 4, 1)
    assert (lo, hi) == (3, 6)  # 3,3,2,2 with extras to low ranks
