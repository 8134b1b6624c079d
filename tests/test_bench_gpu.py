"""bench.py --dump-outputs on the GPU: the dumped sample is what the timed
decode returned for exactly the workload series it names, under both blob
layouts, and a plain run leaves the cpu_baseline leg to --full."""
import json

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

# > one 64-lane wave group per kind, not a multiple of 64, two encode chunks
NSERIES, NPTS, CHUNK = 1500, 70, 1024


def _run(capsys, tmp_path, name, *extra):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / name
    bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1",
                "--nseries", str(NSERIES), "--npts", str(NPTS),
                "--chunk", str(CHUNK), "--dump-outputs", str(out), *extra])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return line, {p.stem: np.load(p) for p in out.iterdir()}


@pytest.mark.parametrize("layout", ["sorted", "index"])
def test_dump_outputs_are_the_named_series(capsys, tmp_path, layout):
    line, got = _run(capsys, tmp_path, layout, "--layout", layout)
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["cpu_baseline"] is None  # plain run: --full only
    series = got["series"].astype(np.int64)
    assert len(series) == NSERIES and sum(a.nbytes for a in got.values()) < 64e6
    from m3_amd import workload
    ts, vals = (np.concatenate(a) for a in zip(
        workload.gen_chunk(0, CHUNK, NPTS),
        workload.gen_chunk(CHUNK, NSERIES - CHUNK, NPTS)))
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.all(got["errs"] == 0) and np.all(got["counts"] == NPTS)
    g_ts = got["ts_sec"].astype(np.int64) * 10**9 + got["ts_nsec"].astype(np.int64)
    assert np.array_equal(g_ts, ts[series])
    assert np.array_equal(got["vals"].view(np.uint64), vals[series].view(np.uint64))
