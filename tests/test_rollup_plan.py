"""The rollup plan builder (m3_amd/csrc/rollup_plan.h: qs, qidx, exact_cap,
extreme_cap) on the CPU: tests/rollup_plan_driver.cpp is compiled as a
stand-alone program with the address and undefined-behaviour sanitizers, run
as a child process, and every field is compared with a python restatement of
the documented rules."""
import json
import math
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
QCAP = 512

AGG = dict(last=1, min=2, max=3, mean=4, median=5, count=6, sum=7, sumsq=8,
           stdev=9, p10=10, p20=11, p30=12, p40=13, p50=14, p60=15, p70=16,
           p80=17, p90=18, p95=19, p99=20, p999=21, p9999=22, p25=23, p75=24)
QUANTILE = dict(median=0.5, p10=0.1, p20=0.2, p25=0.25, p30=0.3, p40=0.4,
                p50=0.5, p60=0.6, p70=0.7, p75=0.75, p80=0.8, p90=0.9,
                p95=0.95, p99=0.99, p999=0.999, p9999=0.9999)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path_factory.mktemp("rollup_plan") / "rollup_plan_driver")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(HERE, "rollup_plan_driver.cpp"), "-o", exe],
                   check=True)

    def run(aggs, eps, every=1024):
        r = subprocess.run([exe, repr(eps), str(every)] +
                           [str(AGG[a]) for a in aggs],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    return run


def exact_cap_py(qs, eps):
    """Last bucket size below which the CKMS compress threshold
    (stream.go:362-385, int64 truncation) never reaches 2."""
    if not qs:
        return QCAP
    for v in range(4, QCAP + 2):
        for mr in range(v + 1):
            thr = min(int(2.0 * eps * mr / q) if mr >= int(q * v)
                      else int(2.0 * eps * (v - mr) / (1.0 - q)) for q in qs)
            if thr >= 2:
                return v - 1
    return QCAP


def all_resolve_to_max(qs, n):
    if n <= 3:      # quantilesFromBuf: index int(q*n), clamped to the last
        return all(min(int(q * n), n - 1) == n - 1 for q in qs)
    k = 0           # calcQuantiles walk: one emission per sample
    for i, q in enumerate(qs):
        k = math.ceil(q * n) if i == 0 else max(math.ceil(q * n), k + 1)
        if min(k, n) != n:
            return False
    return True


def extreme_cap_py(qs, cap):
    n = 0
    while qs and n < min(cap, QCAP) and all_resolve_to_max(qs, n + 1):
        n += 1
    return n


def plan_py(aggs, eps):
    qs = sorted({QUANTILE[a] for a in aggs if a in QUANTILE})
    cap = exact_cap_py(qs, eps)
    return dict(nq=len(qs), qs=qs,
                qidx=[qs.index(QUANTILE[a]) if a in QUANTILE else -1
                      for a in aggs],
                exact_cap=cap, extreme_cap=extreme_cap_py(qs, cap))


# quantile set -> (exact_cap, extreme_cap) at eps 1e-3 and at eps 1e-2
TABLE = [
    (["p99"], (10, 10), (3, 3)),
    (["median", "p95", "p99"], (499, 2), (49, 2)),
    (["p90", "p99"], (99, 9), (9, 9)),
    (["p95", "p99", "p999"], (50, 19), (5, 5)),
    (["p9999"], (3, 3), (3, 3)),
]


@pytest.mark.parametrize("qset,at_1e3,at_1e2", TABLE,
                         ids=["+".join(t[0]) for t in TABLE])
def test_plan_caps_table(driver, qset, at_1e3, at_1e2):
    # non-quantile aggs around and between the quantiles must not matter
    aggs = ["sum"] + qset[:1] + ["max"] + qset[1:] + ["count"]
    for eps, want in ((1e-3, at_1e3), (1e-2, at_1e2)):
        got = driver(aggs, eps)
        assert (got["exact_cap"], got["extreme_cap"]) == want, (eps, got)
        assert got == plan_py(aggs, eps), eps


def test_plan_without_quantiles(driver):
    for aggs in (["sum", "min", "max", "count"], []):
        got = driver(aggs, 1e-3)
        assert got == dict(nq=0, qs=[], qidx=[-1] * len(aggs),
                           exact_cap=QCAP, extreme_cap=0)


def test_plan_duplicate_quantiles_share_an_index(driver):
    aggs = ["median", "p50", "p95"]
    got = driver(aggs, 1e-3)
    assert got["qs"] == [0.5, 0.95]
    assert got["qidx"] == [0, 0, 1]
    assert got == plan_py(aggs, 1e-3)


def test_plan_unsorted_full_width(driver):
    """MAX_AGGS aggs, quantiles given in descending order with repeats."""
    aggs = ["p9999", "p999", "p99", "p95", "p90", "p80", "p75", "p70", "p60",
            "median", "p50", "p40", "p30", "p25", "p20", "p10"]
    for eps in (1e-3, 1e-2):
        got = driver(aggs, eps)
        assert got["nq"] == 15
        assert got == plan_py(aggs, eps)
