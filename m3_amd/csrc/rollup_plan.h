/*
 * rollup_plan.h — the rollup kernels' by-value plan argument, the host code
 * that fills it in, and the exact-quantile index that the builder and the
 * kernels share. Plain C++17, no HIP header: it is compiled on its own by
 * tests/rollup_plan_driver.cpp.
 */
#ifndef M3_ROLLUP_PLAN_H
#define M3_ROLLUP_PLAN_H

#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../include/m3gpu.h"

#define QCAP 512 /* wave-kernel LDS staging capacity per series */
#define MAX_AGGS 16

/* shared by host code and kernels: host+device under hipcc, plain otherwise */
#ifdef __HIPCC__
#include <hip/hip_runtime.h> /* __forceinline__ */
#define M3_HD __host__ __device__
#define M3_INLINE __forceinline__
#else
#define M3_HD
#define M3_INLINE inline
#endif

namespace m3 {

struct RollupPlan {
    int32_t agg_types[MAX_AGGS];
    int8_t qidx[MAX_AGGS];   /* index into qs, or -1 */
    double qs[MAX_AGGS];     /* sorted unique quantiles */
    int32_t nq;
    int32_t naggs;
    /* Largest bucket size for which the production-default CKMS
     * (eps=1e-3, insertAndCompressEvery=1024) provably never compresses
     * for THIS quantile set, so its quantiles are exact order statistics
     * (the calcQuantiles walk). Computed on the host; buckets beyond it
     * flag M3GPU_SERIES_BUCKET_OVERFLOW rather than approximate. */
    int32_t exact_cap;
    /* Largest bucket size for which EVERY requested quantile resolves to
     * the bucket MAX under the reference's walk (all-high quantile sets,
     * e.g. p90+): the lane kernel then needs no value staging at all —
     * running min/max suffice. 0 = extreme mode not applicable. */
    int32_t extreme_cap;
    /* CKMS stream options (quantile/cm/options.go:30-32 defaults:
     * eps=1e-3, insertAndCompressEvery=1024); configurable via the
     * *_opts ABI entries. every is capped at 1024 by validation (the
     * deep-tier LDS buffers are sized for a 2*1024 peak). */
    double eps;
    int32_t every;
};

/* quantile of an aggregation type, or -1 when it is not a quantile */
static inline double agg_quantile_of_host(int32_t t) {
    switch (t) {
    case M3GPU_AGG_MEDIAN: case M3GPU_AGG_P50: return 0.5;
    case M3GPU_AGG_P10: return 0.1;
    case M3GPU_AGG_P20: return 0.2;
    case M3GPU_AGG_P25: return 0.25;
    case M3GPU_AGG_P30: return 0.3;
    case M3GPU_AGG_P40: return 0.4;
    case M3GPU_AGG_P60: return 0.6;
    case M3GPU_AGG_P70: return 0.7;
    case M3GPU_AGG_P75: return 0.75;
    case M3GPU_AGG_P80: return 0.8;
    case M3GPU_AGG_P90: return 0.9;
    case M3GPU_AGG_P95: return 0.95;
    case M3GPU_AGG_P99: return 0.99;
    case M3GPU_AGG_P999: return 0.999;
    case M3GPU_AGG_P9999: return 0.9999;
    default: return -1.0;
    }
}

/* 0-based index into a bucket's n >= 1 sorted values of quantile qs[qi] of
 * the sorted unique list qs, while the CKMS stream never compresses
 * (n <= exact_cap): quantilesFromBuf (stream.go:210-229) for n <= 3, else
 * the closed form of the calcQuantiles walk (:231-277), which emits one
 * sample per quantile: k_i = max(ceil(q_i*n), k_{i-1}+1), index min(k,n)-1. */
M3_HD static M3_INLINE int exact_quantile_index(const double* qs, int qi, int n) {
    if (n <= 3) {
        int idx = (int)(qs[qi] * (double)n);
        return idx < n ? idx : n - 1;
    }
    int k = 0;
    for (int i = 0; i <= qi; i++) {
        int rank = (int)ceil(qs[i] * (double)n);
        k = (i == 0) ? rank : ((rank > k + 1) ? rank : k + 1);
    }
    return (k < n ? k : n) - 1;
}

/* Fill *plan for naggs <= MAX_AGGS aggregation types (the caller bounds
 * naggs). */
static inline void rollup_plan_build(const int32_t* agg_types, int naggs,
                                     double eps, int every, RollupPlan* plan) {
    memset(plan, 0, sizeof(*plan));
    plan->naggs = naggs;
    plan->eps = eps;
    plan->every = every;
    /* sorted unique quantile list + per-agg mapping (timer stream is
     * registered with the sorted unique quantile set) */
    double* qs = plan->qs;
    int nq = 0;
    for (int i = 0; i < naggs; i++) {
        plan->agg_types[i] = agg_types[i];
        double q = agg_quantile_of_host(agg_types[i]);
        if (q >= 0) qs[nq++] = q;
    }
    for (int i = 1; i < nq; i++) {
        double k = qs[i];
        int j = i - 1;
        while (j >= 0 && qs[j] > k) { qs[j + 1] = qs[j]; j--; }
        qs[j + 1] = k;
    }
    int m = 0;
    for (int i = 0; i < nq; i++)
        if (m == 0 || qs[m - 1] != qs[i]) qs[m++] = qs[i];
    for (int i = m; i < nq; i++) qs[i] = 0.0;
    nq = m;
    plan->nq = nq;
    for (int i = 0; i < naggs; i++) {
        plan->qidx[i] = -1;
        double q = agg_quantile_of_host(agg_types[i]);
        if (q >= 0)
            for (int k = 0; k < nq; k++)
                if (qs[k] == q) { plan->qidx[i] = (int8_t)k; break; }
    }
    /* exact_cap: largest n such that for every numVals v <= n and every
     * maxRank mr <= v, the compress merge threshold (stream.go:362-385,
     * int64 truncation exactly as the reference computes it) stays < 2 =
     * the minimum testVal — i.e. compression NEVER merges and quantiles
     * are exact order statistics. */
    plan->exact_cap = QCAP;
    double eps2 = 2.0 * eps;
    for (int v = 4; v <= QCAP + 1; v++) /* minSamplesToCompress=3 */ {
        bool merges = false;
        for (int mr = 0; mr <= v && !merges; mr++) {
            long long thr = LLONG_MAX;
            for (int i = 0; i < nq; i++) {
                long long qmin;
                if (mr >= (long long)(qs[i] * (double)v))
                    qmin = (long long)(eps2 * (double)mr / qs[i]);
                else
                    qmin = (long long)(eps2 * (double)(v - mr) / (1.0 - qs[i]));
                if (qmin < thr) thr = qmin;
            }
            if (nq > 0 && thr >= 2) merges = true;
        }
        if (merges) { plan->exact_cap = v - 1; break; }
    }
    /* extreme_cap: largest n (bounded by exact_cap) for which EVERY
     * requested quantile resolves to sorted[n-1] — the bucket max — by
     * exact_quantile_index, the same function the kernels index with.
     * All-high quantile sets (p90+, e.g. the sum/min/max/p99 rollup) then
     * need no per-point value staging at all: running min/max suffice. */
    plan->extreme_cap = 0;
    if (nq > 0) {
        int capn = plan->exact_cap < QCAP ? plan->exact_cap : QCAP;
        for (int n = 1; n <= capn; n++) {
            bool allmax = true;
            for (int i = 0; i < nq && allmax; i++)
                allmax = exact_quantile_index(qs, i, n) == n - 1;
            if (!allmax) break;
            plan->extreme_cap = n;
        }
    }
}

} // namespace m3

#endif
