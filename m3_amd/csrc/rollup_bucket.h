/*
 * rollup_bucket.h — what every rollup tier shares about one series' buckets:
 * the walk from a point's timestamp to its bucket, the per-bucket state with
 * its per-metric accumulate, and the ValueOf arms that do not depend on how
 * a tier stores a timer's values. Plain C++17 like rollup_plan.h (host+device
 * under hipcc), compiled on its own by tests/rollup_plan_driver.cpp.
 *
 * Reference semantics:
 *  bucket assignment  generic_elem.go:219-221 (truncate to window)
 *  output timestamp   list.go:541-543 (window END)
 *  Counter            counter.go:52-131  (int64 sum/min/max/count/sumSq)
 *  Gauge              gauge.go:73-165    (NaN rules :87-98; last by ts order)
 *  Timer              timer.go:56-153; min, max and the quantiles come from
 *                     the CKMS stream, which each tier restates its own way.
 */
#ifndef M3_ROLLUP_BUCKET_H
#define M3_ROLLUP_BUCKET_H

#include "rollup_plan.h"

namespace m3 {

/* Go float64->int64 (amd64 CVTTSD2SQ): out-of-range/NaN -> INT64_MIN. The
 * counter's cast here, and convertToIntFloat's in the encoder. */
M3_HD static M3_INLINE int64_t go_f2i(double v) {
    if (!(v >= -9223372036854775808.0 && v < 9223372036854775808.0)) return INT64_MIN;
    return (int64_t)v;
}

/* The timer values whose place in the reference's CKMS stream depends on
 * more than their order among the bucket's values: a NaN fails both insert
 * compares and is dropped with what the heap sort left behind it
 * (stream.go:305,325), and a zero with the sign bit set ties with +0.0,
 * where the heaps decide which comes first (heap.go:36-54,92-121). Only
 * the ckms tier restates that; the exact tiers hand such a bucket on. */
M3_HD static M3_INLINE bool timer_value_needs_stream(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return u == 0x8000000000000000ull ||
           (u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
}

/* ---- the bucket walk ---- */
#define WALK_SAME 0      /* the point belongs to the open bucket */
#define WALK_ADVANCE (-1) /* see BucketWalk::step */

struct BucketWalk {
    int64_t base = 0;         /* first timestamp truncated to the window */
    int64_t cur_bucket = -1;  /* the open bucket, -1 before the first point */
    int64_t cur_lo = 0, cur_hi = 0; /* its timestamp bounds */

    /* One decoded point (have, t), or the end of the stream (!have).
     * Returns a per-series error code (> 0), WALK_SAME, or WALK_ADVANCE:
     * the caller then closes the open bucket from-1 (if from > 0), emits
     * buckets [from, to) as empty, and either stops (!have) or starts
     * accumulating into the bucket the walk has just opened.
     * from and to are written on every path: left undefined on the early
     * returns, the series-per-lane kernels' register allocation gets worse
     * (RQ_EXTREME then spills 2 VGPRs). */
    M3_HD M3_INLINE int step(bool have, int64_t t, int64_t window_ns,
                             uint32_t nbuckets, int64_t* from, int64_t* to) {
        int64_t b = (int64_t)nbuckets; /* end of stream: empties to the end */
        *from = cur_bucket + 1;
        *to = b;
        if (have) {
            /* same bucket: two compares instead of a 64-bit division per
             * point */
            if (cur_bucket >= 0 && t >= cur_lo && t < cur_hi) return WALK_SAME;
            if (cur_bucket < 0) base = (t / window_ns) * window_ns; /* Truncate */
            if (t < base) return M3GPU_SERIES_UNSORTED;
            b = (t - base) / window_ns;
            if (b >= (int64_t)nbuckets) return M3GPU_SERIES_CAPACITY;
            if (b < cur_bucket) return M3GPU_SERIES_UNSORTED;
        }
        *to = b;
        if (have) {
            cur_bucket = b;
            cur_lo = base + b * window_ns;
            cur_hi = cur_lo + window_ns;
        }
        return WALK_ADVANCE;
    }

    M3_HD M3_INLINE int64_t window_end(int64_t b, int64_t window_ns) const {
        return base + (b + 1) * window_ns;
    }
};

/* ---- per-bucket state ---- */
struct BucketState {
    int64_t isum, imin, imax, isumsq;
    double fsum, fsumsq, fmin, fmax, last;
    int64_t last_at;
    int64_t count;

    M3_HD M3_INLINE void reset() {
        isum = 0; isumsq = 0;
        imin = INT64_MAX; imax = INT64_MIN;   /* counter.go:44-47 */
        fsum = 0; fsumsq = 0;
        fmin = __builtin_nan("");             /* gauge.go:56-59 */
        fmax = __builtin_nan("");
        last = 0; last_at = 0;
        count = 0;
    }
};

M3_HD static M3_INLINE double m3_stdev(int64_t count, double sum_sq, double sum) { /* common.go:29-36 */
    int64_t div = count * (count - 1);
    if (div == 0) return 0.0;
    return sqrt(((double)count * sum_sq - sum * sum) / (double)div);
}

/* One value into the bucket. The metric is a template parameter: the other
 * metrics' fields are never touched and drop out of the register file. The
 * timer arm is timer.go:56-75 without the stream insert, which is the
 * tier's. f64 order is sum then sum of squares, no contraction. */
template <int METRIC>
M3_HD static M3_INLINE void bucket_add(BucketState& bs, int64_t t, double v) {
    if (METRIC == M3GPU_METRIC_COUNTER) { /* counter.go:52-78 */
        int64_t iv = go_f2i(v);
        /* Go's int64 wraps: add in uint64_t (the same instruction) */
        bs.isum = (int64_t)((uint64_t)bs.isum + (uint64_t)iv);
        bs.count++;
        if (bs.imax < iv) bs.imax = iv;
        if (bs.imin > iv) bs.imin = iv;
        bs.isumsq = (int64_t)((uint64_t)bs.isumsq + (uint64_t)iv * (uint64_t)iv);
    } else if (METRIC == M3GPU_METRIC_GAUGE) { /* gauge.go:73-103 */
        if (bs.last_at == 0 || t > bs.last_at) { bs.last_at = t; bs.last = v; }
        bs.count++;
        if (!__builtin_isnan(v)) {
            bs.fsum += v;
            if (__builtin_isnan(bs.fmax) || bs.fmax < v) bs.fmax = v;
            if (__builtin_isnan(bs.fmin) || bs.fmin > v) bs.fmin = v;
            bs.fsumsq += v * v;
        }
    } else {
        bs.count++;
        bs.fsum += v;
        bs.fsumsq += v * v;
    }
}

/* ValueOf (counter.go:112-131, gauge.go:144-165, timer.go:131-153). For a
 * timer only the arms that read BucketState: min, max and the quantiles are
 * the tier's and give 0 here, like any other unknown type. */
template <int METRIC>
M3_HD static M3_INLINE double bucket_value_of(const BucketState& bs, int32_t agg) {
    const bool counter = METRIC == M3GPU_METRIC_COUNTER;
    const double sum = counter ? (double)bs.isum : bs.fsum;
    const double sumsq = counter ? (double)bs.isumsq : bs.fsumsq;
    switch (agg) {
    case M3GPU_AGG_LAST: return METRIC == M3GPU_METRIC_GAUGE ? bs.last : 0.0;
    case M3GPU_AGG_MIN:
        return counter ? (double)bs.imin
                       : METRIC == M3GPU_METRIC_GAUGE ? bs.fmin : 0.0;
    case M3GPU_AGG_MAX:
        return counter ? (double)bs.imax
                       : METRIC == M3GPU_METRIC_GAUGE ? bs.fmax : 0.0;
    case M3GPU_AGG_MEAN: return bs.count ? sum / (double)bs.count : 0.0;
    case M3GPU_AGG_COUNT: return (double)bs.count;
    case M3GPU_AGG_SUM: return sum;
    case M3GPU_AGG_SUMSQ: return sumsq;
    case M3GPU_AGG_STDEV: return m3_stdev(bs.count, sumsq, sum);
    default: return 0.0;
    }
}

} // namespace m3

#endif
