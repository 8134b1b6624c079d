/*
 * rollup_kernels.h — the fused decode->rollup kernels, all three tiers.
 * Device code, over the decoders of m3tsz_decoder.h.
 *
 *   k_rollup_lane<QMODE, METRIC>  one series per lane; every rollup starts here
 *   k_rollup_batch                one series per wave: timers whose quantile
 *                                 buckets are deeper than RQCAP_LANE
 *   k_rollup_ckms                 one series per workgroup: buckets deeper
 *                                 than plan.exact_cap, the compressing CKMS
 *
 * The tiers share the bucket walk, the bucket state, its accumulate and the
 * ValueOf arms that read it (rollup_bucket.h) and the exact-quantile index
 * (rollup_plan.h). Each tier owns where a timer's min, max and quantiles
 * come from, its capacity check, and how it stores a bucket:
 *
 *   lane RQ_NONE     no quantiles asked; a timer's min/max are then 0
 *   lane RQ_STAGED   per-lane LDS row kept sorted by insertion
 *   lane RQ_EXTREME  running min/max, every quantile being the max
 *   wave             LDS staging, rank-selected into sorted[] at emit
 *   ckms             the reference CKMS sample list (stream.go:77-429)
 *
 * A tier that cannot hold a bucket flags M3GPU_SERIES_BUCKET_OVERFLOW and
 * writes nothing more for that series: the host reruns it on the next tier.
 * The three exact timer-quantile tiers (staged, extreme, wave) do the same
 * on a NaN or a -0.0 (timer_value_needs_stream): where those end up in the
 * reference's stream depends on its heaps, which only the ckms tier keeps.
 */
#ifndef M3_ROLLUP_KERNELS_H
#define M3_ROLLUP_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/m3gpu.h"
#include "m3tsz_decoder.h" /* Decoder, RingDecoder, RF_SPAN */
#include "rollup_bucket.h"

namespace m3 {

/* -------- wave-per-series tier: timers with quantiles -------- */
__global__ void __launch_bounds__(BLOCK_THREADS)
k_rollup_batch(const uint8_t* __restrict__ blobs,
               const uint64_t* __restrict__ offsets,
               const uint32_t* __restrict__ lens,
               const int32_t* __restrict__ select, /* optional series subset */
               uint32_t nseries, int int_optimized, uint8_t default_unit,
               int64_t window_ns, uint32_t nbuckets,
               RollupPlan plan,
               double* __restrict__ out, int64_t* __restrict__ out_window_ts,
               int32_t* __restrict__ out_errs) {
    /* readfirstlane makes the series index provably wave-uniform: the
     * whole parser then compiles to scalar (SGPR) code with scalar
     * branches instead of exec-mask divergence sequences. */
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t slot = blockIdx.x * WAVES_PER_BLOCK + wave;
    const uint32_t series = __builtin_amdgcn_readfirstlane(
        (select && slot < nseries) ? (uint32_t)select[slot] : slot);
    /* per-wave bucket value staging for the quantiles */
    __shared__ double qvals_all[WAVES_PER_BLOCK][QCAP];
    __shared__ double sorted_all[WAVES_PER_BLOCK][QCAP];
    double* qvals = qvals_all[wave];
    double* sorted = sorted_all[wave];
    if (slot >= nseries) return;

    Decoder d;
    d.init(blobs, offsets[series], lens[series], int_optimized != 0, default_unit);

    double* out_row = out + (uint64_t)series * nbuckets * plan.naggs;
    int64_t* wts_row = out_window_ts ? out_window_ts + (uint64_t)series * nbuckets : nullptr;

    BucketWalk walk;
    BucketState bs;
    bs.reset();
    uint32_t n = 0; /* values staged for the open bucket */
    int err = 0;

    auto emit_bucket = [&](int64_t b) {
        if (wts_row && lane == 0) wts_row[b] = walk.window_end(b, window_ns);
        if (n > 0) {
            /* rank-select: each lane ranks elements lane, lane+64, ...
             * LDS ops from one wave retire in order; the fences only stop
             * compiler reordering around the cross-lane LDS use. */
            __builtin_amdgcn_wave_barrier();
            __threadfence_block();
            for (uint32_t e = lane; e < n; e += WAVE) {
                double v = qvals[e];
                uint32_t rank = 0;
                for (uint32_t j = 0; j < n; j++) {
                    double o = qvals[j];
                    rank += (o < v) || (o == v && j < e);
                }
                sorted[rank] = v;
            }
            __builtin_amdgcn_wave_barrier();
            __threadfence_block();
        }
        if (lane < (uint32_t)plan.naggs) { /* one aggregation per lane */
            int32_t t = plan.agg_types[lane];
            int8_t qi = plan.qidx[lane];
            double r;
            if (qi >= 0) /* empty stream Quantile -> 0 */
                r = n ? sorted[exact_quantile_index(plan.qs, qi, (int)n)] : 0.0;
            else if (t == M3GPU_AGG_MIN) r = n ? sorted[0] : 0.0; /* Quantile(0) */
            else if (t == M3GPU_AGG_MAX) r = n ? sorted[n - 1] : 0.0;
            else r = bucket_value_of<M3GPU_METRIC_TIMER>(bs, t);
            out_row[(uint64_t)b * plan.naggs + lane] = r;
        }
    };

    for (;;) {
        int64_t t;
        double v;
        int rstat = d.next(&t, &v);
        if (rstat < 0) { err = -rstat; break; }
        bool have = rstat == 1;
        int64_t from, to;
        int w = walk.step(have, t, window_ns, nbuckets, &from, &to);
        if (w > 0) { err = w; break; }
        if (w == WALK_ADVANCE) {
            if (from > 0) emit_bucket(from - 1);
            for (int64_t eb = from; eb < to; eb++) {
                bs.reset();
                n = 0;
                emit_bucket(eb);
            }
            if (!have) break;
            bs.reset();
            n = 0;
        }
        /* a NaN or a -0.0 needs the stream itself: the ckms tier */
        if (n >= (uint32_t)plan.exact_cap || n >= QCAP ||
            timer_value_needs_stream(v)) {
            err = M3GPU_SERIES_BUCKET_OVERFLOW;
            break;
        }
        bucket_add<M3GPU_METRIC_TIMER>(bs, t, v);
        if (lane == 0) qvals[n] = v;
        n++;
    }
    if (lane == 0) out_errs[series] = err;
}

/* -------- series-per-lane tier --------
 * One series per LANE (64 parsers per wave, like k_decode_batch). */
#define RQCAP_LANE 16 /* RQ_STAGED: values per bucket in the per-lane LDS row */

#define RQ_NONE 0
#define RQ_STAGED 1
#define RQ_EXTREME 2

template <int QMODE, int METRIC>
__global__ void __launch_bounds__(BLOCK_THREADS, QMODE == RQ_STAGED ? 3 : 4)
/* staged: 40KB LDS (qbuf + ring) pins 3 blocks/CU, so 3 waves/SIMD with no
   spills; other modes target the 128-VGPR granule (4 waves/SIMD) */
k_rollup_lane(const uint8_t* __restrict__ blobs,
              const uint64_t* __restrict__ offsets,
              const uint32_t* __restrict__ lens,
              uint32_t nseries, int int_optimized, uint8_t default_unit,
              int64_t window_ns, uint32_t nbuckets,
              RollupPlan plan,
              double* __restrict__ out, int64_t* __restrict__ out_window_ts,
              int32_t* __restrict__ out_errs) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t series = blockIdx.x * BLOCK_THREADS + wave * WAVE + lane;

    constexpr bool WITH_Q = QMODE == RQ_STAGED;
    __shared__ double qbuf_all[WITH_Q ? WAVES_PER_BLOCK : 1]
                              [WITH_Q ? WAVE : 1][WITH_Q ? RQCAP_LANE : 1];
    double* qrow = WITH_Q ? qbuf_all[wave][lane] : nullptr;
    /* per-lane input ring, as in k_decode_batch */
    __shared__ uint64_t rring_all[WAVES_PER_BLOCK][WAVE][IN_WORDS];
    uint64_t* rring = rring_all[wave][lane];

    const bool in_range = series < nseries;
    RingDecoder d;
    d.init(blobs, in_range ? offsets[series] : 0, in_range ? lens[series] : 0,
           int_optimized != 0, default_unit, rring);

    double* out_row = out + (uint64_t)series * nbuckets * plan.naggs;
    int64_t* wts_row = out_window_ts ? out_window_ts + (uint64_t)series * nbuckets : nullptr;

    BucketWalk walk;
    BucketState bs;
    bs.reset();
    uint32_t nq = 0; /* RQ_STAGED: values in qrow */
    int err = 0;
    bool running = in_range;

    auto emit_bucket = [&](int64_t b) {
        if (wts_row) wts_row[b] = walk.window_end(b, window_ns);
        /* even naggs: emit value pairs as aligned 16B stores (the rows are
         * naggs*8B apart, so paired stores halve the line-granular write
         * amplification of the scattered per-lane emission) */
        const bool paired = (plan.naggs & 1) == 0;
        double pend = 0;
        for (int k = 0; k < plan.naggs; k++) {
            int32_t t = plan.agg_types[k];
            int8_t qi = plan.qidx[k];
            double r;
            if (METRIC != M3GPU_METRIC_TIMER || QMODE == RQ_NONE) {
                r = bucket_value_of<METRIC>(bs, t);
            } else if (QMODE == RQ_EXTREME) {
                /* all-high quantile set: every requested quantile is the
                 * bucket max for n <= plan.extreme_cap (the host checked
                 * with exact_quantile_index; deeper buckets overflowed) */
                if (qi >= 0) r = bs.count ? bs.fmax : 0.0;
                else if (t == M3GPU_AGG_MIN) r = bs.count ? bs.fmin : 0.0;
                else if (t == M3GPU_AGG_MAX) r = bs.count ? bs.fmax : 0.0;
                else r = bucket_value_of<METRIC>(bs, t);
            } else { /* qrow holds the sorted bucket values */
                if (qi >= 0) /* empty stream Quantile -> 0 */
                    r = nq ? qrow[exact_quantile_index(plan.qs, qi, (int)nq)] : 0.0;
                else if (t == M3GPU_AGG_MIN) r = nq ? qrow[0] : 0.0;
                else if (t == M3GPU_AGG_MAX) r = nq ? qrow[nq - 1] : 0.0;
                else r = bucket_value_of<METRIC>(bs, t);
            }
            if (paired) {
                if (k & 1) {
                    double2 pr;
                    pr.x = pend;
                    pr.y = r;
                    *(double2*)(out_row + (uint64_t)b * plan.naggs + k - 1) = pr;
                } else {
                    pend = r;
                }
            } else {
                out_row[(uint64_t)b * plan.naggs + k] = r;
            }
        }
    };

    while (__any(running)) {
        const RingPending pd = d.r.refill_issue(running);
#pragma unroll 1
        for (uint32_t jt = 0; jt < RF_SPAN; jt++) {
        if (running) {
            int64_t t;
            double v;
            int rstat = d.next(&t, &v);
            if (rstat < 0) {
                err = -rstat;
                running = false;
            } else {
                bool have = rstat == 1;
                int64_t from, to;
                int w = walk.step(have, t, window_ns, nbuckets, &from, &to);
                bool ok = true;
                if (w > 0) {
                    err = w;
                    running = false;
                    ok = false;
                } else if (w == WALK_ADVANCE) {
                    if (from > 0) emit_bucket(from - 1);
                    for (int64_t eb = from; eb < to; eb++) {
                        bs.reset();
                        nq = 0;
                        emit_bucket(eb);
                    }
                    if (!have) {
                        running = false;
                        ok = false;
                    } else {
                        bs.reset();
                        nq = 0;
                    }
                }
                if (ok) {
                    if (QMODE == RQ_EXTREME &&
                        (timer_value_needs_stream(v) ||
                         bs.count >= (int64_t)plan.extreme_cap)) {
                        /* deep buckets keep the exact staged semantics on
                         * the wave tier; a NaN or a -0.0 passes through it
                         * to the ckms tier */
                        err = M3GPU_SERIES_BUCKET_OVERFLOW;
                        running = false;
                    } else if (WITH_Q && (nq >= RQCAP_LANE ||
                                          nq >= (uint32_t)plan.exact_cap ||
                                          timer_value_needs_stream(v))) {
                        err = M3GPU_SERIES_BUCKET_OVERFLOW;
                        running = false;
                    } else {
                        if (QMODE == RQ_EXTREME) {
                            /* fmin/fmax with "first value initialises",
                             * not the gauge's NaN-initialised compare */
                            if (bs.count == 0) {
                                bs.fmin = v;
                                bs.fmax = v;
                            } else {
                                if (v < bs.fmin) bs.fmin = v;
                                if (v > bs.fmax) bs.fmax = v;
                            }
                        }
                        bucket_add<METRIC>(bs, t, v);
                        if (WITH_Q) {
                            /* insertion into this lane's sorted row */
                            uint32_t j = nq;
                            while (j > 0 && qrow[j - 1] > v) { qrow[j] = qrow[j - 1]; j--; }
                            qrow[j] = v;
                            nq++;
                        }
                    }
                }
            }
        }
        }
        d.r.refill_commit(pd);
    }
    if (in_range) out_errs[series] = err;
}

__global__ void __launch_bounds__(BLOCK_THREADS)
k_count_errcode(const int32_t* __restrict__ errs, uint32_t n, int32_t code,
                uint32_t* __restrict__ out) {
    /* grid-stride count of one per-series error code: lets the rollup
     * dispatch test for tier retries with a 4-byte D2H instead of pulling
     * and scanning the whole error array every call */
    uint32_t cnt = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gridDim.x * blockDim.x)
        if (errs[i] == code) cnt++;
    if (__any(cnt != 0)) {
        cnt += __shfl_down(cnt, 32); cnt += __shfl_down(cnt, 16);
        cnt += __shfl_down(cnt, 8); cnt += __shfl_down(cnt, 4);
        cnt += __shfl_down(cnt, 2); cnt += __shfl_down(cnt, 1);
        if ((threadIdx.x & (WAVE - 1)) == 0 && cnt) atomicAdd(out, cnt);
    }
}

/* ===================== full-CKMS deep-bucket rollup =====================
 * Third tier of the timer-quantile chain (after the per-lane <=16 staging
 * and the wave-kernel exact-order-statistics cap): the reference CKMS
 * stream WITH compression (quantile/cm/stream.go:77-429), ported from the
 * oracle's restatement onto LDS arrays. One WAVE per workgroup, one series
 * per workgroup (rare retry path; correctness, not throughput):
 *  - samples double-buffer (value,numRanks,delta) replaces the linked list;
 *    the insert cursor walk becomes a two-pointer merge (equivalent:
 *    incoming v inserted before the first list element with value >= v,
 *    delta = that element's numRanks+delta-1; the tail appends delta 0);
 *  - compress walks backward tracking the surviving next element; removed
 *    samples are compacted after the walk (same removal order);
 *  - in the AddBatch(1)/Flush usage the compress cursor is always nil on
 *    insert entry, so the compValue/compressMinRank-in-insert branch of the
 *    reference is dead (stream.go:284-287,303) and omitted;
 *  - buffers bufLess/bufMore are the reference's min-heaps (heap.go:36-54
 *    Push, :92-121 SortDesc), kept by lane 0: the heap order decides where
 *    a -0.0 lands among +0.0 and what a NaN takes with it when insert()
 *    drops it, and both show in the output bits;
 *  - insert() keeps the reference's compares (<= the cursor, >= the tail):
 *    a value that fails both is dropped with the rest of the sorted
 *    buffer, and numValues grows by what was inserted;
 *  - capacity overflow (sample list or buffer > CKMS_CAP) flags
 *    M3GPU_SERIES_BUCKET_OVERFLOW — never an approximation. */
#define CKMS_CAP 3072
#define CKMS_BUF 2080 /* bufMore peak = carried bufLess (<=1024) + 1024 new */
#define CKMS_BLOCK 64

/* The kernel's dynamic LDS, as byte offsets: the one statement of the
 * layout. The kernel carves its pointers from it and the host launches
 * with `bytes`. */
struct CkmsLdsLayout {
    static constexpr uint32_t val = 0;                        /* double[2][CKMS_CAP] */
    static constexpr uint32_t nr = val + 2 * CKMS_CAP * 8;    /* int32_t[2][CKMS_CAP] */
    static constexpr uint32_t dl = nr + 2 * CKMS_CAP * 4;     /* int32_t[2][CKMS_CAP] */
    static constexpr uint32_t less = dl + 2 * CKMS_CAP * 4;   /* double[CKMS_BUF] */
    static constexpr uint32_t more = less + CKMS_BUF * 8;     /* double[CKMS_BUF] */
    static constexpr uint32_t computed = more + CKMS_BUF * 8;        /* double[MAX_AGGS] */
    static constexpr uint32_t thr_rank = computed + MAX_AGGS * 8;    /* int64_t[MAX_AGGS] */
    static constexpr uint32_t thr_thresh = thr_rank + MAX_AGGS * 8;  /* int64_t[MAX_AGGS] */
    static constexpr uint32_t bytes = thr_thresh + MAX_AGGS * 8;
};

struct CkmsLds {
    double* val[2];
    int32_t* nr[2];
    int32_t* dl[2];
    double* less;
    double* more;
};

struct CkmsState {
    int cur;           /* active buffer index */
    int32_t len;       /* samples */
    int32_t nless, nmore;
    int64_t num_values;
    int32_t counter;   /* insertAndCompressCounter */
    int err;
};

__device__ __forceinline__ void ckms_reset(CkmsState& st) {
    st.cur = 0;
    st.len = 0;
    st.nless = 0;
    st.nmore = 0;
    st.num_values = 0;
    st.counter = 0;
}

/* heap.go:36-54 Push onto heap[0..n): the new value sifts up while its
 * parent is not <= it (a NaN therefore climbs to the root). Lane 0 only. */
__device__ __forceinline__ void ckms_heap_push(double* heap, int32_t n, double v) {
    int32_t i = n;
    heap[i] = v;
    while (i > 0) {
        int32_t parent = (i - 1) / 2;
        double p = heap[parent];
        if (p <= v) break;
        heap[parent] = v;
        heap[i] = p;
        i = parent;
    }
}

/* heap.go:92-121 SortDesc: pop the minimum to the end, n-1 times, with the
 * reference's strict < in the sift-down. Lane 0 only. */
__device__ void ckms_heap_sort_desc(double* heap, int32_t len) {
    for (int32_t n = len - 1; n > 0; n--) {
        double t = heap[0];
        heap[0] = heap[n];
        heap[n] = t;
        int32_t i = 0;
        for (;;) {
            int32_t smallest = i, left = 2 * i + 1, right = left + 1;
            if (left < n && heap[left] < heap[smallest]) smallest = left;
            if (right < n && heap[right] < heap[smallest]) smallest = right;
            if (smallest == i) break;
            t = heap[i];
            heap[i] = heap[smallest];
            heap[smallest] = t;
            i = smallest;
        }
    }
}

/* stream.go:362-377 threshold(rank), exact int64 truncation */
__device__ __forceinline__ int64_t ckms_threshold(const RollupPlan& plan,
                                                  int64_t num_vals, int64_t rank) {
    int64_t min_val = INT64_MAX;
    double eps = 2.0 * plan.eps;
    for (int i = 0; i < plan.nq; i++) {
        int64_t qmin;
        if (rank >= (int64_t)(plan.qs[i] * (double)num_vals))
            qmin = (int64_t)(eps * (double)rank / plan.qs[i]);
        else
            qmin = (int64_t)(eps * (double)(num_vals - rank) / (1.0 - plan.qs[i]));
        if (qmin < min_val) min_val = qmin;
    }
    return min_val;
}

/* insert the sorted bufMore (stream.go:280-331) + compress (:333-401);
 * lane 0 does the heap sort and the sequential merge/walk. */
__device__ void ckms_insert_compress(CkmsLds& L, CkmsState& st,
                                     const RollupPlan& plan, uint32_t lane) {
    int32_t m = st.nmore;
    if (st.len + m > CKMS_CAP) { /* uniform: all lanes see the same state */
        st.err = M3GPU_SERIES_BUCKET_OVERFLOW;
        return;
    }
    if (lane == 0) {
        int src = st.cur, dst = st.cur ^ 1;
        int32_t n = st.len; /* >= 1: the first value is always a sample */
        {
            /* :294-299 descending sort, consumed from the end */
            double* vals = L.more;
            ckms_heap_sort_desc(vals, m);
            int32_t idx = m - 1;
            /* two-pointer merge == the reference's cursor walk (:301-322) */
            int32_t i = 0, o = 0;
            while (i < n) {
                double insert_point = L.val[src][i];
                while (idx >= 0 && vals[idx] <= insert_point) {
                    L.val[dst][o] = vals[idx];
                    L.nr[dst][o] = 1;
                    L.dl[dst][o] = L.nr[src][i] + L.dl[src][i] - 1;
                    o++; idx--;
                }
                L.val[dst][o] = L.val[src][i];
                L.nr[dst][o] = L.nr[src][i];
                L.dl[dst][o] = L.dl[src][i];
                o++; i++;
            }
            /* PushBack while >= the current tail, delta 0 (:324-335); what
             * fails the compare is dropped with everything behind it */
            while (idx >= 0 && vals[idx] >= L.val[dst][o - 1]) {
                L.val[dst][o] = vals[idx];
                L.nr[dst][o] = 1;
                L.dl[dst][o] = 0;
                o++; idx--;
            }
            st.cur = dst;
            st.len = o;
            st.num_values += o - n; /* numValues++ per inserted sample */
            /* compress (:333-401); entry cursor nil in this usage */
            int32_t len = st.len;
            if (len >= 3) {
                int b = st.cur;
                int64_t cmr = st.num_values - 1 - L.nr[b][len - 2];
                int32_t nxt = len - 2; /* surviving element after curr */
                for (int32_t c = len - 3; c >= 1; c--) {
                    int64_t max_rank = cmr + L.nr[b][c] + L.dl[b][c];
                    int64_t thr = ckms_threshold(plan, st.num_values, max_rank);
                    cmr -= L.nr[b][c];
                    int64_t test_val = L.nr[b][c] + L.nr[b][nxt] + L.dl[b][nxt];
                    if (test_val <= thr) {
                        L.nr[b][nxt] += L.nr[b][c];
                        L.nr[b][c] = -1; /* removed mark */
                    } else {
                        nxt = c;
                    }
                }
                /* compact, preserving order */
                int32_t o2 = 0;
                for (int32_t c = 0; c < len; c++) {
                    if (L.nr[b][c] >= 0) {
                        if (o2 != c) {
                            L.val[b][o2] = L.val[b][c];
                            L.nr[b][o2] = L.nr[b][c];
                            L.dl[b][o2] = L.dl[b][c];
                        }
                        o2++;
                    }
                }
                st.len = o2;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    /* uniform parts every lane must perform itself: the buffer swap
     * (resetInsertCursor, stream.go:425-429) swaps POINTERS held per lane */
    double* t = L.less; L.less = L.more; L.more = t;
    st.nmore = st.nless;
    st.nless = 0;
    /* lane-0-computed scalars: broadcast via readfirstlane */
    st.cur = __builtin_amdgcn_readfirstlane(st.cur);
    st.len = __builtin_amdgcn_readfirstlane(st.len);
    st.num_values = ((int64_t)(uint32_t)__builtin_amdgcn_readfirstlane(
                         (uint32_t)(st.num_values >> 32)) << 32) |
                    (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)st.num_values);
}

/* stream.go:77-116 AddBatch(values[0..1)) — one value at a time, exactly
 * like Timer.AddBatch -> stream per-value adds in the rollup loop. */
__device__ __forceinline__ void ckms_add(CkmsLds& L, CkmsState& st,
                                         const RollupPlan& plan, double v,
                                         uint32_t lane) {
    if (st.err) return;
    if (st.len == 0 && st.nmore == 0 && st.nless == 0 && st.num_values == 0) {
        /* first value becomes the first sample (:88-97) */
        if (lane == 0) {
            L.val[st.cur][0] = v;
            L.nr[st.cur][0] = 1;
            L.dl[st.cur][0] = 0;
        }
        st.len = 1;
        st.num_values = 1;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        return;
    }
    double insert_point = L.val[st.cur][0]; /* insertCursor == head here */
    if (st.nless >= CKMS_BUF || st.nmore >= CKMS_BUF) {
        st.err = M3GPU_SERIES_BUCKET_OVERFLOW;
        return;
    }
    if (v < insert_point) { /* a NaN goes to bufMore (:102-106) */
        if (lane == 0) ckms_heap_push(L.less, st.nless, v);
        st.nless++;
    } else {
        if (lane == 0) ckms_heap_push(L.more, st.nmore, v);
        st.nmore++;
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    if (st.counter == plan.every) { /* insertAndCompressEvery, checked BEFORE ++ */
        ckms_insert_compress(L, st, plan, lane);
        st.counter = 0;
    }
    st.counter++;
}

/* stream.go:123-137 Flush */
__device__ __forceinline__ void ckms_flush(CkmsLds& L, CkmsState& st,
                                           const RollupPlan& plan,
                                           uint32_t lane) {
    while (!st.err && (st.nless > 0 || st.nmore > 0)) {
        if (st.nmore == 0) { /* resetInsertCursor: swap */
            double* t = L.less; L.less = L.more; L.more = t;
            st.nmore = st.nless;
            st.nless = 0;
        }
        ckms_insert_compress(L, st, plan, lane);
    }
}

/* stream.go:231-277 calcQuantiles (+ :210-229 quantilesFromBuf), filling
 * computed[0..nq) for the plan's sorted unique quantile list. computed[]
 * must be zeroed per bucket first: the reference leaves un-emitted
 * quantiles at the zero value (the post-loop condition can fail for the
 * top quantiles at certain numValues — real behavior, preserved). Lane 0
 * only; thr_rank/thr_thresh are LDS scratch (>= plan.nq entries). */
__device__ void ckms_calc_quantiles(const CkmsLds& L, const CkmsState& st,
                                    const RollupPlan& plan, double* computed,
                                    int64_t* thr_rank, int64_t* thr_thresh) {
    if (plan.nq == 0 || st.num_values == 0) return;
    const int b = st.cur;
    if (st.num_values <= 3) { /* quantilesFromBuf over the sample list */
        for (int i = 0; i < plan.nq; i++) {
            int32_t idx = (int32_t)(plan.qs[i] * (double)st.len);
            if (idx >= st.len) idx = st.len - 1;
            computed[i] = L.val[b][idx];
        }
        return;
    }
    for (int i = 0; i < plan.nq; i++) {
        int64_t rank = (int64_t)ceil(plan.qs[i] * (double)st.num_values);
        thr_rank[i] = rank;
        thr_thresh[i] =
            (int64_t)ceil((double)ckms_threshold(plan, st.num_values, rank) / 2.0);
    }
    int64_t min_rank = 0, max_rank = 0;
    int idx = 0;
    int32_t prev = 0;
    for (int32_t c = 0; c < st.len && idx < plan.nq; c++) {
        max_rank = min_rank + L.nr[b][c] + L.dl[b][c];
        if (max_rank > thr_rank[idx] + thr_thresh[idx] || min_rank > thr_rank[idx]) {
            computed[idx] = L.val[b][prev];
            idx++;
        }
        min_rank += L.nr[b][c];
        prev = c;
    }
    for (int i = idx; i < plan.nq; i++) { /* post-loop (:268-276), note >= */
        if (max_rank >= thr_rank[i] + thr_thresh[i] || min_rank > thr_rank[i])
            computed[i] = L.val[b][prev];
    }
}

/* ------------- the deep-bucket rollup kernel (third tier) -------------
 * One series per 64-thread workgroup (one wave), ~129 KB dynamic LDS
 * (CkmsLdsLayout) for the CKMS state. Only TIMER series with quantile aggs
 * can reach this tier (nothing else sets BUCKET_OVERFLOW). */
__global__ void __launch_bounds__(CKMS_BLOCK)
k_rollup_ckms(const uint8_t* __restrict__ blobs,
              const uint64_t* __restrict__ offsets,
              const uint32_t* __restrict__ lens,
              const int32_t* __restrict__ select, uint32_t nseries,
              int int_optimized, uint8_t default_unit,
              int64_t window_ns, uint32_t nbuckets, RollupPlan plan,
              double* __restrict__ out, int64_t* __restrict__ out_window_ts,
              int32_t* __restrict__ out_errs) {
    extern __shared__ uint8_t lds_raw[];
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t slot = blockIdx.x;
    if (slot >= nseries) return;
    const uint32_t series = __builtin_amdgcn_readfirstlane(
        select ? (uint32_t)select[slot] : slot);

    typedef CkmsLdsLayout Lay;
    CkmsLds L;
    L.val[0] = (double*)(lds_raw + Lay::val);
    L.val[1] = L.val[0] + CKMS_CAP;
    L.nr[0] = (int32_t*)(lds_raw + Lay::nr);
    L.nr[1] = L.nr[0] + CKMS_CAP;
    L.dl[0] = (int32_t*)(lds_raw + Lay::dl);
    L.dl[1] = L.dl[0] + CKMS_CAP;
    L.less = (double*)(lds_raw + Lay::less);
    L.more = (double*)(lds_raw + Lay::more);
    double* computed = (double*)(lds_raw + Lay::computed);
    int64_t* thr_rank = (int64_t*)(lds_raw + Lay::thr_rank);
    int64_t* thr_thresh = (int64_t*)(lds_raw + Lay::thr_thresh);

    Decoder d;
    d.init(blobs, offsets[series], lens[series], int_optimized != 0, default_unit);

    double* out_row = out + (uint64_t)series * nbuckets * plan.naggs;
    int64_t* wts_row = out_window_ts ? out_window_ts + (uint64_t)series * nbuckets : nullptr;

    BucketWalk walk;
    BucketState bs;
    bs.reset();
    CkmsState st;
    ckms_reset(st);
    st.err = 0;
    int err = 0;

    auto emit_bucket = [&](int64_t bk) {
        if (wts_row && lane == 0) wts_row[bk] = walk.window_end(bk, window_ns);
        ckms_flush(L, st, plan, lane);
        if (st.err) return;
        if (lane == 0) {
            for (int i = 0; i < plan.nq; i++) computed[i] = 0.0;
            ckms_calc_quantiles(L, st, plan, computed, thr_rank, thr_thresh);
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        if (lane < (uint32_t)plan.naggs) { /* one aggregation per lane */
            int32_t t = plan.agg_types[lane];
            int8_t qi = plan.qidx[lane];
            int cb = st.cur;
            double r;
            if (qi >= 0) r = st.len ? computed[qi] : 0.0; /* Quantile(q): computed */
            else if (t == M3GPU_AGG_MIN) r = st.len ? L.val[cb][0] : 0.0;
            else if (t == M3GPU_AGG_MAX) r = st.len ? L.val[cb][st.len - 1] : 0.0;
            else r = bucket_value_of<M3GPU_METRIC_TIMER>(bs, t);
            out_row[(uint64_t)bk * plan.naggs + lane] = r;
        }
    };

    for (;;) {
        int64_t t;
        double v;
        int rstat = d.next(&t, &v);
        if (rstat < 0) { err = -rstat; break; }
        bool have = rstat == 1;
        int64_t from, to;
        int w = walk.step(have, t, window_ns, nbuckets, &from, &to);
        if (w > 0) { err = w; break; }
        if (w == WALK_ADVANCE) {
            if (from > 0) {
                emit_bucket(from - 1);
                if (st.err) { err = st.err; break; }
            }
            for (int64_t eb = from; eb < to; eb++) {
                bs.reset();
                ckms_reset(st);
                emit_bucket(eb);
            }
            if (!have) break;
            bs.reset();
            ckms_reset(st);
        }
        bucket_add<M3GPU_METRIC_TIMER>(bs, t, v);
        ckms_add(L, st, plan, v, lane); /* one value at a time */
        if (st.err) { err = st.err; break; }
    }
    if (lane == 0) out_errs[series] = err;
}

} // namespace m3

#endif
