/*
 * merge_kernels.h — the two merges over already-decoded rows: k_merge (one
 * block per replica) and k_series_merge (the batched SeriesIterator).
 */
#ifndef M3_MERGE_KERNELS_H
#define M3_MERGE_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/m3gpu.h"
#include "m3tsz_common.h"
#include "out_tile.h"

namespace m3 {

/* ===================== replica-deduplicating merge =====================
 * MultiReaderIterator semantics over one slice of R (<=4) replica rows of
 * already-decoded points (multi_reader_iterator.go:62-155 +
 * iterators.go:56-237, IterateLastPushed default): the `values` order starts
 * as replica order and mutates only by swap-with-tail on exhaustion; among
 * equal earliest timestamps the LAST in `values` order wins; equal-to-prev
 * timestamps are deduped; a decreasing one is errOutOfOrderIterator.
 * One series per lane; order bookkeeping packed in a u32 (a byte per slot)
 * so everything stays in registers. */
#define MERGE_MAX_R 4

/* UNITS = true also carries each point's time unit: `units` rows are laid
 * out like the ts rows, a byte per point, and an emitted point gets the unit
 * of the replica whose value it got (iterators.go current()). UNITS = false
 * touches neither pointer. */
template <bool UNITS>
__global__ void __launch_bounds__(BLOCK_THREADS)
k_merge(const int64_t* __restrict__ ts, const double* __restrict__ vals,
        const uint32_t* __restrict__ counts, uint32_t nreplicas,
        uint32_t nseries, uint32_t stride,
        int64_t* __restrict__ out_ts, double* __restrict__ out_vals,
        uint32_t* __restrict__ out_counts, int32_t* __restrict__ out_errs,
        uint32_t out_stride,
        const uint8_t* __restrict__ units, uint8_t* __restrict__ out_units) {
    const uint32_t series = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    if (series >= nseries) return;

    const int64_t* tr[MERGE_MAX_R];
    const double* vr[MERGE_MAX_R];
    uint32_t cnt[MERGE_MAX_R];
    uint32_t cur[MERGE_MAX_R];
    int64_t cur_ts[MERGE_MAX_R];
    double cur_val[MERGE_MAX_R];
    const uint8_t* ur[MERGE_MAX_R];
    uint8_t cur_unit[MERGE_MAX_R];

    uint32_t ord = 0; /* packed replica ids, byte per slot, slot 0 = lowest */
    uint32_t nvals = 0;
#pragma unroll
    for (uint32_t r = 0; r < MERGE_MAX_R; r++) {
        if (r < nreplicas) {
            tr[r] = ts + ((uint64_t)r * nseries + series) * stride;
            vr[r] = vals + ((uint64_t)r * nseries + series) * stride;
            cnt[r] = counts[(uint64_t)r * nseries + series];
            cur[r] = 0;
            if (cnt[r] > 0) {
                cur_ts[r] = tr[r][0];
                cur_val[r] = vr[r][0];
                if constexpr (UNITS) {
                    ur[r] = units + ((uint64_t)r * nseries + series) * stride;
                    cur_unit[r] = ur[r][0];
                }
                ord |= r << (8 * nvals);
                nvals++;
            }
        }
    }

    int64_t* orow_ts = out_ts + (uint64_t)series * out_stride;
    double* orow_val = out_vals + (uint64_t)series * out_stride;
    uint32_t n = 0;
    int64_t prev_at = 0;
    bool first = true;
    int err = 0;

    while (nvals > 0) {
        /* earliest scan in `ord` order; last min wins (IterateLastPushed) */
        int64_t earliest = INT64_MAX;
        uint32_t winner = 0;
#pragma unroll
        for (uint32_t i = 0; i < MERGE_MAX_R; i++) {
            if (i < nvals) {
                uint32_t r = (ord >> (8 * i)) & 0xff;
                int64_t t = cur_ts[r];
                if (t <= earliest) {
                    earliest = t;
                    winner = r;
                }
            }
        }
        if (!first && earliest < prev_at) { err = M3GPU_SERIES_OUT_OF_ORDER; break; }
        if (first || earliest != prev_at) {
            if (n >= out_stride) { err = M3GPU_SERIES_CAPACITY; break; }
            orow_ts[n] = earliest;
            orow_val[n] = cur_val[winner];
            if constexpr (UNITS)
                out_units[(uint64_t)series * out_stride + n] = cur_unit[winner];
            n++;
            prev_at = earliest;
            first = false;
        }
        /* advance every replica at `earliest`; swap-with-tail on exhaustion
         * (ascending slot order with re-examination == the reference's
         * removal order, see DESIGN.md merge note) */
        for (uint32_t i = 0; i < nvals;) {
            uint32_t r = (ord >> (8 * i)) & 0xff;
            if (cur_ts[r] == earliest) {
                cur[r]++;
                if (cur[r] >= cnt[r]) {
                    uint32_t tail = (ord >> (8 * (nvals - 1))) & 0xff;
                    ord = (ord & ~(0xffu << (8 * i))) | (tail << (8 * i));
                    nvals--;
                    continue; /* re-examine the swapped-in slot */
                }
                cur_ts[r] = tr[r][cur[r]];
                cur_val[r] = vr[r][cur[r]];
                if constexpr (UNITS) cur_unit[r] = ur[r][cur[r]];
            }
            i++;
        }
    }
    out_counts[series] = n;
    out_errs[series] = err;
}

/* ===================== batched SeriesIterator =====================
 * encoding.SeriesIterator (series_iterator.go:74-215) over R (<=4) replicas
 * of B blocks each, all already decoded: TWO levels of `iterators`.
 *  - inner, per replica: a MultiReaderIterator over a slice of slices with
 *    one reader per slice (multi_reader_iterator.go:94-155). Inside a block
 *    an equal timestamp is skipped (first wins) and a smaller one is
 *    errOutOfOrderIterator; across a block boundary nothing is compared
 *    (iters.reset()). A row's error surfaces when the replica moves past the
 *    row's points.
 *  - outer: `iterators` over the replicas with the range filter
 *    (iterators.go:140-158), the four IterateEqualTimestampStrategy values
 *    (:60-109) and moveToValidNext (:160-227), which walks `earliest` in the
 *    order current()'s in-place sort left it.
 * One series per lane, all state in registers: `ord` as in k_merge, plus a
 * cursor per replica. Every lane emits at most one point per step, so the
 * running lanes of a wave share the output index and the output goes the
 * decoder's way: an LDS tile flushed transposed in whole lines. */
#define SM_TILE 8
/* blocks per CU the register allocation is held to (the 32 KB tile allows 5) */
#ifndef SM_MIN_BLOCKS
#define SM_MIN_BLOCKS 1
#endif

struct SmIn {
    const int64_t* ts;
    const double* vals;
    const uint8_t* units;
    const uint32_t* counts;
    const int32_t* errs;
    uint32_t nblocks, nseries, stride, series;
    bool pair;  /* even elements are 16-byte aligned: two per load */
    bool quad;  /* every fourth is 32-byte aligned: four per pair of loads */
    bool uwide; /* the units rows are aligned alike: 2- and 4-byte loads */
};

/* one replica's cursor: its current point and where it sits */
struct SmRep {
    uint64_t idx;  /* element index of the current point */
    uint32_t rem;  /* points of this block after the current one */
    uint32_t blk;  /* ~0u before the first block */
    int64_t t;
    double v;
    uint32_t unit;
    /* up to three points behind the current one, when a wide load brought
     * them: nah of them, the next in t2/v2 and the low byte of ubuf */
    int64_t t2, t3, t4;
    double v2, v3, v4;
    uint32_t ubuf;
    uint32_t nah;
};

/* Load the point at p.idx. A lane walks its own row, so a wave's load touches
 * 64 different lines whatever its width, and the requests, not the bytes, are
 * what the kernel waits for: where alignment allows and the block has the
 * points, one call loads four (two 16-byte loads per array, one 4-byte load
 * of units) or two, and the following calls take theirs from registers. */
template <bool UNITS>
__device__ __forceinline__ void sm_fetch(const SmIn& in, SmRep& p, int64_t& t,
                                         double& v, uint32_t& u) {
    if (p.nah) {
        t = p.t2;
        v = p.v2;
        p.t2 = p.t3;
        p.v2 = p.v3;
        p.t3 = p.t4;
        p.v3 = p.v4;
        if constexpr (UNITS) {
            u = in.uwide ? (p.ubuf & 0xff) : in.units[p.idx];
            p.ubuf >>= 8;
        }
        p.nah--;
    } else if (in.pair && !(p.idx & 1) && p.rem > 0) {
        const bool four = in.quad && !(p.idx & 3) && p.rem >= 3;
        const dec_ll2 ta = *(const dec_ll2*)(in.ts + p.idx);
        const dec_ll2 va = *(const dec_ll2*)(in.vals + p.idx);
        t = ta.x;
        v = __longlong_as_double(va.x);
        p.t2 = ta.y;
        p.v2 = __longlong_as_double(va.y);
        p.nah = 1;
        uint32_t uu = 0;
        if (four) {
            const dec_ll2 tb = *(const dec_ll2*)(in.ts + p.idx + 2);
            const dec_ll2 vb = *(const dec_ll2*)(in.vals + p.idx + 2);
            p.t3 = tb.x;
            p.v3 = __longlong_as_double(vb.x);
            p.t4 = tb.y;
            p.v4 = __longlong_as_double(vb.y);
            p.nah = 3;
            if constexpr (UNITS)
                if (in.uwide) uu = *(const uint32_t*)(in.units + p.idx);
        } else {
            if constexpr (UNITS)
                if (in.uwide) uu = *(const uint16_t*)(in.units + p.idx);
        }
        if constexpr (UNITS) {
            u = in.uwide ? (uu & 0xff) : in.units[p.idx];
            p.ubuf = uu >> 8;
        }
    } else {
        t = in.ts[p.idx];
        v = in.vals[p.idx];
        if constexpr (UNITS) u = in.units[p.idx];
    }
}

template <typename T>
__device__ __forceinline__ T sm_sel(uint32_t r, T a0, T a1, T a2, T a3) {
    return r == 0 ? a0 : r == 1 ? a1 : r == 2 ? a2 : a3;
}

/* The replica's Next(): 1 = on a new point, 0 = ran out, -1 = error in e. */
template <bool UNITS>
__device__ __forceinline__ int sm_next(const SmIn& in, uint32_t r, SmRep& p,
                                       int& e) {
    for (;;) {
        if (p.rem > 0) {
            p.rem--;
            p.idx++;
            int64_t t;
            double v;
            uint32_t u = 0;
            sm_fetch<UNITS>(in, p, t, v, u);
            if (t < p.t) { e = M3GPU_SERIES_OUT_OF_ORDER; return -1; }
            if (t == p.t) continue; /* in-block dedupe: the first wins */
            p.t = t;
            p.v = v;
            p.unit = u;
            return 1;
        }
        /* past the block's points: now its own error shows */
        if (p.blk != ~0u && in.errs) {
            const uint64_t row =
                ((uint64_t)r * in.nblocks + p.blk) * in.nseries + in.series;
            const int re = in.errs[row];
            if (re) { e = re; return -1; }
        }
        for (;;) {
            p.blk++;
            if (p.blk >= in.nblocks) { p.blk = in.nblocks; return 0; }
            const uint64_t row =
                ((uint64_t)r * in.nblocks + p.blk) * in.nseries + in.series;
            const uint32_t c = min(in.counts[row], in.stride);
            if (c) {
                /* first point of a block: taken as it is */
                p.idx = row * in.stride;
                p.rem = c - 1;
                p.nah = 0;
                sm_fetch<UNITS>(in, p, p.t, p.v, p.unit);
                return 1;
            }
            if (in.errs) {
                const int re = in.errs[row];
                if (re) { e = re; return -1; }
            }
        }
    }
}

/* Next() followed by moveIteratorToFilterNext (iterators.go:140-158): below
 * start_ns is skipped, the first point at or past end_ns ends the replica. */
template <bool UNITS>
__device__ __forceinline__ int sm_advance(const SmIn& in, uint32_t r, SmRep& p,
                                          int& e, bool filtering,
                                          int64_t start_ns, int64_t end_ns) {
    int s;
    do {
        s = sm_next<UNITS>(in, r, p, e);
    } while (s > 0 && filtering && p.t < start_ns);
    if (s > 0 && filtering && p.t >= end_ns) s = 0;
    return s;
}

template <bool UNITS>
__global__ void __launch_bounds__(BLOCK_THREADS, SM_MIN_BLOCKS)
k_series_merge(const int64_t* __restrict__ ts, const double* __restrict__ vals,
               const uint8_t* __restrict__ units,
               const uint32_t* __restrict__ counts,
               const int32_t* __restrict__ errs,
               uint32_t nreplicas, uint32_t nblocks, uint32_t nseries,
               uint32_t stride, int64_t start_ns, int64_t end_ns, int strategy,
               int64_t* __restrict__ out_ts, double* __restrict__ out_vals,
               uint8_t* __restrict__ out_units,
               uint32_t* __restrict__ out_counts,
               int32_t* __restrict__ out_errs, uint32_t out_stride) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t series = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    const uint32_t wave_row0 = series - lane; /* the series of lane 0 */
    const bool in_range = series < nseries;

    /* the decoder's output tile: (ts, val) pairs, dec_swz column swizzle */
    __shared__ longlong2 tile_all[WAVES_PER_BLOCK][WAVE][SM_TILE];
    longlong2 (*tile)[SM_TILE] = tile_all[wave];

    /* one decision per launch: an even stride and 16-byte aligned arrays put
     * every even element index on a 16-byte boundary, and so on */
    const bool pair = !(stride & 1) &&
        !(((uintptr_t)ts | (uintptr_t)vals) & 15);
    const bool quad = pair && !(stride & 3);
    const bool uwide = UNITS && pair && !((uintptr_t)units & (quad ? 3 : 1));
    const SmIn in = {ts, vals, units, counts, errs,
                     nblocks, nseries, stride, series, pair, quad, uwide};
    /* series_iterator.go:145 */
    const bool filtering = start_ns != 0 && end_ns != 0;

    SmRep rep[MERGE_MAX_R] = {};
    uint32_t ord = 0;   /* `values`: replica ids, a byte per slot */
    uint32_t nvals = 0;
    uint32_t alive = 0; /* bit r: replica r is in `values` */
    int err = 0;
    uint32_t n = 0;
    bool done = !in_range;

    /* Reset (series_iterator.go:159-169): every replica is positioned and
     * pushed in replica order; an error of any of them is the series' error
     * (the last one stays) and the series then emits nothing */
    if (in_range) {
#pragma unroll
        for (uint32_t r = 0; r < MERGE_MAX_R; r++) {
            if (r < nreplicas) {
                rep[r].rem = 0;
                rep[r].blk = ~0u;
                rep[r].t = 0;
                int e = 0;
                const int s = sm_advance<UNITS>(in, r, rep[r], e, filtering,
                                                start_ns, end_ns);
                if (s < 0) err = e;
                if (s > 0) {
                    ord |= r << (8 * nvals);
                    nvals++;
                    alive |= 1u << r;
                }
            }
        }
        if (err || !nvals) done = true;
    }

    auto member_t = [&](uint32_t r) {
        return sm_sel(r, rep[0].t, rep[1].t, rep[2].t, rep[3].t);
    };
    auto member_v = [&](uint32_t r) {
        return sm_sel(r, rep[0].v, rep[1].v, rep[2].v, rep[3].v);
    };
    /* earliestAt over `values`, and `earliest` in `values` order */
    auto earliest_at = [&]() {
        int64_t e = INT64_MAX;
#pragma unroll
        for (uint32_t r = 0; r < MERGE_MAX_R; r++)
            if ((alive >> r) & 1) e = rep[r].t < e ? rep[r].t : e;
        return e;
    };
    uint32_t es = 0, ne = 0; /* `earliest`: replica ids, a byte per slot */
    auto build_earliest = [&](int64_t at) {
        es = 0;
        ne = 0;
#pragma unroll
        for (uint32_t i = 0; i < MERGE_MAX_R; i++) {
            if (i < nvals) {
                const uint32_t r = (ord >> (8 * i)) & 0xff;
                if (member_t(r) == at) {
                    es |= r << (8 * ne);
                    ne++;
                }
            }
        }
    };
    int64_t at = 0;
    if (!done) {
        at = earliest_at();
        build_earliest(at);
    }

    /* one decision per launch, as in k_decode_batch */
    const bool wide = FLUSH_WIDE && !(out_stride & 1) &&
        !(((uintptr_t)out_ts | (uintptr_t)out_vals) & 15);
    const uint32_t swz = dec_swz(lane & 7);

    /* the transposed flush (out_tile.h): the row of lane rr is wave_row0 + rr,
     * and a lane past nseries has n == 0, so its row is never stored */
    const auto row_of = [wave_row0](uint32_t rr) {
        return (uint64_t)wave_row0 + rr;
    };
    /* a lane's own 8 unit bytes of the tile, stored to its own row: exactly
     * those of the points the flush stores */
    uint64_t tile_units = 0;

    /* Emit Current(), then moveToNext (series_iterator.go:196-215): the lane
     * leaves on its next point or done. */
    auto step = [&](uint32_t j) {
        if (done) return;
        /* current() (iterators.go:60-109): the value strategies sort
         * `earliest` in place; at <= 4 elements sort.Slice is this insertion
         * sort. The winner is the last element. */
        if (strategy != M3GPU_EQUAL_TS_LAST_PUSHED && ne > 1) {
            uint32_t freq = 0; /* byte r: members whose value == replica r's */
            if (strategy == M3GPU_EQUAL_TS_HIGHEST_FREQUENCY) {
#pragma unroll
                for (uint32_t r = 0; r < MERGE_MAX_R; r++) {
                    uint32_t f = 0;
#pragma unroll
                    for (uint32_t q = 0; q < MERGE_MAX_R; q++)
                        if (((alive >> q) & 1) && rep[q].t == at &&
                            rep[q].v == rep[r].v)
                            f++;
                    freq |= f << (8 * r);
                }
            }
            for (uint32_t i = 1; i < ne; i++) {
                for (uint32_t jj = i; jj > 0; jj--) {
                    const uint32_t a = (es >> (8 * jj)) & 0xff;
                    const uint32_t b = (es >> (8 * (jj - 1))) & 0xff;
                    bool less;
                    if (strategy == M3GPU_EQUAL_TS_HIGHEST_VALUE)
                        less = member_v(a) < member_v(b);
                    else if (strategy == M3GPU_EQUAL_TS_LOWEST_VALUE)
                        less = member_v(a) > member_v(b);
                    else
                        less = ((freq >> (8 * a)) & 0xff) <
                               ((freq >> (8 * b)) & 0xff);
                    if (!less) break;
                    es = (es & ~(0xffffu << (8 * (jj - 1)))) |
                         (a << (8 * (jj - 1))) | (b << (8 * jj));
                }
            }
        }
        if (n >= out_stride) {
            err = M3GPU_SERIES_CAPACITY;
            done = true;
            return;
        }
        const uint32_t winner = (es >> (8 * (ne - 1))) & 0xff;
        longlong2 pr;
        pr.x = at;
        pr.y = __double_as_longlong(member_v(winner));
        tile[lane][j ^ swz] = pr;
        if constexpr (UNITS)
            tile_units |= (uint64_t)(sm_sel(winner, rep[0].unit, rep[1].unit,
                                            rep[2].unit, rep[3].unit) & 0xff)
                          << (8 * j);
        n++;

        for (;;) {
            /* moveToValidNext (iterators.go:160-227). Every member of
             * `earliest` advances; the advances do not depend on one another,
             * so they run in replica order and only their results are walked
             * in `earliest` order: the first error ends the series, a replica
             * that ran out is removed by swap-with-tail. */
            uint32_t st = 0; /* 2 bits per replica: 0 ran out, 1 point, 2 error */
            int e0 = 0, e1 = 0, e2 = 0, e3 = 0;
#pragma unroll
            for (uint32_t r = 0; r < MERGE_MAX_R; r++) {
                if (((alive >> r) & 1) && rep[r].t == at) {
                    int e = 0;
                    const int s = sm_advance<UNITS>(in, r, rep[r], e, filtering,
                                                    start_ns, end_ns);
                    st |= (s < 0 ? 2u : (uint32_t)s) << (2 * r);
                    if (r == 0) e0 = e;
                    else if (r == 1) e1 = e;
                    else if (r == 2) e2 = e;
                    else e3 = e;
                }
            }
            for (uint32_t w = 0; w < ne; w++) {
                const uint32_t r = (es >> (8 * w)) & 0xff;
                const uint32_t s = (st >> (2 * r)) & 3;
                if (s == 2) {
                    err = sm_sel(r, e0, e1, e2, e3);
                    done = true;
                    break;
                }
                if (s == 0) {
                    uint32_t i = 0;
                    while (i + 1 < nvals && ((ord >> (8 * i)) & 0xff) != r) i++;
                    const uint32_t tail = (ord >> (8 * (nvals - 1))) & 0xff;
                    ord = (ord & ~(0xffu << (8 * i))) | (tail << (8 * i));
                    nvals--;
                    alive &= ~(1u << r);
                }
            }
            if (done) return;
            if (!nvals) {
                done = true;
                return;
            }
            const int64_t next_at = earliest_at();
            if (next_at < at) { /* validateNext */
                err = M3GPU_SERIES_OUT_OF_ORDER;
                done = true;
                return;
            }
            const bool same = next_at == at;
            at = next_at;
            /* rebuilt in `values` order; a deduped step walks it unsorted,
             * as current() is not called for it */
            build_earliest(at);
            if (!same) return;
        }
    };

    uint32_t k = 0;
    while (__any(!done)) {
#pragma unroll 1
        for (uint32_t j = 0; j < SM_TILE; j++) step(j);
        __builtin_amdgcn_wave_barrier();
        if (wide)
            out_flush_wide<SM_TILE>(tile, lane, n, k, out_ts, out_vals,
                                    out_stride, row_of);
        else
            out_flush_narrow<SM_TILE>(tile, lane, n, k, out_ts, out_vals,
                                      out_stride, row_of);
        __builtin_amdgcn_wave_barrier();
        if constexpr (UNITS) {
            out_flush_units<SM_TILE>(out_units, series, out_stride, n, k,
                                     tile_units);
            tile_units = 0;
        }
        k += SM_TILE;
    }

    if (in_range) {
        out_counts[series] = n;
        out_errs[series] = err;
    }
}

} // namespace m3

#endif /* M3_MERGE_KERNELS_H */
