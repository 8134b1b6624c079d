/*
 * step_kernels.h — the batched StepIter consolidation: k_step_rows over
 * decoded rows and k_step_fused straight from the streams.
 */
#ifndef M3_STEP_KERNELS_H
#define M3_STEP_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/m3gpu.h"
#include "m3tsz_decoder.h"
#include "out_tile.h" /* out_st8 */

namespace m3 {

/* ===================== batched StepIter consolidation =====================
 * What encodedBlock.StepIter() computes for every fetched series
 * (query/storage/m3/encoded_step_iterator.go, nextForStep in
 * encoded_step_iterator_generic.go:63-119, StepLookbackConsolidator in
 * consolidators/step_consolidator.go with TakeLast, consolidators/
 * types.go:207-216): on the grid t_k = start + k*step, value(k) is the value
 * of the last point with t_k - lookback <= ts <= t_k that is not NaN, else
 * NaN. For increasing timestamps the last non-NaN point <= t_k is either
 * inside the window or nothing is, so one carried candidate (ts, value) per
 * series is the whole state.
 *
 * One series per lane. The wave walks the grid in tiles of STEP_TILE steps;
 * a lane takes points until its next one lies past the tile's last step
 * (that point stays pending), writes its column of the LDS tile
 * [STEP_TILE][64], and the wave stores each step row as one 512-byte run of
 * d_out[k*out_pitch + series]. A lane reads only its own column, so the tile
 * is per-lane indexed storage and needs no barrier. Reading stops at the first
 * point past the last step (nextForStep's peeked point): a series' error
 * counts only when reading got that far, and then its whole column is NaN.
 *
 * STEP_TILE 8: 4 waves x 8 x 64 x 8 B = 16 KB next to the 8 KB input ring,
 * 24 KB a block, so the 128-VGPR granule (4 blocks a CU) stays the limit and
 * not the LDS; at a 60 s step over 10 s data a tile is 48 points a lane
 * between flushes, six times the decode's. */
#define STEP_TILE 8
#define STEP_NAN_BITS 0x7FF8000000000001ULL /* Go's math.NaN() */

struct StepGrid {
    int64_t start_ns, step_ns, lookback_ns;
    uint32_t nsteps;
};

struct StepLane {
    int64_t cand_t;    /* the last non-NaN point taken */
    uint64_t cand_v;
    int64_t last_t;    /* the last point read, for the order rule */
    uint64_t pend_v;   /* has_pend: that point lies past the current tile and
                        * this is its value */
    int64_t tk;        /* time of step ks; meaningful while ks < nsteps */
    uint32_t ks;       /* next step of this series to fill */
    bool cand_has, have_last, has_pend;

    __device__ __forceinline__ void init(const StepGrid& g) {
        cand_t = 0; cand_v = 0; last_t = 0; pend_v = 0;
        tk = g.start_ns;
        ks = 0;
        cand_has = false; have_last = false; has_pend = false;
    }
    /* step ks from the candidate; col is this lane's column of the tile */
    __device__ __forceinline__ void emit(const StepGrid& g, uint64_t* col,
                                         uint32_t k0) {
        const bool hit = cand_has && cand_t >= tk - g.lookback_ns;
        col[(ks - k0) * WAVE] = hit ? cand_v : STEP_NAN_BITS;
        ks++;
        if (ks < g.nsteps) tk += g.step_ns;
    }
    /* a point at or before the tile's last step: the steps before it are
     * settled, then it is the candidate unless it is NaN */
    __device__ __forceinline__ void take(const StepGrid& g, uint64_t* col,
                                         uint32_t k0, uint32_t kend,
                                         int64_t t, uint64_t vbits) {
        while (ks < kend && tk < t) emit(g, col, k0);
        const double v = __longlong_as_double((long long)vbits);
        if (v == v) {
            cand_t = t;
            cand_v = vbits;
            cand_has = true;
        }
    }
    /* Tile start: a pending point that now falls inside is taken. Returns
     * whether the lane may read on. */
    __device__ __forceinline__ bool tile_begin(const StepGrid& g, uint64_t* col,
                                               uint32_t k0, uint32_t kend,
                                               int64_t t_hi) {
        if (has_pend && last_t <= t_hi) {
            take(g, col, k0, kend, last_t, pend_v);
            has_pend = false;
        }
        return !has_pend;
    }
    /* A new point in order. Returns true while the lane may read on in this
     * tile; `stop` is set at the first point past the last step. */
    __device__ __forceinline__ bool point(const StepGrid& g, uint64_t* col,
                                          uint32_t k0, uint32_t kend,
                                          int64_t t_hi, int64_t t_last,
                                          int64_t t, uint64_t vbits,
                                          bool& stop) {
        last_t = t;
        have_last = true;
        if (t > t_last) { stop = true; return false; }
        if (t > t_hi) {
            pend_v = vbits;
            has_pend = true;
            return false;
        }
        take(g, col, k0, kend, t, vbits);
        return true;
    }
    __device__ __forceinline__ void tile_end(const StepGrid& g, uint64_t* col,
                                             uint32_t k0, uint32_t kend) {
        while (ks < kend) emit(g, col, k0);
    }
};

/* the tile's rows k0..kend-1: lane l stores its own column, a wave one
 * 512-byte run per step */
__device__ __forceinline__ void step_flush(const uint64_t* col, uint32_t k0,
                                           uint32_t kend, bool in_range,
                                           uint32_t series,
                                           double* __restrict__ out,
                                           uint32_t out_pitch) {
    if (!in_range) return;
    for (uint32_t k = k0; k < kend; k++)
        out_st8(out + (uint64_t)k * out_pitch + series,
                (long long)col[(k - k0) * WAVE]);
}

/* a failed series: its whole column is NaN. Rare; the same store form as the
 * flush, so a lane's two stores to one cell stay in program order. */
__device__ __forceinline__ void step_fail_column(uint32_t nsteps,
                                                 uint32_t series,
                                                 double* __restrict__ out,
                                                 uint32_t out_pitch) {
    for (uint32_t k = 0; k < nsteps; k++)
        out_st8(out + (uint64_t)k * out_pitch + series,
                (long long)STEP_NAN_BITS);
}

/* Rows in, matrix out: the rows are what m3gpu_series_merge_batch_dev or a
 * decode wrote, [nseries, stride] with counts and optional errs. A point at
 * or before its predecessor is M3GPU_SERIES_OUT_OF_ORDER; the row's own error
 * comes after its points.
 *
 * A lane walks its own row, but the wave reads the rows together: each row
 * has a chunk of STEP_CHUNK points in LDS, and when lanes run out of theirs
 * the wave refills those rows, 4 lanes to a row's 64 contiguous bytes per
 * array (the decode's flush in reverse; 8 lanes of 8 bytes when the arrays or
 * the stride do not allow 16-byte loads). A lane on its own would pull a
 * whole line per 16 bytes it uses and share it with no one. Rows advance at
 * their own pace, so a refill round serves only the rows that asked. The
 * chunk rows are STEP_CHUNK + 1 words apart: lane l reads word l*9 + p, on
 * 32 different bank pairs for 32 consecutive lanes. */
#define STEP_CHUNK 8
#define STEP_CHUNK_PITCH (STEP_CHUNK + 1)

__global__ void __launch_bounds__(BLOCK_THREADS)
k_step_rows(const int64_t* __restrict__ ts, const double* __restrict__ vals,
            const uint32_t* __restrict__ counts,
            const int32_t* __restrict__ errs, uint32_t nseries,
            uint32_t stride, StepGrid g, double* __restrict__ out,
            uint32_t out_pitch, int32_t* __restrict__ out_errs) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t series = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    const uint32_t wave_row0 = series - lane;
    const bool in_range = series < nseries;

    __shared__ uint64_t tile_all[WAVES_PER_BLOCK][STEP_TILE][WAVE];
    __shared__ long long chunk_t_all[WAVES_PER_BLOCK][WAVE * STEP_CHUNK_PITCH];
    __shared__ long long chunk_v_all[WAVES_PER_BLOCK][WAVE * STEP_CHUNK_PITCH];
    uint64_t* col = &tile_all[wave][0][lane];
    long long* chunk_t = chunk_t_all[wave];
    long long* chunk_v = chunk_v_all[wave];
    const long long* gts = (const long long*)ts;
    const long long* gvals = (const long long*)vals;

    /* one decision per launch */
    const bool pair = !(stride & 1) &&
        !(((uintptr_t)ts | (uintptr_t)vals) & 15);
    const uint32_t count = in_range ? min(counts[series], stride) : 0;
    uint32_t idx = 0;   /* next point of the row */
    uint32_t cend = 0;  /* the chunk in LDS holds points [cend - 8, cend) */

    /* rows whose lane asked get their next chunk; points past the count but
     * inside the row's stride are loaded and never read */
    auto refill = [&](bool ask) {
        const uint32_t cbase = idx & ~(uint32_t)(STEP_CHUNK - 1);
        if (ask) cend = cbase + STEP_CHUNK;
        __builtin_amdgcn_wave_barrier();
        if (pair) {
            const uint32_t q = 2 * (lane & 3);
#pragma unroll
            for (uint32_t j = 0; j < WAVE / 16; j++) {
                const uint32_t rr = (lane >> 2) + 16 * j;
                const bool on = __shfl((int)ask, (int)rr) != 0;
                const uint32_t pt = (uint32_t)__shfl((int)cbase, (int)rr) + q;
                if (on && pt < stride) {
                    const uint64_t at =
                        ((uint64_t)wave_row0 + rr) * stride + pt;
                    const dec_ll2 a = *(const dec_ll2*)(gts + at);
                    const dec_ll2 b = *(const dec_ll2*)(gvals + at);
                    long long* ct = chunk_t + rr * STEP_CHUNK_PITCH + q;
                    long long* cv = chunk_v + rr * STEP_CHUNK_PITCH + q;
                    ct[0] = a.x;
                    ct[1] = a.y;
                    cv[0] = b.x;
                    cv[1] = b.y;
                }
            }
        } else {
            const uint32_t q = lane & 7;
#pragma unroll
            for (uint32_t j = 0; j < WAVE / 8; j++) {
                const uint32_t rr = (lane >> 3) + 8 * j;
                const bool on = __shfl((int)ask, (int)rr) != 0;
                const uint32_t pt = (uint32_t)__shfl((int)cbase, (int)rr) + q;
                if (on && pt < stride) {
                    const uint64_t at =
                        ((uint64_t)wave_row0 + rr) * stride + pt;
                    chunk_t[rr * STEP_CHUNK_PITCH + q] = gts[at];
                    chunk_v[rr * STEP_CHUNK_PITCH + q] = gvals[at];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    };

    const int64_t t_last = g.start_ns + (int64_t)(g.nsteps - 1) * g.step_ns;
    StepLane s;
    s.init(g);
    int err = 0;
    bool running = in_range; /* more of the row may be read */

    for (uint32_t k0 = 0; k0 < g.nsteps; k0 += STEP_TILE) {
        const uint32_t kend = min(k0 + STEP_TILE, g.nsteps);
        const int64_t t_hi = g.start_ns + (int64_t)(kend - 1) * g.step_ns;
        bool need = s.tile_begin(g, col, k0, kend, t_hi) && running;
        while (__any(need)) {
            const bool ask = need && idx < count && idx >= cend;
            if (__any(ask)) refill(ask);
            if (need) {
                if (idx >= count) {
                    /* the row ran out before a point past the last step:
                     * now its own error shows */
                    running = false;
                    need = false;
                    if (errs) err = errs[series];
                } else {
                    const uint32_t at = lane * STEP_CHUNK_PITCH +
                                        (idx & (STEP_CHUNK - 1));
                    const int64_t t = chunk_t[at];
                    const long long v = chunk_v[at];
                    idx++;
                    if (s.have_last && t <= s.last_t) {
                        err = M3GPU_SERIES_OUT_OF_ORDER;
                        running = false;
                        need = false;
                    } else {
                        bool stop = false;
                        need = s.point(g, col, k0, kend, t_hi, t_last, t,
                                       (uint64_t)v, stop);
                        if (stop) running = false;
                    }
                }
            }
        }
        s.tile_end(g, col, k0, kend);
        step_flush(col, k0, kend, in_range, series, out, out_pitch);
    }
    if (in_range) {
        if (err) step_fail_column(g.nsteps, series, out, out_pitch);
        out_errs[series] = err;
    }
}

/* Streams in, matrix out, no rows in between: series i reads its nblocks
 * streams b*nseries + i in order through one RingDecoder, a zero-length
 * stream being an absent block. An equal timestamp is skipped (the first
 * wins), a smaller one is M3GPU_SERIES_OUT_OF_ORDER, inside a stream
 * (MultiReaderIterator) and across a boundary (validateNext of the
 * one-replica SeriesIterator): the result is k_step_rows over
 * k_series_merge (one replica, no range) over the decode of the streams.
 * A lane moves to its next stream at the top of a refill span, where the
 * wave is converged as RingDecoder::init wants it, under a predicate. */
#ifndef STEP_FUSED_WAVES
#define STEP_FUSED_WAVES 3
#endif
__global__ void __launch_bounds__(BLOCK_THREADS, STEP_FUSED_WAVES)
k_step_fused(const uint8_t* __restrict__ blobs,
             const uint64_t* __restrict__ offsets,
             const uint32_t* __restrict__ lens,
             uint32_t nseries, uint32_t nblocks, int int_optimized,
             uint8_t default_unit, StepGrid g, double* __restrict__ out,
             uint32_t out_pitch, int32_t* __restrict__ out_errs) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t series = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    const bool in_range = series < nseries;

    __shared__ uint64_t ring_all[WAVES_PER_BLOCK][WAVE][IN_WORDS];
    __shared__ uint64_t tile_all[WAVES_PER_BLOCK][STEP_TILE][WAVE];
    uint64_t* ring = ring_all[wave][lane];
    uint64_t* col = &tile_all[wave][0][lane];

    const int64_t t_last = g.start_ns + (int64_t)(g.nsteps - 1) * g.step_ns;
    StepLane s;
    s.init(g);
    RingDecoder d;
    d.init(blobs, 0, 0, int_optimized != 0, default_unit, ring);
    uint32_t blk = ~0u;          /* the stream being read */
    int err = 0;
    bool running = in_range;     /* more points may be read */
    bool want_next = in_range;   /* the stream ended: move to the next one */

    for (uint32_t k0 = 0; k0 < g.nsteps; k0 += STEP_TILE) {
        const uint32_t kend = min(k0 + STEP_TILE, g.nsteps);
        const int64_t t_hi = g.start_ns + (int64_t)(kend - 1) * g.step_ns;
        bool need = s.tile_begin(g, col, k0, kend, t_hi) && running &&
                    !want_next;
        for (;;) {
            if (__any(want_next)) {
                uint64_t off = 0;
                uint32_t len = 0;
                if (want_next) {
                    while (++blk < nblocks) {
                        const uint64_t row = (uint64_t)blk * nseries + series;
                        len = lens[row];
                        if (len) {
                            off = offsets[row];
                            break;
                        }
                    }
                    if (!len) running = false; /* out of streams: no error */
                }
                /* in place, under the lane's predicate: init touches only
                 * the lane's own state and ring row */
                if (want_next && len) {
                    d.init(blobs, off, len, int_optimized != 0, default_unit,
                           ring);
                    need = true;
                }
                want_next = false;
            }
            if (!__any(need)) break;
            const RingPending pd = d.r.refill_issue(need);
#pragma unroll 1
            for (uint32_t jt = 0; jt < RF_SPAN; jt++) {
                if (need) {
                    int64_t t;
                    double v;
                    const int rstat = d.next(&t, &v);
                    if (rstat < 0) {
                        err = -rstat;
                        running = false;
                        need = false;
                    } else if (rstat == 0) {
                        want_next = true;
                        need = false;
                    } else if (s.have_last && t <= s.last_t) {
                        if (t < s.last_t) {
                            err = M3GPU_SERIES_OUT_OF_ORDER;
                            running = false;
                            need = false;
                        }
                    } else {
                        bool stop = false;
                        need = s.point(g, col, k0, kend, t_hi, t_last, t,
                                       (uint64_t)__double_as_longlong(v),
                                       stop);
                        if (stop) running = false;
                    }
                }
            }
            d.r.refill_commit(pd);
        }
        s.tile_end(g, col, k0, kend);
        step_flush(col, k0, kend, in_range, series, out, out_pitch);
    }
    if (in_range) {
        if (err) step_fail_column(g.nsteps, series, out, out_pitch);
        out_errs[series] = err;
    }
}

} // namespace m3

#endif /* M3_STEP_KERNELS_H */
