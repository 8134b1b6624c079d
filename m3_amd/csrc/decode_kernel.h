/*
 * decode_kernel.h — k_decode_batch, the bulk and the full decode, and the
 * knobs of its input ring and top-up schedule.
 */
#ifndef M3_DECODE_KERNEL_H
#define M3_DECODE_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/m3gpu.h"
#include "m3tsz_decoder.h"
#include "out_tile.h"

namespace m3 {

/* ========================= decode kernel ========================= */
/* ONE SERIES PER LANE: a wave decodes 64 independent streams in parallel,
 * one point per active lane per iteration. The VLC parser state lives in
 * per-lane VGPRs; data-dependent branches diverge only where lanes disagree
 * (host-side batches group similar series for lane coherence, but any order
 * is correct).
 *
 * Memory structure:
 *  - INPUT through a per-lane LDS ring (BitReader::refill_issue/_commit):
 *    the global gathers leave the per-point chain — every RF_SPAN points
 *    each lane loads up to DEC_RING consecutive words of its own
 *    stream, commits them to its ring RF_SPAN points later, and the parser
 *    pulls words with ds_read_b64s.
 *  - OUTPUT staged in an LDS tile, [64 lanes][8 points] of (ts, val) pairs
 *    with an XOR column swizzle (dec_swz) — one ds_write_b128 per point —
 *    and flushed every 8 points TRANSPOSED, 16 bytes per lane and array:
 *    lane l covers row (l>>2)+16j, j = 0..3, and the point pair 2*(l&3),
 *    2*(l&3)+1, so 4 lanes write one row's 64 contiguous bytes per array,
 *    a store instruction covers 16 rows, and WRITE_SIZE stays at the
 *    algorithmic 16 B/pt. Outputs that are not 16-byte aligned, or an odd
 *    stride, take the 8-byte form (row (l>>3)+8j, point l&7); the choice
 *    is made once per launch. OUT_POLICY picks the stores' cache policy. */

#define DEC_TILE 8
/* k_decode_batch's input ring: 8 words per lane. The dense stream kinds
 * pull 6-8 words per 8-point tile and counters 2-3: a 4-word ring runs dry
 * inside a tile for the former and about every other calm tile for the
 * latter, and every dry-out is an in-chain load whose vmcnt(0) drains the
 * output stores in flight. 8 words x 64 lanes x 4 waves = 16 KB, with the
 * 32 KB output tile 48 KB/block: 3 blocks/CU, 3 waves/SIMD, and a VGPR
 * budget of 168 instead of 128. Same box, three alternated runs each
 * (DESIGN.md §4): 13.95 / 13.93 / 13.90 ms at 4 words, 12.94 / 12.91 /
 * 11.90 at 8.
 * The ring is lane-major, [wave][lane][8]: rows of 64 bytes put the 32
 * lanes of a ds_read_b64 group on 4 bank pairs, and a word-major ring
 * [wave][8][lane] is conflict-free (SQ_LDS_BANK_CONFLICT 93.5M -> 0 per
 * 250k-series launch, SQ_LDS_IDX_ACTIVE 226M -> 131M) — and 0.6% SLOWER,
 * 11.29 / 11.30 / 11.31 ms against 11.23 / 11.23 / 11.23: the LDS is not
 * what the kernel waits for. */
#ifndef DEC_RING
#define DEC_RING 8
#endif
/* 1: a burst loads 16 bytes per lane and instruction where the address
 * allows (BitReader WIDE); 0: 8 bytes always. A per-lane load costs its
 * line requests whatever its width, so the wide form about halves the
 * burst's requests: same box, three alternated runs each, 11.40 / 11.36 /
 * 11.34 ms narrow against 10.91 / 10.91 / 10.91 wide, `--data production`
 * 4.27 / 4.21 / 4.17 against 4.12 / 4.12 / 3.97. */
#ifndef DEC_REFILL_WIDE
#define DEC_REFILL_WIDE 1
#endif
/* top the 8-word ring up when <= this many words remain. Same box, three
 * alternated runs each: 2 13.02 ms, 3 11.34-11.40, 5 11.47, 7 12.45-13.44
 * against 11.91-12.90 for 3 in that call. */
#ifndef DEC_RF_LOW
#define DEC_RF_LOW 3
#endif
/* k_decode_batch only: the span of a tile whose predecessor left every
 * lane's ring with words to spare (see its tile loop). DEC_TILE = one burst
 * per tile; RF_SPAN = the fixed span everywhere. A tile counts as calm
 * after one in which no lane pulled more than RF_CALM_MAX words. Same box,
 * the fixed span alone, one stream kind at a time: one-decimal
 * gauges (1-2 words a tile) 11.1 ms at span 2, 10.0 at 8; counters (2-3
 * words a tile, dry about every other tile at span 8) 11.75 and 11.91. */
#ifndef RF_SPAN_CALM
#define RF_SPAN_CALM DEC_TILE
#endif
#ifndef RF_CALM_MAX
#define RF_CALM_MAX (DEC_RING - 1)
#endif

/* The optional per-series outputs of the full decode (m3gpu.h,
 * m3gpu_decode_batch_full_dev); each pointer may be null. */
struct DecodeFullOut {
    uint8_t* units;     /* [nseries*stride] per-point unit, any alignment */
    int64_t* start_ns;  /* [nseries] block start */
};

/* FULL = false is the bulk kernel; `full` is not touched. FULL = true also
 * returns ReaderIterator.Current()'s unit for every stored point and the
 * stream's first 64 bits. The units take no LDS (the 48 KB of ring + tile
 * already fill a CU's 160 KB three times): a lane packs its own 8 unit bytes
 * of the tile into one 64-bit register and stores its own row at the flush. */
template <bool FULL>
__global__ void __launch_bounds__(BLOCK_THREADS, 3) /* ring + tiles = 48
    KB/block -> 3 blocks/CU, 3 waves/SIMD: a 168-VGPR budget */
k_decode_batch(const uint8_t* __restrict__ blobs,
               const uint64_t* __restrict__ offsets,
               const uint32_t* __restrict__ lens,
               const int32_t* __restrict__ perm,
               uint32_t nseries, int int_optimized, uint8_t default_unit,
               int64_t* __restrict__ out_ts, double* __restrict__ out_vals,
               uint32_t* __restrict__ out_counts, int32_t* __restrict__ out_errs,
               uint32_t stride,
               uint8_t* __restrict__ out_ann, uint32_t ann_stride,
               DecodeFullOut full) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t slot = blockIdx.x * BLOCK_THREADS + wave * WAVE + lane;
    /* optional scheduling permutation (e.g. length-sorted): waves then get
     * 64 similar-cost streams, removing intra-wave and intra-CU skew.
     * Purely a schedule: outputs still land in series order. */
    const uint32_t series = (perm && slot < nseries) ? (uint32_t)perm[slot] : slot;

    /* input ring + output tile. The tile is AoS — (ts, val) PAIRS, one
     * ds_write_b128 per point instead of two b64s — with a pair-granular
     * XOR column swizzle (col ^ dec_swz(lane & 7), see out_tile.h). */
    __shared__ uint64_t ring_all[WAVES_PER_BLOCK][WAVE][DEC_RING];
    __shared__ longlong2 tile_all[WAVES_PER_BLOCK][WAVE][DEC_TILE];
    uint64_t* ring = ring_all[wave][lane];
    longlong2 (*tile)[DEC_TILE] = tile_all[wave];

    const bool in_range = slot < nseries;
    DecoderT<DEC_RING, DEC_REFILL_WIDE != 0> d;
    d.init(blobs, in_range ? offsets[series] : 0, in_range ? lens[series] : 0,
           int_optimized != 0, default_unit, ring,
           (out_ann && in_range) ? out_ann + (uint64_t)series * ann_stride
                                 : nullptr,
           ann_stride);

    bool running = in_range;
    int err = 0;
    uint32_t cnt = 0;
    uint32_t k = 0;

    const bool discard = out_ts == nullptr; /* parse-only diagnostic */
    /* one decision per launch, wave-uniform (kernel arguments only): the
     * 16-byte flush needs both arrays 16-byte aligned and an even stride */
    const bool wide = FLUSH_WIDE && !discard && !(stride & 1) &&
        !(((uintptr_t)out_ts | (uintptr_t)out_vals) & 15);
    const uint32_t swz = dec_swz(lane & 7); /* this lane's OWN row, for step() */

    /* The kernel's OWN copy of out_tile.h's out_flush_wide and _narrow
     * (k_series_merge calls those), with row_of(rr) = __shfl(series, rr): a
     * fix to one goes into the other. The unit bytes go through the shared
     * out_flush_units, which compiles to the same instructions. Calling the
     * shared wide or narrow template here, either of them alone too,
     * compiles to a different schedule of the same loads and stores, whose
     * cost on the synthetic mix depends on the box: three boxes, alternated
     * runs, 1M x 1440, this copy against shared 11.29 / 11.16 / 11.16 ms
     * against 11.32 / 11.34 / 11.33 (slower by more than the copy's spread),
     * 12.53 / 12.55 / 12.56 against 12.56 / 12.55 / 12.54, and 12.26 /
     * 11.02 / 11.02 against 10.89 / 10.88 / 10.87; `--data production` no
     * slower on any. A by-reference callable and helpers without forced
     * inlining compile to the shared form's code (profiles/README.md, r13).
     *
     * transposed flush, wide form: lane l covers row (l>>2)+16j and the
     * point pair 2*(l&3), 2*(l&3)+1 — two ds_read_b128 pull the two (ts,
     * val) pairs, then one 16B store per array; the 4 lanes of a row write
     * its 64 contiguous bytes = full 64B-line utilization (WRITE_SIZE stays
     * at the algorithmic 16 B/pt). A partial row stores 16 bytes where both
     * points of the pair exist, 8 where only the first does. */
    auto flush_wide = [&](uint32_t base_pt) {
        const uint32_t q = lane & 3;
        const uint32_t r0 = lane >> 2;
        const uint32_t pt = base_pt + 2 * q;
        /* rows r0 + 16j share r0's low three bits, hence one swizzle */
        const uint32_t pc = (2 * q) ^ dec_swz(r0 & 7);
        if (__all(cnt >= base_pt + DEC_TILE)) {
            /* all 64 rows full: unconditional stores, no per-row counts */
            for (uint32_t j = 0; j < DEC_TILE / 2; j++) {
                uint32_t rr = r0 + j * (WAVE / 4);
                uint64_t row = (uint64_t)__shfl((int)series, (int)rr);
                longlong2 p0 = tile[rr][pc];
                longlong2 p1 = tile[rr][pc ^ 1];
                out_st16(out_ts + row * stride + pt, p0.x, p1.x);
                out_st16(out_vals + row * stride + pt, p0.y, p1.y);
            }
        } else {
            for (uint32_t j = 0; j < DEC_TILE / 2; j++) {
                uint32_t rr = r0 + j * (WAVE / 4);
                uint32_t cc = (uint32_t)__shfl((int)cnt, (int)rr);
                uint64_t row = (uint64_t)__shfl((int)series, (int)rr);
                if (pt < cc) {
                    longlong2 p0 = tile[rr][pc];
                    if (pt + 1 < cc) {
                        longlong2 p1 = tile[rr][pc ^ 1];
                        out_st16(out_ts + row * stride + pt, p0.x, p1.x);
                        out_st16(out_vals + row * stride + pt, p0.y, p1.y);
                    } else {
                        out_st8(out_ts + row * stride + pt, p0.x);
                        out_st8(out_vals + row * stride + pt, p0.y);
                    }
                }
            }
        }
    };
    /* 8-byte form, for outputs that are not 16-byte aligned or an odd
     * stride: lane l covers row (l>>3)+8j, point (l&7) — one ds_read_b128,
     * then two 8B stores consecutive across the 8 lanes of a row */
    auto flush_narrow = [&](uint32_t base_pt) {
        const uint32_t p = lane & (DEC_TILE - 1);
        const uint32_t r0 = lane / DEC_TILE;
        const uint32_t pt = base_pt + p;
        const uint32_t pc = p ^ dec_swz(r0 & 7); /* rows r0 + 8j: same swizzle */
        const bool full = __all(cnt >= base_pt + DEC_TILE);
        for (uint32_t j = 0; j < DEC_TILE; j++) {
            uint32_t rr = r0 + j * (WAVE / DEC_TILE);
            uint32_t cc = (uint32_t)__shfl((int)cnt, (int)rr);
            uint64_t row = (uint64_t)__shfl((int)series, (int)rr);
            if (full || pt < cc) {
                longlong2 pr = tile[rr][pc];
                out_st8(out_ts + row * stride + pt, pr.x);
                out_st8(out_vals + row * stride + pt, pr.y);
            }
        }
    };
    auto flush = [&](uint32_t base_pt) {
        if (discard) return;
        __builtin_amdgcn_wave_barrier();
        if (wide) flush_wide(base_pt);
        else flush_narrow(base_pt);
        __builtin_amdgcn_wave_barrier();
    };

    /* full kernel: byte j of tile_units is the unit after this tile's point
     * j; a lane stores its own row's bytes (out_flush_units, out_tile.h) */
    uint64_t tile_units = 0;
    auto flush_units = [&](uint32_t base_pt) {
        if (!full.units) return;
        out_flush_units<DEC_TILE>(full.units, series, stride, cnt, base_pt,
                                  tile_units);
    };

    /* capacity is tile-hoisted: the per-point check only runs on the rare
     * tile that could cross `stride` */
    auto step = [&](uint32_t j, bool check_cap) {
        if (running) {
            int64_t t;
            double v;
            int rstat = d.next(&t, &v);
            if (rstat <= 0) {
                err = -rstat;
                running = false;
            } else if (check_cap && cnt >= stride) {
                err = M3GPU_SERIES_CAPACITY;
                running = false;
            } else {
                if (!discard) {
                    uint32_t col = j ^ swz;
                    longlong2 pr;
                    pr.x = t;
                    pr.y = __double_as_longlong(v);
                    tile[lane][col] = pr;
                }
                if constexpr (FULL)
                    tile_units |= (uint64_t)d.time_unit << (8 * j);
                cnt++;
            }
        }
    };

    /* The top-up span is a per-wave, per-tile choice. A calm tile runs at
     * RF_SPAN_CALM = DEC_TILE: one burst right after the previous tile's
     * flush, one commit right before this tile's, and between them the
     * wave touches VALU and LDS only — it cannot queue behind another
     * wave's output stores. A tile is calm when in the tile before it no
     * running lane pulled more than RF_CALM_MAX words and none ran its
     * ring dry (wnext beyond rfill at a commit: the in-chain load, or the
     * zero words past the stream's end). The first tile, and every tile
     * after a busy one, runs at RF_SPAN. Only the schedule of the loads
     * depends on this: what a lane reads and decodes does not. */
    uint32_t span = RF_SPAN;
    while (__any(running)) {
        /* wave-uniform capacity flag: cnt <= k + j, so the per-point
         * check matters only on a tile that could cross `stride` */
        const bool check_cap = k + DEC_TILE > stride;
        const uint32_t w0 = d.r.wnext;
        bool dry = false;
        /* NOT unrolled, neither loop: the fully-inlined parser is ~10k
         * instructions — it is instantiated exactly once */
#pragma unroll 1
        for (uint32_t h = 0; h < DEC_TILE; h += span) {
            /* scoped to one top-up span: the registers are written by the
             * loads here and first read by the commit below, nothing in
             * between */
            const auto pd = d.r.template refill_issue<DEC_RF_LOW>(running);
#pragma unroll 1
            for (uint32_t j = h; j < h + span; j++) step(j, check_cap);
            dry |= d.r.wnext > d.r.rfill;
            /* the last commit comes BEFORE the flush: its vmcnt wait then
             * covers only this span's loads plus the PREVIOUS tile's
             * stores (issued a tile ago, long retired) — never the 16
             * stores the flush is about to issue */
            d.r.refill_commit(pd);
        }
        span = __all(!running ||
                     (!dry && d.r.wnext - w0 <= RF_CALM_MAX))
                   ? RF_SPAN_CALM : RF_SPAN;
        flush(k);
        if constexpr (FULL) {
            flush_units(k);
            tile_units = 0;
        }
        k += DEC_TILE;
    }

    if (in_range) {
        d.ann_finish(&err);
        out_counts[series] = cnt;
        out_errs[series] = err;
        if constexpr (FULL) {
            if (full.start_ns)
                full.start_ns[series] = d.start_ns(lens[series]);
        }
    }
}

} // namespace m3

#endif /* M3_DECODE_KERNEL_H */
