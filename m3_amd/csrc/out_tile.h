/*
 * out_tile.h — the LDS output tile of the series-per-lane kernels that emit
 * (ts, val) rows (k_decode_batch, k_series_merge): the output stores and
 * their cache policy, the tile's column swizzle, and the transposed flush.
 * k_series_merge calls all of the flush; k_decode_batch calls the unit-byte
 * flush and keeps a copy of the wide and narrow forms, for the measured
 * reason given there. k_step_rows and k_step_fused use the stores
 * alone.
 */
#ifndef M3_OUT_TILE_H
#define M3_OUT_TILE_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "m3tsz_common.h"

namespace m3 {

/* Cache policy of the flush's output stores: 0 plain, 1 non-temporal (nt),
 * 2 write-through (sc1). Plain and nt stores keep their line in the XCD's
 * L2, where the 16 B/pt output stream competes with the lanes' open input
 * lines; sc1 stores drop it. 1M x 1440 decode with the 16-byte flush, same
 * box, alternated with the 8-byte plain parent (13.2-13.8 ms): plain
 * 13.25-13.58, nt 12.76-13.09, sc1 13.11-13.43; `--data production`
 * (parent 4.34-4.43): plain 4.44-4.46, nt 4.03-4.11, sc1 5.20 against a
 * 4.95 parent. sc1 does what it says to the L2 — FETCH_SIZE 21.0 -> 9.6
 * GB, hit rate 26% -> 46%, WRITE_SIZE unchanged — and moves no time: the
 * kernel is not fabric-bound. nt is the default. */
#ifndef OUT_POLICY
#define OUT_POLICY 1
#endif

/* 1: 16 bytes per lane where alignment allows; 0: always the 8-byte form.
 * With nt stores, same box: 8-byte 12.77-13.13 ms, 16-byte 12.76-13.09
 * (a tie on the synthetic mix); `--data production` 4.24-4.27 against
 * 4.03-4.11, where the 16-byte form wins. */
#ifndef FLUSH_WIDE
#define FLUSH_WIDE 1
#endif

typedef long long dec_ll2 __attribute__((ext_vector_type(2)));

/* 8-byte output store. The sc1 form is the relaxed agent-scope atomic
 * store: a global_store_dwordx2 sc1 that the compiler counts in vmcnt. */
template <typename T>
__device__ __forceinline__ void out_st8(T* p, long long x) {
    static_assert(sizeof(T) == 8, "8-byte element");
#if OUT_POLICY == 2
    __hip_atomic_store((long long*)p, x, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
#elif OUT_POLICY == 1
    __builtin_nontemporal_store(x, (long long*)p);
#else
    *(long long*)p = x;
#endif
}

/* 16-byte output store of two consecutive elements; p is 16-byte aligned.
 * No 16-byte atomic store exists, so the sc1 form is the instruction
 * itself. The compiler does not count it in vmcnt, which only makes its
 * own vmcnt(N) waits for counted loads stricter than needed (vmcnt retires
 * in issue order), never laxer; nothing in the kernel reads the outputs
 * back. The trailing s_nop keeps the next instruction from overwriting the
 * data registers while the store still reads them. */
template <typename T>
__device__ __forceinline__ void out_st16(T* p, long long x0, long long x1) {
    static_assert(sizeof(T) == 8, "8-byte element");
    dec_ll2 v;
    v.x = x0;
    v.y = x1;
#if OUT_POLICY == 2
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1"
                 :: "v"(p), "v"(v));
#elif OUT_POLICY == 1
    __builtin_nontemporal_store(v, (dec_ll2*)p);
#else
    *(dec_ll2*)p = v;
#endif
}

/* XOR column swizzle of the output tile for row r (0..7): r with its bits 0
 * and 2 exchanged. A bijection of the row's low three bits keeps the 8
 * lanes of a ds_write_b128 group on 8 different 16-byte columns; bit 0 from
 * row bit 2 puts the four rows that one ds_read_b128 lane group of the wide
 * flush touches ({0,3,5,6} or {1,2,4,7}, mod 8) on four different (row
 * parity, column parity) classes; bit 2 independent of row bit 1 keeps the
 * 8-byte flush's groups (rows {0,1,2,3} mod 4, half a row each)
 * conflict-free as well. */
__device__ __forceinline__ uint32_t dec_swz(uint32_t r) {
    return ((r & 1) << 2) | (r & 2) | ((r >> 2) & 1);
}

/* The transposed flush of one wave's tile, [64 lanes][TILE points] of (ts,
 * val) pairs that lane l wrote at column j ^ dec_swz(l & 7): points base_pt
 * .. base_pt + TILE - 1 of the 64 rows, of which tile row rr holds `cnt`
 * points in all (lane rr's own count) and goes to output row row_of(rr).
 * The caller owns the wave barriers around the flush and the choice of the
 * form; the rows of a wave need not be consecutive. */

/* Wide form: lane l covers row (l>>2)+16j and the point pair 2*(l&3),
 * 2*(l&3)+1 — two ds_read_b128 pull the two (ts, val) pairs, then one 16B
 * store per array; the 4 lanes of a row write its 64 contiguous bytes = full
 * 64B-line utilization (WRITE_SIZE stays at the algorithmic 16 B/pt). A
 * partial row stores 16 bytes where both points of the pair exist, 8 where
 * only the first does. Needs both arrays 16-byte aligned and an even stride. */
template <int TILE, typename RowOf>
__device__ __forceinline__ void out_flush_wide(
        longlong2 (*tile)[TILE], uint32_t lane, uint32_t cnt, uint32_t base_pt,
        int64_t* out_ts, double* out_vals, uint32_t stride, RowOf row_of) {
    static_assert(TILE == 8, "dec_swz swizzles 8 columns");
    const uint32_t q = lane & 3;
    const uint32_t r0 = lane >> 2;
    const uint32_t pt = base_pt + 2 * q;
    /* rows r0 + 16j share r0's low three bits, hence one swizzle */
    const uint32_t pc = (2 * q) ^ dec_swz(r0 & 7);
    if (__all(cnt >= base_pt + TILE)) {
        /* all 64 rows full: unconditional stores, no per-row counts */
        for (uint32_t j = 0; j < TILE / 2; j++) {
            const uint32_t rr = r0 + j * (WAVE / 4);
            const uint64_t row = row_of(rr);
            longlong2 p0 = tile[rr][pc];
            longlong2 p1 = tile[rr][pc ^ 1];
            out_st16(out_ts + row * stride + pt, p0.x, p1.x);
            out_st16(out_vals + row * stride + pt, p0.y, p1.y);
        }
    } else {
        for (uint32_t j = 0; j < TILE / 2; j++) {
            const uint32_t rr = r0 + j * (WAVE / 4);
            const uint32_t cc = (uint32_t)__shfl((int)cnt, (int)rr);
            const uint64_t row = row_of(rr);
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
}

/* 8-byte form, for outputs that are not 16-byte aligned or an odd stride:
 * lane l covers row (l>>3)+8j, point (l&7) — one ds_read_b128, then two 8B
 * stores consecutive across the 8 lanes of a row */
template <int TILE, typename RowOf>
__device__ __forceinline__ void out_flush_narrow(
        longlong2 (*tile)[TILE], uint32_t lane, uint32_t cnt, uint32_t base_pt,
        int64_t* out_ts, double* out_vals, uint32_t stride, RowOf row_of) {
    static_assert(TILE == 8, "dec_swz swizzles 8 columns");
    const uint32_t p = lane & (TILE - 1);
    const uint32_t r0 = lane / TILE;
    const uint32_t pt = base_pt + p;
    const uint32_t pc = p ^ dec_swz(r0 & 7); /* rows r0 + 8j: same swizzle */
    const bool full = __all(cnt >= base_pt + TILE);
    for (uint32_t j = 0; j < TILE; j++) {
        const uint32_t rr = r0 + j * (WAVE / TILE);
        const uint32_t cc = (uint32_t)__shfl((int)cnt, (int)rr);
        const uint64_t row = row_of(rr);
        if (full || pt < cc) {
            longlong2 pr = tile[rr][pc];
            out_st8(out_ts + row * stride + pt, pr.x);
            out_st8(out_vals + row * stride + pt, pr.y);
        }
    }
}

/* The per-point unit bytes of the same tile: byte j of tile_units is the unit
 * of this lane's point base_pt + j. Each lane stores its own row's bytes,
 * exactly those of the points the flush stores (base_pt <= p < cnt, and cnt
 * <= stride): one 8-byte store for a full tile at an 8-byte aligned address,
 * byte stores otherwise. Registers only, so no barrier and no tile. */
template <int TILE>
__device__ __forceinline__ void out_flush_units(
        uint8_t* units, uint64_t row, uint32_t stride, uint32_t cnt,
        uint32_t base_pt, uint64_t tile_units) {
    static_assert(TILE == 8, "a byte per point in one 64-bit register");
    if (cnt <= base_pt) return;
    const uint32_t nb = min(cnt - base_pt, (uint32_t)TILE);
    uint8_t* p = units + row * stride + base_pt;
    if (nb == TILE && !((uintptr_t)p & 7)) {
        *(uint64_t*)p = tile_units;
    } else {
        for (uint32_t i = 0; i < nb; i++)
            p[i] = (uint8_t)(tile_units >> (8 * i));
    }
}

} // namespace m3

#endif /* M3_OUT_TILE_H */
