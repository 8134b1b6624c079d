/*
 * m3tsz_kernels.hip — MI355X (gfx950/CDNA4) native M3TSZ block codec and
 * fused decode->rollup engine, plus the C-ABI host layer (include/m3gpu.h).
 *
 * This is a from-scratch GPU design of the reference's hot path (reference
 * cites per function; format: src/dbnode/encoding/m3tsz + aggregator
 * semantics), NOT a port of its Go code:
 *
 *  - Decode, encode and the lane-tier rollup run one SERIES PER LANE: M3TSZ
 *    is a sequentially-dependent variable-length code, so each lane keeps
 *    its own parser state in VGPRs and a wave works on 64 independent
 *    streams; branches diverge only where the lanes disagree.
 *      decode: each lane pulls its stream through a per-lane LDS word ring
 *        (topped up by deferred global loads, see BitReader) and stages 8
 *        decoded (ts, val) pairs in an LDS tile; the wave then flushes the
 *        tile transposed, 4 consecutive 16B stores per output row segment
 *        (8 of 8B when the outputs are not 16-byte aligned), which keeps
 *        write traffic at the algorithmic 16 B/pt.
 *      encode: each lane emits completed 64-bit words into its own row.
 *      rollup (rollup_kernels.h, included below the decoders): the lane
 *        tier keeps per-bucket state in registers and small quantile
 *        buckets in a per-lane sorted LDS row; deep buckets retry on the
 *        wave-per-series tiers (k_rollup_batch, k_rollup_ckms), which run
 *        ONE series per wavefront with a wave-uniform parser and reproduce
 *        the reference CKMS walk exactly. All three tiers share one bucket
 *        walk, accumulate and ValueOf (rollup_bucket.h) and one
 *        exact-quantile index (rollup_plan.h), both host-compilable.
 *  - Streams are decoded from 8-byte-aligned offsets, zero-padded to an
 *    8-byte boundary (layout contract in m3gpu.h; pack_streams emits 64B
 *    alignment, which satisfies it) so every refill is an aligned u64 load.
 *  - Wave64 only; no CUDA shims, no hipified code.
 *
 * Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (bit-exact f64:
 * convertToIntFloat m3tsz.go:78-119, decode accumulation iterator.go:168-175).
 */
#include <hip/hip_runtime.h>
#include <atomic>
#include <math.h>
#include <string.h>
#include <type_traits>
#include <stdio.h>
#include "../../include/m3gpu.h"
#include "rollup_plan.h" /* QCAP, MAX_AGGS, m3::RollupPlan + its host builder */
#include "rollup_bucket.h" /* go_f2i; the rollup tiers' shared bucket code */

/* ========================= shared constants ========================= */
/* m3tsz.go:28-62, scheme.go:28-52, x/time/unit.go:30-42 */

#define WAVE 64
#define WAVES_PER_BLOCK 4
#define BLOCK_THREADS (WAVE * WAVES_PER_BLOCK)

namespace m3 {

__device__ __constant__ int64_t UNIT_NS_D[9] = {
    0, 1000000000LL, 1000000LL, 1000LL, 1LL,
    60000000000LL, 3600000000000LL, 86400000000000LL, 31536000000000000LL};

#define MARKER_OPCODE 0x100ULL
#define MARKER_BITS 11 /* 9 opcode + 2 value */
#define MARKER_EOS 0
#define MARKER_ANNOTATION 1
#define MARKER_TIMEUNIT 2

#define MAX_MULT 6
#define NUM_SIG_BITS 6
#define NUM_MULT_BITS 3
#define SIG_DIFF_THRESHOLD 3
#define SIG_REPEAT_THRESHOLD 5

__device__ __forceinline__ int unit_valid(uint8_t u) { return u > 0 && u < 9; }

/* scheme.go:42-52: {7,9,12} bucket value bits; default 32 (s/ms) / 64 (us/ns) */
__device__ __forceinline__ int scheme_default_bits(uint8_t unit) {
    if (unit == 1 || unit == 2) return 32;
    if (unit == 3 || unit == 4) return 64;
    return 0;
}

__device__ __forceinline__ uint8_t num_sig(uint64_t v) { /* encoding.go:29-31 */
    return (uint8_t)(64 - (v ? __builtin_clzll(v) : 64));
}
__device__ __forceinline__ int64_t sign_extend(uint64_t v, uint32_t nbits) {
    uint32_t sh = 64 - nbits;
    return ((int64_t)(v << sh)) >> sh;
}
/* 10^m for m in [0,6] as a pure VALU select chain (see exp10_table note:
 * an indexed const array would cost a global load + vmcnt(0) per use) */
__device__ __forceinline__ double exp10_sel(uint8_t m) {
    double r = 1.0;
    r = (m == 1) ? 10.0 : r;
    r = (m == 2) ? 100.0 : r;
    r = (m == 3) ? 1000.0 : r;
    r = (m == 4) ? 10000.0 : r;
    r = (m == 5) ? 100000.0 : r;
    r = (m == 6) ? 1000000.0 : r;
    return r;
}

/* go_f2i (Go's float64->int64) is in rollup_bucket.h: the counter rollup and
 * its host-side test need it too */
__device__ __forceinline__ uint64_t f2bits(double v) { return __double_as_longlong(v); }
__device__ __forceinline__ double bits2f(uint64_t b) { return __longlong_as_double((long long)b); }

/* Go math.Modf: Modf(+-Inf) = (+-Inf, NaN). The finite path is exact
 * trunc-toward-zero + subtract (v - trunc(v) is exact in IEEE — Sterbenz
 * for |v| >= 1, and trunc(v) == 0 below), one v_trunc_f64 + v_add_f64
 * instead of the libm modf sequence. */
__device__ __forceinline__ double go_modf(double v, double* ip) {
    if (isinf(v)) { *ip = v; return __longlong_as_double(0x7ff8000000000000LL); }
    double i = trunc(v);
    *ip = i;
    return v - i;
}

/* ===================== device bit reader ===================== */
/* istream.go:73-115 over reader64.go:40-80, with the m3gpu.h layout
 * contract: stream starts 8B-aligned, buffer zero-padded to 8B. */

/* Per-lane LDS input ring (series-per-lane kernels), rows [wave][lane][depth].
 * The depth (buffered u64 words per lane, a power of two) is a template
 * parameter of the reader, so each kernel picks its own:
 *  - IN_WORDS = 4 (8 KB/block): k_rollup_lane and k_step_fused.
 *  - DEC_RING = 8 (16 KB/block): k_decode_batch, see there. */
#ifndef IN_WORDS
#define IN_WORDS 4
#endif

/* The ring pointer carries its address space in its type: a generic pointer
 * here lets the optimizer merge the ring read with the underrun path's
 * global load into one load through a selected pointer, i.e. a flat load. */
typedef __attribute__((address_space(3))) uint64_t lds_u64;

/* One tile's ring top-up in flight: raw (un-swapped) little-endian words
 * exactly as the loads deliver them, plus how many of them are real. Lives
 * in the tile loop's scope, NOT in the reader: nothing may read, copy or
 * select these registers between refill_issue() and refill_commit(), or
 * the compiler has to wait for the loads (vmcnt) right there. */
template <int DEPTH>
struct RingPendingT {
    uint64_t w[DEPTH];
    uint32_t n;
};
using RingPending = RingPendingT<IN_WORDS>;

/* The same for the 16-byte refill (BitReader WIDE): a burst of n words from
 * `src` is a leading single word where src is not 16-byte aligned, then
 * 16-byte pairs, then a trailing single word where an odd number is left.
 * Every register is written by at most one load. */
typedef unsigned long long ring_u64x2 __attribute__((ext_vector_type(2)));
template <int DEPTH>
struct RingPendingWideT {
    uint64_t head, tail;
    ring_u64x2 pr[DEPTH / 2];
    uint32_t n, odd;
};

/* RING is a compile-time property of the kernel: the ring's depth in words
 * for the series-per-lane kernels (k_decode_batch, k_rollup_lane,
 * k_step_fused), 0 for the wave-per-series rollup and CKMS kernels (direct
 * reader); the ring is the lane's own row of RING consecutive words. WIDE
 * picks the 16-byte form of the top-up's loads (k_decode_batch). */
template <int RING, bool WIDE = false>
struct BitReader {
    static_assert(RING >= 0 && (RING & (RING - 1)) == 0,
                  "ring depth: 0 (direct) or a power of two");
    static_assert(!WIDE || RING >= 2, "16-byte refill: ring mode only");
    using Pending = typename std::conditional<
        WIDE, RingPendingWideT<RING ? RING : 2>,
        RingPendingT<RING ? RING : 1>>::type;
    /* 128-bit register lookahead (`a` = next bits, `b` = following word,
     * both byte-swapped to stream bit order; `p` = bits of `a` already
     * consumed): peek64() is branch-free, consume() crosses at most one
     * word per call (every field is <= 64 bits). EOF semantics match
     * istream.go:73-115 over reader64.go:40-80: `bits_left` counts the
     * un-consumed TRUE stream bits, reads past it fail per series; the
     * blob's zero padding reproduces reader64's zero-filled partial tail
     * word, so the window itself can always hold 128 physical bits.
     *
     * Words arrive one of two ways:
     *  - ring (RING): refill_issue()/refill_commit() top the per-lane
     *    RING-word LDS ring up once per 8-point tile with consecutive
     *    words of the lane's own stream, so the long-latency global
     *    gathers leave the per-point dependency chain: the parser's word
     *    pulls are ds_read_b64s. A lane that drains its ring inside a
     *    tile (dense streams) falls back to an in-chain global load.
     *  - direct (!RING): a 1-deep register prefetch (`pfw`) beyond the
     *    window, i.e. 3 words of lookahead, keeps the refill load issued
     *    ~128 bits before first use. */
    const uint64_t* words;
    uint64_t a, b, c;   /* c: ring-word prefetch — the ds_read latency sits
                         * between one crossing and the NEXT, not in the
                         * peek chain */
    uint32_t p;
    int64_t bits_left;  /* un-consumed stream bits (from the true byte len) */
    uint32_t wnext;     /* next word index to pull into the window */
    uint32_t wtotal;    /* ceil(len/8) */
    lds_u64* lds;       /* ring mode: this lane's ring base */
    uint32_t rfill;     /* ring mode: words fetched into the ring so far */
    uint64_t pfw;       /* direct mode: extra prefetched word */

    __device__ __forceinline__ uint64_t next_word() {
        uint64_t w;
        if constexpr (RING != 0) {
            /* ring hit is the steady state (refill runs per tile); a
             * mid-tile underrun (streams consuming more than the ring
             * holds in 8 points) falls back to a direct load — correct,
             * just slower, and its wait drains every store in flight */
            if (wnext < rfill) w = lds[wnext & (RING - 1)];
            else w = (wnext < wtotal) ? __builtin_bswap64(words[wnext]) : 0;
        } else {
            w = pfw;
            uint32_t nn = wnext + 1;
            pfw = (nn < wtotal) ? __builtin_bswap64(words[nn]) : 0;
        }
        wnext++;
        return w;
    }

    /* Deferred ring top-up. refill_issue() runs at the start of a span of
     * points with the whole wave converged and issues up to RING global
     * loads per lane back to back; refill_commit() byte-swaps them and
     * writes them to the ring at the end of the span, before the tile's
     * output stores issue. gfx9 vmcnt retires in issue order, so the
     * commit's wait covers these loads and whatever was issued before them
     * — the PREVIOUS tile's output stores, a whole tile old — and never
     * the stores the flush is about to issue. The loads' latency hides
     * under the span's parsing.
     *
     * What makes that hold in the compiled kernel: each load is
     * exec-masked to the lanes that want word i (a lane reads words
     * [rfill, rfill + n) of its own stream and nothing else), its
     * destination is zeroed BEFORE the branch and is a value scoped to the
     * span, not reader state carried round the loop — so there is no copy
     * or select at the branch's join, nothing touches the register until
     * the commit, and the compiler places no wait at the issue. */
#ifndef RF_LOW
#define RF_LOW 3 /* 4-word ring: refill when <= this many words remain (that
                  * is always; the 8-word ring of k_decode_batch has its
                  * own DEC_RF_LOW). Topping up
                  * word by word at every chance re-fetches each 64B line
                  * several times (FETCH_SIZE ~5x the stream) but keeps the
                  * ring from drying inside a span; whole-ring-only refills
                  * (RF_LOW 0) were re-measured with the deferred refill in
                  * place and still lose: 16.57 vs 16.11 ms */
#endif
    template <uint32_t LOW = RF_LOW>
    __device__ __forceinline__ Pending refill_issue(bool active) {
        static_assert(RING != 0, "ring mode only");
        if (rfill < wnext) rfill = wnext; /* resync: underrun consumed
                                           * [rfill, wnext) directly */
        const uint32_t used = rfill - wnext;
        uint32_t n = wtotal - rfill;
        const uint32_t room = RING - used;
        if (n > room) n = room;
        if (!(active && used <= LOW && rfill < wtotal)) n = 0;
        Pending pd;
        pd.n = n;
        if constexpr (WIDE) {
            /* words [odd, odd + 2 * npair) of the burst go as 16-byte
             * loads from 16-byte aligned addresses, never past word n - 1
             * (the word behind a stream's last is another stream's, or
             * none); the one in front and the one behind as 8-byte loads */
            const uint64_t* src = words + rfill;
            const uint32_t odd = (uint32_t)((uintptr_t)src >> 3) & 1;
            pd.odd = odd;
            pd.head = 0;
            if (odd && n > 0) pd.head = src[0];
#pragma unroll
            for (uint32_t j = 0; j < RING / 2; j++) {
                pd.pr[j] = ring_u64x2{0, 0};
                if (odd + 2 * j + 1 < n)
                    pd.pr[j] = *(const ring_u64x2*)(src + odd + 2 * j);
            }
            pd.tail = 0;
            if (n > odd && ((n - odd) & 1)) pd.tail = src[n - 1];
        } else {
#pragma unroll
            for (uint32_t i = 0; i < RING; i++) {
                pd.w[i] = 0;
                if (i < n) pd.w[i] = words[rfill + i];
            }
        }
        return pd;
    }
    __device__ __forceinline__ void refill_commit(const Pending& pd) {
        static_assert(RING != 0, "ring mode only");
        /* The one place the burst is waited for, by the whole wave and for
         * all RING loads at once. The empty asm only pins that: it
         * "uses" each raw word here, so (a) the compiler cannot fold the
         * byte swap below back up into refill_issue() (it would wait for
         * the loads right where they issue), and (b) no load is left
         * pending past the commit when no lane wanted its word — the next
         * tile's burst would then have to wait for it behind this tile's
         * output stores. */
        if constexpr (WIDE) {
            uint64_t head = pd.head, tail = pd.tail;
            uint64_t w[RING];
            asm volatile("" : "+v"(head));
#pragma unroll
            for (uint32_t j = 0; j < RING / 2; j++) {
                ring_u64x2 v = pd.pr[j];
                asm volatile("" : "+v"(v));
                w[2 * j] = v.x;
                w[2 * j + 1] = v.y;
            }
            asm volatile("" : "+v"(tail));
            const uint32_t n = pd.n, odd = pd.odd;
            if (odd && n > 0)
                lds[rfill & (RING - 1)] = __builtin_bswap64(head);
#pragma unroll
            for (uint32_t j = 0; j < RING / 2; j++)
                if (odd + 2 * j + 1 < n) {
                    lds[(rfill + odd + 2 * j) & (RING - 1)] =
                        __builtin_bswap64(w[2 * j]);
                    lds[(rfill + odd + 2 * j + 1) & (RING - 1)] =
                        __builtin_bswap64(w[2 * j + 1]);
                }
            if (n > odd && ((n - odd) & 1))
                lds[(rfill + n - 1) & (RING - 1)] =
                    __builtin_bswap64(tail);
            rfill += n;
        } else {
            uint64_t w[RING];
#pragma unroll
            for (uint32_t i = 0; i < RING; i++) {
                w[i] = pd.w[i];
                asm volatile("" : "+v"(w[i]));
            }
#pragma unroll
            for (uint32_t i = 0; i < RING; i++)
                if (i < pd.n)
                    lds[(rfill + i) & (RING - 1)] = __builtin_bswap64(w[i]);
            rfill += pd.n;
        }
    }

    __device__ __forceinline__ void init(const uint8_t* base, uint64_t off,
                                         uint32_t l, uint64_t* ring) {
        words = (const uint64_t*)(base + off);
        wtotal = (l + 7) >> 3;
        bits_left = (int64_t)l * 8;
        wnext = 0;
        if constexpr (RING != 0) {
            lds = (lds_u64*)ring;
            rfill = 0;
            /* called with the whole wave converged */
            const Pending pd = refill_issue(true);
            refill_commit(pd);
        } else {
            pfw = wtotal ? __builtin_bswap64(words[0]) : 0;
        }
        a = next_word();
        b = next_word();
        c = next_word();
        p = 0;
    }

    /* next 64 physical bits (zero-padded past the stream tail); branch-free */
    __device__ __forceinline__ uint64_t peek64() const {
        return (a << p) | (p ? (b >> (64 - p)) : 0);
    }
    /* advance n <= 64 bits already validated against bits_left */
    __device__ __forceinline__ void consume(uint32_t n) {
        bits_left -= n;
        p += n;
        if (p >= 64) {
            a = b;
            b = c;
            c = next_word();
            p -= 64;
        }
    }
    __device__ __forceinline__ int read_bits(uint32_t n, uint64_t* out) {
        if (bits_left < (int64_t)n) return M3GPU_SERIES_EOF;
        *out = n ? (peek64() >> (64 - n)) : 0;
        consume(n);
        return 0;
    }
    __device__ __forceinline__ int peek_bits(uint32_t n, uint64_t* out) {
        if (bits_left < (int64_t)n) return M3GPU_SERIES_EOF;
        *out = n ? (peek64() >> (64 - n)) : 0;
        return 0;
    }
};

/* ===================== device decoder state ===================== */
/* Port of the reference decode state machine: iterator.go:47-219,
 * timestamp_iterator.go:41-361, float_encoder_iterator.go:105-165. */

template <int RING, bool WIDE = false>
struct DecoderT {
    BitReader<RING, WIDE> r;
    int64_t prev_time, prev_time_delta;
    int64_t unit_ns; /* cached UNIT_NS_D[time_unit] (0 when unit invalid) */
    double mult_pow;  /* cached 10^mult (mult changes rarely; keeping the
                       * select chain out of the per-point value emit) */
    double int_val;
    uint64_t prev_float_bits, prev_xor;
    uint8_t time_unit, scheme_unit, mult, sig;
    uint8_t default_unit;
    bool have_scheme, tu_changed, done, is_float;
    bool int_optimized;

    __device__ __forceinline__ void set_unit(uint8_t tu) {
        time_unit = tu;
        /* Series-per-lane kernels (the wave-per-series ones keep this state
         * in scalar registers, where the lookup is a scalar load):
         * the per-lane table lookup is a global load. Pin its wait HERE,
         * on this rare path (the empty asm "uses" the result): left to
         * the compiler, the load stays in flight until the first use of
         * unit_ns, which is in the per-point path, and the vmcnt(0) there
         * drains the ring top-up and every output store in flight. */
        int64_t ns = unit_valid(tu) ? UNIT_NS_D[tu] : 0;
        if constexpr (RING != 0) asm volatile("" : "+v"(ns));
        unit_ns = ns;
    }

    /* optional annotation capture (m3gpu_decode_batch_dev_ann): events
     * {point, off, len} grow from the front of the per-series region,
     * annotation bytes from the tail; collision flags CAPACITY */
    uint8_t* ann_region;
    uint32_t ann_stride_, ann_events, ann_tail, points;
    int ann_err;

    /* The block start: the stream's first 64 bits, what read_first_timestamp
     * reads into `nt`; 0 for a stream of `len` < 8 bytes, whose read fails
     * with EOF. Re-read from the stream (the words of a stream of 8 bytes or
     * more are addressable) instead of carried in registers through the
     * point loop: one load per series, for the full decode's epilogue. */
    __device__ __forceinline__ int64_t start_ns(uint32_t len) const {
        return len >= 8 ? (int64_t)__builtin_bswap64(r.words[0]) : 0;
    }

    __device__ __forceinline__ void init(const uint8_t* base, uint64_t off, uint32_t len,
                         bool intopt, uint8_t dunit, uint64_t* ring = nullptr,
                         uint8_t* ann = nullptr, uint32_t ann_stride = 0) {
        /* `ring` is this lane's LDS ring row (RING), ignored otherwise */
        r.init(base, off, len, ring);
        prev_time = 0; prev_time_delta = 0;
        int_val = 0; prev_float_bits = 0; prev_xor = 0;
        time_unit = 0; unit_ns = 0; scheme_unit = 0; mult = 0; sig = 0;
        mult_pow = 1.0;
        default_unit = dunit;
        have_scheme = false; tu_changed = false; done = false; is_float = false;
        int_optimized = intopt;
        ann_region = ann;
        ann_stride_ = ann_stride;
        ann_events = 0;
        ann_tail = ann_stride;
        points = 0;
        ann_err = 0;
    }

    /* timestamp_iterator.go:115-135 */
    __device__ __forceinline__ int read_time_unit() {
        uint64_t tu_bits;
        int err = r.read_bits(8, &tu_bits);
        if (err) return err;
        uint8_t tu = (uint8_t)tu_bits;
        if (unit_valid(tu) && tu != time_unit) {
            tu_changed = true;
            if (scheme_default_bits(tu)) { have_scheme = true; scheme_unit = tu; }
        }
        set_unit(tu);
        return 0;
    }

    /* binary.ReadVarint via ReadByte */
    __device__ __forceinline__ int read_varint(int64_t* out) {
        uint64_t ux = 0;
        int shift = 0;
        for (int i = 0; i < 10; i++) {
            uint64_t b;
            int err = r.read_bits(8, &b);
            if (err) return err;
            ux |= (b & 0x7f) << shift;
            if (!(b & 0x80)) {
                int64_t x = (int64_t)(ux >> 1);
                if (ux & 1) x = ~x;
                *out = x;
                return 0;
            }
            shift += 7;
        }
        return M3GPU_SERIES_ANNOTATION;
    }

    /* timestamp_iterator.go:327-356. Without a capture region the
     * annotation bytes are skipped; with one (the _ann decode surface)
     * each annotation-set event is recorded as {point, off, len} so the
     * caller can materialize Current()'s sticky PrevAnt
     * (iterator.go:226-231) by carrying events forward. */
    __device__ __forceinline__ int skip_annotation() {
        int64_t alen;
        int err = read_varint(&alen);
        if (err) return err;
        alen += 1;
        if (alen <= 0) return M3GPU_SERIES_ANNOTATION;
        uint8_t* dst = nullptr;
        if (ann_region && !ann_err) {
            uint32_t ev_end = 4 + (ann_events + 1) * 12;
            if (alen > (int64_t)ann_tail || ev_end > ann_tail - (uint32_t)alen) {
                ann_err = M3GPU_SERIES_CAPACITY; /* region full: flag, keep
                                                  * decoding values */
            } else {
                ann_tail -= (uint32_t)alen;
                dst = ann_region + ann_tail;
                uint32_t* ev = (uint32_t*)(ann_region + 4 + ann_events * 12);
                ev[0] = points; /* index of the point this starts applying to */
                ev[1] = ann_tail;
                ev[2] = (uint32_t)alen;
                ann_events++;
            }
        }
        for (int64_t i = 0; i < alen; i++) {
            uint64_t b;
            err = r.read_bits(8, &b);
            if (err) return err;
            if (dst) dst[i] = (uint8_t)b;
        }
        return 0;
    }
    __device__ __forceinline__ void ann_finish(int* err_io) {
        if (!ann_region) return;
        *(uint32_t*)ann_region = ann_events;
        if (ann_err && *err_io == 0) *err_io = ann_err;
    }

    /* timestamp_iterator.go:307-325 */
    __device__ __forceinline__ int read_full_timestamp(int64_t* dod) {
        if (!scheme_default_bits(time_unit)) return M3GPU_SERIES_NO_SCHEME;
        have_scheme = true;
        scheme_unit = time_unit;
        uint64_t bits;
        int err = r.read_bits(64, &bits);
        if (err) return err;
        *dod = (int64_t)bits;
        return 0;
    }

    /* timestamp_iterator.go:250-305 */
    __device__ __forceinline__ int read_dod(int64_t* out) {
        if (tu_changed) return read_full_timestamp(out);
        if (!have_scheme) return M3GPU_SERIES_NO_SCHEME;
        uint64_t cb;
        int err = r.read_bits(1, &cb);
        if (err) return err;
        if (cb == 0) { *out = 0; return 0; }
        const uint32_t opcodes[3] = {0x2, 0x6, 0xe};
        const uint32_t vbits[3] = {7, 9, 12};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            uint64_t nxt;
            err = r.read_bits(1, &nxt);
            if (err) { *out = 0; return 0; } /* swallowed (:271-274) */
            cb = (cb << 1) | nxt;
            if (cb == opcodes[i]) {
                uint64_t db;
                err = r.read_bits(vbits[i], &db);
                if (err) return err;
                if (!unit_valid(time_unit)) { *out = 0; return 0; }
                *out = sign_extend(db, vbits[i]) * unit_ns;
                return 0;
            }
        }
        uint32_t dbits = (uint32_t)scheme_default_bits(scheme_unit);
        uint64_t db;
        err = r.read_bits(dbits, &db);
        if (err) return err;
        if (!unit_valid(time_unit)) { *out = 0; return 0; }
        *out = sign_extend(db, dbits) * unit_ns;
        return 0;
    }

    /* readMarkerOrDeltaOfDelta (:237-248) with tryReadMarker (:174-235)
     * unrolled into a loop (annotation/timeunit markers chain), and the
     * 11-bit marker peek FUSED with the DoD bucket decode: one peek
     * classifies {dod==0 | marker | bucket} (GPU-relevant consequence (ii)
     * of the grammar). Bit-identical to the sequential reference reads;
     * falls back to the bit-by-bit path near end-of-stream (short peek)
     * and for unit-change/no-scheme states. */
    __device__ __forceinline__ int read_marker_or_dod(int64_t* out) {
        /* dominant path: regular cadence emits dod == 0 = a single 0 bit,
         * which can never be a marker (markers start with 1). */
        if (!tu_changed && have_scheme) {
            uint64_t b1;
            if (r.peek_bits(1, &b1) == 0 && b1 == 0) {
                r.consume(1);
                *out = 0;
                return 0;
            }
        }
        for (;;) {
            uint64_t ov;
            /* markers are checked BEFORE any scheme/unit-change gating
             * (tryReadMarker runs first in the reference) */
            if (r.peek_bits(MARKER_BITS, &ov) != 0) return read_dod(out);
            bool fast = !tu_changed && have_scheme;
            if (fast && (ov >> 10) == 0) { /* zero bucket: 1-cadence fast path */
                r.consume(1);
                *out = 0;
                return 0;
            }
            if ((ov >> 2) == MARKER_OPCODE) {
                uint64_t marker = ov & 0x3;
                int err;
                if (marker == MARKER_EOS) {
                    r.consume(MARKER_BITS);
                    done = true;
                    *out = 0;
                    return 0;
                } else if (marker == MARKER_ANNOTATION) {
                    r.consume(MARKER_BITS);
                    err = skip_annotation();
                    if (err) return err;
                    continue;
                } else if (marker == MARKER_TIMEUNIT) {
                    r.consume(MARKER_BITS);
                    err = read_time_unit();
                    if (err) return err;
                    continue;
                }
                /* unknown marker value: falls through and parses as a
                 * bucket (:232-234) — the 10... prefix selects bucket 0,
                 * exactly as the sequential reads would. */
            }
            if (!fast) return read_dod(out); /* unit change / no scheme */
            /* bucket select: count leading ones of the top 4 bits */
            uint32_t top4 = (uint32_t)(ov >> (MARKER_BITS - 4)) & 0xF;
            uint32_t L = __builtin_clz(~(top4 << 28)); /* in [1,4] */
            uint32_t ob = (L <= 3) ? L + 1 : 4;        /* opcode bits */
            uint32_t vb = (L == 1) ? 7 : (L == 2) ? 9 : (L == 3) ? 12
                          : (uint32_t)scheme_default_bits(scheme_unit);
            r.consume(ob);
            uint64_t db;
            int err = r.read_bits(vb, &db);
            if (err) return err;
            if (!unit_valid(time_unit)) { *out = 0; return 0; } /* swallowed */
            *out = sign_extend(db, vb) * unit_ns;
            return 0;
        }
    }

    /* timestamp_iterator.go:137-161 + initialTimeUnit */
    __device__ __forceinline__ int read_first_timestamp() {
        uint64_t nt_bits;
        int err = r.read_bits(64, &nt_bits);
        if (err) return err;
        int64_t nt = (int64_t)nt_bits;
        if (time_unit == 0 && unit_valid(default_unit) &&
            nt % UNIT_NS_D[default_unit] == 0) {
            set_unit(default_unit);
        }
        if (scheme_default_bits(time_unit)) { have_scheme = true; scheme_unit = time_unit; }
        int64_t dod;
        err = read_marker_or_dod(&dod);
        if (err) return err;
        if (!done) prev_time_delta += dod;
        prev_time = nt + prev_time_delta;
        return 0;
    }

    /* timestamp_iterator.go:80-113 */
    __device__ __forceinline__ int read_timestamp(bool* first) {
        *first = false;
        int err;
        if (prev_time != 0) {
            int64_t dod;
            err = read_marker_or_dod(&dod);
            if (err == 0 && !done) {
                prev_time_delta += dod;
                prev_time += prev_time_delta;
            }
        } else {
            *first = true;
            err = read_first_timestamp();
        }
        if (err) return err;
        if (tu_changed) { prev_time_delta = 0; tu_changed = false; }
        return 0;
    }

    /* float_encoder_iterator.go:105-165 */
    __device__ __forceinline__ int read_full_float() {
        uint64_t vb;
        int err = r.read_bits(64, &vb);
        if (err) return err;
        prev_float_bits = vb;
        prev_xor = vb;
        return 0;
    }
    __device__ __forceinline__ int read_next_float() {
        uint64_t cb;
        int err = r.read_bits(1, &cb);
        if (err) return err;
        if (cb == 0) { prev_xor = 0; return 0; }
        uint64_t nxt;
        err = r.read_bits(1, &nxt);
        if (err) return err;
        cb = (cb << 1) | nxt;
        if (cb == 0x2) { /* contained */
            uint32_t lead = prev_xor ? __builtin_clzll(prev_xor) : 64;
            uint32_t trail = prev_xor ? __builtin_ctzll(prev_xor) : 0;
            uint32_t nmean = 64 - lead - trail;
            uint64_t mb;
            err = r.read_bits(nmean, &mb);
            if (err) return err;
            prev_xor = mb << trail;
            prev_float_bits ^= prev_xor;
            return 0;
        }
        uint64_t lm;
        err = r.read_bits(12, &lm);
        if (err) return err;
        uint64_t lead = (lm & 4032) >> 6;
        uint64_t nmean = (lm & 63) + 1;
        uint64_t mb;
        err = r.read_bits((uint32_t)nmean, &mb);
        if (err) return err;
        uint64_t trail = 64 - lead - nmean;
        prev_xor = mb << trail;
        prev_float_bits ^= prev_xor;
        return 0;
    }

    /* iterator.go:178-219 */
    __device__ __forceinline__ int read_int_sig_mult() {
        uint64_t b;
        int err = r.read_bits(1, &b);
        if (err) return err;
        if (b == 1) { /* opcodeUpdateSig */
            err = r.read_bits(1, &b);
            if (err) return err;
            if (b == 0) sig = 0;
            else {
                uint64_t s;
                err = r.read_bits(NUM_SIG_BITS, &s);
                if (err) return err;
                sig = (uint8_t)s + 1;
            }
        }
        err = r.read_bits(1, &b);
        if (err) return err;
        if (b == 1) { /* opcodeUpdateMult */
            uint64_t m;
            err = r.read_bits(NUM_MULT_BITS, &m);
            if (err) return err;
            mult = (uint8_t)m;
            if (mult > MAX_MULT) return M3GPU_SERIES_INVALID_MULT;
            mult_pow = exp10_sel(mult);
        }
        return 0;
    }
    __device__ __forceinline__ int read_int_val_diff() {
        if (sig == 64) { /* readIntValDiffSlow */
            uint64_t sb;
            int err = r.read_bits(1, &sb);
            if (err) return err;
            double sgn = (sb == 1) ? 1.0 : -1.0;
            uint64_t bits;
            err = r.read_bits(sig, &bits);
            if (err) return err;
            int_val += sgn * (double)bits;
            return 0;
        }
        uint64_t bits;
        int err = r.read_bits((uint32_t)sig + 1, &bits);
        if (err) return err;
        double sgn = -1.0;
        if ((bits >> sig) == 1) { sgn = 1.0; bits ^= (1ULL << sig); }
        int_val += sgn * (double)bits;
        return 0;
    }

    /* iterator.go:108-176 */
    __device__ __forceinline__ int read_first_value() {
        if (!int_optimized) return read_full_float();
        uint64_t b;
        int err = r.read_bits(1, &b);
        if (err) return err;
        if (b == 1) { /* float mode */
            err = read_full_float();
            if (err) return err;
            is_float = true;
            return 0;
        }
        err = read_int_sig_mult();
        if (err) return err;
        return read_int_val_diff();
    }
    __device__ __forceinline__ int read_next_value() {
        if (!int_optimized) return read_next_float();
        uint64_t b;
        int err = r.read_bits(1, &b);
        if (err) return err;
        if (b == 0) { /* opcodeUpdate */
            err = r.read_bits(1, &b);
            if (err) return err;
            if (b == 1) return 0; /* repeat */
            err = r.read_bits(1, &b);
            if (err) return err;
            if (b == 1) { /* -> float mode */
                err = read_full_float();
                if (err) return err;
                is_float = true;
                return 0;
            }
            err = read_int_sig_mult();
            if (err) return err;
            err = read_int_val_diff();
            if (err) return err;
            is_float = false;
            return 0;
        }
        if (is_float) return read_next_float();
        return read_int_val_diff();
    }

    /* Fully fused fast path: ONE 64-bit peek decodes the timestamp field
     * AND the common int-mode value field, then ONE consume advances the
     * window. Grammar consequence (i) from SURVEY.md Appendix A: short ts
     * fields (<=16 bits for buckets 0-2) plus a no-update int diff
     * (2+sig bits) fit one 64-bit window. Falls through to the stepwise
     * path (bit-identical) for markers, default buckets, float mode,
     * wide sig, unit changes and near-EOS. Returns 1/0/-err like next().
     * Returns -1000 to mean "take the general path" (nothing consumed). */
    /* XOR field fused from w2 (value bits left-aligned), pre = bits already
     * classified before the XOR control (ts field + optional mode prefix).
     * Returns 0 (consumed + state updated) or -1000 (take stepwise path). */
    __device__ __forceinline__ int fused_xor(uint64_t w2, uint32_t pre) {
        if (!(w2 >> 63)) { /* '0': same value */
            r.consume(pre + 1);
            prev_xor = 0;
            return 0;
        }
        if ((w2 >> 62) == 0x2) { /* '10' contained */
            uint32_t lead = prev_xor ? __builtin_clzll(prev_xor) : 64;
            uint32_t trail = prev_xor ? __builtin_ctzll(prev_xor) : 0;
            uint32_t nmean = 64 - lead - trail;
            if (pre + 2 + nmean > 64) return -1000;
            uint64_t mb = nmean ? ((w2 << 2) >> (64 - nmean)) : 0;
            r.consume(pre + 2 + nmean);
            prev_xor = mb << trail;
            prev_float_bits ^= prev_xor;
            return 0;
        }
        /* '11' + 6b lead + 6b (nmean-1), then payload (may exceed the peek) */
        uint64_t lead = (w2 >> 56) & 0x3f;
        uint64_t nmean = ((w2 >> 50) & 0x3f) + 1;
        r.consume(pre + 14);
        uint64_t mb;
        int err = r.read_bits((uint32_t)nmean, &mb);
        if (err) return -err; /* same EOF point as the stepwise reads */
        uint64_t trail = 64 - lead - nmean;
        prev_xor = mb << trail;
        prev_float_bits ^= prev_xor;
        return 0;
    }

    /* Branch-minimized fast path: ONE branch-free 64-bit peek classifies
     * the timestamp field (dod==0 | bucket 0-2) arithmetically — no
     * per-bucket branching — and the int-mode value field (no-update diff
     * | repeat) with pure select chains, then a single consume advances
     * the window. Per-lane divergence survives only at: the int/float
     * mode split, the rare escapes (markers, default buckets, sig/mode
     * updates, near-EOS) which return -1000 and fall to the stepwise
     * path (bit-identical semantics), and the window crossing inside
     * consume(). Grammar consequence (i), SURVEY.md Appendix A. */
    __device__ __forceinline__ int next_fused(int64_t* t, double* v) {
        if (tu_changed || !have_scheme || prev_time == 0 || r.bits_left < 64)
            return -1000;
        const uint64_t w = r.peek64();
        /* ---- timestamp: '0' => dod 0; '1'^L 0 + {7,9,12}b => bucket ---- */
        const uint64_t b0 = w >> 63;
        uint32_t tsbits = 1;
        int64_t dod = 0;
        if (b0) { /* branched: regular-cadence waves (dod==0 = a single
                   * 0 bit, the dominant shape) skip the bucket block */
            const uint32_t L = (uint32_t)__builtin_clzll(~w); /* leading 1s */
            if (L >= 4 || (w >> 55) == MARKER_OPCODE)
                return -1000; /* default bucket / EOS|annot|timeunit marker */
            const uint32_t vb = (0xC970u >> (L * 4)) & 0xFu; /* {7,9,12} */
            tsbits = L + 1 + vb;
            /* unit_ns==0 swallows invalid units (:271-274) */
            dod = sign_extend((w << (L + 1)) >> (64 - vb), vb) * unit_ns;
        }
        const uint64_t w2 = w << tsbits; /* tsbits <= 16 here */

        if (int_optimized && !is_float) {
            /* int mode: '1' sign+sig diff | '01' repeat | '000' sig/mult
             * update + diff (encoder.go:200-250) | '001' float switch ->
             * stepwise. Covering the update opcode here matters: adaptive
             * sig tracking (int_sig_bits_tracker.go) re-widths every few
             * points on random-walk data, and each stepwise escape drags
             * the whole wave through the big slow path. */
            const uint64_t v0 = w2 >> 63;
            const uint64_t v1 = (w2 >> 62) & 1;
            uint32_t nb;
            if (v0) { /* opcodeNoUpdate: sign + sig diff */
                if (sig > 45u || tsbits + 2u + sig > 64u)
                    return -1000; /* wide sig: field may exceed the peek */
                nb = 2u + sig;
                const uint64_t field = (w2 << 1) >> (63u - sig);
                const uint64_t sbit = (field >> sig) & 1;
                const uint64_t mag = field ^ (sbit << sig);
                int_val += (sbit ? 1.0 : -1.0) * (double)mag;
            } else if (v1) {
                /* repeat: int_val EXACTLY unchanged (adding 0.0 would flip
                 * -0.0; DESIGN.md §6 repeat quirk) */
                nb = 2;
            } else if ((w2 >> 61) & 1) {
                return -1000; /* '001' -> float-mode switch: stepwise */
            } else {
                /* '000' + readIntSigMult + readIntValDiff
                 * (iterator.go:178-219) from the same peek */
                const uint64_t u = w2 << 3;
                uint8_t nsig = sig;
                uint32_t off;
                if (u >> 63) { /* opcodeUpdateSig */
                    const uint64_t z = (u >> 62) & 1;
                    nsig = z ? (uint8_t)(((u >> 56) & 0x3f) + 1) : 0;
                    off = z ? 8u : 2u;
                } else {
                    off = 1u;
                }
                const uint64_t m = u << off;
                uint8_t nmult = mult;
                uint32_t moff;
                if (m >> 63) { /* opcodeUpdateMult */
                    nmult = (uint8_t)((m >> 60) & 0x7);
                    moff = 4u;
                    if (nmult > MAX_MULT)
                        return -1000; /* stepwise raises invalid_mult */
                } else {
                    moff = 1u;
                }
                if (nsig > 45u || tsbits + 3u + off + moff + 1u + nsig > 64u)
                    return -1000;
                const uint64_t f = m << moff;
                const uint64_t sbit = f >> 63;
                const uint64_t mag =
                    nsig ? ((f << 1) >> ((64u - nsig) & 63u)) : 0;
                int_val += (sbit ? 1.0 : -1.0) * (double)mag;
                sig = nsig;
                if (nmult != mult) { mult = nmult; mult_pow = exp10_sel(nmult); }
                nb = 3u + off + moff + 1u + nsig;
            }
            r.consume(tsbits + nb);
            prev_time_delta += dod;
            prev_time += prev_time_delta;
            *t = prev_time;
            /* the f64 divide is ~25 VALU ops: branch it so mult==0 waves
             * (the common case) never pay for a select-discarded divide */
            double outv = int_val;
            if (mult != 0) outv = int_val / mult_pow;
            *v = outv;
            return 1;
        }
        /* float value (pure float stream, or int-optimized float mode) */
        int rx;
        if (!int_optimized) {
            rx = fused_xor(w2, tsbits);
        } else if (w2 >> 63) { /* '1' + XOR */
            rx = fused_xor(w2 << 1, tsbits + 1);
        } else if ((w2 >> 62) & 1) { /* '01' repeat */
            r.consume(tsbits + 2);
            rx = 0;
        } else {
            return -1000; /* '00...' mode change: stepwise */
        }
        if (rx == -1000) return -1000; /* nothing consumed */
        if (rx) return rx; /* negative error, same EOF point as stepwise */
        prev_time_delta += dod;
        prev_time += prev_time_delta;
        *t = prev_time;
        *v = bits2f(prev_float_bits);
        return 1;
    }

    /* One point. Returns 1 = value in (*t,*v), 0 = done, -err on error. */
    __device__ __forceinline__ int next(int64_t* t, double* v) {
        if (done) return 0;
        int f = next_fused(t, v);
        if (f != -1000) {
            points += (f == 1);
            return f;
        }
        bool first;
        int err = read_timestamp(&first);
        if (err) return -err;
        if (done) return 0;
        err = first ? read_first_value() : read_next_value();
        if (err) return -err;
        *t = prev_time;
        if (!int_optimized || is_float) *v = bits2f(prev_float_bits);
        else if (mult != 0) *v = int_val / mult_pow;
        else *v = int_val;
        points++;
        return 1;
    }
    /* select chain, NOT an indexed array: a dynamically-indexed local
     * const table lowers to a .rodata global_load whose vmcnt(0) wait
     * (gfx9 vmcnt counts stores too) drains every in-flight output store
     * right in the per-point value chain */
    __device__ __forceinline__ double exp10_table(uint8_t m) {
        return exp10_sel(m);
    }
};

using Decoder = DecoderT<0>;             /* wave-per-series kernels: direct reader */
using RingDecoder = DecoderT<IN_WORDS>;  /* series-per-lane kernels: 4-word LDS ring */

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
/* points parsed between a ring top-up's issue and its commit; divides
 * DEC_TILE. 2 = four top-ups per tile (figures from the 4-word ring): the
 * dense stream kinds consume 6-8 words per 8 points, and with one top-up per
 * tile they spend half of every tile in the parser's in-chain underrun
 * load, whose vmcnt(0) also drains the output stores. The span trades that
 * against how long a load has to land before its commit waits for it.
 * Same box, 1M x 1440 decode: span 8 16.1 ms, 4 15.9,
 * 2 14.5, 1 15.3. Re-checked with the non-temporal 16-byte flush, where
 * re-requested lines mostly hit the L2, RF_LOW / RF_SPAN one run each on
 * one box: 3/2 14.04, 0/2 14.63, 0/4 15.46, 3/4 15.28 (under sc1 stores:
 * 13.10, 13.75, 14.62, 14.39) — 3 and 2 stay. */
#ifndef RF_SPAN
#define RF_SPAN 2
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
     * XOR column swizzle (col ^ (lane & 7)). */
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

    /* transposed flush, wide form: lane l covers row (l>>2)+16j and the
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
     * j. Each lane stores its own row's bytes, exactly those of the points
     * the flush stores (base_pt <= p < cnt, and cnt <= stride): one 8-byte
     * store for a full tile at an 8-byte aligned address, byte stores
     * otherwise. Registers only, so no barrier and no tile. */
    uint64_t tile_units = 0;
    auto flush_units = [&](uint32_t base_pt) {
        if (!full.units || cnt <= base_pt) return;
        const uint32_t nb = min(cnt - base_pt, (uint32_t)DEC_TILE);
        uint8_t* p = full.units + (uint64_t)series * stride + base_pt;
        if (nb == DEC_TILE && !((uintptr_t)p & 7)) {
            *(uint64_t*)p = tile_units;
        } else {
            for (uint32_t i = 0; i < nb; i++)
                p[i] = (uint8_t)(tile_units >> (8 * i));
        }
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

/* ===================== device encoder ===================== */
/* Word-based big-endian bit emitter producing the byte-identical stream of
 * ostream.go:133-221; lane (w & 63) stages word w, coalesced 512B flushes. */

struct BitWriter {
    /* Per-lane big-endian bit emitter producing the byte-identical stream
     * of ostream.go:133-221. Each lane owns one output row; completed 64-bit
     * words store directly (8B per store; rows padded to 8B). */
    uint64_t acc;       /* left-aligned bit accumulator */
    uint32_t used;      /* bits used in acc */
    uint32_t nwords;    /* full words emitted */
    uint64_t pend;      /* buffered even word: pairs store as aligned 16B */
    uint64_t* out;      /* 16B-aligned output row */
    uint32_t cap_words;
    int err;

    __device__ __forceinline__ void init(uint8_t* row, uint32_t cap_bytes) {
        acc = 0; used = 0; nwords = 0; pend = 0;
        out = (uint64_t*)row;
        cap_words = cap_bytes / 8;
        err = 0;
    }
    __device__ __forceinline__ void emit_word(uint64_t w) {
        if (nwords >= cap_words) { err = M3GPU_SERIES_CAPACITY; return; }
        if (nwords & 1) {
            ulonglong2 pr;
            pr.x = pend;
            pr.y = __builtin_bswap64(w);
            *(ulonglong2*)(out + nwords - 1) = pr;
        } else {
            pend = __builtin_bswap64(w);
        }
        nwords++;
    }
    __device__ __forceinline__ void write_bits(uint64_t v, uint32_t n) {
        if (n == 0 || err) return;
        v = (n >= 64) ? v : (v & ((1ULL << n) - 1)); /* low n bits */
        uint32_t space = 64 - used;
        if (n <= space) {
            acc |= v << (space - n);
            used += n;
            if (used == 64) { emit_word(acc); acc = 0; used = 0; }
        } else {
            uint32_t lo = n - space;      /* remainder */
            acc |= v >> lo;
            emit_word(acc);
            acc = (lo >= 64) ? 0 : (v << (64 - lo));
            used = lo;
        }
    }
    __device__ __forceinline__ void write_bit(uint32_t b) { write_bits(b, 1); }
    /* Flush the buffered word + partial tail word. Returns byte length. */
    __device__ __forceinline__ uint32_t finish() {
        if (nwords & 1) out[nwords - 1] = pend; /* odd word count: flush pend */
        uint32_t nbytes = nwords * 8;
        if (used > 0) {
            if (nwords >= cap_words) { err = M3GPU_SERIES_CAPACITY; return 0; }
            out[nwords] = __builtin_bswap64(acc); /* zero-padded */
            nbytes += (used + 7) / 8;
        }
        return nbytes;
    }
};

/* m3tsz.go:78-119 convertToIntFloat — bit-sensitive: -ffp-contract=off.
 * math.Nextafter on a strictly-positive finite double is a 1-ulp step,
 * which for IEEE positives is an integer inc/dec of the bit pattern —
 * exact, and much cheaper than the libm nextafter sequence inside this
 * up-to-7-iteration loop (val > 0 is guaranteed here: val == 0 has
 * r == 0 and returns first; toward-0 steps down, toward i+1 > val steps
 * up). */
__device__ __forceinline__ double go_next_down(double x) { /* x > 0 finite */
    return __longlong_as_double(__double_as_longlong(x) - 1);
}
__device__ __forceinline__ double go_next_up(double x) { /* x > 0 finite */
    return __longlong_as_double(__double_as_longlong(x) + 1);
}

__device__ __forceinline__ int convert_to_int_float(double v, uint8_t cur_max_mult,
                                    double* out_val, uint8_t* out_mult, bool* out_is_float) {
    const double MAXINT = 9223372036854775808.0;
    if (cur_max_mult == 0 && v < MAXINT) {
        double i, r;
        r = go_modf(v, &i);
        if (r == 0) { *out_val = i; *out_mult = 0; *out_is_float = false; return 0; }
    }
    if (cur_max_mult > MAX_MULT) return M3GPU_SERIES_INVALID_MULT;
    double sign = 1.0;
    if (v < 0) sign = -1.0;
    for (uint8_t m = cur_max_mult; m <= MAX_MULT; m++) {
        double val = v * exp10_sel(m) * sign;
        if (val >= 1e13) break;
        double i, r;
        r = go_modf(val, &i);
        if (r == 0) { *out_val = sign * i; *out_mult = m; *out_is_float = false; return 0; }
        else if (r < 0.1) {
            if (go_next_down(val) <= i) { *out_val = sign * i; *out_mult = m; *out_is_float = false; return 0; }
        } else if (r > 0.9) {
            double nxt = i + 1;
            if (go_next_up(val) >= nxt) { *out_val = sign * nxt; *out_mult = m; *out_is_float = false; return 0; }
        }
    }
    *out_val = v; *out_mult = 0; *out_is_float = true;
    return 0;
}

/* XXH64, seed 0, from the published xxHash specification: the annotation
 * dedupe checksum (timestamp_encoder.go:56,164-170). The bytes sit at any
 * alignment inside an annotation region, hence the memcpy loads. */
#define XXH_P1 11400714785074694791ULL
#define XXH_P2 14029467366897019727ULL
#define XXH_P3 1609587929392839161ULL
#define XXH_P4 9650029242287828579ULL
#define XXH_P5 2870177450012600261ULL
#define XXH_EMPTY 0xEF46DB3751D8E999ULL /* XXH64 of the empty input */

__device__ __forceinline__ uint64_t ld_le64(const uint8_t* p) {
    uint64_t v; __builtin_memcpy(&v, p, 8); return v;
}
__device__ __forceinline__ uint32_t ld_le32(const uint8_t* p) {
    uint32_t v; __builtin_memcpy(&v, p, 4); return v;
}
__device__ __forceinline__ uint64_t xxh_rotl(uint64_t x, uint32_t r) {
    return (x << r) | (x >> (64 - r));
}
__device__ __forceinline__ uint64_t xxh_round(uint64_t acc, uint64_t in) {
    return xxh_rotl(acc + in * XXH_P2, 31) * XXH_P1;
}
__device__ __forceinline__ uint64_t xxh_merge(uint64_t h, uint64_t v) {
    return (h ^ xxh_round(0, v)) * XXH_P1 + XXH_P4;
}
__device__ __noinline__ uint64_t xxh64(const uint8_t* p, uint32_t len) {
    const uint8_t* end = p + len;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = XXH_P1 + XXH_P2, v2 = XXH_P2, v3 = 0, v4 = 0 - XXH_P1;
        do {
            v1 = xxh_round(v1, ld_le64(p));
            v2 = xxh_round(v2, ld_le64(p + 8));
            v3 = xxh_round(v3, ld_le64(p + 16));
            v4 = xxh_round(v4, ld_le64(p + 24));
            p += 32;
        } while (end - p >= 32);
        h = xxh_rotl(v1, 1) + xxh_rotl(v2, 7) + xxh_rotl(v3, 12) + xxh_rotl(v4, 18);
        h = xxh_merge(h, v1); h = xxh_merge(h, v2);
        h = xxh_merge(h, v3); h = xxh_merge(h, v4);
    } else {
        h = XXH_P5;
    }
    h += len;
    for (; end - p >= 8; p += 8)
        h = xxh_rotl(h ^ xxh_round(0, ld_le64(p)), 27) * XXH_P1 + XXH_P4;
    if (end - p >= 4) {
        h = xxh_rotl(h ^ (uint64_t)ld_le32(p) * XXH_P1, 23) * XXH_P2 + XXH_P3;
        p += 4;
    }
    for (; p < end; p++)
        h = xxh_rotl(h ^ (uint64_t)*p * XXH_P5, 11) * XXH_P1;
    h ^= h >> 33; h *= XXH_P2; h ^= h >> 29; h *= XXH_P3; h ^= h >> 32;
    return h;
}

/* Encoder state: encoder.go:42-61 + TimestampEncoder + sig tracker. The bulk
 * kernel drives it with one fixed unit through encode(); the full kernel
 * passes each point's own unit and annotation through encode_full(). */
struct Encoder {
    BitWriter w;
    int64_t unit_ns; /* cached UNIT_NS_D[unit] — the bulk path has one
                      * fixed unit; an indexed read per point would be a
                      * .rodata global load + vmcnt(0) in the hot chain */
    int64_t prev_time, prev_time_delta;
    uint64_t prev_xor, prev_float_bits;
    double int_val;
    uint8_t time_unit, max_mult;
    uint8_t num_sig_state, cur_highest_lower_sig, num_lower_sig;
    bool has_written_first, is_float, int_optimized;
    uint32_t num_encoded;
    uint64_t prev_ann_checksum; /* encode_full only */

    __device__ __forceinline__ void init(uint8_t* row, uint32_t cap_bytes,
                         int64_t start_ns, bool intopt, uint8_t default_unit) {
        w.init(row, cap_bytes);
        prev_time = start_ns;
        prev_time_delta = 0;
        prev_ann_checksum = XXH_EMPTY;
        prev_xor = 0; prev_float_bits = 0;
        int_val = 0;
        /* initialTimeUnit (timestamp_encoder.go:248-259) */
        unit_ns = unit_valid(default_unit) ? UNIT_NS_D[default_unit] : 0;
        time_unit = (unit_valid(default_unit) && unit_ns != 0 &&
                     start_ns % unit_ns == 0) ? default_unit : 0;
        max_mult = 0;
        num_sig_state = 0; cur_highest_lower_sig = 0; num_lower_sig = 0;
        has_written_first = false; is_float = false;
        int_optimized = intopt;
        num_encoded = 0;
    }

    __device__ __forceinline__ void write_marker(uint32_t marker) {
        w.write_bits(MARKER_OPCODE, 9);
        w.write_bits(marker, 2);
    }

    /* unit_ns takes one of a few fixed values (unit.go:30-42); constant-
     * divisor arms (the branch is wave-uniform) let the compiler emit
     * magic-multiply sequences instead of a ~40-op runtime 64-bit
     * division per encoded point */
    __device__ __forceinline__ int64_t div_unit(int64_t x) const {
        switch (unit_ns) {
        case 1LL: return x;
        case 1000LL: return x / 1000LL;
        case 1000000LL: return x / 1000000LL;
        case 1000000000LL: return x / 1000000000LL;
        default: return x / unit_ns;
        }
    }

    /* timestamp_encoder.go:205-246 */
    __device__ __forceinline__ int write_dod_unchanged(int64_t prev_delta, int64_t cur_delta, uint8_t unit) {
        if (!unit_valid(unit)) return M3GPU_SERIES_NO_SCHEME;
        int64_t dod = div_unit(cur_delta - prev_delta);
        if (unit == 1 || unit == 2) {
            if ((int64_t)(int32_t)dod != dod) return M3GPU_SERIES_DOD_OVERFLOW;
        }
        int dbits = scheme_default_bits(unit);
        if (!dbits) return M3GPU_SERIES_NO_SCHEME;
        if (dod == 0) { w.write_bits(0, 1); return 0; }
        /* bucket select arithmetically (the table-lookup form vectorizes
         * into per-lane .rodata global loads): dod fits b two's-complement
         * bits iff bits(|folded|)+1 <= b */
        const uint64_t m = (uint64_t)(dod < 0 ? ~dod : dod);
        const uint32_t nb = (m ? 64u - (uint32_t)__builtin_clzll(m) : 0u) + 1u;
        if (nb <= 12u) {
            const uint32_t sel = (nb <= 7u) ? 0u : (nb <= 9u) ? 1u : 2u;
            const uint32_t opc = (sel == 0) ? 0x2u : (sel == 1) ? 0x6u : 0xeu;
            const uint32_t vb = (sel == 0) ? 7u : (sel == 1) ? 9u : 12u;
            w.write_bits(opc, sel + 2u);
            w.write_bits((uint64_t)dod, vb);
            return 0;
        }
        w.write_bits(0xf, 4);
        w.write_bits((uint64_t)dod, dbits);
        return 0;
    }

    /* timestamp_encoder.go:161-195 shouldWriteAnnotation + writeAnnotation:
     * marker, binary.PutVarint(len - 1), then the bytes at the current bit
     * position, 8 at a time while 8 remain. Caller guarantees len > 0.
     * Inlined, so that the encoder's address never leaves the kernel and its
     * state stays in registers; only the checksum is a real call. */
    __device__ __forceinline__ void write_annotation(const uint8_t* ant, uint32_t len) {
        uint64_t checksum = xxh64(ant, len);
        if (checksum == prev_ann_checksum) return;
        write_marker(MARKER_ANNOTATION);
        uint64_t ux = (uint64_t)(len - 1) << 1; /* zigzag of a value >= 0 */
        for (; ux >= 0x80; ux >>= 7) w.write_bits((ux & 0x7f) | 0x80, 8);
        w.write_bits(ux, 8);
        uint32_t i = 0;
        for (; len - i >= 8; i += 8)
            w.write_bits(__builtin_bswap64(ld_le64(ant + i)), 64);
        for (; i < len; i++) w.write_bits(ant[i], 8);
        prev_ann_checksum = checksum;
    }

    /* timestamp_encoder.go:72-129; the annotation step of WriteNextTime
     * (:104-106) is encode_full's */
    __device__ __forceinline__ int write_time(int64_t cur_time, uint8_t unit) {
        if (!has_written_first) {
            w.write_bits((uint64_t)prev_time, 64);
            has_written_first = true;
        }
        bool tu_changed = false;
        if (unit_valid(unit) && unit != time_unit) { /* maybeWriteTimeUnitChange */
            write_marker(MARKER_TIMEUNIT);
            w.write_bits(unit, 8);
            time_unit = unit;
            unit_ns = UNIT_NS_D[unit];
            tu_changed = true;
        }
        int64_t time_delta = cur_time - prev_time;
        prev_time = cur_time;
        if (tu_changed) {
            w.write_bits((uint64_t)(time_delta - prev_time_delta), 64);
            prev_time_delta = 0;
            return 0;
        }
        int err = write_dod_unchanged(prev_time_delta, time_delta, unit);
        prev_time_delta = time_delta;
        return err;
    }

    /* float_encoder_iterator.go:69-103 */
    __device__ __forceinline__ void write_full_float(uint64_t val) {
        prev_float_bits = val;
        prev_xor = val;
        w.write_bits(val, 64);
    }
    __device__ __forceinline__ void write_xor(uint64_t cur_xor) {
        if (cur_xor == 0) { w.write_bits(0, 1); return; }
        uint32_t pl = prev_xor ? __builtin_clzll(prev_xor) : 64;
        uint32_t pt = prev_xor ? __builtin_ctzll(prev_xor) : 0;
        uint32_t cl = __builtin_clzll(cur_xor);
        uint32_t ct = __builtin_ctzll(cur_xor);
        if (cl >= pl && ct >= pt) {
            w.write_bits(0x2, 2);
            w.write_bits(cur_xor >> pt, 64 - pl - pt);
            return;
        }
        w.write_bits(0x3, 2);
        w.write_bits(cl, 6);
        uint32_t nmean = 64 - cl - ct;
        w.write_bits(nmean - 1, 6);
        w.write_bits(cur_xor >> ct, nmean);
    }
    __device__ __forceinline__ void write_next_float(uint64_t val) {
        uint64_t x = prev_float_bits ^ val;
        write_xor(x);
        prev_xor = x;
        prev_float_bits = val;
    }

    /* int_sig_bits_tracker.go:35-91 */
    __device__ __forceinline__ void tracker_write_int_val_diff(uint64_t val_bits, bool neg) {
        w.write_bit(neg ? 1 : 0);
        w.write_bits(val_bits, num_sig_state);
    }
    __device__ __forceinline__ void tracker_write_int_sig(uint8_t s) {
        if (num_sig_state != s) {
            w.write_bit(1);
            if (s == 0) w.write_bit(0);
            else { w.write_bit(1); w.write_bits((uint64_t)(s - 1), NUM_SIG_BITS); }
        } else {
            w.write_bit(0);
        }
        num_sig_state = s;
    }
    __device__ __forceinline__ uint8_t tracker_track_new_sig(uint8_t nsig) {
        uint8_t new_sig = num_sig_state;
        if (nsig > num_sig_state) {
            new_sig = nsig;
        } else if (num_sig_state - nsig >= SIG_DIFF_THRESHOLD) {
            if (num_lower_sig == 0) cur_highest_lower_sig = nsig;
            else if (nsig > cur_highest_lower_sig) cur_highest_lower_sig = nsig;
            num_lower_sig++;
            if (num_lower_sig >= SIG_REPEAT_THRESHOLD) {
                new_sig = cur_highest_lower_sig;
                num_lower_sig = 0;
            }
        } else {
            num_lower_sig = 0;
        }
        return new_sig;
    }

    /* encoder.go:233-250 */
    __device__ __forceinline__ void write_int_sig_mult(uint8_t s, uint8_t m, bool float_changed) {
        tracker_write_int_sig(s);
        if (m > max_mult) {
            w.write_bit(1);
            w.write_bits(m, NUM_MULT_BITS);
            max_mult = m;
        } else if (num_sig_state == s && max_mult == m && float_changed) {
            w.write_bit(1);
            w.write_bits(max_mult, NUM_MULT_BITS);
        } else {
            w.write_bit(0);
        }
    }

    /* encoder.go:112-146 */
    __device__ __forceinline__ int write_first_value(double v) {
        if (!int_optimized) { write_full_float(f2bits(v)); return 0; }
        double val; uint8_t m; bool isf;
        int err = convert_to_int_float(v, 0, &val, &m, &isf);
        if (err) return err;
        if (isf) {
            w.write_bit(1);
            write_full_float(f2bits(v));
            is_float = true;
            max_mult = m;
            return 0;
        }
        w.write_bit(0);
        int_val = val;
        bool neg_diff = true;
        if (val < 0) { neg_diff = false; val = -1 * val; }
        uint64_t val_bits = (uint64_t)go_f2i(val);
        uint8_t nsig = num_sig(val_bits);
        write_int_sig_mult(nsig, m, false);
        tracker_write_int_val_diff(val_bits, neg_diff);
        return 0;
    }

    /* encoder.go:174-231 */
    __device__ __forceinline__ void write_float_val(uint64_t val, uint8_t m) {
        if (!is_float) {
            w.write_bit(0); w.write_bit(0); w.write_bit(1);
            write_full_float(val);
            is_float = true;
            max_mult = m;
            return;
        }
        if (val == prev_float_bits) { w.write_bit(0); w.write_bit(1); return; }
        w.write_bit(1);
        write_next_float(val);
    }
    __device__ __forceinline__ void write_int_val(double val, uint8_t m, bool isf, double val_diff) {
        if (val_diff == 0 && isf == is_float && m == max_mult) {
            w.write_bit(0); w.write_bit(1);
            return;
        }
        bool neg = false;
        if (val_diff < 0) { neg = true; val_diff = -1 * val_diff; }
        uint64_t diff_bits = (uint64_t)go_f2i(val_diff);
        uint8_t nsig = num_sig(diff_bits);
        uint8_t new_sig = tracker_track_new_sig(nsig);
        bool float_changed = (isf != is_float);
        if (m > max_mult || num_sig_state != new_sig || float_changed) {
            w.write_bit(0); w.write_bit(0); w.write_bit(0);
            write_int_sig_mult(new_sig, m, float_changed);
            tracker_write_int_val_diff(diff_bits, neg);
            is_float = false;
        } else {
            w.write_bit(1);
            tracker_write_int_val_diff(diff_bits, neg);
        }
        int_val = val;
    }

    /* encoder.go:148-172 */
    __device__ __forceinline__ int write_next_value(double v) {
        if (!int_optimized) { write_next_float(f2bits(v)); return 0; }
        double val; uint8_t m; bool isf;
        int err = convert_to_int_float(v, max_mult, &val, &m, &isf);
        if (err) return err;
        double val_diff = 0;
        if (!isf) val_diff = int_val - val;
        if (isf || val_diff >= 9223372036854775808.0 || val_diff <= -9223372036854775808.0) {
            write_float_val(f2bits(val), m);
            return 0;
        }
        write_int_val(val, m, isf, val_diff);
        return 0;
    }

    __device__ __forceinline__ int encode(int64_t t, double v, uint8_t unit) {
        int err = write_time(t, unit);
        if (err) return err;
        err = num_encoded == 0 ? write_first_value(v) : write_next_value(v);
        if (err == 0) num_encoded++;
        return err ? err : w.err;
    }

    /* encoder.go:90 Encode(dp, tu, ant). WriteTime's order: the start (first
     * call only), the annotation, the unit change, the dod. */
    __device__ __forceinline__ int encode_full(int64_t t, double v, uint8_t unit,
                                               const uint8_t* ant, uint32_t ant_len) {
        if (!has_written_first) {
            w.write_bits((uint64_t)prev_time, 64);
            has_written_first = true;
        }
        if (ant_len) write_annotation(ant, ant_len);
        return encode(t, v, unit);
    }

    /* Finalize: appending the EOS marker to the live bitstream produces
     * exactly head[:len-1] + Tail(lastByte, pos) (scheme.go:198-212). */
    __device__ __forceinline__ uint32_t finalize() {
        if (num_encoded == 0 && w.nwords == 0 && w.used == 0) return 0;
        write_marker(MARKER_EOS);
        return w.finish();
    }
};

/* The optional per-series inputs of the full encode (m3gpu.h,
 * m3gpu_encode_batch_full_dev); each pointer may be null. */
struct EncodeFullIn {
    const uint8_t* units;     /* [nseries*stride] per-point unit */
    const int64_t* start_ns;  /* [nseries] block start */
    const uint8_t* ann;       /* [nseries*ann_stride] annotation regions */
    uint32_t ann_stride;      /* multiple of 4, >= 16 */
};

/* Walks one series' annotation region,
 *   [u32 n_events][n_events x {u32 point, u32 off, u32 len}][...bytes],
 * the layout k_decode_batch writes. init() checks the whole event table
 * against the region and the point count before any annotation byte is
 * read, so take() only ever addresses bytes inside the region. */
struct AnnCursor {
    const uint8_t* region;
    uint32_t n_events, next_ev;
    uint32_t next_pt; /* point of event next_ev; UINT32_MAX when exhausted */

    __device__ __forceinline__ const uint32_t* event(uint32_t e) const {
        return (const uint32_t*)(region + 4 + (uint64_t)e * 12);
    }
    __device__ __forceinline__ int init(const uint8_t* r, uint32_t ann_stride,
                                        uint32_t count) {
        region = r;
        n_events = 0; next_ev = 0; next_pt = UINT32_MAX;
        if (!r) return 0;
        uint32_t n = *(const uint32_t*)r;
        if (n > (ann_stride - 4) / 12) return M3GPU_SERIES_ANNOTATION;
        uint32_t prev = 0;
        for (uint32_t e = 0; e < n; e++) {
            const uint32_t* ev = event(e);
            uint32_t pt = ev[0], off = ev[1], len = ev[2];
            if (pt >= count || (e && pt <= prev) ||
                off > ann_stride || len > ann_stride - off)
                return M3GPU_SERIES_ANNOTATION;
            prev = pt;
        }
        n_events = n;
        if (n) next_pt = event(0)[0];
        return 0;
    }
    /* the event at next_pt: its bytes and length (0 = no annotation) */
    __device__ __forceinline__ const uint8_t* take(uint32_t* len) {
        const uint32_t* ev = event(next_ev);
        const uint8_t* p = region + ev[1];
        *len = ev[2];
        next_ev++;
        next_pt = next_ev < n_events ? event(next_ev)[0] : UINT32_MAX;
        return p;
    }
};

/* FULL = false is the bulk kernel: one fixed unit, start = first timestamp,
 * no annotations; `in` is not touched. FULL = true is encoder.go:90
 * Encode(dp, tu, ant) per point: per-point units, annotations and an explicit
 * block start (timestamp_encoder.go:72-259); `unit` is the default unit. */
template <bool FULL>
__global__ void __launch_bounds__(BLOCK_THREADS)
k_encode_batch(const int64_t* __restrict__ ts, const double* __restrict__ vals,
               const uint32_t* __restrict__ counts, uint32_t nseries,
               uint32_t stride, int int_optimized, uint8_t unit,
               uint8_t* __restrict__ out_bytes, uint32_t out_stride,
               uint32_t* __restrict__ out_lens, int32_t* __restrict__ out_errs,
               EncodeFullIn in) {
    /* ONE SERIES PER LANE (like decode). Input points stage through an LDS
     * tile filled cooperatively — fill step j: lane l loads row (l>>3)+8j,
     * point (l&7): 8 consecutive 8B addresses per row = full 64B-line
     * utilization — instead of 64 independent 8B gathers per point. */
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t s_base = blockIdx.x * BLOCK_THREADS + wave * WAVE;
    const uint32_t series = s_base + lane;

    /* unpadded tiles with an XOR column swizzle (col ^ (row & 7)): bank
     * conflict-free for both per-lane access and the coalesced tile pass,
     * and the exact 32 KB/block admits 5 blocks/CU (5 waves/SIMD). */
    __shared__ int64_t ts_tile_all[WAVES_PER_BLOCK][WAVE][DEC_TILE];
    __shared__ double val_tile_all[WAVES_PER_BLOCK][WAVE][DEC_TILE];
    int64_t (*ts_tile)[DEC_TILE] = ts_tile_all[wave];
    double (*val_tile)[DEC_TILE] = val_tile_all[wave];
    /* full kernel only (+2 KB/block): the tile's units, one byte per point,
     * row r's 8 bytes at unit_tile[r] in point order, so each lane takes
     * its tile's units with one 8-byte LDS read */
    __shared__ uint64_t unit_tile_all[FULL ? WAVES_PER_BLOCK : 1][FULL ? WAVE : 1];
    uint64_t* unit_tile = unit_tile_all[FULL ? wave : 0];

    const bool in_range = series < nseries;
    uint32_t n = in_range ? counts[series] : 0;

    Encoder e;
    AnnCursor ac;
    int err = 0;
    if (in_range) {
        int64_t start = n ? ts[(uint64_t)series * stride] : 0;
        if constexpr (FULL) {
            if (in.start_ns) start = in.start_ns[series];
            err = ac.init(in.ann ? in.ann + (uint64_t)series * in.ann_stride
                                 : nullptr, in.ann_stride, n);
        }
        e.init(out_bytes + (uint64_t)series * out_stride, out_stride,
               start, int_optimized != 0, unit);
    }

    auto fill_tile = [&](uint32_t base_pt) {
        __builtin_amdgcn_wave_barrier();
        const uint32_t p = lane & (DEC_TILE - 1);
        const uint32_t r0 = lane / DEC_TILE;
        for (uint32_t j = 0; j < DEC_TILE; j++) {
            uint32_t r = r0 + j * (WAVE / DEC_TILE);
            uint32_t c = (uint32_t)__shfl((int)n, (int)r);
            uint32_t pt = base_pt + p;
            if (pt < c) {
                uint64_t row = (uint64_t)(s_base + r) * stride + pt;
                uint32_t pc = p ^ (r & 7);
                ts_tile[r][pc] = ts[row];
                val_tile[r][pc] = vals[row];
                if constexpr (FULL) {
                    if (in.units)
                        ((uint8_t*)&unit_tile[r])[p] = in.units[row];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    };

    bool running = in_range && n > 0 && !err;
    uint32_t len = 0;
    uint32_t j = 0;
    uint64_t tile_units = 0;
    while (__any(running)) {
        if ((j & (DEC_TILE - 1)) == 0) {
            fill_tile(j);
            if constexpr (FULL) {
                if (in.units) tile_units = unit_tile[lane];
            }
        }
        if (running) {
            uint32_t col = (j & (DEC_TILE - 1)) ^ (lane & 7);
            int64_t t = ts_tile[lane][col];
            double v = val_tile[lane][col];
            if constexpr (FULL) {
                uint8_t u = in.units
                    ? (uint8_t)(tile_units >> (8 * (j & (DEC_TILE - 1)))) : unit;
                const uint8_t* ant = nullptr;
                uint32_t ant_len = 0;
                if (j == ac.next_pt) ant = ac.take(&ant_len);
                err = e.encode_full(t, v, u, ant, ant_len);
            } else {
                err = e.encode(t, v, unit);
            }
            if (err) {
                running = false;
            } else if (j + 1 == n) {
                len = e.finalize();
                err = e.w.err;
                running = false;
            }
        }
        j++;
    }
    if (in_range) {
        out_lens[series] = err ? 0 : len;
        out_errs[series] = err;
    }
}

/* ===================== blob regather (layout pass) ===================== */
/* Physically reorders packed streams: dst series i <- src series perm[i].
 * Used to lay the blob out in wave-schedule order (length-sorted), so the
 * 64 lanes of each decoding wavefront read NEIGHBORING memory instead of
 * scattered streams — the L2-locality companion to the perm scheduling.
 * One series per wavefront, u64 copies (offsets are 16B aligned). */
__global__ void __launch_bounds__(BLOCK_THREADS)
k_regather(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_offsets,
           const uint32_t* __restrict__ lens, const int32_t* __restrict__ perm,
           const uint64_t* __restrict__ dst_offsets, uint32_t nseries,
           uint8_t* __restrict__ dst) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t i = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (i >= nseries) return;
    const uint32_t s = (uint32_t)perm[i];
    const uint64_t* sp = (const uint64_t*)(src + src_offsets[s]);
    uint64_t* dp = (uint64_t*)(dst + dst_offsets[i]);
    uint32_t nwords = (lens[s] + 7) / 8;
    for (uint32_t w = lane; w < nwords; w += WAVE) dp[w] = sp[w];
}

/* ===================== stream compaction kernel ===================== */
/* Packs strided encoder output rows into the tight 8B-aligned blob layout
 * (m3gpu.h): one series per wavefront, u64 copies, coalesced within a row. */
__global__ void __launch_bounds__(BLOCK_THREADS)
k_compact(const uint8_t* __restrict__ src, uint32_t src_stride,
          const uint32_t* __restrict__ lens,
          const uint64_t* __restrict__ dst_offsets, uint32_t nseries,
          uint8_t* __restrict__ dst) {
    /* readfirstlane makes the series index provably wave-uniform: the
     * whole parser then compiles to scalar (SGPR) code with scalar
     * branches instead of exec-mask divergence sequences. */
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t series = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (series >= nseries) return;
    const uint64_t* s = (const uint64_t*)(src + (uint64_t)series * src_stride);
    uint64_t* d = (uint64_t*)(dst + dst_offsets[series]);
    uint32_t nwords = (lens[series] + 7) / 8;
    for (uint32_t w = lane; w < nwords; w += WAVE) d[w] = s[w];
}


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
#define MERGE_ERR_OUT_OF_ORDER 100

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
        if (!first && earliest < prev_at) { err = MERGE_ERR_OUT_OF_ORDER; break; }
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

    /* k_decode_batch's two flush forms; the row of lane rr is wave_row0 + rr,
     * and a lane past nseries has n == 0, so its row is never stored */
    auto flush_wide = [&](uint32_t base_pt) {
        const uint32_t q = lane & 3;
        const uint32_t r0 = lane >> 2;
        const uint32_t pt = base_pt + 2 * q;
        const uint32_t pc = (2 * q) ^ dec_swz(r0 & 7);
        if (__all(n >= base_pt + SM_TILE)) {
            for (uint32_t j = 0; j < SM_TILE / 2; j++) {
                const uint32_t rr = r0 + j * (WAVE / 4);
                const uint64_t row = (uint64_t)wave_row0 + rr;
                longlong2 p0 = tile[rr][pc];
                longlong2 p1 = tile[rr][pc ^ 1];
                out_st16(out_ts + row * out_stride + pt, p0.x, p1.x);
                out_st16(out_vals + row * out_stride + pt, p0.y, p1.y);
            }
        } else {
            for (uint32_t j = 0; j < SM_TILE / 2; j++) {
                const uint32_t rr = r0 + j * (WAVE / 4);
                const uint32_t cc = (uint32_t)__shfl((int)n, (int)rr);
                const uint64_t row = (uint64_t)wave_row0 + rr;
                if (pt < cc) {
                    longlong2 p0 = tile[rr][pc];
                    if (pt + 1 < cc) {
                        longlong2 p1 = tile[rr][pc ^ 1];
                        out_st16(out_ts + row * out_stride + pt, p0.x, p1.x);
                        out_st16(out_vals + row * out_stride + pt, p0.y, p1.y);
                    } else {
                        out_st8(out_ts + row * out_stride + pt, p0.x);
                        out_st8(out_vals + row * out_stride + pt, p0.y);
                    }
                }
            }
        }
    };
    auto flush_narrow = [&](uint32_t base_pt) {
        const uint32_t p = lane & (SM_TILE - 1);
        const uint32_t r0 = lane / SM_TILE;
        const uint32_t pt = base_pt + p;
        const uint32_t pc = p ^ dec_swz(r0 & 7);
        const bool full = __all(n >= base_pt + SM_TILE);
        for (uint32_t j = 0; j < SM_TILE; j++) {
            const uint32_t rr = r0 + j * (WAVE / SM_TILE);
            const uint32_t cc = (uint32_t)__shfl((int)n, (int)rr);
            const uint64_t row = (uint64_t)wave_row0 + rr;
            if (full || pt < cc) {
                longlong2 pr = tile[rr][pc];
                out_st8(out_ts + row * out_stride + pt, pr.x);
                out_st8(out_vals + row * out_stride + pt, pr.y);
            }
        }
    };
    /* a lane's own 8 unit bytes of the tile, stored to its own row: exactly
     * those of the points the flush stores */
    uint64_t tile_units = 0;
    auto flush_units = [&](uint32_t base_pt) {
        if (n <= base_pt) return;
        const uint32_t nb = min(n - base_pt, (uint32_t)SM_TILE);
        uint8_t* p = out_units + (uint64_t)series * out_stride + base_pt;
        if (nb == SM_TILE && !((uintptr_t)p & 7)) {
            *(uint64_t*)p = tile_units;
        } else {
            for (uint32_t i = 0; i < nb; i++)
                p[i] = (uint8_t)(tile_units >> (8 * i));
        }
    };

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
        if (wide) flush_wide(k);
        else flush_narrow(k);
        __builtin_amdgcn_wave_barrier();
        if constexpr (UNITS) {
            flush_units(k);
            tile_units = 0;
        }
        k += SM_TILE;
    }

    if (in_range) {
        out_counts[series] = n;
        out_errs[series] = err;
    }
}


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

/* ===================== fused decode -> rollup kernels ===================== */
#include "rollup_kernels.h" /* all three tiers, over the decoders above */

/* ============================ C-ABI host layer ============================ */

#include <memory>

static __thread char g_err[512];
static int g_device = 0;
static bool g_inited = false;

static int set_hip_err(const char* what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return M3GPU_ERR_HIP;
}
#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return set_hip_err(#expr, _e); } while (0)

/* Owning device allocation of n elements: freed on every return path. */
template <typename T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t n) {
        (void)hipFree(p);
        p = nullptr;
        return hipMalloc(&p, n * sizeof(T));
    }
    /* alloc + blocking H2D copy */
    hipError_t upload(const T* src, size_t n) {
        hipError_t e = alloc(n);
        return e != hipSuccess ? e
             : hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    /* blocking D2H copy */
    hipError_t download(T* dst, size_t n) const {
        return hipMemcpy(dst, p, n * sizeof(T), hipMemcpyDeviceToHost);
    }
};

/* the packed-stream inputs every decoding host form uploads */
struct DevStreams {
    DevBuf<uint8_t> blobs;
    DevBuf<uint64_t> offsets;
    DevBuf<uint32_t> lens;
    hipError_t upload(const uint8_t* h_blobs, uint64_t blobs_len,
                      const uint64_t* h_offsets, const uint32_t* h_lens,
                      uint32_t nseries) {
        hipError_t e = blobs.upload(h_blobs, blobs_len);
        if (e == hipSuccess) e = offsets.upload(h_offsets, (size_t)nseries + 1);
        if (e == hipSuccess) e = lens.upload(h_lens, nseries);
        return e;
    }
};

/* host scratch that cannot throw across the C boundary */
struct FreeDeleter { void operator()(void* p) const { free(p); } };

extern "C" {

const char* m3gpu_last_error(void) { return g_err; }

int m3gpu_init(int device) {
    HIP_TRY(hipSetDevice(device));
    g_device = device;
    g_inited = true;
    return M3GPU_OK;
}

void m3gpu_shutdown(void) { g_inited = false; }

/* wave-per-series kernels (rollup, compact): 4 series per block */
static inline uint32_t grid_for(uint32_t nseries) {
    return (nseries + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
}
/* lane-per-series kernels (decode, encode): 256 series per block */
static inline uint32_t grid_lane(uint32_t nseries) {
    return (nseries + BLOCK_THREADS - 1) / BLOCK_THREADS;
}

int m3gpu_decode_batch_dev(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t stride, void* hip_stream) {
    return m3gpu_decode_batch_dev_perm(d_blobs, d_offsets, d_lens, NULL,
                                       nseries, int_optimized, default_unit,
                                       d_out_ts, d_out_vals, d_out_counts,
                                       d_out_errs, stride, hip_stream);
}

int m3gpu_decode_batch_dev_perm(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    const int32_t* d_perm,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t stride, void* hip_stream) {
    if (!nseries) return M3GPU_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(m3::k_decode_batch<false>, dim3(grid_lane(nseries)),
                       dim3(BLOCK_THREADS), 0, s,
                       d_blobs, d_offsets, d_lens, d_perm, nseries,
                       int_optimized, default_unit, d_out_ts, d_out_vals,
                       d_out_counts, d_out_errs, stride, (uint8_t*)NULL, 0,
                       m3::DecodeFullOut{});
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

/* annotation-region rules of both full-decode forms; touches no HIP state */
static int decode_full_check_args(bool has_ann, uint32_t ann_stride) {
    const char* msg = nullptr;
    if (has_ann && (ann_stride % 4 || ann_stride < 16))
        msg = "ann_stride must be 4-byte aligned and >= 16";
    else if (!has_ann && ann_stride)
        msg = "ann_stride must be 0 without annotation regions";
    if (!msg) return M3GPU_OK;
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return M3GPU_ERR_BADARG;
}

int m3gpu_decode_batch_full_dev(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    const int32_t* d_perm,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t stride,
    uint8_t* d_out_units, int64_t* d_out_start_ns,
    uint8_t* d_out_ann, uint32_t ann_stride, void* hip_stream) {
    if (!nseries) return M3GPU_OK;
    int rc = decode_full_check_args(d_out_ann != nullptr, ann_stride);
    if (rc != M3GPU_OK) return rc;
    if ((uintptr_t)d_out_ann % 4) { /* the event tables are written as u32 */
        snprintf(g_err, sizeof(g_err), "d_out_ann must be 4-byte aligned");
        return M3GPU_ERR_BADARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    m3::DecodeFullOut full{d_out_units, d_out_start_ns};
    hipLaunchKernelGGL(m3::k_decode_batch<true>, dim3(grid_lane(nseries)),
                       dim3(BLOCK_THREADS), 0, s,
                       d_blobs, d_offsets, d_lens, d_perm, nseries,
                       int_optimized, default_unit, d_out_ts, d_out_vals,
                       d_out_counts, d_out_errs, stride, d_out_ann, ann_stride,
                       full);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

int m3gpu_decode_batch_dev_ann(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t stride,
    uint8_t* d_out_ann, uint32_t ann_stride, void* hip_stream) {
    if (!nseries) return M3GPU_OK;
    if (ann_stride % 4 || ann_stride < 16) {
        snprintf(g_err, sizeof(g_err),
                 "ann_stride must be 4-byte aligned and >= 16");
        return M3GPU_ERR_BADARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(m3::k_decode_batch<false>, dim3(grid_lane(nseries)),
                       dim3(BLOCK_THREADS), 0, s,
                       d_blobs, d_offsets, d_lens, (const int32_t*)NULL,
                       nseries, int_optimized, default_unit, d_out_ts,
                       d_out_vals, d_out_counts, d_out_errs, stride,
                       d_out_ann, ann_stride, m3::DecodeFullOut{});
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

int m3gpu_encode_batch_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    uint32_t nseries, uint32_t stride, int int_optimized, uint8_t unit,
    uint8_t* d_out_bytes, uint32_t out_stride, uint32_t* d_out_lens,
    int32_t* d_out_errs, void* hip_stream) {
    if (!nseries) return M3GPU_OK;
    if (out_stride % 8) {
        snprintf(g_err, sizeof(g_err), "out_stride must be a multiple of 8");
        return M3GPU_ERR_BADARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(m3::k_encode_batch<false>, dim3(grid_lane(nseries)),
                       dim3(BLOCK_THREADS), 0, s,
                       d_ts, d_vals, d_counts, nseries, stride, int_optimized,
                       unit, d_out_bytes, out_stride, d_out_lens, d_out_errs,
                       m3::EncodeFullIn{});
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

/* argument rules of both full-encode forms; touches no HIP state */
static int encode_full_check_args(bool has_ann, uint32_t ann_stride,
                                  uint32_t out_stride) {
    const char* msg = nullptr;
    if (out_stride % 8)
        msg = "out_stride must be a multiple of 8";
    else if (has_ann && (ann_stride % 4 || ann_stride < 16))
        msg = "ann_stride must be 4-byte aligned and >= 16";
    else if (!has_ann && ann_stride)
        msg = "ann_stride must be 0 without annotation regions";
    if (!msg) return M3GPU_OK;
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return M3GPU_ERR_BADARG;
}

int m3gpu_encode_batch_full_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    const uint8_t* d_units, const int64_t* d_start_ns,
    const uint8_t* d_ann, uint32_t ann_stride,
    uint32_t nseries, uint32_t stride, int int_optimized, uint8_t default_unit,
    uint8_t* d_out_bytes, uint32_t out_stride, uint32_t* d_out_lens,
    int32_t* d_out_errs, void* hip_stream) {
    if (!nseries) return M3GPU_OK;
    int rc = encode_full_check_args(d_ann != nullptr, ann_stride, out_stride);
    if (rc != M3GPU_OK) return rc;
    if ((uintptr_t)d_ann % 4) { /* the event tables are read as u32 */
        snprintf(g_err, sizeof(g_err), "d_ann must be 4-byte aligned");
        return M3GPU_ERR_BADARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    m3::EncodeFullIn in{d_units, d_start_ns, d_ann, ann_stride};
    hipLaunchKernelGGL(m3::k_encode_batch<true>, dim3(grid_lane(nseries)),
                       dim3(BLOCK_THREADS), 0, s,
                       d_ts, d_vals, d_counts, nseries, stride, int_optimized,
                       default_unit, d_out_bytes, out_stride, d_out_lens,
                       d_out_errs, in);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

int m3gpu_compact_dev(
    const uint8_t* d_src, uint32_t src_stride, const uint32_t* d_lens,
    const uint64_t* d_dst_offsets, uint32_t nseries, uint8_t* d_dst,
    void* hip_stream) {
    if (!nseries) return M3GPU_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(m3::k_compact, dim3(grid_for(nseries)),
                       dim3(BLOCK_THREADS), 0, s,
                       d_src, src_stride, d_lens, d_dst_offsets, nseries, d_dst);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

int m3gpu_regather_dev(
    const uint8_t* d_src, const uint64_t* d_src_offsets,
    const uint32_t* d_lens, const int32_t* d_perm,
    const uint64_t* d_dst_offsets, uint32_t nseries, uint8_t* d_dst,
    void* hip_stream) {
    if (!nseries) return M3GPU_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(m3::k_regather, dim3(grid_for(nseries)),
                       dim3(BLOCK_THREADS), 0, s,
                       d_src, d_src_offsets, d_lens, d_perm, d_dst_offsets,
                       nseries, d_dst);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

/* The plan builder's no-compression cap on its own (rollup_plan.h), for
 * tests and host-side sizing. Aggs past MAX_AGGS are ignored. */
int m3gpu_ckms_exact_cap(const int32_t* agg_types, int naggs, double eps) {
    m3::RollupPlan plan;
    m3::rollup_plan_build(agg_types, naggs < MAX_AGGS ? naggs : MAX_AGGS, eps,
                          1024, &plan);
    return plan.exact_cap;
}

/* Collect the series that d_errs flags M3GPU_SERIES_BUCKET_OVERFLOW into a
 * device selection of *nsel indices (blocking copies; sel stays empty when
 * there are none). */
static int collect_overflow(const int32_t* d_errs, uint32_t nseries,
                            DevBuf<int32_t>* sel, uint32_t* nsel) {
    *nsel = 0;
    std::unique_ptr<int32_t[], FreeDeleter> h(
        (int32_t*)malloc(nseries * sizeof(int32_t)));
    if (!h) { snprintf(g_err, sizeof(g_err), "oom"); return M3GPU_ERR_HIP; }
    HIP_TRY(hipMemcpy(h.get(), d_errs, nseries * sizeof(int32_t),
                      hipMemcpyDeviceToHost));
    /* compact the flagged indices in place: k never passes i */
    uint32_t k = 0;
    for (uint32_t i = 0; i < nseries; i++)
        if (h[i] == M3GPU_SERIES_BUCKET_OVERFLOW) h[k++] = (int32_t)i;
    if (k) HIP_TRY(sel->upload(h.get(), k));
    *nsel = k;
    return M3GPU_OK;
}

int m3gpu_rollup_batch_dev_opts(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int metric_type, int64_t window_ns, uint32_t nbuckets,
    const int32_t* agg_types, int naggs,
    double* d_out, int64_t* d_out_window_ts, int32_t* d_out_errs,
    void* hip_stream, double eps, int every) {
    if (!nseries) return M3GPU_OK;
    if (naggs < 1 || naggs > MAX_AGGS || window_ns <= 0) {
        snprintf(g_err, sizeof(g_err), "bad naggs/window");
        return M3GPU_ERR_BADARG;
    }
    if (!(eps > 0.0 && eps < 0.5) || every < 1 || every > 1024) {
        snprintf(g_err, sizeof(g_err),
                 "eps must be in (0,0.5), every in [1,1024]");
        return M3GPU_ERR_BADARG;
    }
    m3::RollupPlan plan;
    m3::rollup_plan_build(agg_types, naggs, eps, every, &plan);

    hipStream_t s = (hipStream_t)hip_stream;
    bool with_q = plan.nq > 0 && metric_type == M3GPU_METRIC_TIMER;
    /* deeper-than-cap buckets overflow to the wave tier; only use extreme
     * mode when the cap covers normal windows (a lone p99 with the
     * production-default eps has exact_cap 13, which bounds it) */
    bool extreme = with_q && plan.extreme_cap >= 8;
    /* metric type is a template parameter: dead per-metric BucketState
     * fields drop out of the register file. Unknown metric types take the
     * last branch. */
    decltype(&m3::k_rollup_lane<RQ_NONE, M3GPU_METRIC_TIMER>) lane;
    if (extreme)
        lane = m3::k_rollup_lane<RQ_EXTREME, M3GPU_METRIC_TIMER>;
    else if (with_q)
        lane = m3::k_rollup_lane<RQ_STAGED, M3GPU_METRIC_TIMER>;
    else if (metric_type == M3GPU_METRIC_COUNTER)
        lane = m3::k_rollup_lane<RQ_NONE, M3GPU_METRIC_COUNTER>;
    else if (metric_type == M3GPU_METRIC_GAUGE)
        lane = m3::k_rollup_lane<RQ_NONE, M3GPU_METRIC_GAUGE>;
    else
        lane = m3::k_rollup_lane<RQ_NONE, M3GPU_METRIC_TIMER>;
    hipLaunchKernelGGL(lane, dim3(grid_lane(nseries)), dim3(BLOCK_THREADS),
                       0, s,
                       d_blobs, d_offsets, d_lens, nseries, int_optimized,
                       default_unit, window_ns, nbuckets, plan,
                       d_out, d_out_window_ts, d_out_errs);
    HIP_TRY(hipGetLastError());
    if (!with_q) return M3GPU_OK;

    /* buckets deeper than the lane tier's capacity overflow to the
     * wave-per-series kernel. The common case is zero overflows: test
     * with a device-side count + 4-byte D2H instead of pulling and
     * scanning the whole error array every call. */
    /* process-lifetime scratch; atomics guard the one-time alloc
     * (host entry points may be called from multiple threads). One word
     * for every stream and device: splitting it is a separate change. */
    static std::atomic<uint32_t*> g_ovf{nullptr};
    uint32_t* d_ovf = g_ovf.load(std::memory_order_acquire);
    if (!d_ovf) {
        uint32_t* fresh = nullptr;
        HIP_TRY(hipMalloc(&fresh, sizeof(uint32_t)));
        uint32_t* expected = nullptr;
        if (!g_ovf.compare_exchange_strong(expected, fresh,
                                           std::memory_order_acq_rel)) {
            (void)hipFree(fresh); /* another thread won the race */
        }
        d_ovf = g_ovf.load(std::memory_order_acquire);
    }
    HIP_TRY(hipMemsetAsync(d_ovf, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(m3::k_count_errcode, dim3(256), dim3(BLOCK_THREADS),
                       0, s, d_out_errs, nseries,
                       M3GPU_SERIES_BUCKET_OVERFLOW, d_ovf);
    HIP_TRY(hipGetLastError());
    uint32_t h_ovf = 0;
    HIP_TRY(hipMemcpyAsync(&h_ovf, d_ovf, sizeof(uint32_t),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h_ovf == 0) return M3GPU_OK;

    /* One retry tier: rerun the series still flagged as overflowed on the
     * wave-per-series kernel, or (ckms) on the real compressed CKMS
     * (k_rollup_ckms, one series per workgroup, ~129 KB dynamic LDS), and
     * wait for it, since the next step reads the flags it rewrites. */
    auto run_tier = [&](bool ckms) -> int {
        DevBuf<int32_t> sel;
        uint32_t n = 0;
        int rc = collect_overflow(d_out_errs, nseries, &sel, &n);
        if (rc != M3GPU_OK || n == 0) return rc;
        if (!ckms) { /* timers with quantiles only: with_q holds here */
            hipLaunchKernelGGL(m3::k_rollup_batch, dim3(grid_for(n)),
                               dim3(BLOCK_THREADS), 0, s,
                               d_blobs, d_offsets, d_lens, sel.p, n,
                               int_optimized, default_unit,
                               window_ns, nbuckets, plan,
                               d_out, d_out_window_ts, d_out_errs);
        } else {
            size_t lds_bytes = m3::CkmsLdsLayout::bytes;
            HIP_TRY(hipFuncSetAttribute(
                reinterpret_cast<const void*>(m3::k_rollup_ckms),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
            hipLaunchKernelGGL(m3::k_rollup_ckms, dim3(n),
                               dim3(CKMS_BLOCK), lds_bytes, s,
                               d_blobs, d_offsets, d_lens, sel.p, n,
                               int_optimized, default_unit,
                               window_ns, nbuckets, plan,
                               d_out, d_out_window_ts, d_out_errs);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        return M3GPU_OK;
    };
    int rc = run_tier(false);
    /* buckets deeper than the exact-order-statistics cap */
    if (rc == M3GPU_OK) rc = run_tier(true);
    return rc;
}

int m3gpu_rollup_batch_dev(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int metric_type, int64_t window_ns, uint32_t nbuckets,
    const int32_t* agg_types, int naggs,
    double* d_out, int64_t* d_out_window_ts, int32_t* d_out_errs,
    void* hip_stream) {
    return m3gpu_rollup_batch_dev_opts(
        d_blobs, d_offsets, d_lens, nseries, int_optimized, default_unit,
        metric_type, window_ns, nbuckets, agg_types, naggs, d_out,
        d_out_window_ts, d_out_errs, hip_stream, 1e-3, 1024);
}

int m3gpu_merge_batch_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    uint32_t nreplicas, uint32_t nseries, uint32_t stride,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t out_stride, void* hip_stream) {
    if (!nseries) return M3GPU_OK;
    if (nreplicas < 1 || nreplicas > MERGE_MAX_R) {
        snprintf(g_err, sizeof(g_err), "nreplicas must be 1..%d", MERGE_MAX_R);
        return M3GPU_ERR_BADARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(m3::k_merge<false>, dim3(grid_lane(nseries)),
                       dim3(BLOCK_THREADS), 0, s,
                       d_ts, d_vals, d_counts, nreplicas, nseries, stride,
                       d_out_ts, d_out_vals, d_out_counts, d_out_errs,
                       out_stride, (const uint8_t*)NULL, (uint8_t*)NULL);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

int m3gpu_merge_batch_units_dev(
    const int64_t* d_ts, const double* d_vals, const uint8_t* d_units,
    const uint32_t* d_counts, uint32_t nreplicas, uint32_t nseries,
    uint32_t stride, int64_t* d_out_ts, double* d_out_vals,
    uint8_t* d_out_units, uint32_t* d_out_counts, int32_t* d_out_errs,
    uint32_t out_stride, void* hip_stream) {
    if (!nseries) return M3GPU_OK;
    if (nreplicas < 1 || nreplicas > MERGE_MAX_R) {
        snprintf(g_err, sizeof(g_err), "nreplicas must be 1..%d", MERGE_MAX_R);
        return M3GPU_ERR_BADARG;
    }
    if (!d_units || !d_out_units) {
        snprintf(g_err, sizeof(g_err), "d_units and d_out_units must be given");
        return M3GPU_ERR_BADARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(m3::k_merge<true>, dim3(grid_lane(nseries)),
                       dim3(BLOCK_THREADS), 0, s,
                       d_ts, d_vals, d_counts, nreplicas, nseries, stride,
                       d_out_ts, d_out_vals, d_out_counts, d_out_errs,
                       out_stride, d_units, d_out_units);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

/* argument rules of both series-merge forms; touches no HIP state */
static int series_merge_check_args(uint32_t nreplicas, uint32_t nblocks,
                                   uint32_t stride, uint32_t out_stride,
                                   int strategy, bool has_units,
                                   bool has_out_units) {
    if (nreplicas < 1 || nreplicas > MERGE_MAX_R) {
        snprintf(g_err, sizeof(g_err), "nreplicas must be 1..%d", MERGE_MAX_R);
        return M3GPU_ERR_BADARG;
    }
    if (!nblocks || !stride || !out_stride) {
        snprintf(g_err, sizeof(g_err),
                 "nblocks, stride and out_stride must be nonzero");
        return M3GPU_ERR_BADARG;
    }
    if (strategy < M3GPU_EQUAL_TS_LAST_PUSHED ||
        strategy > M3GPU_EQUAL_TS_HIGHEST_FREQUENCY) {
        snprintf(g_err, sizeof(g_err), "strategy must be 0..3");
        return M3GPU_ERR_BADARG;
    }
    if (has_units != has_out_units) {
        snprintf(g_err, sizeof(g_err),
                 "d_units and d_out_units go together: both or neither");
        return M3GPU_ERR_BADARG;
    }
    return M3GPU_OK;
}

int m3gpu_series_merge_batch_dev(
    const int64_t* d_ts, const double* d_vals, const uint8_t* d_units,
    const uint32_t* d_counts, const int32_t* d_errs,
    uint32_t nreplicas, uint32_t nblocks, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t end_ns, int strategy,
    int64_t* d_out_ts, double* d_out_vals, uint8_t* d_out_units,
    uint32_t* d_out_counts, int32_t* d_out_errs, uint32_t out_stride,
    void* hip_stream) {
    int rc = series_merge_check_args(nreplicas, nblocks, stride, out_stride,
                                     strategy, d_units != nullptr,
                                     d_out_units != nullptr);
    if (rc != M3GPU_OK) return rc;
    if (!nseries) return M3GPU_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    if (d_units)
        hipLaunchKernelGGL(m3::k_series_merge<true>, dim3(grid_lane(nseries)),
                           dim3(BLOCK_THREADS), 0, s,
                           d_ts, d_vals, d_units, d_counts, d_errs, nreplicas,
                           nblocks, nseries, stride, start_ns, end_ns,
                           strategy, d_out_ts, d_out_vals, d_out_units,
                           d_out_counts, d_out_errs, out_stride);
    else
        hipLaunchKernelGGL(m3::k_series_merge<false>, dim3(grid_lane(nseries)),
                           dim3(BLOCK_THREADS), 0, s,
                           d_ts, d_vals, d_units, d_counts, d_errs, nreplicas,
                           nblocks, nseries, stride, start_ns, end_ns,
                           strategy, d_out_ts, d_out_vals, d_out_units,
                           d_out_counts, d_out_errs, out_stride);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

/* argument rules of the four step-consolidation forms; touches no HIP state.
 * `rows` is stride (row forms) or nblocks (stream forms). */
static int step_check_args(uint32_t nseries, uint32_t rows,
                           const char* rows_name, int64_t start_ns,
                           int64_t step_ns, uint32_t nsteps,
                           int64_t lookback_ns, uint32_t out_pitch) {
    if (step_ns <= 0 || lookback_ns < 0 || !nsteps) {
        snprintf(g_err, sizeof(g_err),
                 "step_ns must be > 0, lookback_ns >= 0 and nsteps nonzero");
        return M3GPU_ERR_BADARG;
    }
    if (!rows) {
        snprintf(g_err, sizeof(g_err), "%s must be nonzero", rows_name);
        return M3GPU_ERR_BADARG;
    }
    if (out_pitch < nseries) {
        snprintf(g_err, sizeof(g_err), "out_pitch must be >= nseries");
        return M3GPU_ERR_BADARG;
    }
    int64_t span, t_last, lo;
    if (__builtin_mul_overflow((int64_t)(nsteps - 1), step_ns, &span) ||
        __builtin_add_overflow(start_ns, span, &t_last) ||
        __builtin_sub_overflow(start_ns, lookback_ns, &lo)) {
        snprintf(g_err, sizeof(g_err),
                 "the step grid or start_ns - lookback_ns overflows int64");
        return M3GPU_ERR_BADARG;
    }
    return M3GPU_OK;
}

int m3gpu_step_consolidate_batch_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    const int32_t* d_errs, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t lookback_ns,
    double* d_out, uint32_t out_pitch, int32_t* d_out_errs,
    void* hip_stream) {
    int rc = step_check_args(nseries, stride, "stride", start_ns, step_ns,
                             nsteps, lookback_ns, out_pitch);
    if (rc != M3GPU_OK) return rc;
    if (!nseries) return M3GPU_OK;
    const m3::StepGrid g = {start_ns, step_ns, lookback_ns, nsteps};
    hipLaunchKernelGGL(m3::k_step_rows, dim3(grid_lane(nseries)),
                       dim3(BLOCK_THREADS), 0, (hipStream_t)hip_stream,
                       d_ts, d_vals, d_counts, d_errs, nseries, stride, g,
                       d_out, out_pitch, d_out_errs);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

int m3gpu_decode_steps_batch_dev(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, uint32_t nblocks, int int_optimized,
    uint8_t default_unit, int64_t start_ns, int64_t step_ns, uint32_t nsteps,
    int64_t lookback_ns, double* d_out, uint32_t out_pitch,
    int32_t* d_out_errs, void* hip_stream) {
    int rc = step_check_args(nseries, nblocks, "nblocks", start_ns, step_ns,
                             nsteps, lookback_ns, out_pitch);
    if (rc != M3GPU_OK) return rc;
    if (!nseries) return M3GPU_OK;
    const m3::StepGrid g = {start_ns, step_ns, lookback_ns, nsteps};
    hipLaunchKernelGGL(m3::k_step_fused, dim3(grid_lane(nseries)),
                       dim3(BLOCK_THREADS), 0, (hipStream_t)hip_stream,
                       d_blobs, d_offsets, d_lens, nseries, nblocks,
                       int_optimized, default_unit, g, d_out, out_pitch,
                       d_out_errs);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

/* ---------- host-pointer convenience forms (the cgo surface) ---------- */

/* the dense device matrix [nsteps, nseries] into out's rows of out_pitch:
 * the cells between nseries and out_pitch stay as the caller left them */
static int step_download(const DevBuf<double>& d_out,
                         const DevBuf<int32_t>& d_errs, uint32_t nseries,
                         uint32_t nsteps, double* out, uint32_t out_pitch,
                         int32_t* out_errs) {
    HIP_TRY(hipMemcpy2D(out, (size_t)out_pitch * sizeof(double), d_out.p,
                        (size_t)nseries * sizeof(double),
                        (size_t)nseries * sizeof(double), nsteps,
                        hipMemcpyDeviceToHost));
    HIP_TRY(d_errs.download(out_errs, nseries));
    return M3GPU_OK;
}

int m3gpu_step_consolidate_batch(
    const int64_t* ts, const double* vals, const uint32_t* counts,
    const int32_t* errs, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t lookback_ns,
    double* out, uint32_t out_pitch, int32_t* out_errs) {
    int rc = step_check_args(nseries, stride, "stride", start_ns, step_ns,
                             nsteps, lookback_ns, out_pitch);
    if (rc != M3GPU_OK) return rc;
    if (!nseries) return M3GPU_OK;
    DevBuf<int64_t> d_ts;
    DevBuf<double> d_vals, d_out;
    DevBuf<uint32_t> d_counts;
    DevBuf<int32_t> d_errs, d_out_errs;
    const uint64_t npts = (uint64_t)nseries * stride;
    HIP_TRY(d_ts.upload(ts, npts));
    HIP_TRY(d_vals.upload(vals, npts));
    HIP_TRY(d_counts.upload(counts, nseries));
    if (errs) HIP_TRY(d_errs.upload(errs, nseries));
    HIP_TRY(d_out.alloc((uint64_t)nsteps * nseries));
    HIP_TRY(d_out_errs.alloc(nseries));
    rc = m3gpu_step_consolidate_batch_dev(
        d_ts.p, d_vals.p, d_counts.p, d_errs.p, nseries, stride, start_ns,
        step_ns, nsteps, lookback_ns, d_out.p, nseries, d_out_errs.p, nullptr);
    if (rc != M3GPU_OK) return rc;
    return step_download(d_out, d_out_errs, nseries, nsteps, out, out_pitch,
                         out_errs);
}

int m3gpu_decode_steps_batch(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, uint32_t nblocks, int int_optimized,
    uint8_t default_unit, int64_t start_ns, int64_t step_ns, uint32_t nsteps,
    int64_t lookback_ns, double* out, uint32_t out_pitch, int32_t* out_errs) {
    int rc = step_check_args(nseries, nblocks, "nblocks", start_ns, step_ns,
                             nsteps, lookback_ns, out_pitch);
    if (rc != M3GPU_OK) return rc;
    if (!nseries) return M3GPU_OK;
    if ((uint64_t)nseries * nblocks > UINT32_MAX) {
        snprintf(g_err, sizeof(g_err), "nseries * nblocks must fit 32 bits");
        return M3GPU_ERR_BADARG;
    }
    DevStreams in;
    DevBuf<double> d_out;
    DevBuf<int32_t> d_out_errs;
    HIP_TRY(in.upload(blobs, blobs_len, offsets, lens, nseries * nblocks));
    HIP_TRY(d_out.alloc((uint64_t)nsteps * nseries));
    HIP_TRY(d_out_errs.alloc(nseries));
    rc = m3gpu_decode_steps_batch_dev(
        in.blobs.p, in.offsets.p, in.lens.p, nseries, nblocks, int_optimized,
        default_unit, start_ns, step_ns, nsteps, lookback_ns, d_out.p,
        nseries, d_out_errs.p, nullptr);
    if (rc != M3GPU_OK) return rc;
    return step_download(d_out, d_out_errs, nseries, nsteps, out, out_pitch,
                         out_errs);
}

int m3gpu_series_merge_batch(
    const int64_t* ts, const double* vals, const uint8_t* units,
    const uint32_t* counts, const int32_t* errs,
    uint32_t nreplicas, uint32_t nblocks, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t end_ns, int strategy,
    int64_t* out_ts, double* out_vals, uint8_t* out_units,
    uint32_t* out_counts, int32_t* out_errs, uint32_t out_stride) {
    int rc = series_merge_check_args(nreplicas, nblocks, stride, out_stride,
                                     strategy, units != nullptr,
                                     out_units != nullptr);
    if (rc != M3GPU_OK) return rc;
    if (!nseries) return M3GPU_OK;
    DevBuf<int64_t> d_ts, d_out_ts;
    DevBuf<double> d_vals, d_out_vals;
    DevBuf<uint8_t> d_units, d_out_units;
    DevBuf<uint32_t> d_counts, d_out_counts;
    DevBuf<int32_t> d_errs, d_out_errs;
    const uint64_t nrows = (uint64_t)nreplicas * nblocks * nseries;
    const uint64_t npts = nrows * stride;
    const uint64_t out_pts = (uint64_t)nseries * out_stride;
    HIP_TRY(d_ts.upload(ts, npts));
    HIP_TRY(d_vals.upload(vals, npts));
    HIP_TRY(d_counts.upload(counts, nrows));
    if (errs) HIP_TRY(d_errs.upload(errs, nrows));
    HIP_TRY(d_out_ts.alloc(out_pts));
    HIP_TRY(d_out_vals.alloc(out_pts));
    HIP_TRY(d_out_counts.alloc(nseries));
    HIP_TRY(d_out_errs.alloc(nseries));
    if (units) {
        HIP_TRY(d_units.upload(units, npts));
        /* the kernel writes only merged points: the rest comes back 0 */
        HIP_TRY(d_out_units.alloc(out_pts));
        HIP_TRY(hipMemset(d_out_units.p, 0, out_pts));
    }
    rc = m3gpu_series_merge_batch_dev(
        d_ts.p, d_vals.p, d_units.p, d_counts.p, d_errs.p, nreplicas, nblocks,
        nseries, stride, start_ns, end_ns, strategy, d_out_ts.p, d_out_vals.p,
        d_out_units.p, d_out_counts.p, d_out_errs.p, out_stride, nullptr);
    if (rc != M3GPU_OK) return rc;
    HIP_TRY(d_out_ts.download(out_ts, out_pts));
    HIP_TRY(d_out_vals.download(out_vals, out_pts));
    HIP_TRY(d_out_counts.download(out_counts, nseries));
    HIP_TRY(d_out_errs.download(out_errs, nseries));
    if (units) HIP_TRY(d_out_units.download(out_units, out_pts));
    return M3GPU_OK;
}

/* Both decode forms: upload the streams, decode on the null stream, copy
 * the results back. with_ann selects the annotation-capturing entry. */
static int decode_host(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* out_ts, double* out_vals, uint32_t* out_counts,
    int32_t* out_errs, uint32_t stride,
    bool with_ann, uint8_t* out_ann, uint32_t ann_stride) {
    DevStreams in;
    DevBuf<int64_t> d_ts;
    DevBuf<double> d_vals;
    DevBuf<uint32_t> d_counts;
    DevBuf<int32_t> d_errs;
    DevBuf<uint8_t> d_ann;
    uint64_t npts = (uint64_t)nseries * stride;
    uint64_t ann_total = (uint64_t)nseries * ann_stride;
    HIP_TRY(in.upload(blobs, blobs_len, offsets, lens, nseries));
    HIP_TRY(d_ts.alloc(npts));
    HIP_TRY(d_vals.alloc(npts));
    HIP_TRY(d_counts.alloc(nseries));
    HIP_TRY(d_errs.alloc(nseries));
    int rc;
    if (with_ann) {
        HIP_TRY(d_ann.alloc(ann_total));
        HIP_TRY(hipMemset(d_ann.p, 0, ann_total));
        rc = m3gpu_decode_batch_dev_ann(
            in.blobs.p, in.offsets.p, in.lens.p, nseries, int_optimized,
            default_unit, d_ts.p, d_vals.p, d_counts.p, d_errs.p, stride,
            d_ann.p, ann_stride, nullptr);
    } else {
        rc = m3gpu_decode_batch_dev(
            in.blobs.p, in.offsets.p, in.lens.p, nseries, int_optimized,
            default_unit, d_ts.p, d_vals.p, d_counts.p, d_errs.p, stride,
            nullptr);
    }
    if (rc != M3GPU_OK) return rc;
    HIP_TRY(d_ts.download(out_ts, npts));
    HIP_TRY(d_vals.download(out_vals, npts));
    HIP_TRY(d_counts.download(out_counts, nseries));
    HIP_TRY(d_errs.download(out_errs, nseries));
    if (with_ann) HIP_TRY(d_ann.download(out_ann, ann_total));
    return M3GPU_OK;
}

int m3gpu_decode_batch(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* out_ts, double* out_vals, uint32_t* out_counts,
    int32_t* out_errs, uint32_t stride) {
    return decode_host(blobs, blobs_len, offsets, lens, nseries,
                       int_optimized, default_unit, out_ts, out_vals,
                       out_counts, out_errs, stride, false, nullptr, 0);
}

/* what a cgo ReaderIterator shim calls for annotation-bearing blocks */
int m3gpu_decode_batch_ann(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* out_ts, double* out_vals, uint32_t* out_counts,
    int32_t* out_errs, uint32_t stride,
    uint8_t* out_ann, uint32_t ann_stride) {
    return decode_host(blobs, blobs_len, offsets, lens, nseries,
                       int_optimized, default_unit, out_ts, out_vals,
                       out_counts, out_errs, stride, true, out_ann,
                       ann_stride);
}

/* what a cgo ReaderIterator shim calls when Current()'s unit and the block
 * start are wanted too; each optional output that is NULL is skipped */
int m3gpu_decode_batch_full(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* out_ts, double* out_vals, uint32_t* out_counts,
    int32_t* out_errs, uint32_t stride,
    uint8_t* out_units, int64_t* out_start_ns,
    uint8_t* out_ann, uint32_t ann_stride) {
    if (!nseries) return M3GPU_OK;
    int rc = decode_full_check_args(out_ann != nullptr, ann_stride);
    if (rc != M3GPU_OK) return rc;
    DevStreams in;
    DevBuf<int64_t> d_ts, d_start;
    DevBuf<double> d_vals;
    DevBuf<uint32_t> d_counts;
    DevBuf<int32_t> d_errs;
    DevBuf<uint8_t> d_units, d_ann;
    uint64_t npts = (uint64_t)nseries * stride;
    uint64_t ann_total = (uint64_t)nseries * ann_stride;
    HIP_TRY(in.upload(blobs, blobs_len, offsets, lens, nseries));
    HIP_TRY(d_ts.alloc(npts));
    HIP_TRY(d_vals.alloc(npts));
    HIP_TRY(d_counts.alloc(nseries));
    HIP_TRY(d_errs.alloc(nseries));
    if (out_units) {
        /* the kernel writes only decoded points: the rest comes back 0 */
        HIP_TRY(d_units.alloc(npts));
        HIP_TRY(hipMemset(d_units.p, 0, npts));
    }
    if (out_start_ns) HIP_TRY(d_start.alloc(nseries));
    if (out_ann) {
        HIP_TRY(d_ann.alloc(ann_total));
        HIP_TRY(hipMemset(d_ann.p, 0, ann_total));
    }
    rc = m3gpu_decode_batch_full_dev(
        in.blobs.p, in.offsets.p, in.lens.p, nullptr, nseries, int_optimized,
        default_unit, d_ts.p, d_vals.p, d_counts.p, d_errs.p, stride,
        d_units.p, d_start.p, d_ann.p, ann_stride, nullptr);
    if (rc != M3GPU_OK) return rc;
    HIP_TRY(d_ts.download(out_ts, npts));
    HIP_TRY(d_vals.download(out_vals, npts));
    HIP_TRY(d_counts.download(out_counts, nseries));
    HIP_TRY(d_errs.download(out_errs, nseries));
    if (out_units) HIP_TRY(d_units.download(out_units, npts));
    if (out_start_ns) HIP_TRY(d_start.download(out_start_ns, nseries));
    if (out_ann) HIP_TRY(d_ann.download(out_ann, ann_total));
    return M3GPU_OK;
}

/* Both encode forms: upload the points (and, for the full form, whichever
 * optional inputs are given), encode on the null stream, copy the streams
 * back. */
static int encode_host(
    const int64_t* ts, const double* vals, const uint32_t* counts,
    bool full, const uint8_t* units, const int64_t* start_ns,
    const uint8_t* ann, uint32_t ann_stride,
    uint32_t nseries, uint32_t stride, int int_optimized, uint8_t unit,
    uint8_t* out_bytes, uint32_t out_stride, uint32_t* out_lens,
    int32_t* out_errs) {
    DevBuf<int64_t> d_ts, d_start;
    DevBuf<double> d_vals;
    DevBuf<uint32_t> d_counts, d_lens;
    DevBuf<uint8_t> d_out, d_units, d_ann;
    DevBuf<int32_t> d_errs;
    uint64_t npts = (uint64_t)nseries * stride;
    uint64_t outb = (uint64_t)nseries * out_stride;
    HIP_TRY(d_ts.upload(ts, npts));
    HIP_TRY(d_vals.upload(vals, npts));
    HIP_TRY(d_counts.upload(counts, nseries));
    if (units) HIP_TRY(d_units.upload(units, npts));
    if (start_ns) HIP_TRY(d_start.upload(start_ns, nseries));
    if (ann) HIP_TRY(d_ann.upload(ann, (uint64_t)nseries * ann_stride));
    HIP_TRY(d_out.alloc(outb));
    HIP_TRY(hipMemset(d_out.p, 0, outb));
    HIP_TRY(d_lens.alloc(nseries));
    HIP_TRY(d_errs.alloc(nseries));
    int rc = full
        ? m3gpu_encode_batch_full_dev(d_ts.p, d_vals.p, d_counts.p, d_units.p,
                                      d_start.p, d_ann.p, ann_stride, nseries,
                                      stride, int_optimized, unit, d_out.p,
                                      out_stride, d_lens.p, d_errs.p, nullptr)
        : m3gpu_encode_batch_dev(d_ts.p, d_vals.p, d_counts.p, nseries,
                                 stride, int_optimized, unit, d_out.p,
                                 out_stride, d_lens.p, d_errs.p, nullptr);
    if (rc != M3GPU_OK) return rc;
    HIP_TRY(d_out.download(out_bytes, outb));
    HIP_TRY(d_lens.download(out_lens, nseries));
    HIP_TRY(d_errs.download(out_errs, nseries));
    return M3GPU_OK;
}

int m3gpu_encode_batch(
    const int64_t* ts, const double* vals, const uint32_t* counts,
    uint32_t nseries, uint32_t stride, int int_optimized, uint8_t unit,
    uint8_t* out_bytes, uint32_t out_stride, uint32_t* out_lens,
    int32_t* out_errs) {
    return encode_host(ts, vals, counts, false, nullptr, nullptr, nullptr, 0,
                       nseries, stride, int_optimized, unit, out_bytes,
                       out_stride, out_lens, out_errs);
}

/* what a cgo encoding.Encoder shim calls for batched Encode(dp, tu, ant) */
int m3gpu_encode_batch_full(
    const int64_t* ts, const double* vals, const uint32_t* counts,
    const uint8_t* units, const int64_t* start_ns,
    const uint8_t* ann, uint32_t ann_stride,
    uint32_t nseries, uint32_t stride, int int_optimized, uint8_t default_unit,
    uint8_t* out_bytes, uint32_t out_stride, uint32_t* out_lens,
    int32_t* out_errs) {
    int rc = encode_full_check_args(ann != nullptr, ann_stride, out_stride);
    if (rc != M3GPU_OK) return rc;
    return encode_host(ts, vals, counts, true, units, start_ns, ann,
                       ann_stride, nseries, stride, int_optimized,
                       default_unit, out_bytes, out_stride, out_lens,
                       out_errs);
}

int m3gpu_rollup_batch(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int metric_type, int64_t window_ns, uint32_t nbuckets,
    const int32_t* agg_types, int naggs,
    double* out, int64_t* out_window_ts, int32_t* out_errs) {
    DevStreams in;
    DevBuf<double> d_out;
    DevBuf<int64_t> d_wts;
    DevBuf<int32_t> d_errs;
    uint64_t nwin = (uint64_t)nseries * nbuckets;
    uint64_t nout = nwin * naggs;
    HIP_TRY(in.upload(blobs, blobs_len, offsets, lens, nseries));
    HIP_TRY(d_out.alloc(nout));
    HIP_TRY(d_wts.alloc(nwin));
    HIP_TRY(d_errs.alloc(nseries));
    int rc = m3gpu_rollup_batch_dev(in.blobs.p, in.offsets.p, in.lens.p,
                                    nseries, int_optimized, default_unit,
                                    metric_type, window_ns, nbuckets,
                                    agg_types, naggs, d_out.p, d_wts.p,
                                    d_errs.p, nullptr);
    if (rc != M3GPU_OK) return rc;
    HIP_TRY(d_out.download(out, nout));
    if (out_window_ts) HIP_TRY(d_wts.download(out_window_ts, nwin));
    HIP_TRY(d_errs.download(out_errs, nseries));
    return M3GPU_OK;
}

} /* extern "C" */
