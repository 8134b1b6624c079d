/*
 * m3tsz_decoder.h — the device bit reader (direct, or through a per-lane LDS
 * word ring) and the M3TSZ decode state machine over it. Every kernel that
 * reads streams is built on these: k_decode_batch (decode_kernel.h),
 * k_step_fused (step_kernels.h) and the rollup tiers (rollup_kernels.h).
 * RF_SPAN, the ring top-up span the series-per-lane kernels share, is at
 * the end.
 */
#ifndef M3_M3TSZ_DECODER_H
#define M3_M3TSZ_DECODER_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/m3gpu.h" /* M3GPU_SERIES_* */
#include "m3tsz_common.h"

namespace m3 {

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
};

using Decoder = DecoderT<0>;             /* wave-per-series kernels: direct reader */
using RingDecoder = DecoderT<IN_WORDS>;  /* series-per-lane kernels: 4-word LDS ring */

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

} // namespace m3

#endif /* M3_M3TSZ_DECODER_H */
