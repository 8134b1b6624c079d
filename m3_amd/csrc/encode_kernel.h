/*
 * encode_kernel.h — the device encoder and k_encode_batch, and the two
 * layout kernels that move whole streams: k_regather and k_compact.
 */
#ifndef M3_ENCODE_KERNEL_H
#define M3_ENCODE_KERNEL_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/m3gpu.h"
#include "m3tsz_common.h"
#include "rollup_bucket.h" /* go_f2i */

namespace m3 {

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

/* points per lane in k_encode_batch's LDS input tile: the depth of the
 * decoder's output tile (DEC_TILE, decode_kernel.h), but the encoder's own */
#define ENC_TILE 8

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
    __shared__ int64_t ts_tile_all[WAVES_PER_BLOCK][WAVE][ENC_TILE];
    __shared__ double val_tile_all[WAVES_PER_BLOCK][WAVE][ENC_TILE];
    int64_t (*ts_tile)[ENC_TILE] = ts_tile_all[wave];
    double (*val_tile)[ENC_TILE] = val_tile_all[wave];
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
        const uint32_t p = lane & (ENC_TILE - 1);
        const uint32_t r0 = lane / ENC_TILE;
        for (uint32_t j = 0; j < ENC_TILE; j++) {
            uint32_t r = r0 + j * (WAVE / ENC_TILE);
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
        if ((j & (ENC_TILE - 1)) == 0) {
            fill_tile(j);
            if constexpr (FULL) {
                if (in.units) tile_units = unit_tile[lane];
            }
        }
        if (running) {
            uint32_t col = (j & (ENC_TILE - 1)) ^ (lane & 7);
            int64_t t = ts_tile[lane][col];
            double v = val_tile[lane][col];
            if constexpr (FULL) {
                uint8_t u = in.units
                    ? (uint8_t)(tile_units >> (8 * (j & (ENC_TILE - 1)))) : unit;
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
    /* readfirstlane makes the series index provably wave-uniform: the row
     * addresses and the word count are then scalar (SGPR) values */
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t series = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (series >= nseries) return;
    const uint64_t* s = (const uint64_t*)(src + (uint64_t)series * src_stride);
    uint64_t* d = (uint64_t*)(dst + dst_offsets[series]);
    uint32_t nwords = (lens[series] + 7) / 8;
    for (uint32_t w = lane; w < nwords; w += WAVE) d[w] = s[w];
}

} // namespace m3

#endif /* M3_ENCODE_KERNEL_H */
