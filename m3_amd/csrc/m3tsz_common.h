/*
 * m3tsz_common.h — what every M3TSZ kernel family shares: the block shape
 * (WAVE, WAVES_PER_BLOCK), the format's constants and the small bit and
 * float helpers of both the decoder and the encoder. Device code.
 */
#ifndef M3_M3TSZ_COMMON_H
#define M3_M3TSZ_COMMON_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

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
/* 10^m for m in [0,6] as a pure VALU select chain, NOT an indexed array: a
 * dynamically-indexed local const table lowers to a .rodata global_load
 * whose vmcnt(0) wait (gfx9 vmcnt counts stores too) drains every in-flight
 * output store right in the per-point value chain */
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

} // namespace m3

#endif /* M3_M3TSZ_COMMON_H */
