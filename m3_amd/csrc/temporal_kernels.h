/*
 * temporal_kernels.h — the batched temporal functions (range vectors):
 * k_temporal_rows<FAMILY, C> over decoded rows, one window function per step
 * and series.
 */
#ifndef M3_TEMPORAL_KERNELS_H
#define M3_TEMPORAL_KERNELS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/m3gpu.h"
#include "step_kernels.h" /* StepGrid, STEP_TILE, step_flush, step_fail_column */

namespace m3 {

/* ====================== batched temporal functions ======================
 * What the temporal baseNode computes for every series of a block
 * (query/functions/temporal/base.go:255-306 with getIndices, :432-482): on
 * the grid t_k = start + k*step the cell (k, i) is f(W_k), W_k the row's
 * points with t_k - range <= ts <= t_k in row order, NaN points included,
 * and f one of the package's processors, restated below operation for
 * operation: the sums run left to right over the window, so a window is
 * re-walked for every step and never slid.
 *
 * One series per lane, as in k_step_rows, and the same output: the wave
 * fills the LDS tile [STEP_TILE][64] and stores every step row as one
 * 512-byte run. A lane keeps three indices into its row: `nread`, the points
 * read and order-checked so far (up to and including the first point past
 * the step in hand); `r`, the first point past t_k; and `l`, the window's
 * left end, carried from step to step like getIndices' init.
 *
 * Input: the head of every row advances through the cooperative refill of
 * k_step_rows (4 lanes to a row's 64 bytes per array, 8 lanes of 8 bytes for
 * odd strides and unaligned arrays), which here feeds a ring of the row's
 * most recent C points in LDS instead of a single chunk. Windows of
 * neighbouring steps overlap, so a point is read range/step times; a window
 * point whose index is still in the ring comes from LDS, an older one from
 * global memory, so windows longer than C stay correct and slow down by
 * degrees. The ring row of lane l holds point p at word
 * l*C + (p ^ swz(l)) % C: with swz(l) = l*C/32 the 32 lanes of a half wave
 * that read the same p touch 32 different 8-byte columns of the 256-byte
 * bank row, with no padding, so at C = 16 a block is 64 KB of ring and 16 KB
 * of tile and two blocks share a CU's 160 KB.
 *
 * fn is launch-uniform: the kernel is instantiated per family of functions
 * that share an accumulator, and the function inside a family is a
 * wave-uniform branch. No fma, no fast division: the translation unit is
 * compiled with -ffp-contract=off. */
#ifndef TEMPORAL_RING
#define TEMPORAL_RING 16
#endif
/* 1: window points always come from global memory (the measurement of what
 * the ring buys); the head still advances through the ring */
#ifndef TEMPORAL_RING_BYPASS
#define TEMPORAL_RING_BYPASS 0
#endif
#define TEMPORAL_CHUNK 8 /* points a refill loads per row */

enum { TF_SUM = 0, TF_MINMAX, TF_WELFORD, TF_RATE, TF_IRATE, TF_CHANGES,
       TF_REGR };

__device__ __forceinline__ uint64_t t_bits(double v) {
    return (uint64_t)__double_as_longlong(v);
}

/* time.Duration.Seconds(): whole seconds plus the rest, two conversions */
__device__ __forceinline__ double t_dur_seconds(int64_t d) {
    const int64_t sec = d / 1000000000LL;
    const int64_t nsec = d % 1000000000LL;
    return (double)sec + (double)nsec / 1e9;
}

/* subSeconds (linear_regression.go:140-142): one conversion, one division */
__device__ __forceinline__ double t_sub_seconds(int64_t a, int64_t b) {
    return (double)(a - b) / 1e9;
}

/* Go's math.Min / math.Max for operands that are not NaN: a device fmin
 * does not promise Min(0, -0) = -0 */
__device__ __forceinline__ double t_go_min(double x, double y) {
    if (x == 0.0 && x == y) return signbit(x) ? x : y;
    return x < y ? x : y;
}
__device__ __forceinline__ double t_go_max(double x, double y) {
    if (x == 0.0 && x == y) return signbit(x) ? y : x;
    return x > y ? x : y;
}

/* f(W) for the window [l, r) of one row at step time tk; the value's bits.
 * Where the reference returns math.NaN(), and where it only passes that NaN
 * through an operation (avg's NaN/0, stddev's sqrt, predict_linear's
 * NaN*d + NaN), the cell holds STEP_NAN_BITS. */
template <int FAM, typename TsAt, typename ValAt>
__device__ __forceinline__ uint64_t temporal_window(
        int fn, uint32_t l, uint32_t r, int64_t tk, int64_t range_ns,
        double param, TsAt ts_at, ValAt val_at) {
    if (FAM == TF_SUM) { /* aggregation.go:151-163, :199-202, :227-251 */
        if (fn == M3GPU_TEMPORAL_LAST)
            return l < r ? t_bits(val_at(r - 1)) : STEP_NAN_BITS;
        double sum = 0.0, count = 0.0;
        for (uint32_t i = l; i < r; i++) {
            const double v = val_at(i);
            if (v == v) {
                sum += v;
                count += 1.0;
            }
        }
        if (count == 0.0) return STEP_NAN_BITS;
        if (fn == M3GPU_TEMPORAL_SUM) return t_bits(sum);
        if (fn == M3GPU_TEMPORAL_COUNT) return t_bits(count);
        return t_bits(sum / count);
    }
    if (FAM == TF_MINMAX) { /* aggregation.go:165-197 */
        const bool is_min = fn == M3GPU_TEMPORAL_MIN;
        bool seen = false;
        double m = is_min ? INFINITY : -INFINITY;
        for (uint32_t i = l; i < r; i++) {
            const double v = val_at(i);
            if (v == v) {
                seen = true;
                m = is_min ? t_go_min(m, v) : t_go_max(m, v);
            }
        }
        return seen ? t_bits(m) : STEP_NAN_BITS;
    }
    if (FAM == TF_WELFORD) { /* aggregation.go:204-225 */
        double aux = 0.0, count = 0.0, mean = 0.0;
        for (uint32_t i = l; i < r; i++) {
            const double v = val_at(i);
            if (v == v) {
                count += 1.0;
                const double delta = v - mean;
                mean += delta / count;
                aux += delta * (v - mean);
            }
        }
        if (count < 2.0) return STEP_NAN_BITS;
        const double var = aux / count;
        return t_bits(fn == M3GPU_TEMPORAL_STDDEV ? sqrt(var) : var);
    }
    if (FAM == TF_RATE) { /* rate.go:150-240 */
        if (r - l < 2) return STEP_NAN_BITS;
        const bool is_rate = fn == M3GPU_TEMPORAL_RATE;
        const bool is_counter = fn != M3GPU_TEMPORAL_DELTA;
        double correction = 0.0, first_val = 0.0, last_val = 0.0;
        uint32_t first_idx = 0, last_idx = 0;
        int64_t first_ts = 0, last_ts = 0;
        bool found = false;
        for (uint32_t i = l; i < r; i++) {
            const double v = val_at(i);
            if (v != v) continue;
            const int64_t t = ts_at(i);
            if (!found) {
                first_val = v;
                first_ts = t;
                first_idx = i;
                found = true;
            }
            if (is_counter && v < last_val) correction += last_val;
            last_val = v;
            last_ts = t;
            last_idx = i;
        }
        if (first_idx == last_idx) return STEP_NAN_BITS;
        double to_start = t_sub_seconds(first_ts, tk - range_ns);
        const double to_end = t_sub_seconds(tk, last_ts);
        const double sampled = t_sub_seconds(last_ts, first_ts);
        const double avg_gap = sampled / (double)(int32_t)(last_idx - first_idx);
        double result = last_val - first_val + correction;
        if (is_counter && result > 0.0 && first_val >= 0.0) {
            const double to_zero = sampled * (first_val / result);
            if (to_zero < to_start) to_start = to_zero;
        }
        const double threshold = avg_gap * 1.1;
        double extrapolate = sampled;
        if (to_start < threshold) extrapolate += to_start;
        else extrapolate += avg_gap / 2.0;
        if (to_end < threshold) extrapolate += to_end;
        else extrapolate += avg_gap / 2.0;
        result = result * (extrapolate / sampled);
        if (is_rate) result /= t_dur_seconds(range_ns);
        return t_bits(result);
    }
    if (FAM == TF_IRATE) { /* rate.go:242-298 */
        if (r - l < 2) return STEP_NAN_BITS;
        const bool is_rate = fn == M3GPU_TEMPORAL_IRATE;
        uint32_t i = r; /* one past the candidate */
        double last_v = 0.0, prev_v = 0.0;
        bool have_last = false, have_prev = false;
        while (i > l) { /* findNonNanIdx from the window's last point */
            i--;
            last_v = val_at(i);
            if (last_v == last_v) { have_last = true; break; }
        }
        if (!have_last || i == l) return STEP_NAN_BITS;
        const uint32_t i_last = i;
        while (i > l) {
            i--;
            prev_v = val_at(i);
            if (prev_v == prev_v) { have_prev = true; break; }
        }
        if (!have_prev) return STEP_NAN_BITS;
        double result = (is_rate && last_v < prev_v) ? last_v
                                                     : last_v - prev_v;
        if (is_rate) {
            const int64_t interval = ts_at(i_last) - ts_at(i);
            if (interval == 0) return STEP_NAN_BITS;
            result /= t_dur_seconds(interval);
        }
        return t_bits(result);
    }
    if (FAM == TF_CHANGES) { /* functions.go:89-118 */
        if (l >= r) return STEP_NAN_BITS;
        const bool resets = fn == M3GPU_TEMPORAL_RESETS;
        bool all_nan = true;
        double result = 0.0;
        double prev = val_at(l);
        for (uint32_t i = l + 1; i < r; i++) {
            const double cur = val_at(i);
            if (cur != cur) continue;
            all_nan = false;
            if (prev == prev) {
                if (resets ? cur < prev : cur != prev) result += 1.0;
            }
            prev = cur;
        }
        return all_nan ? STEP_NAN_BITS : t_bits(result);
    }
    /* TF_REGR: linear_regression.go:127-191 */
    if (r - l < 2) return STEP_NAN_BITS;
    const bool is_deriv = fn == M3GPU_TEMPORAL_DERIV;
    int64_t intercept_t = tk;
    double n = 0.0, sum_t = 0.0, sum_v = 0.0, sum_tv = 0.0, sum_tt = 0.0;
    uint32_t value_count = 0;
    for (uint32_t i = l; i < r; i++) {
        const double v = val_at(i);
        if (v != v) continue;
        const int64_t t = ts_at(i);
        if (value_count == 0 && is_deriv) intercept_t = t;
        value_count++;
        const double dt = t_sub_seconds(t, intercept_t);
        n += 1.0;
        sum_v += v;
        sum_t += dt;
        sum_tv += dt * v;
        sum_tt += dt * dt;
    }
    if (value_count == 1) return STEP_NAN_BITS;
    const double cov_xy = sum_tv - sum_t * sum_v / n;
    const double var_x = sum_tt - sum_t * sum_t / n;
    const double slope = cov_xy / var_x;
    if (is_deriv) return t_bits(slope);
    const double intercept = sum_v / n - slope * sum_t / n;
    return t_bits(slope * param + intercept);
}

/* Rows in, matrix out; the rows, counts and errs are k_step_rows' inputs.
 * A series fails with its row's error wherever its points lie (the temporal
 * node takes series.Datapoints(), the whole decoded series, before its first
 * window), and with M3GPU_SERIES_OUT_OF_ORDER when a point read, i.e. one up
 * to and including the first past the last step, is at or before its
 * predecessor. Nothing behind that point is read. */
template <int FAM, int C>
__global__ void __launch_bounds__(BLOCK_THREADS)
k_temporal_rows(const int64_t* __restrict__ ts,
                const double* __restrict__ vals,
                const uint32_t* __restrict__ counts,
                const int32_t* __restrict__ errs, uint32_t nseries,
                uint32_t stride, StepGrid g, int fn, double param,
                double* __restrict__ out, uint32_t out_pitch,
                int32_t* __restrict__ out_errs) {
    static_assert(C == 8 || C == 16 || C == 32, "swz covers 8, 16 and 32");
    static_assert(C % TEMPORAL_CHUNK == 0, "whole chunks");
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t series = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    const uint32_t wave_row0 = series - lane;
    const bool in_range = series < nseries;

    __shared__ uint64_t tile_all[WAVES_PER_BLOCK][STEP_TILE][WAVE];
    __shared__ long long ring_t_all[WAVES_PER_BLOCK][WAVE * C];
    __shared__ long long ring_v_all[WAVES_PER_BLOCK][WAVE * C];
    uint64_t* col = &tile_all[wave][0][lane];
    long long* ring_t = ring_t_all[wave];
    long long* ring_v = ring_v_all[wave];
    const long long* gts = (const long long*)ts;
    const long long* gvals = (const long long*)vals;

    /* word of point p in row rr's ring */
    auto ring_at = [](uint32_t rr, uint32_t p) -> uint32_t {
        return rr * C + ((p ^ (rr * C / 32)) & (C - 1));
    };

    /* one decision per launch */
    const bool pair = !(stride & 1) &&
        !(((uintptr_t)ts | (uintptr_t)vals) & 15);

    int err = 0;
    if (in_range && errs) err = errs[series];
    bool active = in_range && !err;
    const uint32_t count = active ? min(counts[series], stride) : 0;
    const uint64_t row = (uint64_t)series * stride; /* used when active */
    uint32_t nread = 0; /* points read and order-checked */
    uint32_t r = 0;     /* points at or before the step in hand; <= nread */
    uint32_t l = 0;     /* the window's left end; <= r */
    uint32_t cend = 0;  /* the ring holds points [cend - C, cend) */
    int64_t prev_t = 0; /* time of point nread - 1 */

    /* rows whose lane asked get their next chunk; points past the count but
     * inside the row's stride are loaded and never read */
    auto refill = [&](bool ask) {
        const uint32_t cbase = nread & ~(uint32_t)(TEMPORAL_CHUNK - 1);
        if (ask) cend = cbase + TEMPORAL_CHUNK;
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
                    const uint32_t w0 = ring_at(rr, pt);
                    const uint32_t w1 = ring_at(rr, pt + 1);
                    ring_t[w0] = a.x;
                    ring_t[w1] = a.y;
                    ring_v[w0] = b.x;
                    ring_v[w1] = b.y;
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
                    const uint32_t w = ring_at(rr, pt);
                    ring_t[w] = gts[at];
                    ring_v[w] = gvals[at];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    };

    /* a window point i < r: from the ring while it is still there */
    auto ts_at = [&](uint32_t i) -> int64_t {
        if (!TEMPORAL_RING_BYPASS && i + C >= cend)
            return ring_t[ring_at(lane, i)];
        return gts[row + i];
    };
    auto val_at = [&](uint32_t i) -> double {
        if (!TEMPORAL_RING_BYPASS && i + C >= cend)
            return __longlong_as_double(ring_v[ring_at(lane, i)]);
        return __longlong_as_double(gvals[row + i]);
    };

    for (uint32_t k0 = 0; k0 < g.nsteps; k0 += STEP_TILE) {
        const uint32_t kend = min(k0 + STEP_TILE, g.nsteps);
        for (uint32_t k = k0; k < kend; k++) {
            const int64_t tk = g.start_ns + (int64_t)k * g.step_ns;
            /* the point read past the previous step may now be inside */
            if (active && nread > r && prev_t <= tk) r = nread;
            bool need = active && nread == r && r < count;
            while (__any(need)) {
                const bool ask = need && nread >= cend;
                if (__any(ask)) refill(ask);
                if (need) {
                    const int64_t t = ring_t[ring_at(lane, nread)];
                    if (nread && t <= prev_t) {
                        err = M3GPU_SERIES_OUT_OF_ORDER;
                        active = false;
                        need = false;
                    } else {
                        prev_t = t;
                        nread++;
                        if (t <= tk) {
                            r = nread;
                            need = r < count;
                        } else {
                            need = false;
                        }
                    }
                }
            }
            uint64_t cell = STEP_NAN_BITS;
            if (active) {
                const int64_t lo = tk - g.lookback_ns;
                while (l < r && ts_at(l) < lo) l++;
                cell = temporal_window<FAM>(fn, l, r, tk, g.lookback_ns,
                                            param, ts_at, val_at);
            }
            col[(k - k0) * WAVE] = cell;
        }
        step_flush(col, k0, kend, in_range, series, out, out_pitch);
    }
    if (in_range) {
        if (err) step_fail_column(g.nsteps, series, out, out_pitch);
        out_errs[series] = err;
    }
}

} // namespace m3

#endif /* M3_TEMPORAL_KERNELS_H */
