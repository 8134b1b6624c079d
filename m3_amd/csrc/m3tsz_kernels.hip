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
 *      rollup: the lane tier keeps per-bucket state in registers and small
 *        quantile buckets in a per-lane sorted LDS row; deep buckets retry
 *        on the wave-per-series tiers (k_rollup_batch, k_rollup_ckms), which
 *        run ONE series per wavefront with a wave-uniform parser and
 *        reproduce the reference CKMS walk exactly.
 *  - Streams are decoded from 8-byte-aligned offsets, zero-padded to an
 *    8-byte boundary (layout contract in m3gpu.h; pack_streams emits 64B
 *    alignment, which satisfies it) so every refill is an aligned u64 load.
 *  - Wave64 only; no CUDA shims, no hipified code.
 *
 * The device code is one header per kernel family; each includes what it
 * uses, so their order here does not matter. This file is the one
 * translation unit they are compiled in, and the host layer that launches
 * them:
 *
 *   m3tsz_common.h    block shape, format constants, bit and float helpers
 *   m3tsz_decoder.h   BitReader (direct / LDS ring), DecoderT, RF_SPAN
 *   out_tile.h        output stores and their cache policy (OUT_POLICY,
 *                     FLUSH_WIDE), the tile swizzle, the transposed tile flush
 *   decode_kernel.h   k_decode_batch<FULL> and its ring / top-up knobs
 *   encode_kernel.h   BitWriter, Encoder, xxh64, k_encode_batch<FULL>;
 *                     k_regather, k_compact
 *   merge_kernels.h   k_merge<UNITS>, k_series_merge<UNITS>
 *   step_kernels.h    k_step_rows, k_step_fused
 *   temporal_kernels.h k_temporal_rows<FAMILY, C>: the window functions of
 *                     query/functions/temporal over the same rows and tile
 *   rollup_kernels.h  k_rollup_lane, k_rollup_batch, k_rollup_ckms, over
 *                     rollup_bucket.h (bucket walk, accumulate, ValueOf) and
 *                     rollup_plan.h (plan + exact-quantile index), both
 *                     host-compilable
 *
 * Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (bit-exact f64:
 * convertToIntFloat m3tsz.go:78-119, decode accumulation iterator.go:168-175).
 */
#include <hip/hip_runtime.h>
#include <atomic>
#include <math.h>
#include <string.h>
#include <stdio.h>
#include "../../include/m3gpu.h"
#include "rollup_plan.h" /* QCAP, MAX_AGGS, m3::RollupPlan + its host builder */
#include "decode_kernel.h"
#include "encode_kernel.h"
#include "merge_kernels.h"
#include "step_kernels.h"
#include "temporal_kernels.h"
#include "rollup_kernels.h"

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

/* argument rules of both temporal forms; touches no HIP state */
static int temporal_check_args(uint32_t nseries, uint32_t stride,
                               int64_t start_ns, int64_t step_ns,
                               uint32_t nsteps, int64_t range_ns, int fn,
                               uint32_t out_pitch) {
    if (range_ns <= 0) {
        snprintf(g_err, sizeof(g_err), "range_ns must be > 0");
        return M3GPU_ERR_BADARG;
    }
    if (fn < 0 || fn >= M3GPU_TEMPORAL_FN_COUNT) {
        snprintf(g_err, sizeof(g_err), "fn must be 0..%d",
                 M3GPU_TEMPORAL_FN_COUNT - 1);
        return M3GPU_ERR_BADARG;
    }
    int64_t lo;
    if (__builtin_sub_overflow(start_ns, range_ns, &lo)) {
        snprintf(g_err, sizeof(g_err), "start_ns - range_ns overflows int64");
        return M3GPU_ERR_BADARG;
    }
    return step_check_args(nseries, stride, "stride", start_ns, step_ns,
                           nsteps, range_ns, out_pitch);
}

/* the family whose accumulator fn uses */
static int temporal_family(int fn) {
    switch (fn) {
    case M3GPU_TEMPORAL_MIN: case M3GPU_TEMPORAL_MAX: return m3::TF_MINMAX;
    case M3GPU_TEMPORAL_STDDEV: case M3GPU_TEMPORAL_STDVAR:
        return m3::TF_WELFORD;
    case M3GPU_TEMPORAL_RATE: case M3GPU_TEMPORAL_INCREASE:
    case M3GPU_TEMPORAL_DELTA: return m3::TF_RATE;
    case M3GPU_TEMPORAL_IRATE: case M3GPU_TEMPORAL_IDELTA: return m3::TF_IRATE;
    case M3GPU_TEMPORAL_RESETS: case M3GPU_TEMPORAL_CHANGES:
        return m3::TF_CHANGES;
    case M3GPU_TEMPORAL_DERIV: case M3GPU_TEMPORAL_PREDICT_LINEAR:
        return m3::TF_REGR;
    default: return m3::TF_SUM; /* sum, count, avg, last */
    }
}

int m3gpu_temporal_batch_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    const int32_t* d_errs, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t range_ns,
    int fn, double param, double* d_out, uint32_t out_pitch,
    int32_t* d_out_errs, void* hip_stream) {
    int rc = temporal_check_args(nseries, stride, start_ns, step_ns, nsteps,
                                 range_ns, fn, out_pitch);
    if (rc != M3GPU_OK) return rc;
    if (!nseries) return M3GPU_OK;
    const m3::StepGrid g = {start_ns, step_ns, range_ns, nsteps};
    decltype(&m3::k_temporal_rows<m3::TF_SUM, TEMPORAL_RING>) kern;
    switch (temporal_family(fn)) {
    case m3::TF_MINMAX:
        kern = m3::k_temporal_rows<m3::TF_MINMAX, TEMPORAL_RING>; break;
    case m3::TF_WELFORD:
        kern = m3::k_temporal_rows<m3::TF_WELFORD, TEMPORAL_RING>; break;
    case m3::TF_RATE:
        kern = m3::k_temporal_rows<m3::TF_RATE, TEMPORAL_RING>; break;
    case m3::TF_IRATE:
        kern = m3::k_temporal_rows<m3::TF_IRATE, TEMPORAL_RING>; break;
    case m3::TF_CHANGES:
        kern = m3::k_temporal_rows<m3::TF_CHANGES, TEMPORAL_RING>; break;
    case m3::TF_REGR:
        kern = m3::k_temporal_rows<m3::TF_REGR, TEMPORAL_RING>; break;
    default:
        kern = m3::k_temporal_rows<m3::TF_SUM, TEMPORAL_RING>; break;
    }
    hipLaunchKernelGGL(kern, dim3(grid_lane(nseries)), dim3(BLOCK_THREADS), 0,
                       (hipStream_t)hip_stream,
                       d_ts, d_vals, d_counts, d_errs, nseries, stride, g, fn,
                       param, d_out, out_pitch, d_out_errs);
    HIP_TRY(hipGetLastError());
    return M3GPU_OK;
}

/* the ring depth this library was built with (TEMPORAL_RING), for tests that
 * size their windows around it */
int m3gpu_temporal_ring_depth(void) { return TEMPORAL_RING; }

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

int m3gpu_temporal_batch(
    const int64_t* ts, const double* vals, const uint32_t* counts,
    const int32_t* errs, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t range_ns,
    int fn, double param, double* out, uint32_t out_pitch,
    int32_t* out_errs) {
    int rc = temporal_check_args(nseries, stride, start_ns, step_ns, nsteps,
                                 range_ns, fn, out_pitch);
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
    rc = m3gpu_temporal_batch_dev(
        d_ts.p, d_vals.p, d_counts.p, d_errs.p, nseries, stride, start_ns,
        step_ns, nsteps, range_ns, fn, param, d_out.p, nseries, d_out_errs.p,
        nullptr);
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
