/*
 * m3gpu.h — C ABI of the MI355X-native M3TSZ + rollup engine (libm3gpu.so).
 *
 * This is the drop-in boundary for the reference's pluggable codec/rollup
 * hot path. On the Go side the reference injects codec constructors into
 * pools (src/dbnode/storage/options.go:498-510, dbnode/server/server.go:
 * 1786-1793, dbnode/client/options.go:504, query/pools/query_pools.go:208)
 * and creates per-window aggregations via typeSpecificElemBase.NewAggregation
 * (aggregator/aggregator/generic_elem.go:94-95). A cgo wrapper implementing
 * encoding.Encoder / encoding.ReaderIterator (dbnode/encoding/types.go:39-96,
 * :197-203) and the aggregation batch path binds to the entry points below —
 * see INTEGRATION.md for the cgo stubs a maintainer would add.
 *
 * Conventions:
 *  - All functions return 0 on success, a negative M3GPU_ERR_* on failure;
 *    m3gpu_last_error() gives a thread-local message.
 *  - `_dev` entry points take DEVICE pointers and an optional hipStream_t
 *    (as void*); they enqueue async work (caller synchronizes the stream).
 *    Host-pointer convenience forms (no suffix) do alloc+H2D+kernel+D2H
 *    internally and block — these are what a cgo caller uses directly.
 *  - Encoded streams are the reference's on-disk M3TSZ block format
 *    (src/dbnode/encoding/m3tsz, incl. the EOS-marker tail), bit-exact.
 *  - Packed stream layout: blobs[offsets[i] .. offsets[i]+lens[i]) is series
 *    i's stream. The kernels REQUIRE offsets[i] to be 8-byte aligned and
 *    every stream zero-padded to an 8-byte boundary (refills are aligned
 *    u64 loads; the zero pad reproduces reader64's zero-filled tail word).
 *    pack_streams and the fileset/regather packers emit 64-byte
 *    alignment (one HBM line per stream chunk), which satisfies this.
 *    lens[] are true stream lengths.
 *  - Time units use the reference's xtime.Unit byte values
 *    (src/x/time/unit.go:30-42): 1=s, 2=ms, 3=us, 4=ns.
 */
#ifndef M3GPU_H
#define M3GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    M3GPU_OK = 0,
    M3GPU_ERR_HIP = -1,        /* HIP runtime failure (see m3gpu_last_error) */
    M3GPU_ERR_BADARG = -2,     /* invalid argument */
    /* per-series error codes written to out_errs[i] (positive) */
    M3GPU_SERIES_OK = 0,
    M3GPU_SERIES_EOF = 1,          /* truncated stream */
    M3GPU_SERIES_DOD_OVERFLOW = 2, /* timestamp_encoder.go:216-221 */
    M3GPU_SERIES_NO_SCHEME = 3,    /* errNoTimeSchemaForUnit */
    M3GPU_SERIES_INVALID_MULT = 4, /* errInvalidMultiplier */
    M3GPU_SERIES_ANNOTATION = 5,   /* bad annotation */
    M3GPU_SERIES_CAPACITY = 6,     /* stride/out buffer too small */
    M3GPU_SERIES_UNSORTED = 7,     /* rollup input crosses buckets backwards */
    M3GPU_SERIES_BUCKET_OVERFLOW = 8, /* rollup bucket beyond CKMS capacity
                                         (sample list > 3072; unreachable for
                                         the reference-default eps/cadence) */
};

/* metric types for the rollup entry (aggregator/aggregation) */
enum { M3GPU_METRIC_COUNTER = 0, M3GPU_METRIC_GAUGE = 1, M3GPU_METRIC_TIMER = 2 };

/* aggregation type ids — the reference's metrics/aggregation Type enum
 * (src/metrics/aggregation/type.go:31-56) */
enum {
    M3GPU_AGG_LAST = 1, M3GPU_AGG_MIN = 2, M3GPU_AGG_MAX = 3, M3GPU_AGG_MEAN = 4,
    M3GPU_AGG_MEDIAN = 5, M3GPU_AGG_COUNT = 6, M3GPU_AGG_SUM = 7,
    M3GPU_AGG_SUMSQ = 8, M3GPU_AGG_STDEV = 9,
    M3GPU_AGG_P10 = 10, M3GPU_AGG_P20 = 11, M3GPU_AGG_P30 = 12, M3GPU_AGG_P40 = 13,
    M3GPU_AGG_P50 = 14, M3GPU_AGG_P60 = 15, M3GPU_AGG_P70 = 16, M3GPU_AGG_P80 = 17,
    M3GPU_AGG_P90 = 18, M3GPU_AGG_P95 = 19, M3GPU_AGG_P99 = 20,
    M3GPU_AGG_P999 = 21, M3GPU_AGG_P9999 = 22, M3GPU_AGG_P25 = 23, M3GPU_AGG_P75 = 24,
};

int m3gpu_init(int device);
void m3gpu_shutdown(void);
const char* m3gpu_last_error(void);

/* -------- batched decode (replaces m3tsz ReaderIterator bulk reads:
 * src/dbnode/encoding/m3tsz/iterator.go:81-219 over xio.Reader64) --------
 * One series per wavefront. Outputs SoA rows: series i writes
 * out_ts[i*stride .. i*stride+count) and out_vals likewise;
 * out_counts[i] = decoded points; out_errs[i] = M3GPU_SERIES_*. */
int m3gpu_decode_batch_dev(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t stride, void* hip_stream);

/* Scheduling variant: d_perm (device, nseries int32) permutes which stream
 * each lane decodes (outputs still land at the stream's own row). Passing a
 * length-sorted order gives every wavefront 64 similar-cost streams. */
int m3gpu_decode_batch_dev_perm(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    const int32_t* d_perm,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t stride, void* hip_stream);

/* Annotation-capturing variant (materializes Current()'s third return,
 * iterator.go:226-231 / timestamp_iterator.go:327-356): d_out_ann is a
 * per-series region of ann_stride bytes (4-aligned, >= 16) laid out as
 *   [u32 n_events][n_events x {u32 point, u32 off, u32 len}][...bytes]
 * where `point` is the 0-based index of the first datapoint the
 * annotation applies to (sticky until replaced), and off/len locate the
 * bytes within the region (they grow from the tail). A region too small
 * for a series' annotations flags M3GPU_SERIES_CAPACITY on that series. */
int m3gpu_decode_batch_dev_ann(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t stride,
    uint8_t* d_out_ann, uint32_t ann_stride, void* hip_stream);

/* host-pointer convenience form of the annotation-capturing decode */
int m3gpu_decode_batch_ann(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* out_ts, double* out_vals, uint32_t* out_counts,
    int32_t* out_errs, uint32_t stride,
    uint8_t* out_ann, uint32_t ann_stride);

int m3gpu_decode_batch(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* out_ts, double* out_vals, uint32_t* out_counts,
    int32_t* out_errs, uint32_t stride);

/* Full decode: the batched form of ReaderIterator.Current(), which returns
 * (datapoint, unit, annotation) (iterator.go:221-231), plus the block start.
 * Streams, d_perm, points, counts and errs are as in
 * m3gpu_decode_batch_dev_perm; three optional outputs are added, each of
 * which may be NULL (skipped):
 *  - d_out_units [nseries*stride]: d_out_units[i*stride + p] is the time
 *    unit in force after point p of series i was read, the unit Current()
 *    reports with it. Written for exactly the points whose ts/vals are
 *    written (p < d_out_counts[i], hence p < stride); no other byte of the
 *    array is touched. A plain byte array: any base address and any stride,
 *    odd ones included.
 *  - d_out_start_ns [nseries]: the first 64 bits of the stream, the block
 *    start (usually not the first timestamp). 0 for a stream whose first 64
 *    bits cannot be read: an empty one, or one that ends before them.
 *  - d_out_ann: one region of ann_stride bytes per series, written as by
 *    m3gpu_decode_batch_dev_ann (4-byte aligned, ann_stride a multiple of 4
 *    and >= 16). NULL (with ann_stride 0): annotations are skipped.
 * With all three NULL, ts, vals, counts and errs equal
 * m3gpu_decode_batch_dev_perm's.
 * (d_out_ts, d_out_vals, d_out_counts, d_out_units, d_out_start_ns,
 * d_out_ann) can be passed unchanged to m3gpu_encode_batch_full_dev with the
 * same default_unit and int_optimized; for any stream the reference encoder
 * wrote, that reproduces the stream byte for byte.
 * M3GPU_ERR_BADARG, before any work is queued: d_out_ann given with
 * ann_stride % 4 != 0 or ann_stride < 16, or itself not 4-byte aligned;
 * d_out_ann NULL with ann_stride != 0. */
int m3gpu_decode_batch_full_dev(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    const int32_t* d_perm,            /* NULL => identity schedule          */
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t stride,
    uint8_t* d_out_units,             /* [nseries*stride], NULL => skip     */
    int64_t* d_out_start_ns,          /* [nseries], NULL => skip            */
    uint8_t* d_out_ann, uint32_t ann_stride, /* NULL,0 => skip              */
    void* hip_stream);

/* host-pointer convenience form of the full decode. out_units comes back 0
 * past each series' count, out_ann zero-filled outside what was written. */
int m3gpu_decode_batch_full(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int64_t* out_ts, double* out_vals, uint32_t* out_counts,
    int32_t* out_errs, uint32_t stride,
    uint8_t* out_units, int64_t* out_start_ns,
    uint8_t* out_ann, uint32_t ann_stride);

/* -------- batched encode (replaces m3tsz.Encoder bulk writes:
 * src/dbnode/encoding/m3tsz/encoder.go:89-250) --------
 * Series i encodes counts[i] points from ts/vals rows (stride elements per
 * row); start time = first timestamp (as dbnode series buffers do). Output:
 * stream bytes at d_out_bytes + i*out_stride (finalized, EOS tail included),
 * length in out_lens[i]. out_stride must be a multiple of 8 and hold the
 * worst case (~20 B/pt + 16). This is the bulk path: one unit for every
 * point and no annotations. m3gpu_encode_batch_full_dev below takes both. */
int m3gpu_encode_batch_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    uint32_t nseries, uint32_t stride, int int_optimized, uint8_t unit,
    uint8_t* d_out_bytes, uint32_t out_stride, uint32_t* d_out_lens,
    int32_t* d_out_errs, void* hip_stream);

int m3gpu_encode_batch(
    const int64_t* ts, const double* vals, const uint32_t* counts,
    uint32_t nseries, uint32_t stride, int int_optimized, uint8_t unit,
    uint8_t* out_bytes, uint32_t out_stride, uint32_t* out_lens,
    int32_t* out_errs);

/* Full encode: the batched form of Encoder.Encode(dp, tu, ant)
 * (src/dbnode/encoding/m3tsz/encoder.go:90) with the timestamp semantics of
 * timestamp_encoder.go:72-195. Points, counts and outputs are as in
 * m3gpu_encode_batch_dev; three optional inputs are added, each of which may
 * be NULL:
 *  - d_units [nseries*stride]: the unit of every point. A valid unit that
 *    differs from the current one writes the time-unit marker, the unit byte
 *    and a 64-bit nanosecond delta-of-delta. A point whose unit is invalid,
 *    or stays at a unit without a time scheme (5..8), fails its series with
 *    M3GPU_SERIES_NO_SCHEME. NULL: every point uses default_unit.
 *  - d_start_ns [nseries]: the block start. It is what the first 64 bits of
 *    the stream hold, and initialTimeUnit(start, default_unit) is the unit
 *    the stream starts in. NULL: the series' first timestamp.
 *  - d_ann: one region of ann_stride bytes per series (4-byte aligned,
 *    ann_stride a multiple of 4 and >= 16), in the layout
 *    m3gpu_decode_batch_dev_ann writes:
 *      [u32 n_events][n_events x {u32 point, u32 off, u32 len}][...bytes]
 *    so a decoded region can be passed back unchanged. `point` must be
 *    strictly increasing and < counts[i]; off + len must lie inside the
 *    region; len == 0 means no annotation. An annotation is written before
 *    its point iff it is non-empty and its XXH64 differs from that of the
 *    last one written (so a repeated annotation is written once). A region
 *    that breaks a rule fails its series with M3GPU_SERIES_ANNOTATION before
 *    any annotation byte is read. NULL (with ann_stride 0): no annotations.
 * With all three NULL the output equals m3gpu_encode_batch_dev's.
 * Worst-case stream size of a series, which out_stride must hold: the bulk
 * bound (~20 B/pt + 16), plus 11 bits + up to 5 varint bytes + len bytes per
 * annotation written, plus 19 bits + 64 bits per unit change. A series that
 * does not fit fails with M3GPU_SERIES_CAPACITY; other series are unaffected.
 * M3GPU_ERR_BADARG, before any work is queued: out_stride not a multiple of
 * 8; d_ann given with ann_stride % 4 != 0 or ann_stride < 16, or itself not
 * 4-byte aligned; d_ann NULL with ann_stride != 0. */
int m3gpu_encode_batch_full_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    const uint8_t* d_units,      /* [nseries*stride], NULL => default_unit  */
    const int64_t* d_start_ns,   /* [nseries], NULL => first timestamp      */
    const uint8_t* d_ann, uint32_t ann_stride, /* NULL,0 => no annotations  */
    uint32_t nseries, uint32_t stride, int int_optimized, uint8_t default_unit,
    uint8_t* d_out_bytes, uint32_t out_stride, uint32_t* d_out_lens,
    int32_t* d_out_errs, void* hip_stream);

/* host-pointer convenience form of the full encode */
int m3gpu_encode_batch_full(
    const int64_t* ts, const double* vals, const uint32_t* counts,
    const uint8_t* units, const int64_t* start_ns,
    const uint8_t* ann, uint32_t ann_stride,
    uint32_t nseries, uint32_t stride, int int_optimized, uint8_t default_unit,
    uint8_t* out_bytes, uint32_t out_stride, uint32_t* out_lens,
    int32_t* out_errs);

/* Pack strided encoder output into the tight 8B-aligned blob layout:
 * series i's first lens[i] bytes (rounded up to whole 8B words, whose pad
 * bytes the encoder zeroes) move from d_src + i*src_stride to
 * d_dst + d_dst_offsets[i]. d_dst must be pre-zeroed. */
int m3gpu_compact_dev(
    const uint8_t* d_src, uint32_t src_stride, const uint32_t* d_lens,
    const uint64_t* d_dst_offsets, uint32_t nseries, uint8_t* d_dst,
    void* hip_stream);

/* -------- fused decode -> windowed rollup (replaces decode +
 * elem.AddValue/Consume: aggregator/aggregator/generic_elem.go:219-235,
 * 424-485 with aggregation/{counter,gauge,timer}.go semantics) --------
 * Decodes each stream and aggregates into ceil-aligned windows of window_ns:
 * bucket b covers [base + b*window, base + (b+1)*window) where base =
 * truncate(first timestamp). Emits naggs doubles per bucket in agg_types[]
 * order (d_out[i*nbuckets*naggs + b*naggs + k]) and the window-END timestamp
 * (list.go:541-543) in d_out_window_ts[i*nbuckets + b]. Quantiles use the
 * production CKMS semantics (exact for <=64 values per bucket; more sets
 * M3GPU_SERIES_BUCKET_OVERFLOW). agg_types is a HOST pointer (naggs <= 16). */
int m3gpu_rollup_batch_dev(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int metric_type, int64_t window_ns, uint32_t nbuckets,
    const int32_t* agg_types, int naggs,
    double* d_out, int64_t* d_out_window_ts, int32_t* d_out_errs,
    void* hip_stream);

/* As above with explicit CKMS stream options (quantile/cm/options.go:30-32;
 * defaults eps=1e-3, insert_and_compress_every=1024). eps in (0, 0.5),
 * every in [1, 1024] (deep-tier buffers are sized for a 2*1024 peak). */
int m3gpu_rollup_batch_dev_opts(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int metric_type, int64_t window_ns, uint32_t nbuckets,
    const int32_t* agg_types, int naggs,
    double* d_out, int64_t* d_out_window_ts, int32_t* d_out_errs,
    void* hip_stream, double eps, int insert_and_compress_every);

/* -------- replica-deduplicating merge (replaces MultiReaderIterator over
 * one slice of R replica iterators: dbnode/encoding/multi_reader_iterator.go
 * :62-155 + iterators.go:56-237, IterateLastPushed default). Decoded replica
 * rows (replica-major: row r*nseries+i) merge into one row per series with
 * equal timestamps deduped (last in values-order wins) and decreasing
 * timestamps flagged (err 100 = errOutOfOrderIterator). R <= 4. -------- */
int m3gpu_merge_batch_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    uint32_t nreplicas, uint32_t nseries, uint32_t stride,
    int64_t* d_out_ts, double* d_out_vals, uint32_t* d_out_counts,
    int32_t* d_out_errs, uint32_t out_stride, void* hip_stream);

/* The same merge, carrying MultiReaderIterator.Current()'s unit: d_units
 * rows are laid out like the d_ts rows (replica-major, stride bytes per
 * row, e.g. m3gpu_decode_batch_full_dev's d_out_units), d_out_units has
 * out_stride bytes per series. Each emitted point gets the unit of the
 * replica whose value it got (iterators.go current()). Both unit pointers
 * are required; ts, vals, counts and errs equal m3gpu_merge_batch_dev's.
 * Annotations are not carried. */
int m3gpu_merge_batch_units_dev(
    const int64_t* d_ts, const double* d_vals, const uint8_t* d_units,
    const uint32_t* d_counts, uint32_t nreplicas, uint32_t nseries,
    uint32_t stride, int64_t* d_out_ts, double* d_out_vals,
    uint8_t* d_out_units, uint32_t* d_out_counts, int32_t* d_out_errs,
    uint32_t out_stride, void* hip_stream);

/* -------- batched SeriesIterator (replaces encoding.SeriesIterator,
 * dbnode/encoding/series_iterator.go:74-215, as client/session.go builds it
 * from fetched blocks): R <= 4 replicas of B blocks each merge into one row
 * per series, with the query range and the tie rule applied. --------
 *
 * Inputs are the rows m3gpu_decode_batch*_dev writes for a batch of
 * nreplicas*nblocks*nseries streams: block b of replica r of series i is row
 * (r*nblocks + b)*nseries + i, with `stride` elements of d_ts and d_vals,
 * `stride` bytes of d_units, and one entry of d_counts and d_errs. A series
 * with fewer blocks has count-0 rows; a replica's blocks are consumed in
 * order b = 0..nblocks-1. d_units NULL: units are not carried. d_errs NULL:
 * every row decoded cleanly. Any alignment works; the kernel reads several
 * points per load, about three times as fast, when d_ts and d_vals are
 * 16-byte aligned, d_units 4-byte aligned and stride a multiple of 4.
 *
 * Per replica (MultiReaderIterator, one reader per block slice): inside a
 * block an equal timestamp is skipped and a smaller one is
 * M3GPU_SERIES_OUT_OF_ORDER; across a block boundary nothing is compared. A
 * row with a nonzero d_errs entry yields its points, then its error.
 * Across replicas (iterators.go): [start_ns, end_ns) filters only when both
 * are nonzero (series_iterator.go:145); below start_ns a point is skipped, at
 * the first point >= end_ns the replica is dropped. `strategy` is the
 * reference's IterateEqualTimestampStrategy (iterators_types.go:37-56). An
 * error while the replicas are first positioned leaves the series empty; a
 * later one keeps the points emitted so far.
 *
 * Outputs: one row of out_stride elements per series; d_out_counts[i] points
 * are written and nothing beyond them; d_out_errs[i] is 0,
 * M3GPU_SERIES_OUT_OF_ORDER, M3GPU_SERIES_CAPACITY (the stored prefix stays)
 * or a row's error. d_out_units (given exactly when d_units is) is a plain
 * byte array, any base address, out_stride bytes per series; a point gets the
 * unit of the replica whose value it got. Annotations and FirstAnnotation()
 * are not carried.
 *
 * M3GPU_ERR_BADARG, before any HIP call: nreplicas 0 or > 4; nblocks, stride
 * or out_stride 0; strategy outside 0..3; exactly one of d_units and
 * d_out_units given. */
enum { M3GPU_EQUAL_TS_LAST_PUSHED = 0, M3GPU_EQUAL_TS_HIGHEST_VALUE = 1,
       M3GPU_EQUAL_TS_LOWEST_VALUE = 2, M3GPU_EQUAL_TS_HIGHEST_FREQUENCY = 3 };
/* errOutOfOrderIterator, in d_out_errs of all three merge entries */
enum { M3GPU_SERIES_OUT_OF_ORDER = 100 };

int m3gpu_series_merge_batch_dev(
    const int64_t* d_ts, const double* d_vals,
    const uint8_t* d_units,      /* NULL => units not carried            */
    const uint32_t* d_counts,
    const int32_t* d_errs,       /* NULL => every row decoded cleanly    */
    uint32_t nreplicas, uint32_t nblocks, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t end_ns, int strategy,
    int64_t* d_out_ts, double* d_out_vals,
    uint8_t* d_out_units,        /* given iff d_units is                 */
    uint32_t* d_out_counts, int32_t* d_out_errs, uint32_t out_stride,
    void* hip_stream);

/* host-pointer form: uploads, merges on the null stream, copies back; blocks.
 * out_units bytes past a series' count come back 0. */
int m3gpu_series_merge_batch(
    const int64_t* ts, const double* vals, const uint8_t* units,
    const uint32_t* counts, const int32_t* errs,
    uint32_t nreplicas, uint32_t nblocks, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t end_ns, int strategy,
    int64_t* out_ts, double* out_vals, uint8_t* out_units,
    uint32_t* out_counts, int32_t* out_errs, uint32_t out_stride);

/* -------- batched StepIter (replaces encodedBlock.StepIter(),
 * query/storage/m3/encoded_step_iterator.go; nextForStep,
 * encoded_step_iterator_generic.go:63-119; StepLookbackConsolidator,
 * consolidators/step_consolidator.go, with TakeLast,
 * consolidators/types.go:207-216): every series is consolidated onto the
 * query's step grid, one float64 per (step, series). --------
 *
 * Grid: t_k = start_ns + k*step_ns, k = 0..nsteps-1. value(k) is the value,
 * bit for bit, of the last point with t_k - lookback_ns <= ts <= t_k (both
 * ends inclusive) whose value is not NaN; with none, the bit pattern
 * 0x7FF8000000000001 (Go's math.NaN()). Output is step-major, the
 * reference's block.ColStep columns: d_out[k*out_pitch + i], out_pitch >=
 * nseries. Exactly nsteps*nseries cells and d_out_errs[nseries] are written.
 *
 * Points are read up to and including the first with ts > t_last (the
 * peeked point of nextForStep) and nothing after it. An error counts only
 * if reading reaches it, i.e. no point read lies past t_last: a stream's
 * decode error, a row's d_errs entry (it comes after the row's points), or
 * M3GPU_SERIES_OUT_OF_ORDER. A series with a nonzero d_out_errs entry has
 * its whole column set to the NaN pattern; the other series are kept (the
 * reference fails the whole block). Only TakeLast is built.
 *
 * m3gpu_step_consolidate_batch_dev takes rows as m3gpu_series_merge_batch_dev
 * or a decode writes them: d_ts, d_vals [nseries, stride], d_counts, and
 * d_errs (NULL: every row is clean). A point with ts <= its predecessor is
 * M3GPU_SERIES_OUT_OF_ORDER: the reference's arrival-order buffer gives an
 * unspecified result there, and a SeriesIterator never yields it for
 * time-ordered blocks. Any alignment works; 16-byte aligned arrays and an
 * even stride read two points a load.
 *
 * m3gpu_decode_steps_batch_dev goes from streams to the matrix with no rows
 * in between, for one replica: series i has nblocks streams at index
 * b*nseries + i (layout contract of m3gpu_decode_batch above), read in order
 * b = 0..nblocks-1; a zero-length stream is an absent block. An equal
 * timestamp is skipped and a smaller one is M3GPU_SERIES_OUT_OF_ORDER, inside
 * a stream and across a boundary, which is what the one-replica
 * m3gpu_series_merge_batch_dev yields: the result equals
 * m3gpu_step_consolidate_batch_dev over that merge (no range) over the
 * decode of the streams with the errors of zero-length streams cleared. It
 * stops decoding a series at the first point past t_last.
 *
 * M3GPU_ERR_BADARG, before any HIP call: step_ns <= 0; lookback_ns < 0;
 * nsteps 0; stride or nblocks 0; out_pitch < nseries; start_ns +
 * (nsteps-1)*step_ns or start_ns - lookback_ns outside int64. nseries 0
 * succeeds and does nothing. */
int m3gpu_step_consolidate_batch_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    const int32_t* d_errs,       /* NULL => every row is clean           */
    uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t lookback_ns,
    double* d_out, uint32_t out_pitch, int32_t* d_out_errs,
    void* hip_stream);

int m3gpu_decode_steps_batch_dev(
    const uint8_t* d_blobs, const uint64_t* d_offsets, const uint32_t* d_lens,
    uint32_t nseries, uint32_t nblocks, int int_optimized,
    uint8_t default_unit,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t lookback_ns,
    double* d_out, uint32_t out_pitch, int32_t* d_out_errs,
    void* hip_stream);

/* host-pointer forms: upload, run on the null stream, copy back; block.
 * out is [nsteps, out_pitch]; cells past nseries in a row are left alone.
 * offsets and lens have nseries*nblocks entries. */
int m3gpu_step_consolidate_batch(
    const int64_t* ts, const double* vals, const uint32_t* counts,
    const int32_t* errs, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t lookback_ns,
    double* out, uint32_t out_pitch, int32_t* out_errs);

int m3gpu_decode_steps_batch(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, uint32_t nblocks, int int_optimized,
    uint8_t default_unit,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t lookback_ns,
    double* out, uint32_t out_pitch, int32_t* out_errs);

/* -------- batched temporal functions (replaces the temporal baseNode's
 * per-series loop, query/functions/temporal/base.go:255-306 with getIndices,
 * base.go:432-482, and the processors of aggregation.go, rate.go,
 * functions.go and linear_regression.go): one range-vector function per
 * (step, series), e.g. rate(x[5m]) for every series of a fetch. --------
 *
 * Rows are as for m3gpu_step_consolidate_batch_dev: d_ts, d_vals [nseries,
 * stride], d_counts, and d_errs (NULL: every row is clean), what
 * m3gpu_series_merge_batch_dev or a decode wrote. The output is the same
 * step-major matrix, d_out[k*out_pitch + i]; exactly nsteps*nseries cells and
 * d_out_errs[nseries] are written.
 *
 * Grid: t_k = start_ns + k*step_ns. The window W_k is the row's points, in
 * row order, with t_k - range_ns <= ts <= t_k: BOTH ends inclusive, as
 * getIndices has it (it skips ts < lBound and keeps ts <= rBound), not
 * Prometheus' left-open window. NaN points are in the window; each function
 * decides what to do with them. cell(k, i) = f(W_k), f the reference's
 * processor operation for operation in its order, compiled without fused
 * multiply-add:
 *  - SUM, COUNT, AVG (sumAndCount, aggregation.go:236-251; :151-163,
 *    :199-202): NaN skipped, left-to-right sum; no non-NaN point gives NaN.
 *  - MIN, MAX (aggregation.go:165-197): Go's math.Min / math.Max over the
 *    non-NaN values from +-Inf, so Min(0, -0) = -0 and Max(-0, 0) = +0.
 *  - LAST (aggregation.go:227-234): the last point's value bit for bit, a NaN
 *    and its payload included.
 *  - STDVAR, STDDEV (aggregation.go:204-225): the Welford loop, one division
 *    per non-NaN point; fewer than 2 gives NaN; STDDEV is its sqrt.
 *  - RATE, INCREASE, DELTA (standardRateFunc, rate.go:150-240): fewer than 2
 *    points, NaN ones counted, gives NaN; firstIdx / lastIdx are window
 *    indices; durations are subSeconds, float64(a-b)/1e9; RATE alone divides
 *    by time.Duration(range_ns).Seconds().
 *  - IRATE, IDELTA (irateFunc, rate.go:242-298): the last two non-NaN points;
 *    IRATE divides by Duration.Seconds() of their distance, which is
 *    float64(d/1e9) + float64(d%1e9)/1e9 and not subSeconds.
 *  - RESETS, CHANGES (functionNode.process, functions.go:89-118): prev starts
 *    as the first point's value, NaN or not; an empty window, or only NaN
 *    behind the first point, gives NaN.
 *  - DERIV, PREDICT_LINEAR (linear_regression.go:127-191): fewer than 2
 *    points, NaN ones counted, gives NaN; the intercept time is t_k for
 *    PREDICT_LINEAR and the first non-NaN timestamp for DERIV; one non-NaN
 *    value gives NaN, none falls through to 0/0. PREDICT_LINEAR returns
 *    slope*param + intercept, param in seconds; other functions ignore param.
 * Where the reference returns math.NaN() the cell holds 0x7FF8000000000001,
 * as in the step matrix; sign and payload of a NaN that arithmetic produced
 * are the hardware's.
 *
 * Errors: a batch keeps its other series. Series i fails when d_errs[i] is
 * nonzero, wherever its points lie: the temporal node takes
 * series.Datapoints(), the whole decoded series, before its first window.
 * (m3gpu_step_consolidate_batch_dev differs: nextForStep meets a row's error
 * only if it reads that far.) It fails with M3GPU_SERIES_OUT_OF_ORDER when,
 * among the points from the row's first up to and including the first one
 * past t_last, a timestamp is at or before its predecessor; nothing behind
 * that point is read. A failed series' column is all 0x7FF8000000000001.
 *
 * Not built: quantile_over_time (a sort per window), holt_winters, a fused
 * streams -> temporal entry, more than 4 replicas in the merge before it.
 *
 * M3GPU_ERR_BADARG, before any HIP call: step_ns <= 0; range_ns <= 0; nsteps
 * 0; stride 0; out_pitch < nseries; fn outside the enum; start_ns +
 * (nsteps-1)*step_ns or start_ns - range_ns outside int64. nseries 0
 * succeeds and does nothing. */
enum {  /* src/query/functions/temporal */
    M3GPU_TEMPORAL_SUM, M3GPU_TEMPORAL_COUNT, M3GPU_TEMPORAL_AVG,
    M3GPU_TEMPORAL_MIN, M3GPU_TEMPORAL_MAX, M3GPU_TEMPORAL_LAST,
    M3GPU_TEMPORAL_STDDEV, M3GPU_TEMPORAL_STDVAR,          /* aggregation.go */
    M3GPU_TEMPORAL_RATE, M3GPU_TEMPORAL_INCREASE, M3GPU_TEMPORAL_DELTA,
    M3GPU_TEMPORAL_IRATE, M3GPU_TEMPORAL_IDELTA,           /* rate.go */
    M3GPU_TEMPORAL_RESETS, M3GPU_TEMPORAL_CHANGES,         /* functions.go */
    M3GPU_TEMPORAL_DERIV, M3GPU_TEMPORAL_PREDICT_LINEAR,   /* linear_regression.go */
    M3GPU_TEMPORAL_FN_COUNT
};

int m3gpu_temporal_batch_dev(
    const int64_t* d_ts, const double* d_vals, const uint32_t* d_counts,
    const int32_t* d_errs,       /* NULL => every row is clean           */
    uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t range_ns,
    int fn, double param,        /* predict_linear's seconds; else ignored */
    double* d_out, uint32_t out_pitch, int32_t* d_out_errs,
    void* hip_stream);

/* host-pointer form (what a cgo temporal.baseNode replacement calls, base.go
 * :227-321): upload, run on the null stream, copy back; blocks. out is
 * [nsteps, out_pitch]; cells past nseries in a row are left alone. */
int m3gpu_temporal_batch(
    const int64_t* ts, const double* vals, const uint32_t* counts,
    const int32_t* errs, uint32_t nseries, uint32_t stride,
    int64_t start_ns, int64_t step_ns, uint32_t nsteps, int64_t range_ns,
    int fn, double param,
    double* out, uint32_t out_pitch, int32_t* out_errs);

/* The depth C of the per-row LDS ring the library's temporal kernels were
 * built with: windows of up to C points are read from LDS, longer ones reach
 * into global memory for their older points. For tests and sizing. */
int m3gpu_temporal_ring_depth(void);

int m3gpu_rollup_batch(
    const uint8_t* blobs, uint64_t blobs_len,
    const uint64_t* offsets, const uint32_t* lens,
    uint32_t nseries, int int_optimized, uint8_t default_unit,
    int metric_type, int64_t window_ns, uint32_t nbuckets,
    const int32_t* agg_types, int naggs,
    double* out, int64_t* out_window_ts, int32_t* out_errs);

/* Layout pass: physically reorder packed streams so dst series i holds
 * src series perm[i] (dst_offsets precomputed from lens[perm], 16B
 * aligned). Lays a batch out in wave-schedule order for L2 locality. */
int m3gpu_regather_dev(
    const uint8_t* d_src, const uint64_t* d_src_offsets,
    const uint32_t* d_lens, const int32_t* d_perm,
    const uint64_t* d_dst_offsets, uint32_t nseries, uint8_t* d_dst,
    void* hip_stream);

/* Largest bucket size for which the CKMS stream with the given eps
 * provably never merges for this agg set (quantiles extracted, sorted
 * unique): up to this depth the wave-tier rollup's quantiles are exact
 * order statistics. For tests and host-side sizing. */
int m3gpu_ckms_exact_cap(const int32_t* agg_types, int naggs, double eps);

/* ======================= fileset volume reader =======================
 * Native reader for the reference's dbnode fileset volumes (persist/fs
 * read.go:145-457 + msgpack/decoder.go + digest): open a volume from a
 * shard directory (reference naming fileset-<blockStartNs>-<volume>-
 * <suffix>.db, legacy no-volume names for volume 0), validate the
 * checkpoint, all five file digests, every index-entry checksum (V3) and
 * every data-block checksum, then expose the entries sorted by data
 * offset ascending and repack the blocks into the decode-batch blob
 * layout above. Pure host code (usable without a GPU). */

/* Returns a handle >= 0, or a negative M3GPU_FS_ERR_* code. */
int m3gpu_fileset_open(const char* shard_dir, int64_t block_start_ns,
                       int volume_index);
int m3gpu_fileset_close(int handle);
const char* m3gpu_fileset_last_error(void);
int m3gpu_fileset_info(int handle, int64_t* block_start, int64_t* block_size,
                       int64_t* entries, int64_t* major_version,
                       int64_t* minor_version, int* volume_index,
                       int64_t* bloom_m, int64_t* bloom_k,
                       int64_t* summaries);
int m3gpu_fileset_entry(int handle, int64_t i, int64_t* size, int64_t* offset,
                        int64_t* data_checksum, const uint8_t** id,
                        int64_t* id_len, const uint8_t** tags,
                        int64_t* tags_len);
int64_t m3gpu_fileset_packed_size(int handle);
int m3gpu_fileset_pack(int handle, uint8_t* blob, uint64_t blob_cap,
                       uint64_t* offsets, uint32_t* lens);

enum {
    M3GPU_FS_ERR_IO = -101,
    M3GPU_FS_ERR_CHECKPOINT = -102,
    M3GPU_FS_ERR_DIGEST = -103,
    M3GPU_FS_ERR_MSGPACK = -104,
    M3GPU_FS_ERR_SCHEMA = -105,
    M3GPU_FS_ERR_ENTRY_CHECKSUM = -106,
    M3GPU_FS_ERR_DATA_CHECKSUM = -107,
    M3GPU_FS_ERR_BOUNDS = -108,
    M3GPU_FS_ERR_BADHANDLE = -109,
    M3GPU_FS_ERR_CAPACITY = -110,
};

/* ======================== commit log reader =========================
 * Native reader for the reference's commit log files (persist/fs/
 * commitlog: 12-byte chunk headers with adler32 size/data checksums,
 * uvarint-framed msgpack LogInfo/LogEntry records, nested LogMetadata on
 * each series' first entry). Series come back in first-seen order with
 * datapoints in log order — the bootstrap-from-commitlog input to the GPU
 * batch encoder. Pure host code. */
int m3gpu_commitlog_open(const char* path); /* handle >= 0 or error */
int m3gpu_commitlog_close(int handle);
const char* m3gpu_commitlog_last_error(void);
int m3gpu_commitlog_info(int handle, int64_t* index, int64_t* num_entries,
                         int64_t* num_series);
int m3gpu_commitlog_series(int handle, int64_t i, uint64_t* unique_index,
                           const uint8_t** id, int64_t* id_len,
                           const uint8_t** ns, int64_t* ns_len,
                           uint32_t* shard, const uint8_t** tags,
                           int64_t* tags_len, int64_t* num_points,
                           int64_t* num_annotations);
int m3gpu_commitlog_series_points(int handle, int64_t i, int64_t* ts,
                                  double* vals, uint8_t* units);
int m3gpu_commitlog_series_annotation(int handle, int64_t i, int64_t j,
                                      int64_t* point_index,
                                      const uint8_t** bytes, int64_t* len);

enum {
    M3GPU_CL_ERR_CHUNK_CHECKSUM = -111,
    M3GPU_CL_ERR_MISSING_METADATA = -112,
    M3GPU_CL_ERR_TRUNCATED = -113,
};

/* ================= unaggregated metric wire parser =================
 * Batch parser for the m3aggregator ingest wire format
 * (metrics/encoding/protobuf): zigzag-varint size-prefixed metricpb
 * MetricWithMetadatas messages. Untimed counter/batch-timer/gauge and
 * timed unions are parsed; metadatas/policies kept as opaque bytes.
 * Pure host code; grouped values feed the GPU encode/rollup path. */
int m3gpu_unagg_parse(const uint8_t* buf, uint64_t len); /* handle or <0 */
int m3gpu_unagg_close(int handle);
const char* m3gpu_unagg_last_error(void);
int64_t m3gpu_unagg_count(int handle);
int m3gpu_unagg_metric(int handle, int64_t i, int32_t* union_type,
                       int32_t* metric_type, const uint8_t** id,
                       int64_t* id_len, int64_t* num_values,
                       int64_t* counter_value, int64_t* time_nanos,
                       const uint8_t** annotation, int64_t* annotation_len,
                       const uint8_t** metadatas, int64_t* metadatas_len);
int m3gpu_unagg_values(int handle, int64_t i, double* out);
/* Field-separated wrapper metadata (StagedMetadatas field 2, StoragePolicy
 * field 3, ...): `metadatas` above is a concatenation and cannot be split
 * back into the individual reference protos. */
int64_t m3gpu_unagg_metadata_count(int handle, int64_t i);
int m3gpu_unagg_metadata(int handle, int64_t i, int64_t j, int32_t* field,
                         const uint8_t** bytes, int64_t* len);

enum {
    M3GPU_UA_ERR_TRUNCATED = -121,
    M3GPU_UA_ERR_PROTO = -122,
    M3GPU_UA_ERR_TYPE = -123,
    M3GPU_UA_ERR_BADHANDLE = -124,
    M3GPU_UA_ERR_SIZE = -125,
};

#ifdef __cplusplus
}
#endif
#endif
