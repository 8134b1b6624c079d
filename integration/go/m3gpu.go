// Package m3gpu binds the MI355X-native M3TSZ + rollup engine
// (libm3gpu.so, C ABI in include/m3gpu.h) for use inside m3db/m3.
//
// This file is the drop-in surface a maintainer vendors into the reference:
// it mirrors the reference's pluggable codec boundary (alloc functions
// registered into pools at dbnode/storage/options.go:498-510,
// dbnode/server/server.go:1786-1793, dbnode/client/options.go:504) for the
// BULK paths — block ingestion, cold-flush merges, AggregateTiles, bulk
// fetches — while single-point streaming stays on the existing Go codec.
// See INTEGRATION.md for the full wiring discussion.
//
// NOTE: this tree's build environment has no Go toolchain (SURVEY.md §0);
// this file is compile-checked only where Go is available. It contains no
// logic beyond argument marshalling — all semantics live behind the C ABI
// and are pinned by the oracle + GPU parity suites.
package m3gpu

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../m3_amd/csrc -lm3gpu
#include <stdlib.h>
#include "m3gpu.h"
*/
import "C"

import (
	"encoding/binary"
	"errors"
	"unsafe"
)

// SeriesError mirrors the per-series M3GPU_SERIES_* codes.
type SeriesError int32

const (
	SeriesOK             SeriesError = 0
	SeriesEOF            SeriesError = 1
	SeriesDodOverflow    SeriesError = 2
	SeriesNoScheme       SeriesError = 3
	SeriesInvalidMult    SeriesError = 4
	SeriesAnnotation     SeriesError = 5
	SeriesCapacity       SeriesError = 6
	SeriesUnsorted       SeriesError = 7
	SeriesBucketOverflow SeriesError = 8
)

func lastError() error {
	return errors.New(C.GoString(C.m3gpu_last_error()))
}

// Init selects the GPU device for this process (one engine per GPU; shard
// the series space across devices exactly as m3 shards across instances).
func Init(device int) error {
	if rc := C.m3gpu_init(C.int(device)); rc != 0 {
		return lastError()
	}
	return nil
}

// DecodeBatch decodes packed M3TSZ streams (layout contract in m3gpu.h:
// offsets 16-byte aligned, zero padded) into SoA rows of `stride` points.
// Replaces a loop of m3tsz.NewReaderIterator/Next/Current
// (dbnode/encoding/m3tsz/iterator.go:81-219) over a batch of blocks.
func DecodeBatch(
	blobs []byte, offsets []uint64, lens []uint32,
	intOptimized bool, defaultUnit byte, stride uint32,
) (ts []int64, vals []float64, counts []uint32, errs []SeriesError, err error) {
	n := uint32(len(lens))
	if n == 0 {
		return nil, nil, nil, nil, nil
	}
	ts = make([]int64, uint64(n)*uint64(stride))
	vals = make([]float64, uint64(n)*uint64(stride))
	counts = make([]uint32, n)
	errs = make([]SeriesError, n)
	intOpt := C.int(0)
	if intOptimized {
		intOpt = 1
	}
	rc := C.m3gpu_decode_batch(
		(*C.uint8_t)(unsafe.Pointer(&blobs[0])), C.uint64_t(len(blobs)),
		(*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		(*C.uint32_t)(unsafe.Pointer(&lens[0])),
		C.uint32_t(n), intOpt, C.uint8_t(defaultUnit),
		(*C.int64_t)(unsafe.Pointer(&ts[0])),
		(*C.double)(unsafe.Pointer(&vals[0])),
		(*C.uint32_t)(unsafe.Pointer(&counts[0])),
		(*C.int32_t)(unsafe.Pointer(&errs[0])), C.uint32_t(stride))
	if rc != 0 {
		return nil, nil, nil, nil, lastError()
	}
	return ts, vals, counts, errs, nil
}

// EncodeBatch encodes SoA rows into finalized M3TSZ streams (EOS tail
// included), byte-identical to m3tsz.Encoder output (encoder.go:89-250).
// outStride must be a multiple of 8 and hold the worst case (~24 B/pt + 32).
func EncodeBatch(
	ts []int64, vals []float64, counts []uint32,
	stride uint32, intOptimized bool, unit byte, outStride uint32,
) (streams []byte, lens []uint32, errs []SeriesError, err error) {
	n := uint32(len(counts))
	if n == 0 {
		return nil, nil, nil, nil
	}
	streams = make([]byte, uint64(n)*uint64(outStride))
	lens = make([]uint32, n)
	errs = make([]SeriesError, n)
	intOpt := C.int(0)
	if intOptimized {
		intOpt = 1
	}
	rc := C.m3gpu_encode_batch(
		(*C.int64_t)(unsafe.Pointer(&ts[0])),
		(*C.double)(unsafe.Pointer(&vals[0])),
		(*C.uint32_t)(unsafe.Pointer(&counts[0])),
		C.uint32_t(n), C.uint32_t(stride), intOpt, C.uint8_t(unit),
		(*C.uint8_t)(unsafe.Pointer(&streams[0])), C.uint32_t(outStride),
		(*C.uint32_t)(unsafe.Pointer(&lens[0])),
		(*C.int32_t)(unsafe.Pointer(&errs[0])))
	if rc != 0 {
		return nil, nil, nil, nil, lastError()
	}
	return streams, lens, errs, nil
}

// RollupBatch runs the fused decode -> windowed rollup with m3aggregator
// semantics (generic_elem.go AddValue/Consume + aggregation/{counter,gauge,
// timer}.go). aggTypes carries the reference's aggregation.Type values
// (metrics/aggregation/type.go:31-56). Output timestamps are window ENDS
// (list.go:541-543), so flush handlers consume them unchanged; this is the
// backend AggregateTiles (storage/shard.go:2682) drives.
func RollupBatch(
	blobs []byte, offsets []uint64, lens []uint32,
	intOptimized bool, defaultUnit byte,
	metricType int, windowNs int64, nbuckets uint32,
	aggTypes []int32,
) (out []float64, windowTs []int64, errs []SeriesError, err error) {
	n := uint32(len(lens))
	if n == 0 || len(aggTypes) == 0 {
		return nil, nil, nil, nil
	}
	out = make([]float64, uint64(n)*uint64(nbuckets)*uint64(len(aggTypes)))
	windowTs = make([]int64, uint64(n)*uint64(nbuckets))
	errs = make([]SeriesError, n)
	intOpt := C.int(0)
	if intOptimized {
		intOpt = 1
	}
	rc := C.m3gpu_rollup_batch(
		(*C.uint8_t)(unsafe.Pointer(&blobs[0])), C.uint64_t(len(blobs)),
		(*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		(*C.uint32_t)(unsafe.Pointer(&lens[0])),
		C.uint32_t(n), intOpt, C.uint8_t(defaultUnit),
		C.int(metricType), C.int64_t(windowNs), C.uint32_t(nbuckets),
		(*C.int32_t)(unsafe.Pointer(&aggTypes[0])), C.int(len(aggTypes)),
		(*C.double)(unsafe.Pointer(&out[0])),
		(*C.int64_t)(unsafe.Pointer(&windowTs[0])),
		(*C.int32_t)(unsafe.Pointer(&errs[0])))
	if rc != 0 {
		return nil, nil, nil, nil, lastError()
	}
	return out, windowTs, errs, nil
}

// AnnotationEvent is one annotation-set event from the annotation-capturing
// decode: the annotation starts applying at Point (0-based) and stays the
// Current() third return (iterator.go:226-231 sticky PrevAnt) until the
// next event.
type AnnotationEvent struct {
	Point uint32
	Bytes []byte
}

// DecodeBatchAnn decodes like DecodeBatch and additionally captures every
// annotation-set event per series (m3gpu_decode_batch_ann; region layout in
// m3gpu.h). annStride sizes the per-series region (4-aligned, >= 16); a
// series whose annotations overflow it flags SeriesCapacity but still
// decodes its values.
func DecodeBatchAnn(
	blobs []byte, offsets []uint64, lens []uint32,
	intOptimized bool, defaultUnit byte, stride uint32, annStride uint32,
) (ts []int64, vals []float64, counts []uint32, errs []SeriesError,
	anns [][]AnnotationEvent, err error) {
	n := uint32(len(lens))
	if n == 0 {
		return nil, nil, nil, nil, nil, nil
	}
	ts = make([]int64, uint64(n)*uint64(stride))
	vals = make([]float64, uint64(n)*uint64(stride))
	counts = make([]uint32, n)
	errs = make([]SeriesError, n)
	region := make([]byte, uint64(n)*uint64(annStride))
	intOpt := C.int(0)
	if intOptimized {
		intOpt = 1
	}
	rc := C.m3gpu_decode_batch_ann(
		(*C.uint8_t)(unsafe.Pointer(&blobs[0])), C.uint64_t(len(blobs)),
		(*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		(*C.uint32_t)(unsafe.Pointer(&lens[0])),
		C.uint32_t(n), intOpt, C.uint8_t(defaultUnit),
		(*C.int64_t)(unsafe.Pointer(&ts[0])),
		(*C.double)(unsafe.Pointer(&vals[0])),
		(*C.uint32_t)(unsafe.Pointer(&counts[0])),
		(*C.int32_t)(unsafe.Pointer(&errs[0])), C.uint32_t(stride),
		(*C.uint8_t)(unsafe.Pointer(&region[0])), C.uint32_t(annStride))
	if rc != 0 {
		return nil, nil, nil, nil, nil, lastError()
	}
	anns = make([][]AnnotationEvent, n)
	le := binary.LittleEndian
	for i := uint32(0); i < n; i++ {
		r := region[uint64(i)*uint64(annStride) : uint64(i+1)*uint64(annStride)]
		nev := le.Uint32(r[0:4])
		evs := make([]AnnotationEvent, 0, nev)
		for j := uint32(0); j < nev; j++ {
			ev := r[4+j*12 : 4+j*12+12]
			off, ln := le.Uint32(ev[4:8]), le.Uint32(ev[8:12])
			evs = append(evs, AnnotationEvent{
				Point: le.Uint32(ev[0:4]),
				Bytes: append([]byte(nil), r[off:off+ln]...),
			})
		}
		anns[i] = evs
	}
	return ts, vals, counts, errs, anns, nil
}

// FullDecoded is what DecodeBatchFull returns: DecodeBatch's rows plus, per
// point, the time unit ReaderIterator.Current() reports with it, per series
// the block start (the stream's first 64 bits) and the annotation-set
// events. Ts, Vals, Counts, Units, StartNs and Anns can be passed unchanged
// to EncodeBatchFull, which reproduces the streams.
type FullDecoded struct {
	Ts      []int64
	Vals    []float64
	Units   []byte // len n*stride, 0 past each series' count
	Counts  []uint32
	Errs    []SeriesError
	StartNs []int64
	Anns    [][]AnnotationEvent // nil when annStride == 0
}

// DecodeBatchFull is the batched form of ReaderIterator.Current()'s full
// return, (datapoint, unit, annotation), plus the block start
// (m3gpu_decode_batch_full). annStride == 0 skips the annotations; otherwise
// it sizes the per-series region (4-aligned, >= 16) as in DecodeBatchAnn.
// The device wrote the region headers: each is checked against annStride
// before anything is sliced by it.
func DecodeBatchFull(
	blobs []byte, offsets []uint64, lens []uint32,
	intOptimized bool, defaultUnit byte, stride uint32, annStride uint32,
) (*FullDecoded, error) {
	n := uint32(len(lens))
	if n == 0 {
		return &FullDecoded{}, nil
	}
	if len(blobs) == 0 || uint32(len(offsets)) < n+1 {
		return nil, errors.New("m3gpu: need blobs and n+1 offsets")
	}
	if annStride != 0 && (annStride%4 != 0 || annStride < 16) {
		return nil, errors.New("m3gpu: annStride must be 4-aligned and >= 16")
	}
	if stride == 0 {
		return nil, errors.New("m3gpu: stride must be > 0")
	}
	npts := uint64(n) * uint64(stride)
	d := &FullDecoded{
		Ts:      make([]int64, npts),
		Vals:    make([]float64, npts),
		Units:   make([]byte, npts),
		Counts:  make([]uint32, n),
		Errs:    make([]SeriesError, n),
		StartNs: make([]int64, n),
	}
	var region []byte
	var annPtr *C.uint8_t
	if annStride != 0 {
		region = make([]byte, uint64(n)*uint64(annStride))
		annPtr = (*C.uint8_t)(unsafe.Pointer(&region[0]))
	}
	intOpt := C.int(0)
	if intOptimized {
		intOpt = 1
	}
	rc := C.m3gpu_decode_batch_full(
		(*C.uint8_t)(unsafe.Pointer(&blobs[0])), C.uint64_t(len(blobs)),
		(*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		(*C.uint32_t)(unsafe.Pointer(&lens[0])),
		C.uint32_t(n), intOpt, C.uint8_t(defaultUnit),
		(*C.int64_t)(unsafe.Pointer(&d.Ts[0])),
		(*C.double)(unsafe.Pointer(&d.Vals[0])),
		(*C.uint32_t)(unsafe.Pointer(&d.Counts[0])),
		(*C.int32_t)(unsafe.Pointer(&d.Errs[0])), C.uint32_t(stride),
		(*C.uint8_t)(unsafe.Pointer(&d.Units[0])),
		(*C.int64_t)(unsafe.Pointer(&d.StartNs[0])),
		annPtr, C.uint32_t(annStride))
	if rc != 0 {
		return nil, lastError()
	}
	if annStride == 0 {
		return d, nil
	}
	d.Anns = make([][]AnnotationEvent, n)
	le := binary.LittleEndian
	for i := uint32(0); i < n; i++ {
		r := region[uint64(i)*uint64(annStride) : uint64(i+1)*uint64(annStride)]
		nev := le.Uint32(r[0:4])
		if nev > (annStride-4)/12 {
			return nil, errors.New("m3gpu: annotation region: event count beyond the region")
		}
		evs := make([]AnnotationEvent, 0, nev)
		for j := uint32(0); j < nev; j++ {
			ev := r[4+j*12 : 4+j*12+12]
			off, ln := le.Uint32(ev[4:8]), le.Uint32(ev[8:12])
			if uint64(off)+uint64(ln) > uint64(annStride) {
				return nil, errors.New("m3gpu: annotation region: event bytes beyond the region")
			}
			evs = append(evs, AnnotationEvent{
				Point: le.Uint32(ev[0:4]),
				Bytes: append([]byte(nil), r[off:off+ln]...),
			})
		}
		d.Anns[i] = evs
	}
	return d, nil
}

// MergeBatchUnits is the replica-deduplicating merge that also carries
// MultiReaderIterator.Current()'s unit (m3gpu_merge_batch_units_dev). Like
// the C entry it works on DEVICE buffers: dTs/dVals/dUnits hold
// nreplicas*nseries rows of stride points (replica-major), dCounts their
// counts; the outputs hold nseries rows of outStride points. Every emitted
// point gets the unit of the replica whose value it got. The work is
// enqueued on hipStream (nil: the null stream); the caller synchronizes.
func MergeBatchUnits(
	dTs, dVals, dUnits, dCounts unsafe.Pointer,
	nreplicas, nseries, stride uint32,
	dOutTs, dOutVals, dOutUnits, dOutCounts, dOutErrs unsafe.Pointer,
	outStride uint32, hipStream unsafe.Pointer,
) error {
	rc := C.m3gpu_merge_batch_units_dev(
		(*C.int64_t)(dTs), (*C.double)(dVals), (*C.uint8_t)(dUnits),
		(*C.uint32_t)(dCounts), C.uint32_t(nreplicas), C.uint32_t(nseries),
		C.uint32_t(stride), (*C.int64_t)(dOutTs), (*C.double)(dOutVals),
		(*C.uint8_t)(dOutUnits), (*C.uint32_t)(dOutCounts),
		(*C.int32_t)(dOutErrs), C.uint32_t(outStride), hipStream)
	if rc != 0 {
		return lastError()
	}
	return nil
}

// The IterateEqualTimestampStrategy values SeriesMergeBatch takes
// (M3GPU_EQUAL_TS_*; the order of encoding.IterateEqualTimestampStrategy).
const (
	EqualTsLastPushed       = 0
	EqualTsHighestValue     = 1
	EqualTsLowestValue      = 2
	EqualTsHighestFrequency = 3
)

// SeriesMergeBatch is the batched encoding.SeriesIterator
// (m3gpu_series_merge_batch_dev): nreplicas replicas of nblocks decoded
// blocks per series merge into one row per series, with the query range
// [startNs, endNs) (on only when both are nonzero) and the equal-timestamp
// strategy applied. Like the C entry it works on DEVICE buffers: block b of
// replica r of series i is row (r*nblocks+b)*nseries+i of dTs/dVals/dUnits
// and entry of dCounts/dErrs — what DecodeBatch's device form writes for the
// streams packed in that order. dUnits and dOutUnits go together (both nil:
// units are not carried); dErrs may be nil. A per-series error leaves the
// points emitted before it in place. Annotations are not carried. The work
// is enqueued on hipStream (nil: the null stream); the caller synchronizes.
func SeriesMergeBatch(
	dTs, dVals, dUnits, dCounts, dErrs unsafe.Pointer,
	nreplicas, nblocks, nseries, stride uint32,
	startNs, endNs int64, strategy int,
	dOutTs, dOutVals, dOutUnits, dOutCounts, dOutErrs unsafe.Pointer,
	outStride uint32, hipStream unsafe.Pointer,
) error {
	rc := C.m3gpu_series_merge_batch_dev(
		(*C.int64_t)(dTs), (*C.double)(dVals), (*C.uint8_t)(dUnits),
		(*C.uint32_t)(dCounts), (*C.int32_t)(dErrs), C.uint32_t(nreplicas),
		C.uint32_t(nblocks), C.uint32_t(nseries), C.uint32_t(stride),
		C.int64_t(startNs), C.int64_t(endNs), C.int(strategy),
		(*C.int64_t)(dOutTs), (*C.double)(dOutVals), (*C.uint8_t)(dOutUnits),
		(*C.uint32_t)(dOutCounts), (*C.int32_t)(dOutErrs),
		C.uint32_t(outStride), hipStream)
	if rc != 0 {
		return lastError()
	}
	return nil
}

// StepNaNBits is what a step without a value holds: Go's math.NaN().
const StepNaNBits = 0x7FF8000000000001

// StepConsolidateBatch is the batched encodedBlock.StepIter() over rows
// (m3gpu_step_consolidate_batch_dev; query/storage/m3/
// encoded_step_iterator_generic.go:63-119 nextForStep,
// consolidators/step_consolidator.go, consolidators/types.go:207-216
// TakeLast): the rows SeriesMergeBatch or DecodeBatch's device form wrote
// (dTs, dVals [nseries, stride], dCounts, dErrs or nil) are consolidated onto
// the grid startNs + k*stepNs, k < nsteps, with the last non-NaN value in
// [t_k - lookbackNs, t_k]. dOut is step-major, the block.ColStep layout:
// dOut[k*outPitch + i], a step without a value holding StepNaNBits.
// dOutErrs[i] != 0 (a row's error that reading reached, or 100 for a
// timestamp at or before its predecessor) means series i's column is all
// NaN; the reference fails the whole block there. DEVICE buffers, enqueued on
// hipStream (nil: the null stream); the caller synchronizes.
func StepConsolidateBatch(
	dTs, dVals, dCounts, dErrs unsafe.Pointer,
	nseries, stride uint32,
	startNs, stepNs int64, nsteps uint32, lookbackNs int64,
	dOut unsafe.Pointer, outPitch uint32, dOutErrs unsafe.Pointer,
	hipStream unsafe.Pointer,
) error {
	rc := C.m3gpu_step_consolidate_batch_dev(
		(*C.int64_t)(dTs), (*C.double)(dVals), (*C.uint32_t)(dCounts),
		(*C.int32_t)(dErrs), C.uint32_t(nseries), C.uint32_t(stride),
		C.int64_t(startNs), C.int64_t(stepNs), C.uint32_t(nsteps),
		C.int64_t(lookbackNs), (*C.double)(dOut), C.uint32_t(outPitch),
		(*C.int32_t)(dOutErrs), hipStream)
	if rc != 0 {
		return lastError()
	}
	return nil
}

// DecodeStepsBatch goes from streams to the step matrix in one kernel, for
// one replica (m3gpu_decode_steps_batch_dev): series i has nblocks streams
// at index b*nseries+i of dOffsets/dLens, read in block order, a zero-length
// stream being an absent block. No rows are written, and a series stops
// decoding at its first point past the last step. Outputs as in
// StepConsolidateBatch; with more than one replica use DecodeBatch,
// SeriesMergeBatch and StepConsolidateBatch.
func DecodeStepsBatch(
	dBlobs, dOffsets, dLens unsafe.Pointer,
	nseries, nblocks uint32, intOptimized bool, defaultUnit byte,
	startNs, stepNs int64, nsteps uint32, lookbackNs int64,
	dOut unsafe.Pointer, outPitch uint32, dOutErrs unsafe.Pointer,
	hipStream unsafe.Pointer,
) error {
	intOpt := C.int(0)
	if intOptimized {
		intOpt = 1
	}
	rc := C.m3gpu_decode_steps_batch_dev(
		(*C.uint8_t)(dBlobs), (*C.uint64_t)(dOffsets), (*C.uint32_t)(dLens),
		C.uint32_t(nseries), C.uint32_t(nblocks), intOpt,
		C.uint8_t(defaultUnit), C.int64_t(startNs), C.int64_t(stepNs),
		C.uint32_t(nsteps), C.int64_t(lookbackNs), (*C.double)(dOut),
		C.uint32_t(outPitch), (*C.int32_t)(dOutErrs), hipStream)
	if rc != 0 {
		return lastError()
	}
	return nil
}

// TemporalFn is one of the range-vector functions of
// src/query/functions/temporal (M3GPU_TEMPORAL_* in m3gpu.h).
type TemporalFn int32

const (
	TemporalSum TemporalFn = iota // aggregation.go
	TemporalCount
	TemporalAvg
	TemporalMin
	TemporalMax
	TemporalLast
	TemporalStdDev
	TemporalStdVar
	TemporalRate // rate.go
	TemporalIncrease
	TemporalDelta
	TemporalIRate
	TemporalIDelta
	TemporalResets // functions.go
	TemporalChanges
	TemporalDeriv // linear_regression.go
	TemporalPredictLinear
)

// TemporalOpTypes maps the temporal package's op types to TemporalFn.
// quantile_over_time and holt_winters are not built and stay with Go.
var TemporalOpTypes = map[string]TemporalFn{
	"sum_over_time": TemporalSum, "count_over_time": TemporalCount,
	"avg_over_time": TemporalAvg, "min_over_time": TemporalMin,
	"max_over_time": TemporalMax, "last_over_time": TemporalLast,
	"stddev_over_time": TemporalStdDev, "stdvar_over_time": TemporalStdVar,
	"rate": TemporalRate, "increase": TemporalIncrease, "delta": TemporalDelta,
	"irate": TemporalIRate, "idelta": TemporalIDelta,
	"resets": TemporalResets, "changes": TemporalChanges,
	"deriv": TemporalDeriv, "predict_linear": TemporalPredictLinear,
}

// TemporalBatch runs one temporal function for every series and step
// (m3gpu_temporal_batch; query/functions/temporal/base.go:227-321 with
// getIndices, base.go:432-482): what parallelProcess computes with one
// processor per batch. ts and vals are rows of `stride` points, counts[i] of
// them valid, rowErrs nil or one decode/merge error per series. The grid is
// startNs + k*stepNs, k < nsteps; the window of a step is [t_k - rangeNs,
// t_k], both ends inclusive as getIndices has them. param is
// predict_linear's seconds. out is step-major, out[k*nseries + i], the
// builder's columns; math.NaN() cells hold StepNaNBits. errs[i] != 0 (the
// row's error, wherever its points lie, or 100 for a timestamp at or before
// its predecessor) means series i's column is all NaN: fail the block as
// iter.Err() would, or keep the other series.
func TemporalBatch(
	ts []int64, vals []float64, counts []uint32, rowErrs []SeriesError,
	stride uint32, startNs, stepNs int64, nsteps uint32, rangeNs int64,
	fn TemporalFn, param float64,
) (out []float64, errs []SeriesError, err error) {
	n := uint32(len(counts))
	if n == 0 {
		return nil, nil, nil
	}
	out = make([]float64, uint64(nsteps)*uint64(n))
	errs = make([]SeriesError, n)
	var rowErrsPtr *C.int32_t
	if rowErrs != nil {
		rowErrsPtr = (*C.int32_t)(unsafe.Pointer(&rowErrs[0]))
	}
	var outPtr *C.double
	if len(out) > 0 {
		outPtr = (*C.double)(unsafe.Pointer(&out[0]))
	}
	var tsPtr *C.int64_t
	var valsPtr *C.double
	if len(ts) > 0 {
		tsPtr = (*C.int64_t)(unsafe.Pointer(&ts[0]))
		valsPtr = (*C.double)(unsafe.Pointer(&vals[0]))
	}
	rc := C.m3gpu_temporal_batch(
		tsPtr, valsPtr, (*C.uint32_t)(unsafe.Pointer(&counts[0])), rowErrsPtr,
		C.uint32_t(n), C.uint32_t(stride), C.int64_t(startNs),
		C.int64_t(stepNs), C.uint32_t(nsteps), C.int64_t(rangeNs), C.int(fn),
		C.double(param), outPtr, C.uint32_t(n),
		(*C.int32_t)(unsafe.Pointer(&errs[0])))
	if rc != 0 {
		return nil, nil, lastError()
	}
	return out, errs, nil
}

// TemporalBatchDev is TemporalBatch over DEVICE rows
// (m3gpu_temporal_batch_dev): the rows SeriesMergeBatch or DecodeBatch's
// device form wrote go in where they lie, dOut is [nsteps, outPitch] like
// StepConsolidateBatch's. Enqueued on hipStream (nil: the null stream); the
// caller synchronizes.
func TemporalBatchDev(
	dTs, dVals, dCounts, dErrs unsafe.Pointer,
	nseries, stride uint32,
	startNs, stepNs int64, nsteps uint32, rangeNs int64,
	fn TemporalFn, param float64,
	dOut unsafe.Pointer, outPitch uint32, dOutErrs unsafe.Pointer,
	hipStream unsafe.Pointer,
) error {
	rc := C.m3gpu_temporal_batch_dev(
		(*C.int64_t)(dTs), (*C.double)(dVals), (*C.uint32_t)(dCounts),
		(*C.int32_t)(dErrs), C.uint32_t(nseries), C.uint32_t(stride),
		C.int64_t(startNs), C.int64_t(stepNs), C.uint32_t(nsteps),
		C.int64_t(rangeNs), C.int(fn), C.double(param), (*C.double)(dOut),
		C.uint32_t(outPitch), (*C.int32_t)(dOutErrs), hipStream)
	if rc != 0 {
		return lastError()
	}
	return nil
}

// annRegionSize is the bytes one series' events need in an annotation
// region: the event count, one 12-byte table entry per event, the bytes.
func annRegionSize(evs []AnnotationEvent) uint64 {
	n := uint64(4)
	for _, ev := range evs {
		n += 12 + uint64(len(ev.Bytes))
	}
	return n
}

// buildAnnRegions lays every series' events out in the region layout of
// m3gpu.h (the one DecodeBatchAnn parses), annStride bytes per series. It
// returns an error, and writes nothing out of bounds, when a series' events
// do not fit annStride or their points are not strictly increasing and below
// the series' count.
func buildAnnRegions(
	anns [][]AnnotationEvent, counts []uint32, annStride uint32,
) ([]byte, error) {
	if annStride%4 != 0 || annStride < 16 {
		return nil, errors.New("m3gpu: annStride must be 4-aligned and >= 16")
	}
	region := make([]byte, uint64(len(anns))*uint64(annStride))
	le := binary.LittleEndian
	for i, evs := range anns {
		if annRegionSize(evs) > uint64(annStride) {
			return nil, errors.New("m3gpu: annotations do not fit annStride")
		}
		r := region[uint64(i)*uint64(annStride) : uint64(i+1)*uint64(annStride)]
		le.PutUint32(r[0:4], uint32(len(evs)))
		tail := annStride
		for j, ev := range evs {
			if ev.Point >= counts[i] || (j > 0 && ev.Point <= evs[j-1].Point) {
				return nil, errors.New("m3gpu: annotation points must be " +
					"strictly increasing and below the series' count")
			}
			tail -= uint32(len(ev.Bytes))
			copy(r[tail:], ev.Bytes)
			e := r[4+j*12 : 4+j*12+12]
			le.PutUint32(e[0:4], ev.Point)
			le.PutUint32(e[4:8], tail)
			le.PutUint32(e[8:12], uint32(len(ev.Bytes)))
		}
	}
	return region, nil
}

// EncodeBatchFull is the batched form of Encoder.Encode(dp, tu, ant)
// (dbnode/encoding/m3tsz/encoder.go:90; timestamp_encoder.go:72-195): like
// EncodeBatch, with each point's own time unit, per-series annotation
// events (what DecodeBatchAnn returns can be passed back unchanged) and an
// explicit block start per series. units (len n*stride), startNs (len n)
// and anns (len n) may each be nil: default unit for every point, start =
// first timestamp, no annotations. outStride must hold the worst case given
// in m3gpu.h (EncodeBatch's bound, plus 7 bytes + len per annotation, plus
// 11 bytes per unit change).
func EncodeBatchFull(
	ts []int64, vals []float64, counts []uint32,
	units []byte, startNs []int64, anns [][]AnnotationEvent,
	stride uint32, intOptimized bool, defaultUnit byte, outStride uint32,
) (streams []byte, lens []uint32, errs []SeriesError, err error) {
	n := uint32(len(counts))
	if n == 0 {
		return nil, nil, nil, nil
	}
	npts := uint64(n) * uint64(stride)
	if uint64(len(ts)) < npts || uint64(len(vals)) < npts ||
		(units != nil && uint64(len(units)) < npts) ||
		(startNs != nil && uint32(len(startNs)) < n) ||
		(anns != nil && uint32(len(anns)) != n) {
		return nil, nil, nil, errors.New("m3gpu: input slices shorter than the batch")
	}
	var unitsPtr *C.uint8_t
	if units != nil {
		unitsPtr = (*C.uint8_t)(unsafe.Pointer(&units[0]))
	}
	var startPtr *C.int64_t
	if startNs != nil {
		startPtr = (*C.int64_t)(unsafe.Pointer(&startNs[0]))
	}
	var annPtr *C.uint8_t
	annStride := uint32(0)
	if anns != nil {
		need := uint64(16)
		for _, evs := range anns {
			if s := annRegionSize(evs); s > need {
				need = s
			}
		}
		if need > 1<<31 {
			return nil, nil, nil, errors.New("m3gpu: annotations too large")
		}
		annStride = (uint32(need) + 3) &^ 3
		region, rerr := buildAnnRegions(anns, counts, annStride)
		if rerr != nil {
			return nil, nil, nil, rerr
		}
		annPtr = (*C.uint8_t)(unsafe.Pointer(&region[0]))
	}
	streams = make([]byte, uint64(n)*uint64(outStride))
	lens = make([]uint32, n)
	errs = make([]SeriesError, n)
	intOpt := C.int(0)
	if intOptimized {
		intOpt = 1
	}
	rc := C.m3gpu_encode_batch_full(
		(*C.int64_t)(unsafe.Pointer(&ts[0])),
		(*C.double)(unsafe.Pointer(&vals[0])),
		(*C.uint32_t)(unsafe.Pointer(&counts[0])),
		unitsPtr, startPtr, annPtr, C.uint32_t(annStride),
		C.uint32_t(n), C.uint32_t(stride), intOpt, C.uint8_t(defaultUnit),
		(*C.uint8_t)(unsafe.Pointer(&streams[0])), C.uint32_t(outStride),
		(*C.uint32_t)(unsafe.Pointer(&lens[0])),
		(*C.int32_t)(unsafe.Pointer(&errs[0])))
	if rc != 0 {
		return nil, nil, nil, lastError()
	}
	return streams, lens, errs, nil
}
