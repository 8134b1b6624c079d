"""Full encode (m3gpu_encode_batch_full*): the parts that need no GPU — the
annotation region builder, the argument checks that return before any HIP
call, and the exported symbols."""
import ctypes

import numpy as np
import pytest

from m3_amd import engine

pytestmark = pytest.mark.skipif(not engine.engine_available(),
                                reason="libm3gpu.so not built")

M3GPU_ERR_BADARG = -2


def test_ann_region_round_trip():
    events = [(0, b"\x00"), (3, b"\xff\x00\xfe" * 11), (4, b""),
              (9, bytes(range(256)))]
    stride = engine.ann_region_size(events)
    assert stride % 4 == 0 and stride >= 16
    for s in (stride, stride + 4, stride + 64):
        region = engine.build_ann_region(events, s)
        assert region.dtype == np.uint8 and region.shape == (s,)
        assert engine.parse_ann_region(region) == events
    # every event's bytes lie inside the region, behind the event table
    region = engine.build_ann_region(events, stride)
    table = region[:4 + 12 * len(events)].view(np.uint32)
    assert table[0] == len(events)
    for i in range(len(events)):
        point, off, ln = (int(x) for x in table[1 + 3 * i: 4 + 3 * i])
        assert 4 + 12 * len(events) <= off and off + ln <= stride


def test_ann_region_empty():
    region = engine.build_ann_region([], 16)
    assert engine.parse_ann_region(region) == []
    assert not region.any()


def test_ann_region_overflow_raises():
    events = [(0, b"abcd"), (1, b"efghijkl")]
    need = 4 + 12 * 2 + 12  # 40
    engine.build_ann_region(events, need)
    with pytest.raises(ValueError):
        engine.build_ann_region(events, need - 4)
    with pytest.raises(ValueError):
        engine.build_ann_region([(0, b"x" * 13)], 28)  # 4 + 12 + 13 = 29


def test_ann_region_rejects_bad_input():
    with pytest.raises(ValueError):
        engine.build_ann_region([(2, b"a"), (2, b"b")], 64)
    with pytest.raises(ValueError):
        engine.build_ann_region([(3, b"a"), (1, b"b")], 64)
    with pytest.raises(ValueError):
        engine.build_ann_region([], 18)
    with pytest.raises(ValueError):
        engine.build_ann_region([], 12)


def test_new_symbols_exported():
    L = engine.lib()
    for sym in ("m3gpu_encode_batch_full_dev", "m3gpu_encode_batch_full"):
        assert hasattr(L, sym), sym
    for name in ("encode_batch_full_dev", "encode_batch_full",
                 "build_ann_region"):
        assert callable(getattr(engine, name))


def _full_dev(ann, ann_stride, out_stride):
    """m3gpu_encode_batch_full_dev with nseries = 1 and argument values the
    checks must reject before anything dereferences a pointer."""
    L = engine.lib()
    fake = ctypes.c_void_p(4096)  # never dereferenced: BADARG returns first
    return L.m3gpu_encode_batch_full_dev(
        fake, fake, fake, None, None, ann, ann_stride, 1, 8, 1, 1,
        fake, out_stride, fake, fake, None)


@pytest.mark.parametrize("ann,ann_stride,out_stride,msg", [
    (None, 0, 252, "out_stride"),                    # out_stride % 8 != 0
    (ctypes.c_void_p(4096), 18, 256, "ann_stride"),  # ann_stride % 4 != 0
    (ctypes.c_void_p(4096), 12, 256, "ann_stride"),  # ann_stride < 16
    (ctypes.c_void_p(4096), 0, 256, "ann_stride"),   # regions, ann_stride 0
    (None, 16, 256, "ann_stride"),                   # no regions, stride != 0
])
def test_full_dev_badarg(ann, ann_stride, out_stride, msg):
    L = engine.lib()
    assert _full_dev(ann, ann_stride, out_stride) == M3GPU_ERR_BADARG
    assert msg in L.m3gpu_last_error().decode()


def test_full_host_badarg():
    """The host form checks the same rules before it allocates anything."""
    ts = np.zeros((1, 8), np.int64)
    vals = np.zeros((1, 8), np.float64)
    counts = np.ones(1, np.uint32)
    with pytest.raises(engine.M3GpuError, match="out_stride"):
        engine.encode_batch_full(ts, vals, counts, out_stride=252)
    with pytest.raises(engine.M3GpuError, match="ann_stride"):
        engine.encode_batch_full(ts, vals, counts,
                                 ann=np.zeros((1, 12), np.uint8))
