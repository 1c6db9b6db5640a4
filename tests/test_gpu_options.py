"""GPU: gcn10_gpu_set_option value by value, what "defaults" and gcn10_gpu_tune_single_raster do to the launch shape
of the strips, and the return codes of the context's memory, stream and event wrappers for null and empty arguments.
Needs an MI355X (a context), launches almost nothing.

The accepted ranges are those of include/gcn10_gpu.h; the codes are the ones the library returned before
gcn10_gpu_set_option became a table (this module was run against that library first).
"""
import ctypes as C

import numpy as np
import pytest

from gcn10_amd import gpu
from tests.test_gpu_strip_choice import Strips

pytestmark = pytest.mark.gpu

OK, E_INVAL = 0, -1
ONE, ALL = 0x004, 0x1FF
DEFAULT_ONE = "cn_strip_kernel<1, 3, true, 2, true, true>"
DEFAULT_ALL = "cn_strip_kernel<0, 3, true, 1, true, true>"      # 18 store streams: one sub-chunk per trip

# name: (lowest accepted, highest accepted, further accepted values, further refused values)
OPTIONS = {
    "grid_blocks_per_cu": (1, 64, (16,), ()),
    "ilp16": (0, 2, (1,), ()),
    "ilp1": (1, 4, (2,), (3,)),
    "nontemporal": (0, 1, (), ()),
    "xcd_slabs": (0, 1, (), ()),
    "prefetch": (-1, 1, (0,), ()),
    "compact_soil": (0, 1, (), ()),
    "deflate_wave_codes": (0, 1, (), ()),
    "arena_segment_align": (16, 4096, (32, 256, 2048), (0, 17, 48, 4095, 4097, 1 << 20)),
    "fused_emit": (0, 1, (), ()),
    "fused_parse": (0, 1, (), ()),
    "event_sync_sleep_us": (0, 100000, (50,), ()),
}


@pytest.fixture
def eng9(engine, tables):
    engine.set_tables(tables)
    yield engine
    engine.set_option("defaults", 0)


@pytest.fixture
def strips(eng9, tables):
    s = Strips(eng9, tables)
    yield s
    s.close()


def set_option(eng, name, value):
    return gpu.lib().gcn10_gpu_set_option(eng._ctx, name, value)


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_accepted_and_refused_values(eng9, name):
    lo, hi, more_ok, more_bad = OPTIONS[name]
    for v in (lo, hi) + more_ok:
        assert set_option(eng9, name.encode(), v) == OK, "%s=%d" % (name, v)
    for v in (lo - 1, hi + 1, -2 ** 31, 2 ** 31 - 1) + more_bad:
        assert set_option(eng9, name.encode(), v) == E_INVAL, "%s=%d" % (name, v)
        msg = gpu.lib().gcn10_gpu_last_error().decode()
        assert "gcn10_gpu_set_option" in msg and "%s=%d" % (name, v) in msg, msg


def test_unknown_and_null_names(eng9):
    assert set_option(eng9, b"no_such_option", 1) == E_INVAL
    assert set_option(eng9, b"", 1) == E_INVAL
    assert set_option(eng9, b"ilp", 1) == E_INVAL               # a prefix of two names
    assert set_option(eng9, None, 1) == E_INVAL
    assert gpu.lib().gcn10_gpu_set_option(None, b"ilp1", 1) == E_INVAL
    for v in (0, 1, -7):
        assert set_option(eng9, b"defaults", v) == OK


def launch(strips, table):
    """One strip of the 1040-wide tile with the options as they are (Strips.run would reset them); its kernel."""
    eng, t = strips.eng, strips.tile("1040")
    t.prepare()
    ptrs = [strips.arena.at(r * strips.slot) for r in range(18)]
    eng.cn_strip(t.bufs[0].ptr, t.W, 3, t.bufs[3].ptr, 3, table, ptrs)
    eng.sync()
    return eng.last_kernel_name()


def test_defaults_restores_the_strip_kernels(strips):
    eng = strips.eng
    assert (launch(strips, ONE), launch(strips, ALL)) == (DEFAULT_ONE, DEFAULT_ALL)
    for name, v in (("grid_blocks_per_cu", 3), ("ilp16", 2), ("ilp1", 4), ("nontemporal", 0), ("xcd_slabs", 0),
                    ("prefetch", 0), ("compact_soil", 0)):
        eng.set_option(name, v)
    assert launch(strips, ONE) == "cn_strip_kernel<1, 3, true, 4, false, false>"
    assert launch(strips, ALL) == "cn_strip_kernel<0, 3, true, 2, false, false>"
    assert eng.soil_words_state() == 0
    eng.set_option("defaults", 0)
    assert (launch(strips, ONE), launch(strips, ALL)) == (DEFAULT_ONE, DEFAULT_ALL)
    assert eng.soil_words_state() == 1
    # and the rasters are right under the restored options
    assert strips.run(dict(tile="1040", table=ONE)) == DEFAULT_ONE


def tune(strips, W=1040):
    """gcn10_gpu_tune_single_raster over two candidate positions of a tiny arena; (rc, report or None)."""
    eng, t = strips.eng, strips.tile("1040")
    t.prepare()
    npix, step = 1040 * 3, 256
    best, ms, rep = C.c_void_p(), C.c_float(), C.create_string_buffer(512)
    rc = gpu.lib().gcn10_gpu_tune_single_raster(eng._ctx, t.bufs[0].ptr, W, 3, t.bufs[3].ptr, 1, ONE, strips.arena.ptr,
                                                npix + step, step, C.byref(best), C.byref(ms), rep, 512, None)
    eng.sync()
    if rc != OK:
        return rc, None
    import json
    report = json.loads(rep.value.decode())
    assert report["positions"] == 2 and best.value in (strips.arena.ptr, strips.arena.ptr + step)
    return rc, report


def shape_name(cond, ilp, pf):
    return "cn_strip_kernel<1, %d, true, %d, true, %s>" % (cond, ilp, "true" if pf and ilp <= 2 else "false")


def test_ilp1_replaces_a_calibrated_shape(strips):
    eng = strips.eng
    rc, report = tune(strips)
    assert rc == OK
    assert launch(strips, ONE) == shape_name(3, report["ilp1"], report["prefetch"])
    other = 4 if report["ilp1"] != 4 else 1
    eng.set_option("ilp1", other)
    assert launch(strips, ONE) == shape_name(3, other, 1)       # the context's own prefetch option again
    assert launch(strips, ALL) == DEFAULT_ALL


def test_a_refused_tune_leaves_the_shape_as_it_was(strips):
    """W = 1056 is not the prepared tile's width: the first strip of the calibration is refused, after the candidate
    shape was put into the context."""
    eng = strips.eng
    eng.set_option("ilp1", 4)
    eng.set_option("prefetch", 0)
    before = launch(strips, ONE)
    assert before == shape_name(3, 4, 0)
    assert tune(strips, W=1056) == (E_INVAL, None)
    assert "gcn10_gpu_cn_strip" in gpu.lib().gcn10_gpu_last_error().decode()
    assert launch(strips, ONE) == before
    # the same with a calibrated shape in place
    rc, report = tune(strips)
    assert rc == OK
    tuned = launch(strips, ONE)
    assert tuned == shape_name(3, report["ilp1"], report["prefetch"])
    assert tune(strips, W=1056) == (E_INVAL, None)
    assert launch(strips, ONE) == tuned
    # and arguments refused before anything is touched
    L, t = gpu.lib(), strips.tile("1040")
    best = C.c_void_p()
    for cond, table, arena, nbytes, step in ((3, ONE, strips.arena.ptr, 4096, 256), (1, 0x005, strips.arena.ptr, 4096, 256),
                                             (1, ONE, None, 4096, 256), (1, ONE, strips.arena.ptr, 3119, 256),
                                             (1, ONE, strips.arena.ptr, 4096, 0), (1, ONE, strips.arena.ptr, 4096, 100),
                                             (1, ONE, strips.arena.ptr + 1, 4096, 256)):
        assert L.gcn10_gpu_tune_single_raster(eng._ctx, t.bufs[0].ptr, 1040, 3, t.bufs[3].ptr, cond, table, arena, nbytes,
                                              step, C.byref(best), None, None, 0, None) == E_INVAL
    assert launch(strips, ONE) == tuned


# ---- the wrappers: null and empty arguments ------------------------------------------------------------------------

def test_memory_wrappers(engine):
    L, c = gpu.lib(), engine._ctx
    p = C.c_void_p()
    for fn, free in ((L.gcn10_gpu_malloc, L.gcn10_gpu_free), (L.gcn10_gpu_host_alloc, L.gcn10_gpu_host_free)):
        assert fn(None, 16, C.byref(p)) == E_INVAL
        assert fn(c, 16, None) == E_INVAL
        assert fn(c, 0, C.byref(p)) == OK and p.value       # an empty allocation is a valid pointer
        assert free(c, p) == OK
        assert free(c, None) == OK
        assert free(None, None) == E_INVAL
    host = np.arange(32, dtype=np.uint8)
    dev = engine.alloc(32)
    try:
        for fn, dst, src in ((L.gcn10_gpu_memcpy_h2d, dev.ptr, host.ctypes.data),
                             (L.gcn10_gpu_memcpy_d2h, host.ctypes.data, dev.ptr)):
            assert fn(None, dst, src, 32, None) == E_INVAL
            assert fn(c, None, src, 32, None) == E_INVAL
            assert fn(c, dst, None, 32, None) == E_INVAL
            assert fn(c, None, None, 0, None) == OK
        assert L.gcn10_gpu_memset(None, dev.ptr, 0, 32, None) == E_INVAL
        assert L.gcn10_gpu_memset(c, None, 0, 32, None) == E_INVAL
        assert L.gcn10_gpu_memset(c, None, 0, 0, None) == OK
        assert L.gcn10_gpu_memset(c, dev.ptr, 7, 32, None) == OK
        assert (engine.download(dev.ptr, (32,)) == 7).all()
    finally:
        dev.close()


def test_stream_and_event_wrappers(engine):
    L, c = gpu.lib(), engine._ctx
    s, e = C.c_void_p(), C.c_void_p()
    ms = C.c_float()
    assert L.gcn10_gpu_stream_create(None, C.byref(s)) == E_INVAL
    assert L.gcn10_gpu_stream_create(c, None) == E_INVAL
    assert L.gcn10_gpu_stream_destroy(c, None) == OK
    assert L.gcn10_gpu_stream_sync(c, None) == OK               # the context's own stream
    assert L.gcn10_gpu_stream_sync(None, None) == E_INVAL
    assert L.gcn10_gpu_device_sync(None) == E_INVAL
    assert L.gcn10_gpu_event_create(None, C.byref(e)) == E_INVAL
    assert L.gcn10_gpu_event_create(c, None) == E_INVAL
    assert L.gcn10_gpu_event_destroy(c, None) == OK
    assert L.gcn10_gpu_event_record(c, None, None) == E_INVAL
    assert L.gcn10_gpu_event_sync(c, None) == E_INVAL
    assert L.gcn10_gpu_stream_wait_event(c, None, None) == E_INVAL
    e0, e1 = engine.event_create(), engine.event_create()
    try:
        assert L.gcn10_gpu_event_record(None, e0, None) == E_INVAL
        for a, b, out in ((None, e1, C.byref(ms)), (e0, None, C.byref(ms)), (e0, e1, None)):
            assert L.gcn10_gpu_event_elapsed_ms(c, a, b, out) == E_INVAL
        for a, b in ((None, e1), (e0, None)):
            assert L.gcn10_gpu_time_next_strip(c, a, b) == E_INVAL
        assert L.gcn10_gpu_time_next_strip(None, e0, e1) == E_INVAL
        # a good pair brackets the next launch that takes it, here a copy, and is used up by it
        src, dst = engine.upload(np.arange(4096, dtype=np.uint8)), engine.alloc(4096)
        try:
            assert L.gcn10_gpu_time_next_strip(c, e0, e1) == OK
            assert L.gcn10_gpu_stream_copy(c, src.ptr, dst.ptr, 4096, None) == OK
            assert L.gcn10_gpu_event_sync(c, e1) == OK
            assert L.gcn10_gpu_event_elapsed_ms(c, e0, e1, C.byref(ms)) == OK and ms.value >= 0.0
            assert (engine.download(dst.ptr, (4096,)) == np.arange(4096, dtype=np.uint8)).all()
            assert L.gcn10_gpu_stream_copy(c, None, None, 0, None) == OK
            for a, b, n in ((None, dst.ptr, 4096), (src.ptr, None, 4096), (src.ptr, dst.ptr, 4088),
                            (src.ptr + 1, dst.ptr, 4080), (src.ptr, dst.ptr + 8, 4080)):
                assert L.gcn10_gpu_stream_copy(c, a, b, n, None) == E_INVAL
            assert L.gcn10_gpu_stream_copy(None, src.ptr, dst.ptr, 4096, None) == E_INVAL
            engine.sync()
        finally:
            src.close()
            dst.close()
    finally:
        engine.event_destroy(e0)
        engine.event_destroy(e1)


def test_pci_bus_id(engine):
    L = gpu.lib()
    buf = C.create_string_buffer(32)
    assert L.gcn10_gpu_pci_bus_id(0, None, 32) == E_INVAL
    assert L.gcn10_gpu_pci_bus_id(0, buf, 12) == E_INVAL
    assert L.gcn10_gpu_pci_bus_id(0, buf, 13) == OK and buf.value.count(b":") == 2
