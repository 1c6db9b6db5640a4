"""ctypes face of ``libgcn10_gpu.so`` -- the C ABI of ``include/gcn10_gpu.h``.

Nothing here computes: every method forwards to the HIP library, and a missing
library or a missing gfx950 device raises (there is no CPU fallback, by design).
Device memory is owned through the ABI's own allocator, so neither this module
nor the tests need torch.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import host as _host

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GCN10_GPU_LIB") or os.path.join(_HERE, "libgcn10_gpu.so")
_lib = None

N_TABLES = 9
N_RASTERS = 18
COND_DRAINED = 1
COND_UNDRAINED = 2
ALL_TABLES = 0x1FF
NODATA = 255

#: every symbol include/gcn10_gpu.h declares (checked by the CPU test-suite)
ABI_SYMBOLS = (
    "gcn10_gpu_abi_version", "gcn10_gpu_device_count", "gcn10_gpu_init", "gcn10_gpu_destroy",
    "gcn10_gpu_last_error", "gcn10_gpu_device_info", "gcn10_gpu_malloc", "gcn10_gpu_free",
    "gcn10_gpu_host_alloc", "gcn10_gpu_host_free", "gcn10_gpu_memcpy_h2d",
    "gcn10_gpu_memcpy_d2h", "gcn10_gpu_memset", "gcn10_gpu_stream_create",
    "gcn10_gpu_stream_destroy", "gcn10_gpu_stream_sync", "gcn10_gpu_device_sync",
    "gcn10_gpu_event_create", "gcn10_gpu_event_destroy", "gcn10_gpu_event_record",
    "gcn10_gpu_event_sync", "gcn10_gpu_stream_wait_event", "gcn10_gpu_event_elapsed_ms",
    "gcn10_gpu_set_tables", "gcn10_gpu_resample", "gcn10_gpu_modify_hysogs_data",
    "gcn10_gpu_calculate_cn", "gcn10_gpu_prepare_tile", "gcn10_gpu_cn_strip",
    "gcn10_gpu_strip_algorithmic_bytes", "gcn10_gpu_last_kernel_name", "gcn10_gpu_set_option",
    "gcn10_gpu_deflate_arena_bound", "gcn10_gpu_deflate_strip", "gcn10_gpu_time_next_strip",
    "gcn10_gpu_pci_bus_id", "gcn10_gpu_deflate_fused_strip",
    "gcn10_gpu_deflate_fused_available",
    "gcn10_gpu_inflate_tiles", "gcn10_gpu_stream_copy", "gcn10_gpu_tune_single_raster",
    "gcn10_gpu_soil_words_state", "gcn10_gpu_lzw_arena_bound", "gcn10_gpu_lzw_strip",
    "gcn10_gpu_inflate_codecs", "gcn10_gpu_overview_nearest", "gcn10_gpu_overview_average",
    "gcn10_gpu_pair_histogram_codes", "gcn10_gpu_pair_histogram",
    "gcn10_gpu_verify_strip", "gcn10_gpu_verify_buffers", "gcn10_gpu_zonal_pair_histogram",
    "gcn10_gpu_aggregate", "gcn10_gpu_grid_sums", "gcn10_gpu_grid_finish",
    "gcn10_gpu_set_weights", "gcn10_gpu_grid_sums_weighted", "gcn10_gpu_grid_finish_weighted",
    "gcn10_gpu_set_weight_tables", "gcn10_gpu_grid_sums_storms", "gcn10_gpu_grid_finish_storms",
    "gcn10_gpu_grid_rain_item", "gcn10_gpu_set_rain_tables", "gcn10_gpu_grid_sums_rain", "gcn10_gpu_grid_finish_rain",
    "gcn10_gpu_zonal_sums_rain", "gcn10_gpu_grid_sums_rains", "gcn10_gpu_grid_finish_rains",
    "gcn10_gpu_zonal_sums_rains", "gcn10_gpu_set_cell_byte_tables", "gcn10_gpu_runoff_strip",
)


def grid_rain_item():
    """(columns, rows) of an item of the rain sums, the most a wave counts in one histogram
    (gcn10_gpu_grid_rain_item; no device needed)."""
    cols, rows = C.c_int(0), C.c_int(0)
    n = lib().gcn10_gpu_grid_rain_item(C.byref(cols), C.byref(rows))
    if n != cols.value * rows.value:
        raise RuntimeError("gcn10_gpu_grid_rain_item returned %d" % n)
    return cols.value, rows.value


def pair_histogram_codes() -> np.ndarray:
    """codes[b] = the soil code byte (drained plane | undrained plane << 4) counted in bin b of the pair histogram
    (gcn10_gpu_pair_histogram_codes; no device needed)."""
    codes = np.zeros(PAIR_HIST_BINS, np.uint8)
    n = lib().gcn10_gpu_pair_histogram_codes(codes.ctypes.data_as(C.POINTER(C.c_uint8)))
    if n != PAIR_HIST_BINS:
        raise RuntimeError("gcn10_gpu_pair_histogram_codes returned %d" % n)
    return codes


# struct gcn10_inflate_tile (include/gcn10_gpu.h)
TILE_RAW, TILE_PREDICTOR2, TILE_LZW = 1, 2, 4     # gcn10_inflate_tile.flags (include/gcn10_gpu.h)
CODEC_DEFLATE, CODEC_RAW, CODEC_LZW = 1, 2, 4       # gcn10_gpu_inflate_codecs() bits
PAIR_HIST_BINS = 16                                 # GCN10_PAIR_HIST_BINS: pair histogram = [bin][landcover] counters
# gcn10_inflate_tiles status words of LZW tiles (GCN10_INFLATE_E_LZW_*)
INFLATE_E_LZW_CODE, INFLATE_E_LZW_FIRST, INFLATE_E_LZW_INPUT = 9, 10, 11
# struct gcn10_verify_count (include/gcn10_gpu.h); first == VERIFY_NONE: nothing differs
VERIFY_COUNT_DTYPE = np.dtype([("mismatches", "<u8"), ("first", "<u8"), ("want", "<u4"), ("got", "<u4")])
VERIFY_NONE = 0xFFFFFFFFFFFFFFFF
INFLATE_TILE_DTYPE = np.dtype([("in_off", "<u8"), ("in_len", "<u4"), ("out_len", "<u4"), ("chunk_w", "<u4"),
                               ("src_x", "<u4"), ("src_y", "<u4"), ("copy_w", "<u4"), ("copy_h", "<u4"),
                               ("flags", "<u4"), ("dst_off", "<u8")])


class Gcn10GpuError(RuntimeError):
    def __init__(self, code: int, where: str, message: str):
        super().__init__("%s failed (%d): %s" % (where, code, message))
        self.code = code


def lib():
    """Loads the HIP library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s is missing: run `make gpu` (or __graft_entry__.build()); "
                          "there is no CPU fallback for the CN path" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, i, sz, u = C.c_void_p, C.c_int, C.c_size_t, C.c_uint
        sig = {
            "gcn10_gpu_abi_version": (i, []),
            "gcn10_gpu_device_count": (i, []),
            "gcn10_gpu_init": (i, [i, C.POINTER(vp)]),
            "gcn10_gpu_destroy": (None, [vp]),
            "gcn10_gpu_last_error": (C.c_char_p, []),
            "gcn10_gpu_device_info": (i, [vp, C.c_char_p, sz, C.POINTER(sz)]),
            "gcn10_gpu_malloc": (i, [vp, sz, C.POINTER(vp)]),
            "gcn10_gpu_free": (i, [vp, vp]),
            "gcn10_gpu_host_alloc": (i, [vp, sz, C.POINTER(vp)]),
            "gcn10_gpu_host_free": (i, [vp, vp]),
            "gcn10_gpu_memcpy_h2d": (i, [vp, vp, vp, sz, vp]),
            "gcn10_gpu_memcpy_d2h": (i, [vp, vp, vp, sz, vp]),
            "gcn10_gpu_memset": (i, [vp, vp, i, sz, vp]),
            "gcn10_gpu_stream_create": (i, [vp, C.POINTER(vp)]),
            "gcn10_gpu_stream_destroy": (i, [vp, vp]),
            "gcn10_gpu_stream_sync": (i, [vp, vp]),
            "gcn10_gpu_device_sync": (i, [vp]),
            "gcn10_gpu_event_create": (i, [vp, C.POINTER(vp)]),
            "gcn10_gpu_event_destroy": (i, [vp, vp]),
            "gcn10_gpu_event_record": (i, [vp, vp, vp]),
            "gcn10_gpu_event_sync": (i, [vp, vp]),
            "gcn10_gpu_stream_wait_event": (i, [vp, vp, vp]),
            "gcn10_gpu_event_elapsed_ms": (i, [vp, vp, vp, C.POINTER(C.c_float)]),
            "gcn10_gpu_set_tables": (i, [vp, vp, i]),
            "gcn10_gpu_resample": (i, [vp, vp, i, i, vp, vp, i, i, vp, vp]),
            "gcn10_gpu_modify_hysogs_data": (i, [vp, vp, sz, i, vp]),
            "gcn10_gpu_calculate_cn": (i, [vp, vp, vp, sz, i, vp, vp]),
            "gcn10_gpu_prepare_tile": (i, [vp, vp, i, i, vp, i, vp]),
            "gcn10_gpu_cn_strip": (i, [vp, vp, i, i, vp, u, u, C.POINTER(vp), vp]),
            "gcn10_gpu_strip_algorithmic_bytes": (sz, [i, i, i, i, u, u]),
            "gcn10_gpu_last_kernel_name": (C.c_char_p, [vp]),
            "gcn10_gpu_set_option": (i, [vp, C.c_char_p, i]),
            "gcn10_gpu_time_next_strip": (i, [vp, vp, vp]),
            "gcn10_gpu_stream_copy": (i, [vp, vp, vp, sz, vp]),
            "gcn10_gpu_tune_single_raster": (i, [vp, vp, i, i, vp, u, u, vp, sz, sz, C.POINTER(vp),
                                                 C.POINTER(C.c_float), C.c_char_p, sz, vp]),
            "gcn10_gpu_pci_bus_id": (i, [i, C.c_char_p, sz]),
            "gcn10_gpu_soil_words_state": (i, [vp, vp]),
            "gcn10_gpu_deflate_fused_strip": (i, [vp, vp, i, i, vp, u, u, vp, sz, vp, vp, vp]),
            "gcn10_gpu_deflate_fused_available": (i, [vp]),
            "gcn10_gpu_inflate_tiles": (i, [vp, vp, vp, i, u, vp, sz, vp, vp]),
            "gcn10_gpu_inflate_codecs": (i, []),
            "gcn10_gpu_deflate_arena_bound": (sz, [i, i, i]),
            "gcn10_gpu_deflate_strip": (i, [vp, vp, i, i, i, vp, sz, vp, vp, vp]),
            "gcn10_gpu_lzw_arena_bound": (sz, [i, i, i]),
            "gcn10_gpu_lzw_strip": (i, [vp, vp, i, i, i, vp, sz, vp, vp, vp]),
            "gcn10_gpu_overview_nearest": (i, [vp, vp, i, i, i, vp, vp]),
            "gcn10_gpu_overview_average": (i, [vp, vp, i, i, i, i, vp, u, u, i, C.POINTER(vp), vp]),
            "gcn10_gpu_pair_histogram_codes": (i, [C.POINTER(C.c_uint8)]),
            "gcn10_gpu_pair_histogram": (i, [vp, vp, i, i, vp, vp, vp]),
            "gcn10_gpu_verify_strip": (i, [vp, vp, i, i, vp, C.c_uint, C.c_uint, vp, sz, i, vp, vp]),
            "gcn10_gpu_verify_buffers": (i, [vp, vp, sz, vp, sz, i, i, i, C.c_uint, vp, vp]),
            "gcn10_gpu_zonal_pair_histogram": (i, [vp, vp, i, i, vp, vp, vp, sz, i, vp, vp]),
            "gcn10_gpu_aggregate": (i, [vp, vp, i, i, vp, i, i, i, u, u, C.POINTER(vp), sz, vp]),
            "gcn10_gpu_grid_sums": (i, [vp, vp, i, i, vp, vp, vp, i, i, u, u, vp, vp]),
            "gcn10_gpu_grid_finish": (i, [vp, vp, i, sz, vp, vp, C.c_uint32, vp, vp]),
            "gcn10_gpu_set_weights": (i, [vp, vp]),
            "gcn10_gpu_grid_sums_weighted": (i, [vp, vp, i, i, vp, vp, vp, i, i, u, u, vp, vp]),
            "gcn10_gpu_grid_finish_weighted": (i, [vp, vp, i, sz, vp, vp, vp, C.c_uint32, vp, vp]),
            "gcn10_gpu_set_weight_tables": (i, [vp, vp, i]),
            "gcn10_gpu_grid_sums_storms": (i, [vp, vp, i, i, vp, vp, vp, i, i, u, u, vp, vp]),
            "gcn10_gpu_grid_finish_storms": (i, [vp, vp, i, sz, vp, vp, vp, C.c_uint32, vp, vp]),
            "gcn10_gpu_grid_rain_item": (i, [C.POINTER(i), C.POINTER(i)]),
            "gcn10_gpu_set_rain_tables": (i, [vp, vp, i]),
            "gcn10_gpu_grid_sums_rain": (i, [vp, vp, i, i, vp, vp, vp, i, i, u, u, vp, vp, vp]),
            "gcn10_gpu_grid_finish_rain": (i, [vp, vp, i, sz, vp, vp, vp, vp, C.c_uint32, vp, vp]),
            "gcn10_gpu_zonal_sums_rain": (i, [vp, vp, i, i, vp, vp, vp, sz, i, u, u, vp, vp]),
            "gcn10_gpu_zonal_sums_rains": (i, [vp, vp, i, i, vp, vp, vp, sz, i, u, u, i, vp, vp]),
            "gcn10_gpu_grid_sums_rains": (i, [vp, vp, i, i, vp, vp, vp, i, i, u, u, vp, i, vp, vp]),
            "gcn10_gpu_grid_finish_rains": (i, [vp, vp, i, sz, vp, i, vp, vp, vp, C.c_uint32, vp, vp]),
            "gcn10_gpu_set_cell_byte_tables": (i, [vp, vp, i]),
            "gcn10_gpu_runoff_strip": (i, [vp, vp, i, i, vp, vp, vp, i, i, vp, u, u, C.POINTER(vp), vp]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def device_count() -> int:
    return int(lib().gcn10_gpu_device_count())


def strip_algorithmic_bytes(W: int, rows: int, hsx: int, hsy: int, cond_mask: int,
                            table_mask: int) -> int:
    return int(lib().gcn10_gpu_strip_algorithmic_bytes(W, rows, hsx, hsy, cond_mask, table_mask))


class DevBuf:
    """A device allocation made through the C ABI (freed with the engine or on close())."""

    def __init__(self, eng: "Engine", nbytes: int):
        self.eng = eng
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        eng._chk(lib().gcn10_gpu_malloc(eng._ctx, self.nbytes, C.byref(p)), "gcn10_gpu_malloc")
        self.ptr = p.value or 0
        eng._bufs.append(self)

    def at(self, offset: int) -> int:
        assert 0 <= offset <= self.nbytes
        return self.ptr + offset

    def close(self):
        if self.ptr:
            lib().gcn10_gpu_free(self.eng._ctx, self.ptr)
            self.ptr = 0
            if self in self.eng._bufs:
                self.eng._bufs.remove(self)


class Engine:
    """One GPU context (``gcn10_gpu_ctx``): the device-side stand-in of one MPI rank."""

    def __init__(self, device: int = 0):
        self._ctx = C.c_void_p()
        self._bufs = []
        rc = lib().gcn10_gpu_init(device, C.byref(self._ctx))
        if rc != 0:
            self._ctx = C.c_void_p()
            raise Gcn10GpuError(rc, "gcn10_gpu_init", lib().gcn10_gpu_last_error().decode())
        self.device = device
        self.n_tables = 0

    # -- plumbing ---------------------------------------------------------
    def _chk(self, rc: int, where: str):
        if rc != 0:
            raise Gcn10GpuError(rc, where, lib().gcn10_gpu_last_error().decode())

    def close(self):
        if self._ctx:
            for b in list(self._bufs):
                b.close()
            lib().gcn10_gpu_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_info(self):
        name = C.create_string_buffer(256)
        hbm = C.c_size_t()
        cus = lib().gcn10_gpu_device_info(self._ctx, name, 256, C.byref(hbm))
        if cus < 0:
            self._chk(cus, "gcn10_gpu_device_info")
        return {"name": name.value.decode(), "cus": cus, "hbm_bytes": hbm.value}

    def pci_bus_id(self) -> str:
        """PCI bus id of this engine's device, e.g. 0000:05:00.0."""
        buf = C.create_string_buffer(32)
        self._chk(lib().gcn10_gpu_pci_bus_id(self.device, buf, 32), "gcn10_gpu_pci_bus_id")
        return buf.value.decode()

    def alloc(self, nbytes: int) -> DevBuf:
        return DevBuf(self, nbytes)

    def upload(self, arr: np.ndarray, stream=None) -> DevBuf:
        a = np.ascontiguousarray(arr)
        buf = DevBuf(self, max(a.nbytes, 1))
        self.h2d(buf.ptr, a, stream)
        self.sync(stream)
        return buf

    def h2d(self, dptr: int, arr: np.ndarray, stream=None):
        a = np.ascontiguousarray(arr)
        self._chk(lib().gcn10_gpu_memcpy_h2d(self._ctx, dptr, a.ctypes.data, a.nbytes, stream),
                  "gcn10_gpu_memcpy_h2d")

    def download(self, dptr: int, shape, dtype=np.uint8, stream=None) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        if out.nbytes:
            self._chk(lib().gcn10_gpu_memcpy_d2h(self._ctx, out.ctypes.data, dptr, out.nbytes,
                                                 stream), "gcn10_gpu_memcpy_d2h")
        self.sync(stream)
        return out

    def memset(self, dptr: int, value: int, nbytes: int, stream=None):
        self._chk(lib().gcn10_gpu_memset(self._ctx, dptr, value, nbytes, stream), "gcn10_gpu_memset")

    def sync(self, stream=None):
        self._chk(lib().gcn10_gpu_stream_sync(self._ctx, stream), "gcn10_gpu_stream_sync")

    def device_sync(self):
        self._chk(lib().gcn10_gpu_device_sync(self._ctx), "gcn10_gpu_device_sync")

    def stream_create(self) -> int:
        s = C.c_void_p()
        self._chk(lib().gcn10_gpu_stream_create(self._ctx, C.byref(s)), "gcn10_gpu_stream_create")
        return s.value

    def stream_destroy(self, s):
        self._chk(lib().gcn10_gpu_stream_destroy(self._ctx, s), "gcn10_gpu_stream_destroy")

    def event_create(self) -> int:
        e = C.c_void_p()
        self._chk(lib().gcn10_gpu_event_create(self._ctx, C.byref(e)), "gcn10_gpu_event_create")
        return e.value

    def event_destroy(self, e):
        self._chk(lib().gcn10_gpu_event_destroy(self._ctx, e), "gcn10_gpu_event_destroy")

    def event_record(self, e, stream=None):
        self._chk(lib().gcn10_gpu_event_record(self._ctx, e, stream), "gcn10_gpu_event_record")

    def event_sync(self, e):
        self._chk(lib().gcn10_gpu_event_sync(self._ctx, e), "gcn10_gpu_event_sync")

    def stream_wait_event(self, stream, e):
        self._chk(lib().gcn10_gpu_stream_wait_event(self._ctx, stream, e),
                  "gcn10_gpu_stream_wait_event")

    def elapsed_ms(self, e0, e1) -> float:
        ms = C.c_float()
        self._chk(lib().gcn10_gpu_event_elapsed_ms(self._ctx, e0, e1, C.byref(ms)),
                  "gcn10_gpu_event_elapsed_ms")
        return float(ms.value)

    def set_option(self, name: str, value: int):
        self._chk(lib().gcn10_gpu_set_option(self._ctx, name.encode(), int(value)),
                  "gcn10_gpu_set_option")

    def time_next_strip(self, e0, e1):
        self._chk(lib().gcn10_gpu_time_next_strip(self._ctx, e0, e1), "gcn10_gpu_time_next_strip")

    def tune_single_raster(self, esa, W: int, rows: int, cj, cond_mask: int, table_mask: int, arena, arena_bytes: int,
                           step: int = 16 << 20, stream=None):
        """gcn10_gpu_tune_single_raster: (best raster pointer inside the arena, best ms, report dict)."""
        import json as _json
        best = C.c_void_p()
        ms = C.c_float()
        rep = C.create_string_buffer(512)
        self._chk(lib().gcn10_gpu_tune_single_raster(self._ctx, esa, W, rows, cj, cond_mask, table_mask, arena,
                                                     int(arena_bytes), int(step), C.byref(best), C.byref(ms), rep, 512,
                                                     stream), "gcn10_gpu_tune_single_raster")
        return best.value, float(ms.value), _json.loads(rep.value.decode() or "{}")

    def stream_copy(self, src, dst, nbytes: int, stream=None):
        """Plain 1R:1W copy with the strip kernel's launch shape (the same-run streaming ceiling)."""
        self._chk(lib().gcn10_gpu_stream_copy(self._ctx, src, dst, int(nbytes), stream), "gcn10_gpu_stream_copy")

    def soil_words_state(self, stream=None) -> int:
        """What aligned strips of the prepared tile read: 0 = code bytes (option off), 1 = one column entry per lane,
        2 = the cell codes through the column map, pixel by pixel (a column group of the tile spans more than two soil cells); see
        include/gcn10_gpu.h."""
        rc = lib().gcn10_gpu_soil_words_state(self._ctx, stream)
        if rc < 0:
            self._chk(rc, "gcn10_gpu_soil_words_state")
        return rc

    def last_kernel_name(self) -> str:
        return lib().gcn10_gpu_last_kernel_name(self._ctx).decode()

    # -- the reference's functions ------------------------------------------
    def set_tables(self, tables: np.ndarray):
        """int32[n,256,5] reference-format tables (src/cn.c:148)."""
        t = np.ascontiguousarray(tables, dtype=np.int32)
        if t.ndim == 2:
            t = t[None]
        if t.ndim != 3 or t.shape[1:] != (256, 5):
            raise ValueError("tables must be int32[n,256,5]")
        self._chk(lib().gcn10_gpu_set_tables(self._ctx, t.ctypes.data, t.shape[0]),
                  "gcn10_gpu_set_tables")
        self.n_tables = t.shape[0]

    def resample(self, coarse_d: int, hsx: int, hsy: int, ci_d: int, cj_d: int, W: int,
                 rows: int, out_d: int, stream=None):
        self._chk(lib().gcn10_gpu_resample(self._ctx, coarse_d, hsx, hsy, ci_d, cj_d, W, rows,
                                           out_d, stream), "gcn10_gpu_resample")

    def modify_hysogs_data(self, h_d: int, npix: int, drained: bool, stream=None):
        self._chk(lib().gcn10_gpu_modify_hysogs_data(self._ctx, h_d, npix, int(bool(drained)),
                                                     stream), "gcn10_gpu_modify_hysogs_data")

    def calculate_cn(self, esa_d: int, hsg_d: int, npix: int, table_index: int, out_d: int,
                     stream=None):
        self._chk(lib().gcn10_gpu_calculate_cn(self._ctx, esa_d, hsg_d, npix, table_index, out_d,
                                               stream), "gcn10_gpu_calculate_cn")

    def prepare_tile(self, coarse_d: int, hsx: int, hsy: int, ci_d: int, W: int, stream=None):
        self._chk(lib().gcn10_gpu_prepare_tile(self._ctx, coarse_d, hsx, hsy, ci_d, W, stream),
                  "gcn10_gpu_prepare_tile")

    def cn_strip(self, esa_d: int, W: int, rows: int, cj_d: int, cond_mask: int, table_mask: int,
                 outs: Sequence[Optional[int]], stream=None):
        arr = (C.c_void_p * N_RASTERS)()
        for r in range(N_RASTERS):
            arr[r] = outs[r] if r < len(outs) and outs[r] else None
        self._chk(lib().gcn10_gpu_cn_strip(self._ctx, esa_d, W, rows, cj_d, cond_mask, table_mask,
                                           arr, stream), "gcn10_gpu_cn_strip")

    def set_cell_byte_tables(self, t):
        """k tables of 256 bytes ([k][256], 1 <= k <= 256) for runoff_strip, one of them named per cell
        (gcn10_gpu_set_cell_byte_tables).  Independent of set_tables and of the weight and rain tables.  Synchronous."""
        a = np.ascontiguousarray(t, np.uint8).reshape(-1, 256)
        self._chk(lib().gcn10_gpu_set_cell_byte_tables(self._ctx, a.ctypes.data, a.shape[0]),
                  "gcn10_gpu_set_cell_byte_tables")

    def runoff_strip(self, esa_d: int, W: int, rows: int, cj_d: int, cellx_ptr: int, celly_ptr: int, ncx: int, ncy: int,
                     cell_table_ptr: int, cond_mask: int, table_mask: int, outs: Sequence[Optional[int]], stream=None):
        """cn_strip with every value v sent through T[cell_table[celly[y]][cellx[x]]][v] of set_cell_byte_tables, 255
        where a map names no cell; cell_table_ptr: uint8[ncy][ncx] on the device (gcn10_gpu_runoff_strip).
        Asynchronous on `stream`."""
        arr = (C.c_void_p * N_RASTERS)()
        for r in range(N_RASTERS):
            arr[r] = outs[r] if r < len(outs) and outs[r] else None
        self._chk(lib().gcn10_gpu_runoff_strip(self._ctx, esa_d, W, rows, cj_d, cellx_ptr, celly_ptr, ncx, ncy,
                                               cell_table_ptr, cond_mask, table_mask, arr, stream),
                  "gcn10_gpu_runoff_strip")

    # -- output encode (src/raster.c:204-219 on the GPU) ----------------------
    def _encode_into_arena(self, launch, where: str, n: int, W: int, rows: int, cap: int, stream, poison: Optional[int],
                           guard: int, held=()):
        """The arena / table / cursor contract the three tile encoders share: launch(arena, cap, table, cursor) runs
        one of them.  Returns (arena bytes, table uint32[n, down, across, 2], used).  poison = a byte value (tests):
        the arena and `guard` bytes behind arena_cap are filled with it before the launch and the whole image of
        cap + guard bytes is returned instead of the bytes used."""
        across, down = (W + 255) // 256, (rows + 255) // 256
        image = cap + int(guard) if poison is not None else cap
        bufs = list(held)
        try:
            arena = self.alloc(max(image, 16))
            bufs.append(arena)
            table = self.alloc(n * across * down * 8)
            bufs.append(table)
            cursor = self.alloc(8)
            bufs.append(cursor)
            if poison is not None:
                self.memset(arena.ptr, int(poison), max(image, 16), stream)
            self._chk(launch(arena.ptr, cap, table.ptr, cursor.ptr), where)
            used = int(self.download(cursor.ptr, (1,), dtype=np.uint64, stream=stream)[0])
            tab = self.download(table.ptr, (n, down, across, 2), dtype=np.uint32, stream=stream)
            data = self.download(arena.ptr, (image if poison is not None else min(used, cap),), stream=stream)
        finally:
            for b in bufs:
                b.close()
        return data, tab, used

    def deflate_rasters(self, raster_ptrs: Sequence[int], W: int, rows: int, stream=None, arena_cap: Optional[int] = None,
                        poison: Optional[int] = None, guard: int = 0):
        """zlib-encodes every 256x256 tile of the given device rasters.

        Returns (arena bytes as uint8 array, table uint32[n, down, across, 2], used).
        arena_cap: an arena smaller than gcn10_gpu_deflate_arena_bound (tests: streams that do not fit);
        poison, guard: see _encode_into_arena."""
        n = len(raster_ptrs)
        cap = int(lib().gcn10_gpu_deflate_arena_bound(W, rows, n)) if arena_cap is None else int(arena_cap)
        ptrs = self.upload(np.array(raster_ptrs, dtype=np.uint64))
        return self._encode_into_arena(
            lambda arena, c, table, cursor: lib().gcn10_gpu_deflate_strip(self._ctx, ptrs.ptr, n, W, rows, arena, c, table,
                                                                          cursor, stream),
            "gcn10_gpu_deflate_strip", n, W, rows, cap, stream, poison, guard, held=(ptrs,))

    def overview_nearest(self, src_ptr: int, W: int, H: int, level: int, dst_ptr: int, stream=None):
        """Level `level` of a W x H device landcover, nearest sampling, into dst (gcn10_gpu_overview_nearest)."""
        self._chk(lib().gcn10_gpu_overview_nearest(self._ctx, src_ptr, W, H, level, dst_ptr, stream),
                  "gcn10_gpu_overview_nearest")

    def overview_average(self, esa_ptr: int, W: int, H: int, y0: int, rows: int, cj_ptr: int, cond_mask: int,
                         table_mask: int, n_levels: int, level_ptrs: Sequence[int], stream=None):
        """Average overview levels 1..n_levels of the selected rasters for full-resolution rows [y0, y0+rows)
        (gcn10_gpu_overview_average).  level_ptrs: [q * n_levels + k - 1] device pointers."""
        arr = (C.c_void_p * len(level_ptrs))(*[int(p) for p in level_ptrs])
        self._chk(lib().gcn10_gpu_overview_average(self._ctx, esa_ptr, W, H, y0, rows, cj_ptr, cond_mask, table_mask,
                                                   n_levels, arr, stream), "gcn10_gpu_overview_average")

    def aggregate(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, x0: int, x1: int, factor: int, cond_mask: int,
                  table_mask: int, out_ptrs: Sequence[int], out_stride: int, stream=None):
        """Area means of the selected rasters over factor x factor pixels, columns [x0, x1) of a W x rows device strip
        that starts at a cell-row boundary, with the soil of the last prepare_tile (gcn10_gpu_aggregate).  out_ptrs[q]:
        device raster of the q-th selected raster, ceil(rows / factor) rows of ceil((x1 - x0) / factor) bytes,
        out_stride bytes apart.  Asynchronous on `stream`."""
        arr = (C.c_void_p * max(len(out_ptrs), 1))(*[int(p) if p else None for p in out_ptrs])
        self._chk(lib().gcn10_gpu_aggregate(self._ctx, esa_ptr, W, rows, cj_ptr, x0, x1, factor, cond_mask, table_mask,
                                            arr, out_stride, stream), "gcn10_gpu_aggregate")

    def grid_sums(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, cellx_ptr: int, celly_ptr: int, ncx: int,
                  ncy: int, cond_mask: int, table_mask: int, acc_ptr: int, stream=None):
        """ADDS the sum and the count of the values != 255 of every selected raster to acc[q][celly[y]][cellx[x]] =
        {s, n} (uint64 pairs on the device, [n_sel][ncy][ncx][2]) over a W x rows device strip, with the soil of the
        last prepare_tile (gcn10_gpu_grid_sums).  cellx_ptr / celly_ptr: int32[W] / int32[rows] on the device, the
        cell column and row of every pixel column and strip row, -1 = in none (host.grid_plan_block makes them).
        Asynchronous on `stream`."""
        self._chk(lib().gcn10_gpu_grid_sums(self._ctx, esa_ptr, W, rows, cj_ptr, cellx_ptr, celly_ptr, ncx, ncy,
                                            cond_mask, table_mask, acc_ptr, stream), "gcn10_gpu_grid_sums")

    def grid_finish(self, acc_ptr: int, n_sel: int, n_cells: int, means_ptr: int, shared_idx_ptr, n_shared: int,
                    shared_ptr, stream=None):
        """means[q][c] = n ? (2 s + n) // (2 n) : 255 of the n_sel * n_cells pairs of acc, and the pairs of the n_shared
        cells shared_idx (uint32 on the device) names, packed into shared[q][i] (gcn10_gpu_grid_finish).  Asynchronous
        on `stream`."""
        self._chk(lib().gcn10_gpu_grid_finish(self._ctx, acc_ptr, n_sel, n_cells, means_ptr, shared_idx_ptr or None,
                                              n_shared, shared_ptr or None, stream), "gcn10_gpu_grid_finish")

    def set_weights(self, w):
        """The 256 16-bit weights of the weighted grid sums, folded into the loaded tables (gcn10_gpu_set_weights):
        after set_tables, and again after every later set_tables.  Synchronous."""
        a = np.ascontiguousarray(w, dtype=np.uint16).reshape(256)
        self._chk(lib().gcn10_gpu_set_weights(self._ctx, a.ctypes.data), "gcn10_gpu_set_weights")

    def grid_sums_weighted(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, cellx_ptr: int, celly_ptr: int, ncx: int,
                           ncy: int, cond_mask: int, table_mask: int, acc_ptr: int, stream=None):
        """grid_sums with triples: ADDS {s, n, sw} to acc[q][celly[y]][cellx[x]] (uint64 on the device,
        [n_sel][ncy][ncx][3]), s and n exactly as grid_sums, sw the sum of w[v] over the same pixels for the weights of
        set_weights (gcn10_gpu_grid_sums_weighted).  Asynchronous on `stream`."""
        self._chk(lib().gcn10_gpu_grid_sums_weighted(self._ctx, esa_ptr, W, rows, cj_ptr, cellx_ptr, celly_ptr, ncx, ncy,
                                                     cond_mask, table_mask, acc_ptr, stream),
                  "gcn10_gpu_grid_sums_weighted")

    def grid_finish_weighted(self, acc_ptr: int, n_sel: int, n_cells: int, means_ptr: int, cnq_ptr: int, shared_idx_ptr,
                             n_shared: int, shared_ptr, stream=None):
        """means[q][c] as grid_finish, cnq[q][c] = host.runoff_cn of the triple with the weights of set_weights, and the
        triples of the n_shared cells shared_idx names, packed into shared[q][i]
        (gcn10_gpu_grid_finish_weighted).  Asynchronous on `stream`."""
        self._chk(lib().gcn10_gpu_grid_finish_weighted(self._ctx, acc_ptr, n_sel, n_cells, means_ptr, cnq_ptr,
                                                       shared_idx_ptr or None, n_shared, shared_ptr or None, stream),
                  "gcn10_gpu_grid_finish_weighted")

    def set_weight_tables(self, w):
        """k tables of 256 16-bit weights ([k][256], 1 <= k <= 8), folded into the loaded tables as set_weights folds
        one (gcn10_gpu_set_weight_tables): after set_tables, and again after every later set_tables.  Synchronous."""
        a = np.ascontiguousarray(w, dtype=np.uint16).reshape(-1, 256)
        self._chk(lib().gcn10_gpu_set_weight_tables(self._ctx, a.ctypes.data, a.shape[0]),
                  "gcn10_gpu_set_weight_tables")

    def grid_sums_storms(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, cellx_ptr: int, celly_ptr: int, ncx: int,
                         ncy: int, cond_mask: int, table_mask: int, acc_ptr: int, stream=None):
        """grid_sums with 2 + k words: ADDS {s, n, sw_0, ..., sw_(k-1)} to acc[q][celly[y]][cellx[x]] (uint64 on the
        device, [n_sel][ncy][ncx][2 + k]), s and n exactly as grid_sums, sw_j the sum of w_j[v] over the same pixels
        for the k tables of set_weight_tables (gcn10_gpu_grid_sums_storms).  Asynchronous on `stream`."""
        self._chk(lib().gcn10_gpu_grid_sums_storms(self._ctx, esa_ptr, W, rows, cj_ptr, cellx_ptr, celly_ptr, ncx, ncy,
                                                   cond_mask, table_mask, acc_ptr, stream),
                  "gcn10_gpu_grid_sums_storms")

    def grid_finish_storms(self, acc_ptr: int, n_sel: int, n_cells: int, means_ptr: int, cnq_ptr: int, shared_idx_ptr,
                           n_shared: int, shared_ptr, stream=None):
        """means[q][c] as grid_finish, cnq[j][q][c] = host.runoff_cn of (s, n, sw_j) with table j of set_weight_tables,
        and the 2 + k words of the n_shared cells shared_idx names, packed into shared[q][i]
        (gcn10_gpu_grid_finish_storms).  Asynchronous on `stream`."""
        self._chk(lib().gcn10_gpu_grid_finish_storms(self._ctx, acc_ptr, n_sel, n_cells, means_ptr, cnq_ptr,
                                                     shared_idx_ptr or None, n_shared, shared_ptr or None, stream),
                  "gcn10_gpu_grid_finish_storms")

    def set_rain_tables(self, w):
        """k tables of 256 16-bit weights ([k][256], 1 <= k <= 256) for the rain sums, one of them named per cell
        (gcn10_gpu_set_rain_tables).  Independent of set_weights, set_weight_tables and set_tables.  Synchronous."""
        a = np.ascontiguousarray(w, dtype=np.uint16).reshape(-1, 256)
        self._chk(lib().gcn10_gpu_set_rain_tables(self._ctx, a.ctypes.data, a.shape[0]), "gcn10_gpu_set_rain_tables")

    def grid_sums_rain(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, cellx_ptr: int, celly_ptr: int, ncx: int,
                       ncy: int, cond_mask: int, table_mask: int, cell_table_ptr: int, acc_ptr: int, stream=None):
        """grid_sums_weighted with a table per cell: ADDS {s, n, sw} to acc[q][celly[y]][cellx[x]] (uint64 on the
        device, [n_sel][ncy][ncx][3]), sw the sum of w[cell_table[cy][cx]][v] for the tables of set_rain_tables;
        cell_table_ptr: uint8[ncy][ncx] on the device (gcn10_gpu_grid_sums_rain).  Asynchronous on `stream`."""
        self._chk(lib().gcn10_gpu_grid_sums_rain(self._ctx, esa_ptr, W, rows, cj_ptr, cellx_ptr, celly_ptr, ncx, ncy,
                                                 cond_mask, table_mask, cell_table_ptr, acc_ptr, stream),
                  "gcn10_gpu_grid_sums_rain")

    def grid_finish_rain(self, acc_ptr: int, n_sel: int, n_cells: int, cell_table_ptr: int, means_ptr: int,
                         cnq_ptr: int, shared_idx_ptr, n_shared: int, shared_ptr, stream=None):
        """means[q][c] as grid_finish, cnq[q][c] = host.runoff_cn of the triple with table cell_table[c] of
        set_rain_tables, and the triples of the n_shared cells shared_idx names, packed into shared[q][i]
        (gcn10_gpu_grid_finish_rain).  Asynchronous on `stream`."""
        self._chk(lib().gcn10_gpu_grid_finish_rain(self._ctx, acc_ptr, n_sel, n_cells, cell_table_ptr, means_ptr,
                                                   cnq_ptr, shared_idx_ptr or None, n_shared, shared_ptr or None,
                                                   stream), "gcn10_gpu_grid_finish_rain")

    def grid_sums_rains(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, cellx_ptr: int, celly_ptr: int, ncx: int,
                        ncy: int, cond_mask: int, table_mask: int, cell_tables_ptr: int, k: int, acc_ptr: int,
                        stream=None):
        """grid_sums_rain with k tables per cell, the pixels counted once: ADDS {s, n, sw_1 .. sw_k} to
        acc[q][celly[y]][cellx[x]] (uint64 on the device, [n_sel][ncy][ncx][2 + k]), sw_j the sum of
        w[cell_tables[j][cy][cx]][v] for the tables of set_rain_tables; cell_tables_ptr: uint8[k][ncy][ncx] on the
        device, 1 <= k <= 8 (gcn10_gpu_grid_sums_rains).  Asynchronous on `stream`."""
        self._chk(lib().gcn10_gpu_grid_sums_rains(self._ctx, esa_ptr, W, rows, cj_ptr, cellx_ptr, celly_ptr, ncx, ncy,
                                                  cond_mask, table_mask, cell_tables_ptr, k, acc_ptr, stream),
                  "gcn10_gpu_grid_sums_rains")

    def grid_finish_rains(self, acc_ptr: int, n_sel: int, n_cells: int, cell_tables_ptr: int, k: int, means_ptr: int,
                          cnq_ptr: int, shared_idx_ptr, n_shared: int, shared_ptr, stream=None):
        """means[q][c] as grid_finish, cnq[j][q][c] = host.runoff_cn of {word 0, word 1, word 2 + j} with table
        cell_tables[j][c] of set_rain_tables, and the 2 + k words of the n_shared cells shared_idx names, packed into
        shared[q][i] (gcn10_gpu_grid_finish_rains).  Asynchronous on `stream`."""
        self._chk(lib().gcn10_gpu_grid_finish_rains(self._ctx, acc_ptr, n_sel, n_cells, cell_tables_ptr, k, means_ptr,
                                                    cnq_ptr, shared_idx_ptr or None, n_shared, shared_ptr or None,
                                                    stream), "gcn10_gpu_grid_finish_rains")

    def zonal_pair_histogram(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, spans, items, n_zones: int,
                             hist_ptr: int, stream=None):
        """ADDS the pair counts of the pixels of every span to hist[zone] ([n_zones][16][256] uint64 on the device) with
        the soil codes prepare_tile prepared for width W (gcn10_gpu_zonal_pair_histogram).  spans (host.ZONE_SPAN_DTYPE,
        sorted by zone) and items (host.ZONE_ITEM_DTYPE), as host.Zones.build_plan / host.zone_items make them, are
        checked here -- the kernel trusts them --, uploaded, and freed when the call has run."""
        sp = np.ascontiguousarray(spans, dtype=_host.ZONE_SPAN_DTYPE)
        it = np.ascontiguousarray(items, dtype=_host.ZONE_ITEM_DTYPE)
        if sp.size and not ((sp["y"] >= 0).all() and (sp["y"] < rows).all() and (sp["x0"] >= 0).all() and
                            (sp["x0"] < sp["x1"]).all() and (sp["x1"] <= W).all() and (sp["zone"] >= 0).all() and
                            (sp["zone"] < n_zones).all()):
            raise ValueError("a span lies outside the %d x %d strip or its zone outside 0..%d" % (W, rows, n_zones - 1))
        first, n = it["first_span"].astype(np.int64), it["n_spans"].astype(np.int64)
        if it.size and not ((n > 0).all() and first[0] == 0 and (first[1:] == (first + n)[:-1]).all() and
                            int(first[-1] + n[-1]) == sp.size and
                            all(len(set(sp["zone"][a:a + m].tolist())) == 1 for a, m in zip(first, n))):
            raise ValueError("the items must name every span once, in order, each item the spans of one zone")
        if it.size == 0 and sp.size:
            raise ValueError("spans without items")
        bufs = [self.upload(sp), self.upload(it)] if it.size else []
        try:
            self.zonal_pair_histogram_device(esa_ptr, W, rows, cj_ptr, bufs[0].ptr if bufs else None,
                                             bufs[1].ptr if bufs else None, it.size, n_zones, hist_ptr, stream)
            self.sync(stream)
        finally:
            for b in bufs:
                b.close()

    def zonal_pair_histogram_device(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, spans_ptr, items_ptr,
                                    n_items: int, n_zones: int, hist_ptr: int, stream=None):
        """gcn10_gpu_zonal_pair_histogram over spans and items that are on the device already: asynchronous on `stream`
        and UNCHECKED -- for spans and items that zonal_pair_histogram has taken once, launched again (timing)."""
        self._chk(lib().gcn10_gpu_zonal_pair_histogram(self._ctx, esa_ptr, W, rows, cj_ptr, spans_ptr, items_ptr, n_items,
                                                       n_zones, hist_ptr, stream), "gcn10_gpu_zonal_pair_histogram")

    def zonal_sums_rain(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, spans, items, n_zones: int, cond_mask: int,
                        table_mask: int, acc_ptr: int, stream=None):
        """ADDS {s, n, sw} of the pixels of every span to acc[zone][q] ([n_zones][n_sel][3] uint64 on the device), sw the
        sum of w[item.table][v] for the tables of set_rain_tables (gcn10_gpu_zonal_sums_rain).  spans
        (host.ZONE_SPAN_DTYPE) and items (host.ZONE_RAIN_ITEM_DTYPE: the spans of one zone under one table each), as
        host.zone_rain_cut makes them, are checked here -- the kernel trusts them --, uploaded, and freed when the call
        has run."""
        sp = np.ascontiguousarray(spans, dtype=_host.ZONE_SPAN_DTYPE)
        it = np.ascontiguousarray(items, dtype=_host.ZONE_RAIN_ITEM_DTYPE)
        if sp.size and not ((sp["y"] >= 0).all() and (sp["y"] < rows).all() and (sp["x0"] >= 0).all() and
                            (sp["x0"] < sp["x1"]).all() and (sp["x1"] <= W).all() and (sp["zone"] >= 0).all() and
                            (sp["zone"] < n_zones).all()):
            raise ValueError("a span lies outside the %d x %d strip or its zone outside 0..%d" % (W, rows, n_zones - 1))
        first, n = it["first_span"].astype(np.int64), it["n_spans"].astype(np.int64)
        if it.size and not ((n > 0).all() and (first >= 0).all() and int((first + n).max()) <= sp.size and
                            all(len(set(sp["zone"][a:a + m].tolist())) == 1 for a, m in zip(first, n))):
            raise ValueError("an item names spans that are not there, or the spans of two zones")
        bufs = [self.upload(sp), self.upload(it)] if it.size else []
        try:
            self.zonal_sums_rain_device(esa_ptr, W, rows, cj_ptr, bufs[0].ptr if bufs else None,
                                        bufs[1].ptr if bufs else None, it.size, n_zones, cond_mask, table_mask, acc_ptr,
                                        stream)
            self.sync(stream)
        finally:
            for b in bufs:
                b.close()

    def zonal_sums_rain_device(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, spans_ptr, items_ptr, n_items: int,
                               n_zones: int, cond_mask: int, table_mask: int, acc_ptr: int, stream=None):
        """gcn10_gpu_zonal_sums_rain over spans and items that are on the device already: asynchronous on `stream` and
        UNCHECKED (timing)."""
        self._chk(lib().gcn10_gpu_zonal_sums_rain(self._ctx, esa_ptr, W, rows, cj_ptr, spans_ptr, items_ptr, n_items,
                                                  n_zones, cond_mask, table_mask, acc_ptr, stream),
                  "gcn10_gpu_zonal_sums_rain")

    def zonal_sums_rains(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, spans, items, n_zones: int, cond_mask: int,
                         table_mask: int, k: int, acc_ptr: int, stream=None):
        """ADDS {s, n, sw_1 .. sw_k} of the pixels of every span to acc[zone][q] ([n_zones][n_sel][2 + k] uint64 on the
        device), sw_j the sum of w[item.table[j]][v] for the tables of set_rain_tables (gcn10_gpu_zonal_sums_rains).  spans
        (host.ZONE_SPAN_DTYPE) and items (host.ZONE_RAINS_ITEM_DTYPE: the spans of one zone under one tuple of tables
        each), as host.zone_rains_cut makes them, are checked here -- the kernel trusts them --, uploaded, and freed
        when the call has run."""
        sp = np.ascontiguousarray(spans, dtype=_host.ZONE_SPAN_DTYPE)
        it = np.ascontiguousarray(items, dtype=_host.ZONE_RAINS_ITEM_DTYPE)
        if sp.size and not ((sp["y"] >= 0).all() and (sp["y"] < rows).all() and (sp["x0"] >= 0).all() and
                            (sp["x0"] < sp["x1"]).all() and (sp["x1"] <= W).all() and (sp["zone"] >= 0).all() and
                            (sp["zone"] < n_zones).all()):
            raise ValueError("a span lies outside the %d x %d strip or its zone outside 0..%d" % (W, rows, n_zones - 1))
        first, n = it["first_span"].astype(np.int64), it["n_spans"].astype(np.int64)
        if it.size and not ((n > 0).all() and (first >= 0).all() and int((first + n).max()) <= sp.size and
                            all(len(set(sp["zone"][a:a + m].tolist())) == 1 for a, m in zip(first, n))):
            raise ValueError("an item names spans that are not there, or the spans of two zones")
        bufs = [self.upload(sp), self.upload(it)] if it.size else []
        try:
            self.zonal_sums_rains_device(esa_ptr, W, rows, cj_ptr, bufs[0].ptr if bufs else None,
                                         bufs[1].ptr if bufs else None, it.size, n_zones, cond_mask, table_mask, k,
                                         acc_ptr, stream)
            self.sync(stream)
        finally:
            for b in bufs:
                b.close()

    def zonal_sums_rains_device(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, spans_ptr, items_ptr, n_items: int,
                                n_zones: int, cond_mask: int, table_mask: int, k: int, acc_ptr: int, stream=None):
        """gcn10_gpu_zonal_sums_rains over spans and items that are on the device already: asynchronous on `stream` and
        UNCHECKED (timing)."""
        self._chk(lib().gcn10_gpu_zonal_sums_rains(self._ctx, esa_ptr, W, rows, cj_ptr, spans_ptr, items_ptr, n_items,
                                                   n_zones, cond_mask, table_mask, k, acc_ptr, stream),
                  "gcn10_gpu_zonal_sums_rains")

    def pair_histogram(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, hist_ptr: int, stream=None):
        """Adds the (landcover, soil code) pair counts of a W x rows device strip to the device histogram hist_ptr
        (PAIR_HIST_BINS * 256 uint64, [bin][landcover]), with the soil of the last prepare_tile
        (gcn10_gpu_pair_histogram)."""
        self._chk(lib().gcn10_gpu_pair_histogram(self._ctx, esa_ptr, W, rows, cj_ptr, hist_ptr, stream),
                  "gcn10_gpu_pair_histogram")

    def verify_counts_alloc(self, stream=None) -> DevBuf:
        """A cleared gcn10_verify_count[N_RASTERS] on the device: no mismatches, first = UINT64_MAX."""
        buf = self.alloc(N_RASTERS * VERIFY_COUNT_DTYPE.itemsize)
        clear = np.zeros(N_RASTERS, VERIFY_COUNT_DTYPE)
        clear["first"] = VERIFY_NONE
        self.h2d(buf.ptr, clear, stream)
        self.sync(stream)
        return buf

    def verify_counts(self, counts_ptr: int, stream=None) -> np.ndarray:
        """The device counters as a VERIFY_COUNT_DTYPE array of N_RASTERS records."""
        return self.download(counts_ptr, (N_RASTERS,), dtype=VERIFY_COUNT_DTYPE, stream=stream)

    def verify_strip(self, esa_ptr: int, W: int, rows: int, cj_ptr: int, cond_mask: int, table_mask: int,
                     got: Sequence[Optional[int]], got_stride: int, y0: int, counts_ptr: int, stream=None):
        """Compares the decoded strips got[r] (device pointers, rows got_stride bytes apart) of rows [y0, y0 + rows)
        with the values computed from the landcover strip and the prepared soil, and adds what differs to the device
        counters (gcn10_gpu_verify_strip)."""
        arr = (C.c_void_p * N_RASTERS)()
        for r in range(N_RASTERS):
            arr[r] = got[r] if r < len(got) and got[r] else None
        self._chk(lib().gcn10_gpu_verify_strip(self._ctx, esa_ptr, W, rows, cj_ptr, cond_mask, table_mask, arr,
                                               got_stride, y0, counts_ptr, stream), "gcn10_gpu_verify_strip")

    def verify_buffers(self, want: Sequence[Optional[int]], want_stride: int, got: Sequence[Optional[int]],
                       got_stride: int, W: int, rows: int, y0: int, raster_mask: int, counts_ptr: int, stream=None):
        """The same counting for expected rasters that exist in device memory (gcn10_gpu_verify_buffers)."""
        wa, ga = (C.c_void_p * N_RASTERS)(), (C.c_void_p * N_RASTERS)()
        for r in range(N_RASTERS):
            wa[r] = want[r] if r < len(want) and want[r] else None
            ga[r] = got[r] if r < len(got) and got[r] else None
        self._chk(lib().gcn10_gpu_verify_buffers(self._ctx, wa, want_stride, ga, got_stride, W, rows, y0,
                                                 raster_mask, counts_ptr, stream), "gcn10_gpu_verify_buffers")

    def lzw_arena_bound(self, W: int, rows: int, n_rasters: int) -> int:
        """Worst-case arena bytes of gcn10_gpu_lzw_strip for n_rasters strips of W x rows."""
        return int(lib().gcn10_gpu_lzw_arena_bound(W, rows, n_rasters))

    def lzw_strip(self, raster_ptrs: Sequence[int], W: int, rows: int, stream=None, arena_cap: Optional[int] = None,
                  poison: Optional[int] = None, guard: int = 0):
        """TIFF-LZW-encodes every 256x256 tile of the given device rasters (gcn10_gpu_lzw_strip).

        Returns (arena bytes as uint8 array, table uint32[n, down, across, 2], used).
        arena_cap: an arena smaller than lzw_arena_bound (tests: streams that do not fit);
        poison, guard: see _encode_into_arena."""
        n = len(raster_ptrs)
        cap = self.lzw_arena_bound(W, rows, n) if arena_cap is None else int(arena_cap)
        ptrs = self.upload(np.array(raster_ptrs, dtype=np.uint64))
        return self._encode_into_arena(
            lambda arena, c, table, cursor: lib().gcn10_gpu_lzw_strip(self._ctx, ptrs.ptr, n, W, rows, arena, c, table,
                                                                      cursor, stream),
            "gcn10_gpu_lzw_strip", n, W, rows, cap, stream, poison, guard, held=(ptrs,))

    def deflate_fused(self, esa_d: int, W: int, rows: int, cj_d: int, cond_mask: int = 3,
                      table_mask: int = ALL_TABLES, stream=None, arena_cap: Optional[int] = None,
                      poison: Optional[int] = None, guard: int = 0):
        """Encoded tiles of the selected rasters straight from landcover + prepared soil
        (gcn10_gpu_deflate_fused_strip).  Returns (arena bytes, table uint32[n, down, across, 2], used).
        arena_cap: an arena smaller than gcn10_gpu_deflate_arena_bound (tests: streams that do not fit);
        poison, guard: see _encode_into_arena."""
        n = bin(cond_mask & 3).count("1") * bin(table_mask & ALL_TABLES).count("1")
        cap = int(lib().gcn10_gpu_deflate_arena_bound(W, rows, n)) if arena_cap is None else int(arena_cap)
        return self._encode_into_arena(
            lambda arena, c, table, cursor: lib().gcn10_gpu_deflate_fused_strip(self._ctx, esa_d, W, rows, cj_d, cond_mask,
                                                                                table_mask, arena, c, table, cursor,
                                                                                stream),
            "gcn10_gpu_deflate_fused_strip", n, W, rows, cap, stream, poison, guard)

    @staticmethod
    def inflate_codecs() -> int:
        """CODEC_* bits of the chunk codecs inflate_tiles decodes (gcn10_gpu_inflate_codecs)."""
        return int(lib().gcn10_gpu_inflate_codecs())

    def inflate_tiles(self, streams: Sequence[bytes], chunk_w, chunk_rows: Sequence[int],
                      windows: Sequence[tuple], dst_shape: tuple, stream=None, flags: Optional[Sequence[int]] = None,
                      out_lens: Optional[Sequence[int]] = None):
        """Decodes zlib and TIFF LZW streams on the GPU (gcn10_gpu_inflate_tiles).

        streams[i] decodes to a chunk of chunk_rows[i] x chunk_w pixels (chunk_w: one width, or one per
        stream); windows[i] =
        (src_x, src_y, copy_w, copy_h, dst_x, dst_y) places part of it in a zero-filled uint8
        raster of dst_shape.  flags[i]: TILE_RAW (streams[i] is the chunk's pixels as they are) or
        TILE_LZW (a TIFF LZW stream; 0 = a zlib stream), either with
        TILE_PREDICTOR2 (rows are horizontal differences); out_lens[i] overrides the decoded size
        (a raw chunk staged from its first wanted row on).  Returns (raster, status uint32[n])."""
        n = len(streams)
        H, W = dst_shape
        widths = [int(chunk_w)] * n if np.isscalar(chunk_w) else [int(w) for w in chunk_w]
        tiles = np.zeros(n, dtype=INFLATE_TILE_DTYPE)
        parts, off = [], 0
        for k, st in enumerate(streams):
            sx, sy, cw, ch, dx, dy = windows[k]
            tiles[k] = (off, len(st), out_lens[k] if out_lens else widths[k] * chunk_rows[k], widths[k], sx, sy, cw,
                        ch, flags[k] if flags else 0, dy * W + dx)
            pad = (-len(st)) % 16 + 16
            parts.append(st)
            parts.append(bytes(pad))
            off += len(st) + pad
        comp = np.frombuffer(b"".join(parts) or bytes(16), dtype=np.uint8)
        bufs = [self.upload(comp, stream), self.upload(tiles.view(np.uint8), stream), self.alloc(max(H * W, 1)),
                self.alloc(4 * max(n, 1))]
        try:
            self.memset(bufs[2].ptr, 0, max(H * W, 1), stream)
            self.memset(bufs[3].ptr, 0xFF, 4 * max(n, 1), stream)
            self._chk(lib().gcn10_gpu_inflate_tiles(self._ctx, bufs[0].ptr, bufs[1].ptr, n,
                                                    max([w * r for w, r in zip(widths, chunk_rows)] + [1]),
                                                    bufs[2].ptr, W,
                                                    bufs[3].ptr, stream), "gcn10_gpu_inflate_tiles")
            out = self.download(bufs[2].ptr, (H, W), stream=stream)
            status = self.download(bufs[3].ptr, (n,), dtype=np.uint32, stream=stream)
        finally:
            for b in bufs:
                b.close()
        return out, status

    # -- block level: src/cn.c:205-290 in memory -----------------------------
    def process_block_mem(self, esa: np.ndarray, gt, coarse: np.ndarray, soil_gt,
                          cond_mask: int = 3, table_mask: int = ALL_TABLES,
                          strip_rows: Optional[int] = None) -> np.ndarray:
        """What process_block() computes between load_raster and save_raster.

        Returns uint8[18,H,W] in the reference's raster order (unselected
        rasters stay 0).  Index maps come from the host library, every pixel
        from the HIP kernels.
        """
        esa = np.ascontiguousarray(esa, dtype=np.uint8)
        coarse = np.ascontiguousarray(coarse, dtype=np.uint8)
        H, W = esa.shape
        hsy, hsx = coarse.shape
        out = np.zeros((N_RASTERS, H, W), dtype=np.uint8)
        if H == 0 or W == 0:
            return out
        ci, cj = _host.build_index_maps(gt, soil_gt, W, H, hsx, hsy)
        bufs = []
        try:
            esa_d = self.upload(esa); bufs.append(esa_d)
            coarse_d = self.upload(coarse); bufs.append(coarse_d)
            ci_d = self.upload(ci); bufs.append(ci_d)
            cj_d = self.upload(cj); bufs.append(cj_d)
            sel = [r for r in range(N_RASTERS)
                   if (cond_mask >> (r // 9)) & 1 and (table_mask >> (r % 9)) & 1]
            out_d = {}
            for r in sel:
                out_d[r] = self.alloc(H * W)
                bufs.append(out_d[r])
                self.memset(out_d[r].ptr, 0xA5, H * W)     # poison: every byte must be written
            self.prepare_tile(coarse_d.ptr, hsx, hsy, ci_d.ptr, W)
            step = H if not strip_rows else int(strip_rows)
            for y0 in range(0, H, step):
                rows = min(step, H - y0)
                ptrs = [out_d[r].at(y0 * W) if r in out_d else None for r in range(N_RASTERS)]
                self.cn_strip(esa_d.at(y0 * W), W, rows, cj_d.at(4 * y0), cond_mask, table_mask,
                              ptrs)
            self.sync()
            for r in sel:
                out[r] = self.download(out_d[r].ptr, (H, W))
        finally:
            for b in bufs:
                b.close()
        return out
