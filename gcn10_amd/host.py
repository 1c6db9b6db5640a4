"""ctypes face of ``libgcn10_host.so`` (``include/gcn10_host.h``)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GCN10_HOST_LIB") or os.path.join(_HERE, "libgcn10_host.so")
_lib = None

HCS = ("p", "f", "g")               # src/cn.c:146
ARCS = ("i", "ii", "iii")           # src/cn.c:147
CONDS = ("drained", "undrained")    # src/cn.c:145

_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
ROW_ERROR_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s is missing: run `make host` (or __graft_entry__.build())" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.gcn10_load_lookup_file.argtypes = [C.c_char_p, _i32p, ROW_ERROR_FN, C.c_void_p]
        L.gcn10_load_lookup_file.restype = C.c_int
        L.gcn10_load_lookup_table.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, _i32p,
                                              ROW_ERROR_FN, C.c_void_p]
        L.gcn10_load_lookup_table.restype = C.c_int
        L.gcn10_load_all_lookup_tables.argtypes = [C.c_char_p, _i32p, C.POINTER(C.c_int),
                                                   ROW_ERROR_FN, C.c_void_p]
        L.gcn10_load_all_lookup_tables.restype = C.c_int
        L.gcn10_build_index_maps.argtypes = [_f64p, _f64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             _i32p, _i32p]
        L.gcn10_build_index_maps.restype = None
        L.gcn10_raster_window.argtypes = [_f64p, C.c_int, C.c_int, _f64p, C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), _f64p]
        L.gcn10_raster_window.restype = C.c_int
        vp, ip, cp = C.c_void_p, C.POINTER(C.c_int), C.c_char_p
        L.gcn10_config_parse.argtypes = [cp, C.POINTER(Config), cp, C.c_size_t]
        L.gcn10_config_parse.restype = C.c_int
        L.gcn10_config_free.argtypes = [C.POINTER(Config)]
        L.gcn10_config_free.restype = None
        L.gcn10_log_open.argtypes = [cp, C.c_int]
        L.gcn10_log_open.restype = vp
        L.gcn10_log_message.argtypes = [vp, cp, cp, C.c_bool]
        L.gcn10_log_message.restype = None
        L.gcn10_log_close.argtypes = [vp]
        L.gcn10_log_close.restype = None
        L.gcn10_read_block_list.argtypes = [cp, ip]
        L.gcn10_read_block_list.restype = C.POINTER(C.c_int)
        L.gcn10_blocks_open.argtypes = [cp, C.POINTER(Blocks), cp, C.c_size_t]
        L.gcn10_blocks_open.restype = C.c_int
        L.gcn10_blocks_free.argtypes = [C.POINTER(Blocks)]
        L.gcn10_blocks_free.restype = None
        L.gcn10_blocks_find.argtypes = [C.POINTER(Blocks), C.c_int]
        L.gcn10_blocks_find.restype = C.c_int
        L.gcn10_raster_open.argtypes = [cp, cp, cp, C.c_size_t]
        L.gcn10_raster_open.restype = vp
        L.gcn10_raster_close.argtypes = [vp]
        L.gcn10_raster_close.restype = None
        L.gcn10_raster_info.argtypes = [vp, ip, ip, _f64p]
        L.gcn10_raster_info.restype = None
        L.gcn10_raster_read.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, cp, C.c_size_t]
        L.gcn10_raster_read.restype = C.c_int
        L.gcn10_raster_georef.argtypes = [vp]
        L.gcn10_raster_georef.restype = vp
        L.gcn10_save_raster.argtypes = [vp, C.c_int, C.c_int, _f64p, vp, cp, C.c_int, cp, C.c_size_t]
        L.gcn10_save_raster.restype = C.c_int
        L.gcn10_tiff_create_cog.argtypes = [cp, C.c_int, C.c_int, _f64p, vp, C.c_int, cp, C.c_size_t]
        L.gcn10_tiff_create_cog.restype = vp
        L.gcn10_tiff_create.argtypes = [cp, C.c_int, C.c_int, _f64p, vp, cp, C.c_size_t]
        L.gcn10_tiff_create.restype = vp
        # TiffWriter's own handle on it: callers that bind the shared attribute to other argtypes do not reach it
        L.tiff_create_ = L["gcn10_tiff_create"]
        L.tiff_create_.argtypes = [cp, C.c_int, C.c_int, _f64p, vp, cp, C.c_size_t]
        L.tiff_create_.restype = vp
        L.gcn10_cog_levels.argtypes = [C.c_int, C.c_int]
        L.gcn10_cog_levels.restype = C.c_int
        L.gcn10_tiff_level.argtypes = [vp, C.c_int]
        L.gcn10_tiff_level.restype = vp
        L.gcn10_tiff_n_levels.argtypes = [vp]
        L.gcn10_tiff_n_levels.restype = C.c_int
        L.gcn10_tiff_tiles_across.argtypes = [vp]
        L.gcn10_tiff_tiles_across.restype = C.c_int
        L.gcn10_tiff_tiles_down.argtypes = [vp]
        L.gcn10_tiff_tiles_down.restype = C.c_int
        L.gcn10_tiff_put_tile.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
        L.gcn10_tiff_put_tile.restype = C.c_int
        L.gcn10_tiff_put_tiles.argtypes = [vp, C.c_int, ip, ip, C.POINTER(vp), C.POINTER(C.c_uint32)]
        L.gcn10_tiff_put_tiles.restype = C.c_int
        L.gcn10_tiff_put_extent.argtypes = [vp, vp, C.c_size_t, C.c_int, ip, ip, C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint32)]
        L.gcn10_tiff_put_extent.restype = C.c_int
        L.gcn10_tiff_set_compression.argtypes = [vp, C.c_int]
        L.gcn10_tiff_set_compression.restype = C.c_int
        L.gcn10_tiff_set_direct.argtypes = [vp, C.c_bool]
        L.gcn10_tiff_set_direct.restype = C.c_int
        L.gcn10_tiff_set_nodata.argtypes = [vp, C.c_int]
        L.gcn10_tiff_set_nodata.restype = C.c_int
        L.gcn10_tiff_set_metadata_xml.argtypes = [vp, cp]
        L.gcn10_tiff_set_metadata_xml.restype = C.c_int
        L.gcn10_tiff_reserve_metadata.argtypes = [vp, C.c_size_t]
        L.gcn10_tiff_reserve_metadata.restype = C.c_int
        u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
        L.gcn10_raster_histogram.argtypes = [u64p, np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS"),
                                             _i32p, C.c_int, u64p]
        L.gcn10_raster_histogram.restype = None
        L.gcn10_band_stats_of.argtypes = [u64p, C.c_int, C.POINTER(BandStats)]
        L.gcn10_band_stats_of.restype = None
        L.gcn10_stats_xml.argtypes = [C.POINTER(BandStats), cp, C.c_size_t]
        L.gcn10_stats_xml.restype = C.c_size_t
        L.gcn10_tiff_finish.argtypes = [vp, cp, C.c_size_t]
        L.gcn10_tiff_finish.restype = C.c_int
        L.gcn10_zones_open.argtypes = [cp, cp, C.POINTER(ZonesStruct), cp, C.c_size_t]
        L.gcn10_zones_open.restype = C.c_int
        L.gcn10_zones_free.argtypes = [C.POINTER(ZonesStruct)]
        L.gcn10_zones_free.restype = None
        L.gcn10_zones_build_plan.argtypes = [C.POINTER(ZonesStruct), _f64p, C.c_int, C.c_int, vp, C.c_uint32,
                                             C.c_uint32, C.POINTER(ZonePlan), cp, C.c_size_t]
        L.gcn10_zones_build_plan.restype = C.c_int
        L.gcn10_zone_plan_free.argtypes = [C.POINTER(ZonePlan)]
        L.gcn10_zone_plan_free.restype = None
        L.gcn10_aggregate_geometry.argtypes = [C.c_int, C.c_int, _f64p, vp, C.c_int, C.POINTER(AggregateGeom)]
        L.gcn10_aggregate_geometry.restype = C.c_int
        L.gcn10_parse_grid.argtypes = [cp, C.POINTER(Grid)]
        L.gcn10_parse_grid.restype = C.c_int
        L.gcn10_grid_plan_block.argtypes = [C.POINTER(Grid), C.c_int, C.c_int, _f64p, vp, C.POINTER(GridPlan)]
        L.gcn10_grid_plan_block.restype = C.c_int
        L.gcn10_grid_plan_free.argtypes = [C.POINTER(GridPlan)]
        L.gcn10_grid_plan_free.restype = None
        L.gcn10_parse_storm.argtypes = [cp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.gcn10_parse_storm.restype = C.c_int
        L.gcn10_parse_storms.argtypes = [cp, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.gcn10_parse_storms.restype = C.c_int
        L.gcn10_runoff_table.argtypes = [C.c_double, C.c_double, np.ctypeslib.ndpointer(dtype=np.uint16,
                                                                                       flags="C_CONTIGUOUS")]
        L.gcn10_runoff_table.restype = None
        L.gcn10_runoff_cn.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64,
                                      np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS")]
        L.gcn10_runoff_cn.restype = C.c_int
        L.gcn10_parse_rain_unit.argtypes = [cp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.gcn10_parse_rain_unit.restype = C.c_int
        L.gcn10_rain_tables.argtypes = [C.c_double, C.c_double, np.ctypeslib.ndpointer(dtype=np.uint16,
                                                                                      flags="C_CONTIGUOUS")]
        L.gcn10_rain_tables.restype = None
        L.gcn10_runoff_bytes.argtypes = [np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS"), C.c_uint,
                                         np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")]
        L.gcn10_runoff_bytes.restype = None
        L.gcn10_parse_runoff_unit.argtypes = [cp, C.POINTER(C.c_uint)]
        L.gcn10_parse_runoff_unit.restype = C.c_int
        L.gcn10_runoff_unit_of.argtypes = [C.c_double]
        L.gcn10_runoff_unit_of.restype = C.c_uint
        L.gcn10_rain_raster_load.argtypes = [cp, cp, C.POINTER(Grid), C.POINTER(vp), cp, C.c_size_t]
        L.gcn10_rain_raster_load.restype = C.c_int
        L.gcn10_parse_rains.argtypes = [cp, C.POINTER(vp), C.POINTER(cp), C.POINTER(C.c_int)]
        L.gcn10_parse_rains.restype = C.c_int
        L.gcn10_rains_load.argtypes = [C.POINTER(cp), C.c_int, C.POINTER(Grid), C.POINTER(vp), cp, C.c_size_t]
        L.gcn10_rains_load.restype = C.c_int
        L.gcn10_rains_cell.argtypes = [vp, C.c_int, vp, vp, vp]
        L.gcn10_rains_cell.restype = None
        L.gcn10_rain_load.argtypes = [cp, C.POINTER(Grid), C.POINTER(vp), cp, C.c_size_t]
        L.gcn10_rain_load.restype = C.c_int
        L.gcn10_zone_items_build.argtypes = [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(ZonePlan)]
        L.gcn10_zone_items_build.restype = C.c_int
        L.gcn10_zone_rain_load.argtypes = [cp, C.POINTER(Grid), C.POINTER(vp), cp, C.c_size_t]
        L.gcn10_zone_rain_load.restype = C.c_int
        L.gcn10_zone_rain_values.argtypes = [C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_uint64,
                                             C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.POINTER(C.c_int)]
        L.gcn10_zone_rain_values.restype = C.c_int
        L.gcn10_zone_rain_cut.argtypes = [C.POINTER(ZonePlan), C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int,
                                          C.c_int, C.c_uint32, C.c_uint32, C.POINTER(ZoneRainPlan)]
        L.gcn10_zone_rain_cut.restype = C.c_int
        L.gcn10_zone_rain_plan_free.argtypes = [C.POINTER(ZoneRainPlan)]
        L.gcn10_zone_rain_plan_free.restype = None
        L.gcn10_zone_rains_load.argtypes = [C.POINTER(cp), C.c_int, C.POINTER(Grid), C.POINTER(vp), cp, C.c_size_t]
        L.gcn10_zone_rains_load.restype = C.c_int
        L.gcn10_zone_rains_cut.argtypes = [C.POINTER(ZonePlan), C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.POINTER(vp),
                                           C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(ZoneRainsPlan)]
        L.gcn10_zone_rains_cut.restype = C.c_int
        L.gcn10_zone_rains_plan_free.argtypes = [C.POINTER(ZoneRainsPlan)]
        L.gcn10_zone_rains_plan_free.restype = None
        L.gcn10_tiff_abort.argtypes = [vp]
        L.gcn10_tiff_abort.restype = None
        L.free_ = C.CDLL(None).free
        L.free_.argtypes = [vp]
        L.free_.restype = None
        _lib = L
    return _lib


class Config(C.Structure):
    """``gcn10_config`` of include/gcn10_host.h."""
    _fields_ = [("hysogs_data_path", C.c_char_p), ("esa_data_path", C.c_char_p),
                ("blocks_shp_path", C.c_char_p), ("lookup_table_path", C.c_char_p),
                ("log_dir", C.c_char_p), ("gpus", C.c_int), ("workers_per_gpu", C.c_int),
                ("strip_rows", C.c_int),
                ("io_threads", C.c_int), ("deflate_level", C.c_int), ("esa_tile_dir", C.c_char_p),
                ("gpu_deflate", C.c_int), ("gpu_inflate", C.c_int), ("direct_io", C.c_int),
                ("prefetch_blocks", C.c_int),
                ("table_mask", C.c_uint), ("cond_mask", C.c_uint), ("compress", C.c_int),
                ("gpu_inflate_lzw", C.c_int), ("cog", C.c_int), ("overview_resampling", C.c_int),
                ("stats", C.c_int), ("nodata", C.c_int)]


class ConfigFull(Config):
    """The whole ``gcn10_config``: ``Config`` is the struct as it stood when the statistics keys were added (its
    field list is pinned by the tests of that change); fields appended to the C struct since then are appended here.
    ``Config`` ends on a multiple of 8 bytes, so the fields below lie where the C compiler puts them."""
    _fields_ = [("verify", C.c_int), ("zonal", C.c_int), ("zones_shp_path", C.c_char_p),
                ("zones_id_field", C.c_char_p), ("zonal_output", C.c_char_p), ("aggregate", C.c_int)]


class ConfigGrid(ConfigFull):
    """``gcn10_config`` with the key of the model grid, appended behind ``ConfigFull`` (whose field list is pinned by
    the tests of the aggregate key) as the C struct appends it; the pointer lies behind the padding of ``aggregate``."""
    _fields_ = [("grid", C.c_char_p)]


class ConfigStorm(ConfigGrid):
    """``gcn10_config`` with the key of the design storm, appended behind ``ConfigGrid`` as the C struct appends it."""
    _fields_ = [("storm", C.c_char_p), ("storm_p", C.c_double), ("storm_lambda", C.c_double)]


MAX_STORMS = 8      # GCN10_MAX_STORMS


class ConfigStorms(ConfigStorm):
    """``gcn10_config`` with the key of several design storms, appended behind ``ConfigStorm`` as the C struct appends
    it."""
    _fields_ = [("storms", C.c_char_p), ("n_storms", C.c_int), ("storms_p", C.c_double * MAX_STORMS),
                ("storms_lambda", C.c_double)]


class ConfigRain(ConfigStorms):
    """``gcn10_config`` with the keys of the rainfall raster, appended behind ``ConfigStorms`` as the C struct appends
    them."""
    _fields_ = [("rain", C.c_char_p), ("rain_unit", C.c_char_p)]


class ConfigZoneRain(ConfigRain):
    """``gcn10_config`` with the keys of the rainfall raster under zones, appended behind ``ConfigRain`` as the C struct
    appends them."""
    _fields_ = [("zone_rain", C.c_char_p), ("zone_rain_unit", C.c_char_p)]


class ConfigRains(ConfigZoneRain):
    """``gcn10_config`` with the key of several rainfall rasters, appended behind ``ConfigZoneRain`` as the C struct
    appends it."""
    _fields_ = [("rains", C.c_char_p)]


class ConfigZoneRains(ConfigRains):
    """``gcn10_config`` with the key of several rainfall rasters under zones, appended behind ``ConfigRains`` as the C
    struct appends it."""
    _fields_ = [("zone_rains", C.c_char_p)]


class ConfigRunoffRain(ConfigZoneRains):
    """``gcn10_config`` with the keys of the runoff rasters under a rainfall raster, appended behind ``ConfigZoneRains``
    as the C struct appends them."""
    _fields_ = [("runoff_rain", C.c_char_p), ("runoff_rain_unit", C.c_char_p), ("runoff_unit", C.c_char_p)]


assert C.sizeof(Config) % 8 == 0


class BandStats(C.Structure):
    """``gcn10_band_stats`` of include/gcn10_host.h."""
    _fields_ = [("total", C.c_uint64), ("valid", C.c_uint64), ("min", C.c_int), ("max", C.c_int),
                ("mean", C.c_double), ("stddev", C.c_double), ("valid_percent", C.c_double)]


class Blocks(C.Structure):
    _fields_ = [("n", C.c_int), ("id", C.POINTER(C.c_int)), ("bbox", C.POINTER(C.c_double * 4))]


class ZonesStruct(C.Structure):
    """``gcn10_zones`` of include/gcn10_host.h."""
    _fields_ = [("n", C.c_int), ("id", C.POINTER(C.c_int64)), ("bbox", C.POINTER(C.c_double * 4)),
                ("ring_first", C.POINTER(C.c_uint64)), ("ring_pt", C.POINTER(C.c_uint64)),
                ("xy", C.POINTER(C.c_double)), ("n_rings", C.c_uint64), ("n_points", C.c_uint64)]


class ZonePlan(C.Structure):
    """``gcn10_zone_plan`` of include/gcn10_host.h."""
    _fields_ = [("n_local", C.c_int), ("local_zone", C.POINTER(C.c_int32)), ("local_pixels", C.POINTER(C.c_uint64)),
                ("n_spans", C.c_size_t), ("n_items", C.c_size_t), ("spans", C.c_void_p), ("items", C.c_void_p)]


class ZoneRainPlan(C.Structure):
    """``gcn10_zone_rain_plan`` of include/gcn10_host.h."""
    _fields_ = [("n_local", C.c_int), ("rain_pixels", C.POINTER(C.c_uint64)), ("rain_sum", C.POINTER(C.c_uint64)),
                ("n_spans", C.c_size_t), ("n_items", C.c_size_t), ("spans", C.c_void_p), ("items", C.c_void_p)]


class ZoneRainsPlan(C.Structure):
    """``gcn10_zone_rains_plan`` of include/gcn10_host.h."""
    _fields_ = [("n_local", C.c_int), ("k", C.c_int), ("rain_pixels", C.POINTER(C.c_uint64)),
                ("rain_sum", C.POINTER(C.c_uint64) * 8), ("n_spans", C.c_size_t), ("n_items", C.c_size_t),
                ("spans", C.c_void_p), ("items", C.c_void_p)]


class AggregateGeom(C.Structure):
    """``gcn10_aggregate_geom`` of include/gcn10_host.h."""
    _fields_ = [("x0", C.c_int), ("x1", C.c_int), ("y0", C.c_int), ("y1", C.c_int), ("Wa", C.c_int), ("Ha", C.c_int),
                ("gt", C.c_double * 6)]


class Grid(C.Structure):
    """``gcn10_grid`` of include/gcn10_host.h."""
    _fields_ = [("xmin", C.c_double), ("ymax", C.c_double), ("dx", C.c_double), ("dy", C.c_double), ("nx", C.c_int),
                ("ny", C.c_int)]


class GridPlan(C.Structure):
    """``gcn10_grid_plan`` of include/gcn10_host.h."""
    _fields_ = [("x0", C.c_int), ("x1", C.c_int), ("y0", C.c_int), ("y1", C.c_int), ("cx0", C.c_int), ("cx1", C.c_int),
                ("cy0", C.c_int), ("cy1", C.c_int), ("cellx", C.POINTER(C.c_int32)), ("celly", C.POINTER(C.c_int32)),
                ("complete_x", C.POINTER(C.c_uint8)), ("complete_y", C.POINTER(C.c_uint8)),
                ("shared", C.POINTER(C.c_uint32)), ("n_shared", C.c_size_t)]


# struct gcn10_zone_span / gcn10_zone_item (include/gcn10_host.h, include/gcn10_gpu.h)
ZONE_SPAN_DTYPE = np.dtype([("y", "<i4"), ("x0", "<i4"), ("x1", "<i4"), ("zone", "<i4")])
ZONE_ITEM_DTYPE = np.dtype([("first_span", "<u4"), ("n_spans", "<u4")])
# struct gcn10_zone_rain_item
ZONE_RAIN_ITEM_DTYPE = np.dtype([("first_span", "<u4"), ("n_spans", "<u4"), ("table", "<u4"), ("reserved", "<u4")])
# struct gcn10_zone_rains_item: a tuple of up to eight tables, layer 0 first
ZONE_RAINS_ITEM_DTYPE = np.dtype([("first_span", "<u4"), ("n_spans", "<u4"), ("table", "u1", (8,))])


class HostError(RuntimeError):
    pass


def _copy(ptr, n, dtype):
    """n elements of dtype at a ctypes pointer / address, copied."""
    n = int(n)
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    addr = ptr if isinstance(ptr, int) else C.cast(ptr, C.c_void_p).value
    nbytes = n * np.dtype(dtype).itemsize
    return np.frombuffer(C.string_at(addr, nbytes), dtype=dtype).copy()


def _plan_out(plan: ZonePlan) -> dict:
    out = {"local_zone": _copy(plan.local_zone, plan.n_local, np.int32),
           "local_pixels": _copy(plan.local_pixels, plan.n_local, np.uint64),
           "spans": _copy(plan.spans, plan.n_spans, ZONE_SPAN_DTYPE),
           "items": _copy(plan.items, plan.n_items, ZONE_ITEM_DTYPE)}
    lib().gcn10_zone_plan_free(C.byref(plan))
    return out


class Zones:
    """A polygon shapefile of zones (``gcn10_zones_open``): ``ids`` (int64), ``bbox`` (float64[n,4]), ``ring_first``
    (rings of record i: ring_first[i] .. ring_first[i+1]), ``ring_pt`` (points of ring k: ring_pt[k] .. ring_pt[k+1])
    and ``xy`` (float64[n_points,2])."""

    def __init__(self, path: str, id_field: str | None = None):
        self._z = ZonesStruct()
        err = C.create_string_buffer(1024)
        if lib().gcn10_zones_open(os.fsencode(path), id_field.encode() if id_field else None, C.byref(self._z),
                                  err, 1024) != 0:
            self._z = None
            raise HostError(err.value.decode(errors="replace"))
        z = self._z
        self.n = z.n
        self.ids = _copy(z.id, z.n, np.int64)
        self.bbox = _copy(z.bbox, z.n * 4, np.float64).reshape(z.n, 4)
        self.ring_first = _copy(z.ring_first, z.n + 1, np.uint64)
        self.ring_pt = _copy(z.ring_pt, z.n_rings + 1, np.uint64)
        self.xy = _copy(z.xy, z.n_points * 2, np.float64).reshape(-1, 2)

    def n_rings(self, i: int) -> int:
        return int(self.ring_first[i + 1] - self.ring_first[i])

    def rings(self, i: int):
        """The rings of record i, float64[m,2] each."""
        return [self.xy[int(self.ring_pt[k]):int(self.ring_pt[k + 1])]
                for k in range(int(self.ring_first[i]), int(self.ring_first[i + 1]))]

    def build_plan(self, gt, W: int, H: int, own=None, max_span_px: int = 0, max_item_px: int = 0) -> dict:
        """Spans and work items of the zones over a block (``gcn10_zones_build_plan``): ``local_zone``, ``local_pixels``,
        ``spans`` (ZONE_SPAN_DTYPE) and ``items`` (ZONE_ITEM_DTYPE)."""
        plan = ZonePlan()
        err = C.create_string_buffer(1024)
        o = None if own is None else _f(own, 4)
        rc = lib().gcn10_zones_build_plan(C.byref(self._z), _f(gt, 6), int(W), int(H),
                                          None if o is None else o.ctypes.data, int(max_span_px), int(max_item_px),
                                          C.byref(plan), err, 1024)
        if rc != 0:
            raise HostError(err.value.decode(errors="replace"))
        return _plan_out(plan)

    def close(self):
        if self._z is not None:
            lib().gcn10_zones_free(C.byref(self._z))
            self._z = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def zone_items(spans, max_span_px: int = 0, max_item_px: int = 0):
    """Spans sorted by (zone, y, x0) -> (spans split at max_span_px, items of at most max_item_px pixels)
    (``gcn10_zone_items_build``; 0 = the built-in bounds)."""
    a = np.ascontiguousarray(spans, dtype=ZONE_SPAN_DTYPE)
    plan = ZonePlan()
    if lib().gcn10_zone_items_build(a.ctypes.data if a.size else None, a.size, int(max_span_px), int(max_item_px),
                                    C.byref(plan)) != 0:
        raise HostError("gcn10_zone_items_build: an empty span, or out of memory")
    out = _plan_out(plan)
    return out["spans"], out["items"]


def aggregate_geometry(W: int, H: int, gt, own, f: int) -> dict:
    """The grid of f x f pixel cells over the owned pixels of a W x H block (``gcn10_aggregate_geometry``): x0, x1, y0,
    y1, Wa, Ha and gt (float64[6]).  own: the block's box {minx, miny, maxx, maxy}, None = every pixel."""
    geom = AggregateGeom()
    o = None if own is None else _f(own, 4)
    if lib().gcn10_aggregate_geometry(int(W), int(H), _f(gt, 6), None if o is None else o.ctypes.data, int(f),
                                      C.byref(geom)) != 0:
        raise HostError("gcn10_aggregate_geometry: factor outside 2..256, a block that is not north up, or no owned pixel")
    out = {name: getattr(geom, name) for name in ("x0", "x1", "y0", "y1", "Wa", "Ha")}
    out["gt"] = np.array(list(geom.gt), np.float64)
    return out


def _grid(grid) -> Grid:
    if isinstance(grid, dict):
        return Grid(*[grid[k] for k in ("xmin", "ymax", "dx", "dy", "nx", "ny")])
    return Grid(*grid)


def parse_grid(text: str) -> dict:
    """"<xmin>,<ymax>,<dx>,<dy>,<nx>,<ny>" -> dict of the six (``gcn10_parse_grid``); raises HostError for any other
    text."""
    g = Grid()
    if lib().gcn10_parse_grid(text.encode(), C.byref(g)) != 0:
        raise HostError("bad value for grid: '%s' (xmin,ymax,dx,dy,nx,ny)" % text)
    return {name: getattr(g, name) for name, _t in Grid._fields_}


def grid_plan_block(grid, W: int, H: int, gt, own=None) -> dict:
    """A W x H block on a model grid (``gcn10_grid_plan_block``).  grid: the dict of parse_grid or the six values; own:
    the block's box {minx, miny, maxx, maxy}, None = every pixel.  x0, x1, y0, y1 (the owned pixels), cx0, cx1, cy0,
    cy1 (the block's cells), cellx (int32[W]) and celly (int32[H]) (local cell column / row, -1 = none; empty when the
    block has no cell), complete_x, complete_y (bool per local cell column / row) and shared (uint32 local indices)."""
    plan = GridPlan()
    g = _grid(grid)
    o = None if own is None else _f(own, 4)
    if lib().gcn10_grid_plan_block(C.byref(g), int(W), int(H), _f(gt, 6), None if o is None else o.ctypes.data,
                                   C.byref(plan)) != 0:
        raise HostError("gcn10_grid_plan_block: a bad size, a block that is not north up, or out of memory")
    out = {name: getattr(plan, name) for name in ("x0", "x1", "y0", "y1", "cx0", "cx1", "cy0", "cy1")}
    ncx, ncy = plan.cx1 - plan.cx0, plan.cy1 - plan.cy0
    out["cellx"] = _copy(plan.cellx, W if plan.cellx else 0, np.int32)
    out["celly"] = _copy(plan.celly, H if plan.celly else 0, np.int32)
    out["complete_x"] = _copy(plan.complete_x, ncx, np.uint8).astype(bool)
    out["complete_y"] = _copy(plan.complete_y, ncy, np.uint8).astype(bool)
    out["shared"] = _copy(plan.shared, plan.n_shared, np.uint32)
    lib().gcn10_grid_plan_free(C.byref(plan))
    return out


def parse_storm(text: str):
    """"<P>[,<lambda>]" -> (P, lambda) (``gcn10_parse_storm``; lambda 0.2 when absent); raises HostError for any other
    text."""
    p, lam = C.c_double(), C.c_double()
    if lib().gcn10_parse_storm(text.encode(), C.byref(p), C.byref(lam)) != 0:
        raise HostError("bad value for storm: '%s' (P[,lambda]: 0 < P <= 650 mm, 0 <= lambda < 1)" % text)
    return p.value, lam.value


def parse_storms(text: str):
    """"<P1>[:<P2>...][,<lambda>]" -> ([P1, P2, ...], lambda) (``gcn10_parse_storms``; 1 to 8 rising depths, lambda 0.2
    when absent); raises HostError for any other text."""
    p, k, lam = (C.c_double * MAX_STORMS)(), C.c_int(), C.c_double()
    if lib().gcn10_parse_storms(text.encode(), p, C.byref(k), C.byref(lam)) != 0:
        raise HostError("bad value for storms: '%s' (P1[:P2...][,lambda]: 1 to 8 rising depths, 0 < P <= 650 mm, "
                        "0 <= lambda < 1)" % text)
    return list(p[:k.value]), lam.value


def runoff_table(P: float, lam: float = 0.2) -> np.ndarray:
    """The runoff depth of every raster value for a storm of P mm and initial-abstraction ratio lam, uint16[256] in units
    of 0.01 mm (``gcn10_runoff_table``)."""
    q = np.zeros(256, np.uint16)
    lib().gcn10_runoff_table(float(P), float(lam), q)
    return q


def runoff_cn(s: int, n: int, sw: int, q) -> int:
    """The runoff-equivalent curve number of a cell with sum s, count n and sum of q[value] sw
    (``gcn10_runoff_cn``)."""
    return int(lib().gcn10_runoff_cn(int(s), int(n), int(sw), np.ascontiguousarray(q, dtype=np.uint16).reshape(256)))


def parse_rain_unit(text: str):
    """"<unit>[,<lambda>]" -> (unit, lambda) (``gcn10_parse_rain_unit``; lambda 0.2 when absent); raises HostError for any
    other text."""
    unit, lam = C.c_double(), C.c_double()
    if lib().gcn10_parse_rain_unit(text.encode(), C.byref(unit), C.byref(lam)) != 0:
        raise HostError("bad value for rain_unit: '%s' (unit[,lambda]: 0 < unit, 255 unit <= 650 mm, 0 <= lambda < 1)"
                        % text)
    return unit.value, lam.value


def rain_tables(unit: float = 1.0, lam: float = 0.2) -> np.ndarray:
    """uint16[256][256]: table b is ``runoff_table(b * unit, lam)`` (``gcn10_rain_tables``)."""
    q = np.zeros((256, 256), np.uint16)
    lib().gcn10_rain_tables(float(unit), float(lam), q)
    return q


def runoff_bytes(q: np.ndarray, u: int) -> np.ndarray:
    """uint8[256][256]: the tables of rain_tables as bytes of an output unit of u hundredths of a millimetre, round half
    up, saturating at 254, 255 kept (``gcn10_runoff_bytes``)."""
    q = np.ascontiguousarray(q, np.uint16)
    if q.shape != (256, 256) or int(u) < 1:
        raise ValueError("runoff_bytes: q is uint16[256][256], u >= 1")
    t = np.zeros((256, 256), np.uint8)
    lib().gcn10_runoff_bytes(q, int(u), t)
    return t


def parse_runoff_unit(text: str) -> int:
    """"<mm>" -> the output unit in hundredths of a millimetre (``gcn10_parse_runoff_unit``); raises HostError for any
    other text."""
    u = C.c_uint()
    if lib().gcn10_parse_runoff_unit(text.encode(), C.byref(u)) != 0:
        raise HostError("bad value for runoff_unit: '%s' (millimetres per count, 0.01 to 650)" % text)
    return u.value


def rain_load(path: str, grid) -> np.ndarray:
    """The rainfall raster of the grid (a dict as parse_grid returns it), uint8[ny][nx] (``gcn10_rain_load``); raises
    HostError with the run's refusal text when the file cannot be read, has another size or does not lie on the grid."""
    g = Grid(**grid)
    out = C.c_void_p()
    err = C.create_string_buffer(4096 + 512)
    rc = lib().gcn10_rain_load(os.fsencode(path), C.byref(g), C.byref(out), err, len(err))
    if rc != 0:
        e = HostError(err.value.decode(errors="replace"))
        e.code = rc
        raise e
    try:
        n = grid["nx"] * grid["ny"]
        return np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), (n,)).copy().reshape(grid["ny"], grid["nx"])
    finally:
        lib().free_(out)


MAX_RAINS = 8       # GCN10_MAX_RAINS


def parse_rains(text: str):
    """"<file1>[:<file2>...]" -> [file1, file2, ...] (``gcn10_parse_rains``; 1 to 8 names, none empty); raises HostError
    for any other text."""
    copy, files, k = C.c_void_p(), (C.c_char_p * MAX_RAINS)(), C.c_int()
    if lib().gcn10_parse_rains(os.fsencode(text), C.byref(copy), files, C.byref(k)) != 0:
        raise HostError("bad value for rains: '%s' (file1[:file2...]: 1 to 8 files)" % text)
    try:
        return [os.fsdecode(files[j]) for j in range(k.value)]
    finally:
        lib().free_(copy)


def rains_load(paths, grid) -> np.ndarray:
    """The rainfall rasters of the grid, uint8[k][ny][nx] (``gcn10_rains_load``); raises HostError with the run's refusal
    text ("rains: ...") for the first file that cannot be read, has another size or does not lie on the grid."""
    g = Grid(**grid)
    k = len(paths)
    names = (C.c_char_p * max(k, 1))(*[os.fsencode(p) for p in paths])
    out = (C.c_void_p * MAX_RAINS)()
    err = C.create_string_buffer(8192)
    rc = lib().gcn10_rains_load(names, k, C.byref(g), out, err, len(err))
    if rc != 0:
        e = HostError(err.value.decode(errors="replace"))
        e.code = rc
        raise e
    try:
        n = grid["nx"] * grid["ny"]
        return np.stack([np.ctypeslib.as_array(C.cast(out[j], C.POINTER(C.c_uint8)), (n,)).copy()
                         for j in range(k)]).reshape(k, grid["ny"], grid["nx"])
    finally:
        for j in range(k):
            lib().free_(out[j])


def rains_cell(words, bytes_of_layers, q) -> list:
    """[cn_1 .. cn_k] of a cell with the words {s, n, sw_1 .. sw_k} and byte bytes_of_layers[j] in layer j, for the 256
    tables q (``gcn10_rains_cell``)."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    b = np.ascontiguousarray(bytes_of_layers, dtype=np.uint8)
    t = np.ascontiguousarray(q, dtype=np.uint16).reshape(256, 256)
    k = len(b)
    assert len(w) == 2 + k
    cn = np.zeros(k, np.uint8)
    lib().gcn10_rains_cell(w.ctypes.data, k, b.ctypes.data, t.ctypes.data, cn.ctypes.data)
    return cn.tolist()


def zone_rain_load(path: str):
    """The rainfall raster of a zonal run: (grid, bytes) -- the raster as a model grid (the dict of parse_grid) and
    uint8[ny][nx] (``gcn10_zone_rain_load``); raises HostError with the run's refusal text."""
    g = Grid()
    out = C.c_void_p()
    err = C.create_string_buffer(4096 + 512)
    if lib().gcn10_zone_rain_load(os.fsencode(path), C.byref(g), C.byref(out), err, len(err)) != 0:
        raise HostError(err.value.decode(errors="replace"))
    try:
        grid = {name: getattr(g, name) for name, _t in Grid._fields_}
        n = g.nx * g.ny
        return grid, np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), (n,)).copy().reshape(g.ny, g.nx)
    finally:
        lib().free_(out)


def rain_raster_load(prefix: str, path: str):
    """zone_rain_load with the messages under the key name `prefix` (``gcn10_rain_raster_load``): a runoff_rain run
    passes "runoff_rain"."""
    g = Grid()
    out = C.c_void_p()
    err = C.create_string_buffer(4096 + 512)
    if lib().gcn10_rain_raster_load(prefix.encode(), os.fsencode(path), C.byref(g), C.byref(out), err, len(err)) != 0:
        raise HostError(err.value.decode(errors="replace"))
    try:
        grid = {name: getattr(g, name) for name, _t in Grid._fields_}
        n = g.nx * g.ny
        return grid, np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), (n,)).copy().reshape(g.ny, g.nx)
    finally:
        lib().free_(out)


def runoff_unit_of(mm: float) -> int:
    """The output unit, in hundredths of a millimetre, that stands for a rain unit of `mm` (``gcn10_runoff_unit_of``)."""
    return lib().gcn10_runoff_unit_of(float(mm))


def zone_rain_values(rain_pixels: int, rain_sum: int, unit: float, lam: float, s: int, n: int, sw: int):
    """(rain_mm, runoff_mm_rain, cn_runoff_rain) of one row of the zonal table under a rainfall raster, None where the
    table leaves the field empty (``gcn10_zone_rain_values``)."""
    mm, ro, cn = C.c_double(), C.c_double(), C.c_int()
    f = lib().gcn10_zone_rain_values(int(rain_pixels), int(rain_sum), float(unit), float(lam), int(s), int(n), int(sw),
                                     C.byref(mm), C.byref(ro), C.byref(cn))
    return (mm.value if f & 1 else None, ro.value if f & 2 else None, cn.value if f & 2 else None)


def zone_rain_cut(plan: dict, W: int, H: int, gplan: dict, rain, max_span_px: int = 0, max_item_px: int = 0,
                  n_local: int | None = None) -> dict:
    """The spans of a block's zone plan (the dict of Zones.build_plan, or anything with ``spans``) cut where the byte of
    the rainfall raster changes (``gcn10_zone_rain_cut``).  gplan: the dict of grid_plan_block for the block on the
    raster's grid; rain: uint8[ny][nx].  ``spans`` (ZONE_SPAN_DTYPE, sorted by (zone, byte, y, x0)), ``items``
    (ZONE_RAIN_ITEM_DTYPE), ``rain_pixels`` and ``rain_sum`` (uint64 per local zone)."""
    sp = np.ascontiguousarray(plan["spans"], dtype=ZONE_SPAN_DTYPE)
    if n_local is None:
        n_local = len(plan["local_zone"]) if "local_zone" in plan else (int(sp["zone"].max()) + 1 if sp.size else 0)
    zp = ZonePlan()
    zp.n_local = int(n_local)
    zp.n_spans = sp.size
    zp.spans = sp.ctypes.data if sp.size else None
    r = np.ascontiguousarray(rain, dtype=np.uint8)
    cellx = np.ascontiguousarray(gplan["cellx"], dtype=np.int32)
    celly = np.ascontiguousarray(gplan["celly"], dtype=np.int32)
    if (cellx.size not in (0, W)) or (celly.size not in (0, H)) or r.ndim != 2:
        raise ValueError("cellx / celly must have W / H entries (or none), the raster two dimensions")
    out = ZoneRainPlan()
    rc = lib().gcn10_zone_rain_cut(C.byref(zp), int(W), int(H), cellx.ctypes.data if cellx.size else None,
                                   celly.ctypes.data if celly.size else None, int(gplan["cx0"]), int(gplan["cy0"]),
                                   r.ctypes.data, r.shape[1], r.shape[0], int(max_span_px), int(max_item_px),
                                   C.byref(out))
    if rc != 0:
        raise HostError("gcn10_zone_rain_cut: a span outside the block, a zone outside the plan, or out of memory")
    res = {"spans": _copy(out.spans, out.n_spans, ZONE_SPAN_DTYPE),
           "items": _copy(out.items, out.n_items, ZONE_RAIN_ITEM_DTYPE),
           "rain_pixels": _copy(out.rain_pixels, out.n_local, np.uint64),
           "rain_sum": _copy(out.rain_sum, out.n_local, np.uint64)}
    lib().gcn10_zone_rain_plan_free(C.byref(out))
    return res


def zone_rains_load(paths):
    """The rainfall rasters of a zonal run that takes several: (grid, uint8[k][ny][nx]), the grid that of the first file
    (``gcn10_zone_rains_load``); raises HostError with the run's refusal text ("zone_rains: ...") for the first file that
    cannot be taken, has another size than the first or does not lie on its grid."""
    g = Grid()
    k = len(paths)
    names = (C.c_char_p * max(k, 1))(*[os.fsencode(p) for p in paths])
    out = (C.c_void_p * MAX_RAINS)()
    err = C.create_string_buffer(8192)
    if lib().gcn10_zone_rains_load(names, k, C.byref(g), out, err, len(err)) != 0:
        e = HostError(err.value.decode(errors="replace"))
        e.left = [out[j] for j in range(MAX_RAINS)]     # what stayed allocated: all None
        raise e
    try:
        grid = {name: getattr(g, name) for name, _t in Grid._fields_}
        n = g.nx * g.ny
        return grid, np.stack([np.ctypeslib.as_array(C.cast(out[j], C.POINTER(C.c_uint8)), (n,)).copy()
                               for j in range(k)]).reshape(k, g.ny, g.nx)
    finally:
        for j in range(k):
            lib().free_(out[j])


def zone_rains_cut(plan: dict, W: int, H: int, gplan: dict, rains, max_span_px: int = 0, max_item_px: int = 0,
                   n_local: int | None = None) -> dict:
    """The spans of a block's zone plan cut where the byte of ANY of the k rainfall rasters changes
    (``gcn10_zone_rains_cut``).  gplan: the dict of grid_plan_block for the block on the rasters' grid; rains:
    uint8[k][ny][nx].  ``spans`` (ZONE_SPAN_DTYPE, sorted by (zone, tuple, y, x0)), ``items`` (ZONE_RAINS_ITEM_DTYPE),
    ``rain_pixels`` (uint64 per local zone) and ``rain_sum`` (uint64[k][n_local])."""
    sp = np.ascontiguousarray(plan["spans"], dtype=ZONE_SPAN_DTYPE)
    if n_local is None:
        n_local = len(plan["local_zone"]) if "local_zone" in plan else (int(sp["zone"].max()) + 1 if sp.size else 0)
    zp = ZonePlan()
    zp.n_local = int(n_local)
    zp.n_spans = sp.size
    zp.spans = sp.ctypes.data if sp.size else None
    r = np.ascontiguousarray(rains, dtype=np.uint8)
    cellx = np.ascontiguousarray(gplan["cellx"], dtype=np.int32)
    celly = np.ascontiguousarray(gplan["celly"], dtype=np.int32)
    if (cellx.size not in (0, W)) or (celly.size not in (0, H)) or r.ndim != 3:
        raise ValueError("cellx / celly must have W / H entries (or none), the rasters three dimensions")
    k = r.shape[0]
    layers = (C.c_void_p * max(k, 1))(*[r[j].ctypes.data for j in range(k)])
    out = ZoneRainsPlan()
    rc = lib().gcn10_zone_rains_cut(C.byref(zp), int(W), int(H), cellx.ctypes.data if cellx.size else None,
                                    celly.ctypes.data if celly.size else None, int(gplan["cx0"]), int(gplan["cy0"]),
                                    layers, k, r.shape[2], r.shape[1], int(max_span_px), int(max_item_px), C.byref(out))
    if rc != 0:
        raise HostError("gcn10_zone_rains_cut: k outside 1..8, a span outside the block, a zone outside the plan, or out "
                        "of memory")
    res = {"spans": _copy(out.spans, out.n_spans, ZONE_SPAN_DTYPE),
           "items": _copy(out.items, out.n_items, ZONE_RAINS_ITEM_DTYPE),
           "rain_pixels": _copy(out.rain_pixels, out.n_local, np.uint64),
           "rain_sum": np.stack([_copy(out.rain_sum[j], out.n_local, np.uint64) for j in range(k)])}
    lib().gcn10_zone_rains_plan_free(C.byref(out))
    return res


def parse_config(path: str) -> dict:
    """src/config.c:44-114 -> dict of the keys; raises HostError like the reference aborts."""
    cfg = ConfigRunoffRain()
    err = C.create_string_buffer(1024)
    rc = lib().gcn10_config_parse(os.fsencode(path), C.cast(C.pointer(cfg), C.POINTER(Config)), err, 1024)
    if rc != 0:
        raise HostError(err.value.decode(errors="replace"))
    out = {}
    for name, _t in (Config._fields_ + ConfigFull._fields_ + ConfigGrid._fields_ + ConfigStorm._fields_ +
                     ConfigStorms._fields_ + ConfigRain._fields_ + ConfigZoneRain._fields_ + ConfigRains._fields_ +
                     ConfigZoneRains._fields_ + ConfigRunoffRain._fields_):
        v = getattr(cfg, name)
        out[name] = v.decode() if isinstance(v, bytes) else list(v) if isinstance(v, C.Array) else v
    lib().gcn10_config_free(C.cast(C.pointer(cfg), C.POINTER(Config)))
    return out


class Log:
    def __init__(self, log_dir: str, rank: int):
        self._h = lib().gcn10_log_open(os.fsencode(log_dir), rank)

    def message(self, level, msg, also_console=False):
        lib().gcn10_log_message(self._h, None if level is None else level.encode(),
                                None if msg is None else msg.encode(), also_console)

    def close(self):
        if self._h:
            lib().gcn10_log_close(self._h)
            self._h = None


def read_block_list(path: str):
    n = C.c_int(0)
    p = lib().gcn10_read_block_list(os.fsencode(path), C.byref(n))
    if not p:
        return None
    ids = [p[i] for i in range(n.value)]
    lib().free_(C.cast(p, C.c_void_p))
    return ids


def read_blocks_shapefile(path: str):
    """-> (ids list, bbox float64[n,4] {minx,miny,maxx,maxy})."""
    b = Blocks()
    err = C.create_string_buffer(1024)
    if lib().gcn10_blocks_open(os.fsencode(path), C.byref(b), err, 1024) != 0:
        raise HostError(err.value.decode(errors="replace"))
    ids = [b.id[i] for i in range(b.n)]
    bbox = np.array([list(b.bbox[i]) for i in range(b.n)], dtype=np.float64).reshape(b.n, 4)
    lib().gcn10_blocks_free(C.byref(b))
    return ids, bbox


class _ChunkRef(C.Structure):
    """``struct gcn10_chunk_ref`` of csrc/host/host_internal.h."""
    _fields_ = [("fd", C.c_int), ("file_off", C.c_uint64), ("nbytes", C.c_uint32), ("chunk_w", C.c_uint32),
                ("rows", C.c_uint32), ("src_x", C.c_uint32), ("src_y", C.c_uint32), ("copy_w", C.c_uint32),
                ("copy_h", C.c_uint32), ("dst_x", C.c_uint32), ("dst_y", C.c_uint32), ("flags", C.c_uint32),
                ("out_len", C.c_uint32)]


class _ReadPlan(C.Structure):
    """``struct gcn10_read_plan`` of csrc/host/host_internal.h."""
    _fields_ = [("chunks", C.POINTER(_ChunkRef)), ("n", C.c_size_t), ("cap", C.c_size_t),
                ("opened", C.c_void_p), ("n_opened", C.c_int), ("covered", C.c_uint64),
                ("max_chunk_bytes", C.c_uint32), ("staged_bytes", C.c_uint64)]


# GCN10_CODEC_DEFLATE | GCN10_CODEC_RAW | GCN10_CODEC_LZW (include/gcn10_gpu.h)
PLAN_CODECS_LZW = 1 | 2 | 4


class Raster:
    """An open GeoTIFF / VRT (``gcn10_raster``)."""

    def __init__(self, path: str, tile_dir: str | None = None):
        err = C.create_string_buffer(1024)
        self._h = lib().gcn10_raster_open(os.fsencode(path),
                                          os.fsencode(tile_dir) if tile_dir else None, err, 1024)
        if not self._h:
            raise HostError(err.value.decode(errors="replace"))
        xs, ys = C.c_int(), C.c_int()
        gt = np.empty(6, dtype=np.float64)
        lib().gcn10_raster_info(self._h, C.byref(xs), C.byref(ys), gt)
        self.xsize, self.ysize, self.gt = xs.value, ys.value, gt.tolist()

    def read(self, xoff, yoff, xcount, ycount) -> np.ndarray:
        out = np.empty((ycount, xcount), dtype=np.uint8)
        err = C.create_string_buffer(1024)
        if lib().gcn10_raster_read(self._h, xoff, yoff, xcount, ycount, out.ctypes.data, err, 1024) != 0:
            raise HostError(err.value.decode(errors="replace"))
        return out

    def georef_ptr(self):
        return lib().gcn10_raster_georef(self._h)

    def plan(self, xoff, yoff, xcount, ycount, lzw=False):
        """The read plan the pipeline hands to the GPU decoder (gcn10_raster_plan_window,
        host_internal.h): None when the window has to go through the host reader, else
        (chunks, covered_pixels, max_chunk_bytes) with chunks = list of dicts holding the
        compressed bytes of a tile or strip and where its wanted part goes.  lzw=True: LZW chunks
        are planned too (gcn10_raster_plan_window_codecs with the LZW codec, what the pipeline
        asks for with gpu_inflate_lzw=1)."""
        plan = _ReadPlan()
        err = C.create_string_buffer(1024)
        L = lib()
        L.gcn10_raster_plan_window.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(_ReadPlan), C.c_char_p, C.c_size_t]
        L.gcn10_raster_plan_window.restype = C.c_int
        L.gcn10_raster_plan_window_codecs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint,
                                                      C.POINTER(_ReadPlan), C.c_char_p, C.c_size_t]
        L.gcn10_raster_plan_window_codecs.restype = C.c_int
        L.gcn10_read_plan_free.argtypes = [C.POINTER(_ReadPlan)]
        L.gcn10_read_plan_free.restype = None
        if lzw:
            rc = L.gcn10_raster_plan_window_codecs(self._h, xoff, yoff, xcount, ycount, PLAN_CODECS_LZW,
                                                   C.byref(plan), err, 1024)
        else:
            rc = L.gcn10_raster_plan_window(self._h, xoff, yoff, xcount, ycount, C.byref(plan), err, 1024)
        if rc < 0:
            raise HostError(err.value.decode(errors="replace"))
        if rc > 0:
            return None
        try:
            chunks = []
            for i in range(plan.n):
                c = plan.chunks[i]
                chunks.append({"data": os.pread(c.fd, c.nbytes, c.file_off), "chunk_w": c.chunk_w, "rows": c.rows,
                               "src_x": c.src_x, "src_y": c.src_y, "copy_w": c.copy_w, "copy_h": c.copy_h,
                               "dst_x": c.dst_x, "dst_y": c.dst_y, "flags": c.flags, "out_len": c.out_len})
            return chunks, plan.covered, plan.max_chunk_bytes
        finally:
            L.gcn10_read_plan_free(C.byref(plan))

    def close(self):
        if self._h:
            lib().gcn10_raster_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def save_raster(data: np.ndarray, gt, path: str, georef_ptr=None, level: int = 0):
    """src/raster.c:192-227: tiled DEFLATE GeoTIFF of a uint8 raster."""
    a = np.ascontiguousarray(data, dtype=np.uint8)
    err = C.create_string_buffer(1024)
    rc = lib().gcn10_save_raster(a.ctypes.data, a.shape[1], a.shape[0], _f(gt, 6), georef_ptr,
                                 os.fsencode(path), level, err, 1024)
    if rc != 0:
        raise HostError(err.value.decode(errors="replace"))


def cog_levels(xsize: int, ysize: int) -> int:
    """Overview levels of a COG of that size (GDAL's rule with BLOCKSIZE=256)."""
    return lib().gcn10_cog_levels(xsize, ysize)


class TiffWriter:
    """The streaming GeoTIFF writer (``gcn10_tiff_create`` / ``gcn10_tiff_create_cog``): tiles go in already
    compressed.  ``n_levels=None``: a plain file; an int: a COG with that many overview levels.  ``put_*`` return
    the C result (0 or -1) so that refused puts can be seen."""

    def __init__(self, path: str, xsize: int, ysize: int, gt, n_levels=None, georef_ptr=None,
                 compression: int = 8, direct: bool = False):
        err = C.create_string_buffer(1024)
        L = lib()
        if n_levels is None:
            self._h = L.tiff_create_(os.fsencode(path), xsize, ysize, _f(gt, 6), georef_ptr, err, 1024)
        else:
            self._h = L.gcn10_tiff_create_cog(os.fsencode(path), xsize, ysize, _f(gt, 6), georef_ptr, n_levels,
                                              err, 1024)
        if not self._h:
            raise HostError(err.value.decode(errors="replace"))
        if compression != 8 and L.gcn10_tiff_set_compression(self._h, compression) != 0:
            self.abort()
            raise HostError("bad compression %d" % compression)
        self.direct = bool(direct) and L.gcn10_tiff_set_direct(self._h, True) == 0

    def _level(self, level):
        v = lib().gcn10_tiff_level(self._h, level)
        if not v:
            raise HostError("no overview level %d" % level)
        return v

    @property
    def n_levels(self):
        return lib().gcn10_tiff_n_levels(self._h)

    def tiles(self, level=0):
        v = self._level(level)
        return lib().gcn10_tiff_tiles_across(v), lib().gcn10_tiff_tiles_down(v)

    def put_tile(self, tx, ty, data: bytes, level=0) -> int:
        return lib().gcn10_tiff_put_tile(self._level(level), tx, ty, data, len(data))

    def put_tiles(self, tiles, level=0) -> int:
        """tiles: [(tx, ty, bytes)] put with one gcn10_tiff_put_tiles (gathered writes from separate buffers)."""
        n = len(tiles)
        bufs = [C.create_string_buffer(bytes(t[2]), len(t[2])) for t in tiles]
        txs = (C.c_int * n)(*[t[0] for t in tiles])
        tys = (C.c_int * n)(*[t[1] for t in tiles])
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_uint32 * n)(*[len(t[2]) for t in tiles])
        return lib().gcn10_tiff_put_tiles(self._level(level), n, txs, tys, ptrs, sizes)

    def put_extent(self, tiles, level=0) -> int:
        """tiles: [(tx, ty, bytes)] laid out back to back (16-byte slots, as the GPU encoders do) and put
        with one gcn10_tiff_put_extent.  The extent buffer is 4096-aligned and padded for direct I/O."""
        rel, off = [], 0
        for _tx, _ty, d in tiles:
            rel.append(off)
            off = (off + len(d) + 15) & ~15
        size = max(off, 1)
        buf = np.zeros(((size + 4095) // 4096 + 2) * 4096, np.uint8)
        base = (-buf.ctypes.data) % 4096
        for (_tx, _ty, d), r in zip(tiles, rel):
            buf[base + r:base + r + len(d)] = np.frombuffer(d, np.uint8)
        n = len(tiles)
        txs = (C.c_int * n)(*[t[0] for t in tiles])
        tys = (C.c_int * n)(*[t[1] for t in tiles])
        rels = (C.c_uint32 * n)(*rel)
        sizes = (C.c_uint32 * n)(*[len(t[2]) for t in tiles])
        end = rel[-1] + len(tiles[-1][2]) if n else 0
        return lib().gcn10_tiff_put_extent(self._level(level), buf.ctypes.data + base, end, n, txs, tys, rels, sizes)

    def set_nodata(self, v: int) -> int:
        return lib().gcn10_tiff_set_nodata(self._h, v)

    def set_metadata_xml(self, xml) -> int:
        return lib().gcn10_tiff_set_metadata_xml(self._h, None if xml is None else xml.encode())

    def reserve_metadata(self, nbytes: int = None) -> int:
        return lib().gcn10_tiff_reserve_metadata(self._h, STATS_XML_MAX if nbytes is None else nbytes)

    def finish(self):
        err = C.create_string_buffer(1024)
        h, self._h = self._h, None
        if lib().gcn10_tiff_finish(h, err, 1024) != 0:
            raise HostError(err.value.decode(errors="replace"))

    def abort(self):
        if self._h:
            lib().gcn10_tiff_abort(self._h)
            self._h = None


STATS_XML_MAX = 512        # GCN10_STATS_XML_MAX


def raster_histogram(pair_hist, codes, table, drained: bool) -> np.ndarray:
    """One raster's histogram (256 uint64) from a block's pair histogram ([16][256] uint64, gcn10_gpu_pair_histogram),
    the bins' soil codes (gpu.pair_histogram_codes()) and the raster's lookup table (int[256][5])
    (gcn10_raster_histogram)."""
    pair = np.ascontiguousarray(pair_hist, dtype=np.uint64).reshape(-1)
    if pair.size != 16 * 256:
        raise ValueError("pair histogram must have 16 x 256 counters")
    out = np.zeros(256, np.uint64)
    lib().gcn10_raster_histogram(pair, np.ascontiguousarray(codes, dtype=np.uint8).reshape(16),
                                 np.ascontiguousarray(table, dtype=np.int32).reshape(256, 5), int(bool(drained)), out)
    return out


#: findings of verify_structure (GCN10_VERIFY_* of include/gcn10_host.h), by code
VERIFY_FINDINGS = ("ok", "missing", "not a TIFF", "not 1 band Byte", "size", "geotransform", "chunk", "overview size",
                   "decode", "pixels")


def verify_structure(path: str, xsize: int, ysize: int, gt) -> dict:
    """The structure checks a verify run makes on one output raster before any pixel work (gcn10_verify_structure):
    ``finding`` (a VERIFY_FINDINGS name, "ok" = none), ``code``, ``reason`` and ``n_levels``, the overview directories
    behind the raster."""
    L = lib()
    L.gcn10_verify_structure.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                         C.c_char_p, C.c_size_t]
    L.gcn10_verify_structure.restype = C.c_int
    g = (C.c_double * 6)(*[float(v) for v in gt])
    n = C.c_int(0)
    reason = C.create_string_buffer(1024)
    code = L.gcn10_verify_structure(os.fsencode(path), int(xsize), int(ysize), g, C.byref(n), reason, 1024)
    return {"code": code, "finding": VERIFY_FINDINGS[code], "reason": reason.value.decode(errors="replace"),
            "n_levels": n.value}


def band_stats(hist, nodata=None) -> dict:
    """GDAL's statistics of a Byte band from its histogram (gcn10_band_stats_of): total, valid, min, max, mean,
    stddev, valid_percent, and ``xml``, the GDAL_METADATA text gcn10_stats_xml makes of them (None: no valid pixel)."""
    h = np.ascontiguousarray(hist, dtype=np.uint64).reshape(256)
    st = BandStats()
    lib().gcn10_band_stats_of(h, -1 if nodata is None else int(nodata), C.byref(st))
    buf = C.create_string_buffer(STATS_XML_MAX)
    n = lib().gcn10_stats_xml(C.byref(st), buf, STATS_XML_MAX)
    out = {name: getattr(st, name) for name, _t in BandStats._fields_}
    out["xml"] = buf.value.decode() if n else None
    return out


def _f(v, n):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(n))


class LookupError_(RuntimeError):
    pass


def load_lookup_file(path: str):
    """One CSV -> (int32[256,5] table, [messages of rejected rows])."""
    table = np.empty((256, 5), dtype=np.int32)
    msgs = []
    cb = ROW_ERROR_FN(lambda _u, m: msgs.append(m.decode(errors="replace")))
    rc = lib().gcn10_load_lookup_file(os.fsencode(path), table, cb, None)
    if rc == -1:
        raise LookupError_("cannot open lookup table %s" % path)       # src/cn.c:30
    if rc == -2:
        raise LookupError_("empty lookup table %s" % path)             # src/cn.c:44
    return table, msgs


def load_all_lookup_tables(lookup_dir: str) -> np.ndarray:
    """The nine tables of a run, int32[9,256,5], k = hc*3 + arc."""
    tables = np.empty((9, 256, 5), dtype=np.int32)
    failed = C.c_int(-1)
    cb = ROW_ERROR_FN(lambda _u, m: None)
    rc = lib().gcn10_load_all_lookup_tables(os.fsencode(lookup_dir), tables.reshape(-1),
                                            C.byref(failed), cb, None)
    if rc != 0:
        k = failed.value
        raise LookupError_("lookup table %s_%s in %s: error %d" %
                           (HCS[k // 3], ARCS[k % 3], lookup_dir, rc))
    return tables


def build_index_maps(gt, soil_gt, W: int, H: int, hsx: int, hsy: int):
    ci = np.empty(W, dtype=np.int32)
    cj = np.empty(H, dtype=np.int32)
    lib().gcn10_build_index_maps(_f(gt, 6), _f(soil_gt, 6), W, H, hsx, hsy, ci, cj)
    return ci, cj


def raster_window(t, rx: int, ry: int, bbox):
    """src/raster.c:126-162 -> (xoff, yoff, xcount, ycount, gt) or None."""
    xo, yo, xc, yc = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    gt = np.empty(6, dtype=np.float64)
    rc = lib().gcn10_raster_window(_f(t, 6), rx, ry, _f(bbox, 4), C.byref(xo), C.byref(yo),
                                   C.byref(xc), C.byref(yc), gt)
    if rc != 0:
        return None
    return xo.value, yo.value, xc.value, yc.value, gt.tolist()
