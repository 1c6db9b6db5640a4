"""GPU: the verification mode of the gcn10 program (--verify / verify=1) end to end on a small synthetic world.
Rasters the program wrote verify and stay untouched; rasters an independent writer (tests/tiffutil.py) made from the
oracle's pixels verify in layouts the program never produces; every kind of damage is reported as what it is, with
exit code 2 and the block in verify_failed_blocks.txt.  The expected pixels always come from the oracle."""
import hashlib
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from oracle import cn_oracle_c as oc
from tests import tiffutil
from tests.conftest import LOOKUPS, ROOT
from tests.util import ESA_NASTY, HSG_NASTY

pytestmark = pytest.mark.gpu

GCN10 = os.path.join(ROOT, "bin", "gcn10")
CONDS, HCS, ARCS = ("drained", "undrained"), ("p", "f", "g"), ("i", "ii", "iii")
ESA_GT = [10.0, 0.001, 0.0, 50.0, 0.0, -0.001]
SOIL_GT = [9.9875, 0.025, 0.0, 50.0125, 0.0, -0.025]
BLOCKS = [(101, 10.0, 49.0, 11.0, 50.0),       # 1000 x 1000: 2 overview levels
          (103, 12.5, 47.5, 13.5, 48.5),       # cut by the landcover's edge: 500 px wide, 1 level
          (105, 11.3, 49.6, 11.5, 49.85),      # 200 x 250: no overview level
          (106, 10.5, 48.2, 10.7, 48.8)]       # 200 x 600: 2 levels


def raster_path(tmp_path, r, bid):
    c, k = divmod(r, 9)
    return tmp_path / ("cn_rasters_%s" % CONDS[c]) / ("cn_%s_%s_%d.tif" % (HCS[k // 3], ARCS[k % 3], bid))


def raster_name(r):
    c, k = divmod(r, 9)
    return "%s/%s/%s" % (CONDS[c], HCS[k // 3], ARCS[k % 3])


def world(tmp_path, ids, seed=5, extra_cfg="", lookups=LOOKUPS):
    rng = np.random.default_rng(seed)
    small = rng.choice(ESA_NASTY, size=(2000 // 20, 3000 // 20))
    esa = np.repeat(np.repeat(small, 20, axis=0), 20, axis=1)
    noise = rng.integers(0, 256, size=esa.shape, dtype=np.uint8)
    esa = np.where(noise < 30, rng.choice(ESA_NASTY, size=esa.shape), esa).astype(np.uint8)
    soil = rng.choice(HSG_NASTY, size=(2000 // 25 + 2, 3000 // 25 + 2)).astype(np.uint8)
    tiffutil.write_tiff(str(tmp_path / "esa.tif"), esa, gt=ESA_GT, compression=8, tile=(512, 512))
    tiffutil.write_tiff(str(tmp_path / "soil.tif"), soil, gt=SOIL_GT, compression=8, tile=(64, 64))
    tiffutil.write_block_shapefile(str(tmp_path / "blocks"), BLOCKS)
    config(tmp_path, extra_cfg, lookups)
    (tmp_path / "ids.txt").write_text(" ".join(str(i) for i in ids) + "\n")
    return esa, soil


def config(tmp_path, extra_cfg="", lookups=LOOKUPS, name="config.txt"):
    (tmp_path / name).write_text(
        "hysogs_data_path=%s\nesa_data_path=%s\nblocks_shp_path=%s\nlookup_table_path=%s\nlog_dir=%s\n"
        "strip_rows=256\nio_threads=4\nworkers_per_gpu=1\n%s"
        % (tmp_path / "soil.tif", tmp_path / "esa.tif", tmp_path / "blocks.shp", lookups, tmp_path / "logs", extra_cfg))


def run(tmp_path, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([GCN10, *args], cwd=str(tmp_path), capture_output=True, text=True, env=e, timeout=600)


def verify(tmp_path, *args, ids="ids.txt", cfg="config.txt"):
    """Runs --verify; returns (process, the log lines this run added to every rank's log, the failed list)."""
    logs = tmp_path / "logs"
    before = {p.name: len(p.read_text().splitlines()) for p in logs.glob("rank_*.log")} if logs.exists() else {}
    out = run(tmp_path, "-c", cfg, "-l", ids, "--verify", *args)
    lines = []
    for p in sorted(logs.glob("rank_*.log")):
        lines += p.read_text().splitlines()[before.get(p.name, 0):]
    failed = logs / "verify_failed_blocks.txt"
    return out, lines, (failed.read_text() if failed.exists() else None)


def digest(tmp_path):
    """names, sizes, bytes and mtimes of everything under the two output directories"""
    h = hashlib.sha256()
    n = 0
    for c in CONDS:
        d = tmp_path / ("cn_rasters_%s" % c)
        for name in sorted(os.listdir(d)) if d.exists() else []:
            st = os.stat(d / name)
            h.update(("%s/%s %d %d\n" % (c, name, st.st_size, st.st_mtime_ns)).encode())
            h.update((d / name).read_bytes())
            n += 1
    return n, h.hexdigest()


def oracle_block(esa, soil, tables, bid):
    bbox = [b[1:] for b in BLOCKS if b[0] == bid][0]
    xo, yo, W, H, gt = oc.window(ESA_GT, esa.shape[1], esa.shape[0], list(bbox))
    sxo, syo, hsx, hsy, sgt = oc.window(SOIL_GT, soil.shape[1], soil.shape[0], list(bbox))
    want = oc.process_block_mem(esa[yo:yo + H, xo:xo + W], gt, soil[syo:syo + hsy, sxo:sxo + hsx], sgt, tables)
    return want, gt


def write_oracle_block(tmp_path, want, gt, bid, layout, replace=None):
    """The 18 oracle rasters of a block through the independent writer; replace: {raster: pixels} instead."""
    for c in CONDS:
        os.makedirs(tmp_path / ("cn_rasters_%s" % c), exist_ok=True)
    for r in range(18):
        img = want[r] if not replace or r not in replace else replace[r]
        tiffutil.write_tiff(str(raster_path(tmp_path, r, bid)), img, gt=gt, **layout)


def count(lines, word, bid=None):
    return sum(1 for l in lines if re.search(r"\] %s block %s:" % (word, bid if bid is not None else r"\d+"), l))


LAYOUTS = {
    "lzw strips predictor 2": dict(compression=5, rows_per_strip=37, predictor=2),
    "deflate tiles 512": dict(compression=8, tile=(512, 512)),
    "uncompressed": dict(compression=1, rows_per_strip=64),
    "deflate tiles 256": dict(compression=8, tile=(256, 256)),
}


# ---- what the program wrote ------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [(), ("--compress", "lzw"), ("--cog",), ("--cog", "--overview-resampling", "average"),
                                  ("--stats", "--nodata", "255")], ids=lambda a: " ".join(a) or "default")
def test_written_rasters_verify_and_stay_untouched(tmp_path, args):
    ids = [106, 105, 101, 103]
    world(tmp_path, ids)
    out = run(tmp_path, "-c", "config.txt", "-l", "ids.txt", *args)
    assert out.returncode == 0, out.stderr[-2000:]
    before = digest(tmp_path)
    assert before[0] == 18 * len(ids)
    out, lines, failed = verify(tmp_path, *args)
    print("\n".join(l for l in lines if "verif" in l or "MISMATCH" in l or "UNREADABLE" in l)[-3000:])
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    for bid in ids:
        assert count(lines, "verified", bid) == 18, bid
    assert count(lines, "MISMATCH") == count(lines, "MISSING") == count(lines, "UNREADABLE") == 0
    assert failed == ""
    assert ("verify: 4 blocks, 72 files verified, 0 bad, 0 missing, 0 overview levels not checked"
            in out.stdout + out.stderr)
    assert digest(tmp_path) == before           # nothing written, nothing touched, no `..._.tif` beside the files


def test_subset_of_rasters(tmp_path):
    world(tmp_path, [101, 105])
    sel = ("--lookups", "g_ii,p_i", "--conditions", "undrained")
    assert run(tmp_path, "-c", "config.txt", "-l", "ids.txt", *sel).returncode == 0
    out, lines, failed = verify(tmp_path, *sel)
    assert out.returncode == 0 and count(lines, "verified") == 4 and failed == ""
    # the whole set is not there: the other 16 rasters of each block are missing
    out, lines, failed = verify(tmp_path)
    assert out.returncode == 2
    assert count(lines, "verified") == 4 and count(lines, "MISSING") == 32
    assert failed == "101\n105\n"


# ---- what an independent writer wrote ----------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(LAYOUTS)[:3])
def test_oracle_rasters_of_an_independent_writer_verify(tmp_path, tables, layout):
    ids = [101, 103, 105]
    esa, soil = world(tmp_path, ids)
    for bid in ids:
        want, gt = oracle_block(esa, soil, tables, bid)
        write_oracle_block(tmp_path, want, gt, bid, LAYOUTS[layout])
    before = digest(tmp_path)
    out, lines, failed = verify(tmp_path)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert count(lines, "verified") == 54 and failed == ""
    assert digest(tmp_path) == before


@pytest.mark.parametrize("layout,r,where", [
    ("lzw strips predictor 2", 7, "first"), ("deflate tiles 512", 0, "last"), ("uncompressed", 13, "middle"),
    ("deflate tiles 256", 17, "first"), ("deflate tiles 256", 9, "last"), ("deflate tiles 256", 4, "middle")])
def test_one_changed_pixel_is_found(tmp_path, tables, layout, r, where):
    esa, soil = world(tmp_path, [101, 105])
    for bid in (101, 105):
        want, gt = oracle_block(esa, soil, tables, bid)
        if bid == 101:
            H, W = want[r].shape
            y, x = {"first": (0, 0), "last": (H - 1, W - 1), "middle": (517, 259)}[where]
            bad = want[r].copy()
            bad[y, x] = (int(bad[y, x]) + 3) % 256
            expected, in_file = int(want[r][y, x]), int(bad[y, x])
            write_oracle_block(tmp_path, want, gt, bid, LAYOUTS[layout], replace={r: bad})
        else:
            write_oracle_block(tmp_path, want, gt, bid, LAYOUTS[layout])
    out, lines, failed = verify(tmp_path)
    assert out.returncode == 2, (out.stdout[-2000:], out.stderr[-2000:])
    mism = [l for l in lines if "MISMATCH" in l]
    assert len(mism) == 1, mism
    assert ("MISMATCH block 101: %s: 1 pixels differ, first at x=%d y=%d (level 0): file %d, expected %d"
            % (raster_name(r), x, y, in_file, expected)) in mism[0]
    assert "MISMATCH block 101" in out.stdout + out.stderr          # also on the console
    assert count(lines, "verified", 101) == 17 and count(lines, "verified", 105) == 18
    assert failed == "101\n"
    assert "verify: 2 blocks, 35 files verified, 1 bad, 0 missing" in out.stdout + out.stderr


# ---- damaged files -------------------------------------------------------------------------------------------------

def damage(tmp_path, kind, want, gt, r, bid):
    p = raster_path(tmp_path, r, bid)
    if kind == "deleted":
        os.unlink(p)
    elif kind == "cut":                         # in the middle of its tile data
        data = p.read_bytes()
        p.write_bytes(data[:len(data) // 2])
    elif kind == "noise":                       # the bytes of the first tile (a zlib stream at offset 8) overwritten
        first = np.zeros((256, 256), np.uint8)
        first[:, :] = want[r][:256, :256]
        n = len(zlib.compress(first.tobytes(), 6))
        data = bytearray(p.read_bytes())
        assert bytes(data[8:8 + n]) == zlib.compress(first.tobytes(), 6)
        data[8:8 + n] = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8).tobytes()
        p.write_bytes(bytes(data))
    elif kind == "width":
        tiffutil.write_tiff(str(p), want[r][:, :-1], gt=gt, **LAYOUTS["deflate tiles 256"])
    elif kind == "shifted":
        g = list(gt)
        g[0] += g[1]
        tiffutil.write_tiff(str(p), want[r], gt=g, **LAYOUTS["deflate tiles 256"])
    elif kind == "not a tiff":
        p.write_bytes(b"not a raster at all\n" * 10)


@pytest.mark.parametrize("kind,word,reason", [
    ("deleted", "MISSING", ""),
    ("cut", "UNREADABLE", ""),
    ("noise", "UNREADABLE|MISMATCH", ""),
    ("width", "UNREADABLE", "size 999x1000, the block's window is 1000x1000"),
    ("shifted", "UNREADABLE", "geotransform"),
    ("not a tiff", "UNREADABLE", "not a TIFF"),
])
def test_damaged_file_is_reported_and_the_rest_verified(tmp_path, tables, kind, word, reason):
    esa, soil = world(tmp_path, [101, 106])
    for bid in (101, 106):
        want, gt = oracle_block(esa, soil, tables, bid)
        write_oracle_block(tmp_path, want, gt, bid, LAYOUTS["deflate tiles 256"])
    want, gt = oracle_block(esa, soil, tables, 101)
    r = 11
    damage(tmp_path, kind, want, gt, r, 101)
    out, lines, failed = verify(tmp_path)
    found = [l for l in lines if re.search(r"\] (%s) block 101: %s" % (word, raster_name(r)), l)]
    print("\n".join(found), out.returncode)
    assert out.returncode == 2, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])      # ended normally
    assert len(found) == 1 and reason in found[0], [l for l in lines if "block 101" in l and "verified" not in l]
    assert count(lines, "verified", 101) == 17 and count(lines, "verified", 106) == 18
    assert failed == "101\n"
    assert "processed 2 blocks" in "\n".join(lines)


def test_cut_cog_names_the_chunk_beyond_the_end(tmp_path):
    world(tmp_path, [101])
    assert run(tmp_path, "-c", "config.txt", "-l", "ids.txt", "--cog").returncode == 0
    p = raster_path(tmp_path, 4, 101)
    data = p.read_bytes()
    p.write_bytes(data[:len(data) * 3 // 4])
    out, lines, failed = verify(tmp_path, "--cog")
    assert out.returncode == 2
    found = [l for l in lines if "UNREADABLE block 101: %s" % raster_name(4) in l]
    assert len(found) == 1 and "chunk" in found[0] and "beyond the end of the file" in found[0], found
    assert count(lines, "verified", 101) == 17 and failed == "101\n"


def test_tables_of_another_condition_show_in_that_table_only(tmp_path):
    world(tmp_path, [101, 106])
    assert run(tmp_path, "-c", "config.txt", "-l", "ids.txt").returncode == 0
    other = tmp_path / "lookups"
    shutil.copytree(LOOKUPS, other)
    shutil.copyfile(other / "default_lookup_p_i.csv", other / "default_lookup_g_ii.csv")
    config(tmp_path, lookups=other, name="other.txt")
    out, lines, failed = verify(tmp_path, cfg="other.txt")
    assert out.returncode == 2
    mism = sorted(l.split("MISMATCH ")[1].split(": ")[1] for l in lines if "MISMATCH" in l)
    assert mism == sorted(["drained/g/ii", "undrained/g/ii"] * 2), mism
    assert count(lines, "verified") == 32 and failed == "101\n106\n"


# ---- overviews -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("built,checked", [("nearest", "average"), ("average", "nearest")])
def test_overviews_of_the_other_resampling_differ_above_level_0(tmp_path, built, checked):
    world(tmp_path, [101, 105, 106])
    assert run(tmp_path, "-c", "config.txt", "-l", "ids.txt", "--cog", "--overview-resampling", built).returncode == 0
    out, lines, failed = verify(tmp_path, "--overview-resampling", built)          # (cog=... is not needed to verify)
    assert out.returncode == 0 and count(lines, "verified") == 54
    out, lines, failed = verify(tmp_path, "--overview-resampling", checked)
    assert out.returncode == 2
    mism = [l for l in lines if "MISMATCH" in l]
    levels = [int(re.search(r"\(level (\d+)\)", l).group(1)) for l in mism]
    assert mism and min(levels) >= 1, mism[:3]
    assert all("block 105" not in l for l in mism)         # 200 x 250: no level, nothing to differ
    assert count(lines, "verified", 105) == 18 and failed == "101\n106\n"


# ---- the failed list feeds a write run -------------------------------------------------------------------------------

def test_failed_list_regenerates_exactly_those_blocks(tmp_path):
    ids = [101, 103, 105, 106]
    world(tmp_path, ids)
    assert run(tmp_path, "-c", "config.txt", "-l", "ids.txt").returncode == 0
    os.unlink(raster_path(tmp_path, 3, 106))
    p = raster_path(tmp_path, 16, 103)
    data = bytearray(p.read_bytes())
    data[len(data) // 3:len(data) // 3 + 64] = bytes(64)
    p.write_bytes(bytes(data))
    untouched = {bid: [os.stat(raster_path(tmp_path, r, bid)).st_mtime_ns for r in range(18)] for bid in (101, 105)}
    out, lines, failed = verify(tmp_path)
    assert out.returncode == 2 and failed == "103\n106\n", (out.returncode, failed)
    out = run(tmp_path, "-c", "config.txt", "-l", "logs/verify_failed_blocks.txt", "-o")
    assert out.returncode == 0 and "processing 2 blocks" in out.stdout + out.stderr
    for bid in (101, 105):
        assert untouched[bid] == [os.stat(raster_path(tmp_path, r, bid)).st_mtime_ns for r in range(18)]
    out, lines, failed = verify(tmp_path)
    assert out.returncode == 0 and count(lines, "verified") == 72 and failed == ""


def test_two_blocks_two_workers(tmp_path):
    world(tmp_path, [101, 106], extra_cfg="workers_per_gpu=2\n")
    assert run(tmp_path, "-c", "config.txt", "-l", "ids.txt", "--gpus", "1").returncode == 0
    os.unlink(raster_path(tmp_path, 9, 106))
    out, lines, failed = verify(tmp_path, "--gpus", "1")
    assert out.returncode == 2
    assert (tmp_path / "logs" / "rank_1.log").exists()
    assert count(lines, "verified", 101) == 18 and count(lines, "verified", 106) == 17
    assert count(lines, "MISSING", 106) == 1 and failed == "106\n"
    assert "verify: 2 blocks, 35 files verified, 0 bad, 1 missing" in out.stdout + out.stderr
