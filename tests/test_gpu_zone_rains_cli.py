"""GPU: a zonal run under several rainfall rasters (bin/gcn10 --zones ... --zone-rains a:b:c) end to end, on the small
world of tests/test_gpu_zonal_cli.py with the grid of tests/test_gpu_zone_rain_cli.py.  Three files: a random field, a
second random field and a constant.  Every new column against the numpy oracle of that file, per layer; each layer's three
columns, rain_pixels and rain_valid, as text, against the run --zone-rain <file_j>; the old columns, as text, against the
run without the key; the two log lines per raster; and with one file the table of --zone-rain, byte for byte."""
import numpy as np
import pytest

from tests import runoffutil as ru
from tests import tiffutil
from tests.test_gpu_zonal_cli import ZONES, _run, world  # noqa: F401  (the world and its one plain run)
from tests.test_gpu_zone_rain_cli import ATLAS, BASE, LAM, NEW, UNIT, _config, _expected, _gt, _rows

pytestmark = pytest.mark.gpu

FILES = ["first.tif", "second.tif", "flat.tif"]
MANY = BASE + ",rain_pixels,rain_valid" + "".join(",rain_mm_rain%d,runoff_mm_rain%d,cn_runoff_rain%d" % (j, j, j)
                                                  for j in (1, 2, 3))


def _fields():
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, (ATLAS["ny"], ATLAS["nx"])).astype(np.uint8)
    a[0, :3] = (0, 255, 0)
    b = rng.integers(0, 256, (ATLAS["ny"], ATLAS["nx"])).astype(np.uint8)
    b[:, ::2] = a[:, ::2]                               # half of the cells share the byte of the first layer
    b[0, :3] = (255, 0, 0)
    return [a, b, np.full_like(a, 20)]


@pytest.fixture(scope="module")
def runs(world):  # noqa: F811
    """the run with three files (table 21), and --zone-rain with each of them alone (tables 22 to 24)"""
    d = world["dir"]
    assert world["run1"].returncode == 0
    fields = _fields()
    for name, f, kw in zip(FILES, fields, (dict(compression=8, tile=(16, 16)), {}, {})):
        tiffutil.write_tiff(str(d / name), f, gt=_gt(ATLAS), **kw)
    many = _run(d, "-c", _config(d, 21), "--zones", "zones.shp", "--zone-rains", ":".join(FILES), "--zone-rain-unit", "2.5")
    assert many.returncode == 0, many.stdout[-2000:] + many.stderr[-2000:]
    for j, name in enumerate(FILES):
        one = _run(d, "-c", _config(d, 22 + j), "--zones", "zones.shp", "--zone-rain", name, "--zone-rain-unit", "2.5")
        assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-2000:]
    return {"dir": d, "fields": fields, "many": many, "rows": _rows(d / "table21.csv", MANY)}


def test_every_new_column_equals_the_numpy_oracle_per_layer(world, runs):  # noqa: F811
    q = np.stack([ru.table(b * UNIT, LAM) for b in range(256)]).astype(np.int64)
    rows = runs["rows"]
    assert len(rows) == len(ZONES) * 18 and all(len(r) == 11 + 2 + 9 for r in rows)
    some = 0
    for j, field in enumerate(runs["fields"]):
        want = _expected(world["blocks"], ATLAS, field, q)
        assert 0 < want[0][0] < world["want"][0][0][0] and want[6][0] == 0     # partly under the rasters; wholly outside
        it = iter(rows)
        for zi in range(len(ZONES)):
            pixels, total, triples = want[zi]
            for r in range(18):
                row = next(it)
                s, n, sw = triples[r]
                assert [int(row[11]), int(row[12])] == [pixels, n], (j, zi, r, row)        # counted once
                mine = row[13 + 3 * j:16 + 3 * j]
                if pixels == 0:
                    assert mine == ["", "", ""], (j, zi, r, row)
                    continue
                mm = (total / pixels) * UNIT
                assert mine[0] == "%.14g" % mm, (j, zi, r, row)
                if n == 0:
                    assert mine[1:] == ["", ""], (j, zi, r, row)
                    continue
                assert mine[1] == "%.14g" % (sw / n / 100.0), (j, zi, r, row)
                assert int(mine[2]) == ru.cn(s, n, sw, ru.table(mm, LAM)), (j, zi, r, row)
                some += 1
    assert some > 3 * 18


def test_each_layer_is_as_text_what_zone_rain_prints_for_its_file(runs):
    d, rows = runs["dir"], runs["rows"]
    for j in range(3):
        one = _rows(d / ("table%d.csv" % (22 + j)), BASE + "," + NEW)
        assert len(one) == len(rows)
        for many, single in zip(rows, one):
            assert many[:11] == single[:11]
            assert [many[11], many[12]] == [single[11], single[13]]                        # rain_pixels, rain_valid
            assert many[13 + 3 * j:16 + 3 * j] == [single[12], single[14], single[15]], (j, many, single)
    # the layers differ: the test compares three different triples
    assert any(r[13:16] != r[16:19] for r in rows) and any(r[16:19] != r[19:22] for r in rows)


def test_the_old_columns_are_as_text_those_of_the_run_without_the_key(runs):
    old = _rows(runs["dir"] / "table1.csv", BASE)
    assert [r[:11] for r in runs["rows"]] == old


def test_two_log_lines_per_raster_in_the_order_given(runs):
    err = runs["many"].stderr
    at = []
    for j, name in enumerate(FILES):
        first = "zone_rain[%d]: %s, 12 x 8 cells" % (j + 1, name)
        second = "zone_rain[%d]: depths %s counts" % (j + 1, "20..20" if name == "flat.tif" else "0..255")
        assert err.count(first) == 1 and err.count(second) == 1, err[-3000:]
        at += [err.index(first), err.index(second)]
    assert at == sorted(at)
    assert "unit = 2.5 mm, lambda = 0.2" in err


def test_one_file_writes_the_table_of_zone_rain_byte_for_byte(runs):
    d = runs["dir"]
    one = _run(d, "-c", _config(d, 25), "--zones", "zones.shp", "--zone-rains", FILES[0], "--zone-rain-unit", "2.5")
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-2000:]
    assert (d / "table25.csv").read_bytes() == (d / "table22.csv").read_bytes()
    assert "zone_rain: first.tif, 12 x 8 cells" in one.stderr
