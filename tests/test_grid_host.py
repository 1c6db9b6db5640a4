"""CPU: the host geometry of the model-grid run mode (config key grid, --grid): the grid's text (gcn10_parse_grid, the
config key) and the plan of a block on the grid (gcn10_grid_plan_block) against the membership rule restated in numpy
on np.float64 (tests/gridutil.py): the same expressions and comparisons, per centre, no division."""
import numpy as np
import pytest

from gcn10_amd import host
from tests import gridutil as gu
from tests import zoneutil

PX = 8.3333333333330430e-05         # the landcover's pixel size
P10 = 2.0 ** -10


def _config(tmp_path, **extra):
    p = tmp_path / "cfg.txt"
    keys = dict(hysogs_data_path="h", esa_data_path="e", blocks_shp_path="b", lookup_table_path="l",
                log_dir=str(tmp_path / "logs"))
    keys.update({k: str(v) for k, v in extra.items()})
    p.write_text("".join("%s=%s\n" % kv for kv in keys.items()))
    return str(p)


# ---- the text -----------------------------------------------------------------------------------------------------

GOOD = {
    "9.9995,50.0005,0.0021,0.0021,30,22": (9.9995, 50.0005, 0.0021, 0.0021, 30, 22),
    "-180,84,1e-2,.5,8192,8192": (-180.0, 84.0, 0.01, 0.5, 8192, 8192),                    # nx * ny = 2^26
    "+1.5e2,-0.25,8.3333333333330430e-04,0.008333333333333333,1,67108864": (150.0, -0.25, 8.3333333333330430e-04,
                                                                          0.008333333333333333, 1, 67108864),
}
BAD = ["", "1,2,3,4,5", "1,2,3,4,5,", "1,2,3,4,5,6x", "1,2,3,4,5,6,7", "1,2,3,4,5,6 ", " 1,2,3,4,5,6", "1, 2,3,4,5,6",
       "1,2,0,4,5,6", "1,2,3,0,5,6", "1,2,-3,4,5,6", "1,2,3,4,-5,6", "1,2,3,4,5,-6", "1,2,3,4,0,6", "1,2,3,4,5,0",
       "1,2,3,4,5,13421773",                        # nx * ny = 2^26 + 1
       "1,2,3,4,8193,8192", "1,2,3,4,99999999999999999999,1", "nan,2,3,4,5,6", "1,2,nan,4,5,6", "1,inf,3,4,5,6",
       "1,2,3,4,5.5,6", "1,2,3,4,5e1,6", "1;2;3;4;5;6", "x"]


@pytest.mark.parametrize("text", sorted(GOOD))
def test_a_good_grid_is_parsed_to_its_doubles_and_counts(text):
    g = host.parse_grid(text)
    assert (g["xmin"], g["ymax"], g["dx"], g["dy"], g["nx"], g["ny"]) == GOOD[text]
    assert [float(t) for t in text.split(",")[:4]] == [g["xmin"], g["ymax"], g["dx"], g["dy"]]     # strtod's doubles


@pytest.mark.parametrize("text", BAD)
def test_a_malformed_grid_is_refused(text):
    with pytest.raises(host.HostError) as e:
        host.parse_grid(text)
    assert str(e.value) == "bad value for grid: '%s' (xmin,ymax,dx,dy,nx,ny)" % text


def test_the_config_key(tmp_path):
    assert host.parse_config(_config(tmp_path))["grid"] is None
    text = "9.9995,50.0005,0.0021,0.0021,30,22"
    cfg = host.parse_config(_config(tmp_path, grid=text, aggregate=0))
    assert cfg["grid"] == text and cfg["aggregate"] == 0
    for bad in ("1,2,3,4,5", "1,2,3,4,5,13421773", "1,2,0,4,5,6"):
        with pytest.raises(host.HostError) as e:
            host.parse_config(_config(tmp_path, grid=bad))
        assert str(e.value) == "bad value for grid: '%s' (xmin,ymax,dx,dy,nx,ny)" % bad
    # the key is appended behind the struct as it stood
    assert [n for n, _t in host.ConfigGrid._fields_] == ["grid"] and issubclass(host.ConfigGrid, host.ConfigFull)


# ---- the plan of a block ------------------------------------------------------------------------------------------

def _grid(xmin, ymax, dx, dy, nx, ny):
    return dict(xmin=xmin, ymax=ymax, dx=dx, dy=dy, nx=nx, ny=ny)


def _check_invariants(p, W, H):
    ncx, ncy = p["cx1"] - p["cx0"], p["cy1"] - p["cy0"]
    for name, n, m in (("cellx", W, ncx), ("celly", H, ncy)):
        a = p[name]
        assert a.shape == (n,) and a.min() >= -1 and a.max() == m - 1
        inside = a[a >= 0]
        assert (np.diff(inside) >= 0).all() and (np.diff(inside) <= 1).all(), name     # never decreasing, no cell skipped
        assert inside[0] == 0
        nz = np.flatnonzero(a >= 0)
        assert (np.diff(nz) == 1).all(), name       # -1 only before and behind
    complete = p["complete_y"][:, None] & p["complete_x"][None, :]
    shared = np.zeros(ncx * ncy, bool)
    shared[p["shared"]] = True
    assert (np.diff(p["shared"].astype(np.int64)) > 0).all()
    # complete and shared partition the rectangle
    assert (shared.reshape(ncy, ncx) ^ complete).all()


def test_centres_on_cell_edges_belong_to_one_cell():
    """(i) Pixels of 2^-10 and a grid half a pixel off the window's origin with cells of 8 pixels: ex(k) is the centre
    of column 8 k and ey(k) the centre of row 8 k, exactly.  A centre on ex(k) is in column k, one on ey(k) in row k."""
    W, H = 40, 33
    gt = [3.0, P10, 0.0, 7.0, 0.0, -P10]
    g = _grid(3.0 + 0.5 * P10, 7.0 - 0.5 * P10, 8 * P10, 8 * P10, 4, 3)
    ex, ey = gu.edges(g)
    px, py = zoneutil.centres(gt, W, H)
    assert (ex == px[0:33:8]).all() and (ey == py[0:25:8]).all()       # the ties are exact
    p = host.grid_plan_block(g, W, H, gt)
    assert (p["cx0"], p["cx1"], p["cy0"], p["cy1"]) == (0, 4, 0, 3)
    for k in range(4):
        assert p["cellx"][8 * k] == k and (k == 0 or p["cellx"][8 * k - 1] == k - 1)
    for k in range(3):
        assert p["celly"][8 * k] == k and (k == 0 or p["celly"][8 * k - 1] == k - 1)
    assert p["cellx"][32] == -1 and p["cellx"][31] == 3             # px = ex(nx) is outside, half open
    assert p["celly"][24] == -1 and p["celly"][23] == 2             # py = ey(ny) is outside
    gu.same_plan(p, gu.plan(g, gt, W, H, dense=True))
    gu.same_plan(p, gu.plan(g, gt, W, H))
    _check_invariants(p, W, H)
    # the same grid moved by half a pixel: no tie is left, column 8 k - 4 starts cell k
    g2 = _grid(3.0, 7.0, 8 * P10, 8 * P10, 4, 3)
    p2 = host.grid_plan_block(g2, W, H, gt)
    gu.same_plan(p2, gu.plan(g2, gt, W, H, dense=True))
    assert p2["cellx"][:9].tolist() == [0] * 8 + [1]
    # ownership on ties as well: own edges on centres
    own = [px[5], py[20], px[30], py[2]]
    p3 = host.grid_plan_block(g, W, H, gt, own)
    gu.same_plan(p3, gu.plan(g, gt, W, H, own, dense=True))
    assert (p3["x0"], p3["x1"], p3["y0"], p3["y1"]) == (5, 30, 2, 20)
    assert p3["cellx"][4] == -1 and p3["cellx"][5] == 0 and p3["cellx"][29] == 3 and p3["cellx"][30] == -1
    _check_invariants(p3, W, H)


@pytest.mark.parametrize("own", [None, [-110.9999, 38.9975, -108.0002, 38.99999]])
def test_the_real_pixel_size_and_cells_of_25_6_pixels(own):
    """(ii) A 36001-pixel row of a real block."""
    W, H = 36001, 50
    gt = [-111.0000000000024, PX, 0.0, 39.00000000000157, 0.0, -PX]
    g = _grid(gt[0] - 3.3 * PX, gt[3] + 1.7 * PX, 25.6 * PX, 25.6 * PX, 2000, 3)
    p = host.grid_plan_block(g, W, H, gt, own)
    gu.same_plan(p, gu.plan(g, gt, W, H, own))
    _check_invariants(p, W, H)
    widths = np.bincount(p["cellx"][p["cellx"] >= 0])
    assert set(widths[1:-1].tolist()) == {25, 26}
    if own is None:
        assert p["shared"].size == (p["cx1"] - p["cx0"]) * (p["cy1"] - p["cy0"])      # nothing is known complete


def test_a_grid_that_ends_inside_the_window_on_all_sides():
    """(iii) -1 before and behind the cells, in both maps."""
    W, H = 100, 80
    gt = [12.3, 0.0125, 0.0, 48.7, 0.0, -0.0075]
    g = _grid(12.3 + 10.3 * 0.0125, 48.7 - 7.6 * 0.0075, 9.7 * 0.0125, 11.2 * 0.0075, 8, 6)
    p = host.grid_plan_block(g, W, H, gt)
    gu.same_plan(p, gu.plan(g, gt, W, H, dense=True))
    _check_invariants(p, W, H)
    assert (p["cx0"], p["cx1"], p["cy0"], p["cy1"]) == (0, 8, 0, 6)
    assert (p["cellx"][:10] == -1).all() and p["cellx"][10] == 0 and (p["cellx"][88:] == -1).all()
    assert (p["celly"][:8] == -1).all() and p["celly"][8] == 0 and (p["celly"][75:] == -1).all()
    # the window inside the grid: cells cut by the window's sides, the first one not cell 0
    g2 = _grid(12.3 - 20.25 * 0.0125, 48.7 + 33.1 * 0.0075, 9.7 * 0.0125, 11.2 * 0.0075, 40, 40)
    p2 = host.grid_plan_block(g2, W, H, gt)
    gu.same_plan(p2, gu.plan(g2, gt, W, H, dense=True))
    _check_invariants(p2, W, H)
    assert p2["cx0"] == 2 and p2["cy0"] == 2 and (p2["cellx"] >= 0).all() and (p2["celly"] >= 0).all()


@pytest.mark.parametrize("where", ["east", "west", "north", "south", "beside the owned part"])
def test_a_grid_that_misses_the_window(where):
    """(iv) The cell rectangle is empty and there are no maps."""
    W, H = 100, 80
    gt = [12.3, 0.0125, 0.0, 48.7, 0.0, -0.0075]
    x, y = {"east": (14.0, 48.7), "west": (10.0, 48.7), "north": (12.3, 50.0), "south": (12.3, 47.0),
            "beside the owned part": (12.3, 48.7)}[where]
    g = _grid(x, y, 0.11, 0.1, 5, 5)
    own = [12.3 + 60 * 0.0125, 40.0, 20.0, 50.0] if where == "beside the owned part" else None
    p = host.grid_plan_block(g, W, H, gt, own)
    assert (p["cx0"], p["cx1"], p["cy0"], p["cy1"]) == (0, 0, 0, 0)
    assert p["cellx"].size == 0 and p["celly"].size == 0 and p["shared"].size == 0
    assert (gu.plan(g, gt, W, H, own, dense=True)["cx1"], gu.plan(g, gt, W, H, own)["cy1"]) == (0, 0)
    if own is not None:
        assert (p["x0"], p["x1"]) == (60, 100)


def test_two_abutting_blocks_share_a_pixel_column_and_no_pixel():
    """(v) The windows of two blocks that meet at x = 10.028 share a pixel column; every column is owned once, the two
    maps together are the map of the undivided row, a cell column through the seam is shared in both plans, and one
    that ends exactly on the seam is complete in one."""
    esa_gt = [10.0, PX, 0.0, 50.0, 0.0, -PX]
    RX, RY = 700, 500
    boxes = [[10.0, 49.96, 10.028, 50.0], [10.028, 49.96, 10.056, 50.0]]
    wins = [host.raster_window(esa_gt, RX, RY, b) for b in boxes]
    (xa, _ya, Wa, Ha, gta), (xb, _yb, Wb, Hb, gtb) = wins
    assert xa + Wa == xb + 1 and Ha == Hb                            # one shared pixel column
    # cells of 25.2 px; cell column 13 straddles the seam, and a second grid has an edge exactly on it
    grids = [_grid(9.9995, 50.0005, 0.0021, 0.0021, 30, 22), _grid(10.028 - 7 * 0.004, 50.0005, 0.004, 0.0021, 14, 22)]
    for g in grids:
        pa = host.grid_plan_block(g, Wa, Ha, gta, boxes[0])
        pb = host.grid_plan_block(g, Wb, Hb, gtb, boxes[1])
        gu.same_plan(pa, gu.plan(g, gta, Wa, Ha, boxes[0]))
        gu.same_plan(pb, gu.plan(g, gtb, Wb, Hb, boxes[1]))
        _check_invariants(pa, Wa, Ha)
        _check_invariants(pb, Wb, Hb)
        # every column of the mosaic is owned by exactly one block
        owned = np.zeros(RX, np.int64)
        owned[xa + pa["x0"]:xa + pa["x1"]] += 1
        owned[xb + pb["x0"]:xb + pb["x1"]] += 1
        N = xb + pb["x1"]                   # the blocks end at 10.056, the data a little east of it
        assert (owned[:N] == 1).all() and (owned[N:] == 0).all() and N > 650
        # the union of the maps is the map of the undivided row
        whole = gu.plan(g, esa_gt, RX, RY)
        union = np.full(RX, -1, np.int64)
        for p, xo in ((pa, xa), (pb, xb)):
            m = p["cellx"] >= 0
            assert (union[xo + np.flatnonzero(m)] == -1).all()
            union[xo + np.flatnonzero(m)] = p["cellx"][m] + p["cx0"]
        np.testing.assert_array_equal(union[:N], np.where(whole["cellx"] >= 0, whole["cellx"] + whole["cx0"], -1)[:N])
        assert (union[N:] == -1).all()
    ex, _ey = gu.edges(grids[0])
    k = int(np.searchsorted(ex, 10.028, side="right") - 1)
    assert k == 13 and ex[13] < 10.028 < ex[14]
    pa = host.grid_plan_block(grids[0], Wa, Ha, gta, boxes[0])
    pb = host.grid_plan_block(grids[0], Wb, Hb, gtb, boxes[1])
    assert pa["cx1"] == 14 and pb["cx0"] == 13                       # both plans hold cell column 13 ...
    assert not pa["complete_x"][13 - pa["cx0"]] and not pb["complete_x"][0]          # ... complete in neither
    assert pa["complete_x"][12 - pa["cx0"]] and pb["complete_x"][1]
    ncx = pa["cx1"] - pa["cx0"]
    assert set((pa["shared"] % ncx).tolist()) >= {13 - pa["cx0"]}
    # an edge exactly on the seam: the cell column west of it is complete in block 7's plan and absent from block 8's
    ex, _ey = gu.edges(grids[1])
    assert ex[7] == 10.028
    pa = host.grid_plan_block(grids[1], Wa, Ha, gta, boxes[0])
    pb = host.grid_plan_block(grids[1], Wb, Hb, gtb, boxes[1])
    assert pa["cx1"] == 7 and pb["cx0"] == 7
    assert pa["complete_x"][6 - pa["cx0"]] and pb["complete_x"][0]
    # rows: the grid reaches above the data, so its first cell row is not complete
    assert not pa["complete_y"][0] and pa["complete_y"][1]
