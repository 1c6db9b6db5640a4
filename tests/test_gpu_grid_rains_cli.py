"""GPU: several rainfall rasters in one grid run end to end.  The two-block world of tests/test_gpu_grid_cli.py and the
`random`, `fifty` and `dry` rasters of tests/test_gpu_grid_rain_cli.py (their fixtures and helpers), and what
`bin/gcn10 --grid ... --rains <file1>:<file2>...` writes under cn_grid_<cond>/: the mean rasters, byte for byte those of
the run without rain, and cnq_<hc>_<arc>_rain<j>.tif per file beside each.

Expected: the restatement of tests/test_gpu_grid_rain_cli.py per layer (the oracle's rasters of both blocks, summed per
cell with the table of the cell's own byte in that layer, runoffutil.cn per cell); beside it what `--rain <file_j>` alone
writes, what `--storm 50` writes for the constant layer at unit 1, and the means for the dry layer."""
import os

import numpy as np
import pytest

from tests import rainutil as rn
from tests import runoffutil as ru
from tests.test_gpu_grid_cli import GRID_TEXT, NX, NY, _config, _name, _read, _run, world  # noqa: F401
from tests.test_gpu_grid_rain_cli import LAMBDA, UNIT, _files, _qname, _triples, fields  # noqa: F401

pytestmark = pytest.mark.gpu

TAGS = (33550, 33922, 34735)


def _logs(run):
    return "".join((run / "logs" / f).read_text() for f in os.listdir(run / "logs"))


@pytest.fixture(scope="module")
def runs(world, fields):  # noqa: F811
    """run A: three rasters at 2.5 mm per count; run B: two at the default unit"""
    d = world["dir"]
    a, b = _config(d, "rains_a"), _config(d, "rains_b")
    files_a = "%s:%s:%s" % (d / "random.tif", d / "fifty.tif", d / "dry.tif")
    files_b = "%s:%s" % (d / "fifty.tif", d / "dry.tif")
    out_a = _run(a, "-c", "config.txt", "--grid", GRID_TEXT, "--rains", files_a, "--rain-unit", "%r,%r" % (UNIT, LAMBDA))
    out_b = _run(b, "-c", "config.txt", "--grid", GRID_TEXT, "--rains", files_b)
    assert world["base"].returncode == 0
    for out in (out_a, out_b):
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return dict(a=a, b=b, out_a=out_a.stdout + out_a.stderr, out_b=out_b.stdout + out_b.stderr, files_a=files_a,
                files_b=files_b)


def test_the_files_and_the_means_of_both_runs(world, runs):  # noqa: F811
    d = world["dir"]
    for run, k in ((runs["a"], 3), (runs["b"], 2)):
        files = _files(run)
        assert len(files) == 18 * (1 + k) and not [f for f in files if ".part" in f]
        for j in range(1, k + 1):
            assert len([f for f in files if f.endswith("_rain%d.tif" % j)]) == 18
        assert not [f for f in files if f.endswith("_rain.tif")]
        for r in range(18):
            assert (run / _name(r)).read_bytes() == (d / "base" / _name(r)).read_bytes(), _name(r)
            mean_tags, _ = _read(str(run / _name(r)))
            for j in range(1, k + 1):
                tags, _ = _read(str(run / _qname(r, "_rain%d" % j)))
                assert all(tags[t] == mean_tags[t] for t in TAGS), _qname(r, "_rain%d" % j)
        assert "ERROR" not in _logs(run)
    assert len(_files(runs["a"])) == len(_files(runs["b"])) + 18 == 72


def test_run_a_layer_1_equals_the_restatement_and_the_run_of_rain_alone(world, fields, runs):  # noqa: F811
    """Cell column 13 lies astride the seam of the two blocks: its cells carry 2 + 3 words and are finished on the host,
    per layer, with the table of their own byte in that layer."""
    d, run = world["dir"], runs["a"]
    alone = _config(d, "rains_random_alone")
    out = _run(alone, "-c", "config.txt", "--grid", GRID_TEXT, "--rain", str(d / "random.tif"), "--rain-unit",
               "%r,%r" % (UNIT, LAMBDA))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    tables = np.stack([ru.table(b * UNIT, LAMBDA) for b in range(256)])
    assert "shared with other blocks" in _logs(run)
    for j, name in enumerate(("random", "fifty", "dry")):
        acc = _triples(world, fields[name], tables)
        np.testing.assert_array_equal(acc[..., :2], world["both"])
        if name == "random":
            assert (acc[:, :, 13, 2] > 0).any()
        for r in range(18):
            want = rn.cn_cells(acc[r].reshape(1, -1, 3), fields[name], tables).reshape(NY, NX)
            _tags, got = _read(str(run / _qname(r, "_rain%d" % (j + 1))))
            bad = np.argwhere(got != want)
            assert bad.size == 0, "%s: %d cells differ, first %s: got %d, want %d" % (
                _qname(r, "_rain%d" % (j + 1)), len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    for r in range(18):
        tags, got = _read(str(run / _qname(r, "_rain1")))
        tags1, want = _read(str(alone / _qname(r)))
        np.testing.assert_array_equal(got, want, err_msg=_qname(r))
        assert all(tags[t] == tags1[t] for t in TAGS)


def test_run_b_layer_1_is_the_storm_of_50_mm_and_the_dry_layers_are_the_means(world, runs):  # noqa: F811
    """A byte of 50 is 50 mm at unit 1 only: run B's first layer against --storm 50, not run A's second."""
    d = world["dir"]
    storm = _config(d, "rains_storm50")
    out = _run(storm, "-c", "config.txt", "--grid", GRID_TEXT, "--storm", "50")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    differs = False
    for r in range(18):
        _tags, got = _read(str(runs["b"] / _qname(r, "_rain1")))
        _tags, want = _read(str(storm / _qname(r, "_p5000")))
        np.testing.assert_array_equal(got, want, err_msg=_qname(r))
        _tags, at_125_mm = _read(str(runs["a"] / _qname(r, "_rain2")))
        differs = differs or (at_125_mm != want).any()
        for run, j in ((runs["a"], 3), (runs["b"], 2)):
            _tags, dry = _read(str(run / _qname(r, "_rain%d" % j)))
            _tags, mean = _read(str(run / _name(r)))
            np.testing.assert_array_equal(dry, mean, err_msg=_qname(r, "_rain%d" % j))
    assert differs


def test_the_log_lines_and_the_closing_line(world, fields, runs):  # noqa: F811
    d = world["dir"]
    text = runs["out_a"]
    unit = "unit = 2.5 mm, lambda = 0.050000000000000003"
    assert "rain[1]: %s, %d x %d cells, %s" % (d / "random.tif", NX, NY, unit) in text
    assert "rain[1]: depths 0..255 counts, %d cells without rain" % int((fields["random"] == 0).sum()) in text
    assert "rain[2]: %s, %d x %d cells, %s" % (d / "fifty.tif", NX, NY, unit) in text
    assert "rain[2]: depths 50..50 counts, 0 cells without rain" in text
    assert "rain[3]: %s, %d x %d cells, %s" % (d / "dry.tif", NX, NY, unit) in text
    assert "rain[3]: depths 0..0 counts, %d cells without rain" % (NX * NY) in text
    assert text.index("rain[1]: depths") < text.index("rain[2]: %s" % (d / "fifty.tif")) < text.index("rain[3]: depths")
    assert "under cn_grid_<cond>/: cn_<hc>_<arc>.tif (mean) and cnq_<hc>_<arc>_rain1.tif, _rain2.tif, _rain3.tif " \
           "(runoff-equivalent)" in text
    assert " rain: " not in text and _logs(runs["a"]).count("]: depths ") == 3
    text = runs["out_b"]
    assert "rain[1]: %s, %d x %d cells, unit = 1 mm, lambda = 0.20000000000000001" % (d / "fifty.tif", NX, NY) in text
    assert "rain[2]: depths 0..0 counts, %d cells without rain" % (NX * NY) in text
    assert "cnq_<hc>_<arc>_rain1.tif, _rain2.tif (runoff-equivalent)" in text and "rain[3]" not in text


def test_one_file_writes_what_rain_writes(world, fields):  # noqa: F811
    d = world["dir"]
    one, rain = _config(d, "rains_one"), _config(d, "rains_one_rain")
    out1 = _run(one, "-c", "config.txt", "--grid", GRID_TEXT, "--rains", str(d / "fifty.tif"))
    out2 = _run(rain, "-c", "config.txt", "--grid", GRID_TEXT, "--rain", str(d / "fifty.tif"))
    for out in (out1, out2):
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert _files(one) == _files(rain) and len(_files(one)) == 36
    assert len([f for f in _files(one) if f.endswith("_rain.tif")]) == 18
    for f in _files(one):
        assert (one / f).read_bytes() == (rain / f).read_bytes(), f
    text = out1.stdout + out1.stderr
    assert "rain: %s, %d x %d cells, unit = 1 mm, lambda = 0.20000000000000001" % (d / "fifty.tif", NX, NY) in text
    assert "rain: depths 50..50 counts, 0 cells without rain" in text and "rain[" not in text
    closing = "under cn_grid_<cond>/: cn_<hc>_<arc>.tif (mean) and cnq_<hc>_<arc>_rain.tif (runoff-equivalent)"
    assert closing in text and closing in out2.stdout + out2.stderr


def test_workers_block_order_and_the_key_do_not_change_a_byte(world, runs):  # noqa: F811
    d, run = world["dir"], runs["a"]
    rev = _config(d, "rains_reversed")
    (rev / "blocks.txt").write_text("8\n7\n")
    out = _run(rev, "-c", "config.txt", "-l", "blocks.txt", "--grid", GRID_TEXT, "--rains", runs["files_a"],
               "--rain-unit", "%r,%r" % (UNIT, LAMBDA), "--gpus", "1", env={"GCN10_OVERSUBSCRIBE": "1"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    two = _config(d, "rains_two", extra="grid=%s\nrains=%s\nrain_unit=%r,%r\n" % (GRID_TEXT, runs["files_a"], UNIT, LAMBDA))
    assert len("rains=%s" % runs["files_a"]) < 500              # a line of the config file holds 511 bytes
    out = _run(two, "-c", "config.txt", "--gpus", "2", env={"GCN10_OVERSUBSCRIBE": "1"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for other in (rev, two):
        assert _files(other) == _files(run) and len(_files(run)) == 72
        for f in _files(other):
            assert (other / f).read_bytes() == (run / f).read_bytes(), f
