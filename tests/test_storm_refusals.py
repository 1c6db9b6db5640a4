"""CPU: every way a run with a design storm (config key storm, --storm) stops before a GPU is opened: exit status 1, the
exact text on stderr, nothing created -- run the way tests/test_grid_refusals.py runs its table --; then the start-up
failure of a grid run with a storm on a GPU library that lacks the weighted entry points (the stub of tests/stub_gpu),
and what a grid run without a storm asks of that library."""
import pytest

from tests.test_grid_refusals import GRID, _config, _gcn10, _nothing_written, stub, zones  # noqa: F401

BAD = "(P[,lambda]: 0 < P <= 650 mm, 0 <= lambda < 1)"

# name -> (config keys, arguments behind "-c <config>", stderr); "{zones}" stands for the zone file; a message without
# "[rank 0] " comes from the config parser, as it words it
REFUSALS = {
    "storm alone": ({}, ["--storm", "50"], "[rank 0] storm needs --grid or --zones\n"),
    "storm key alone": (dict(storm="50,0.05"), [], "[rank 0] storm needs --grid or --zones\n"),
    "storm with --aggregate": ({}, ["--storm", "50", "--aggregate", "25"],
                               "[rank 0] storm cannot be combined with aggregate (use --grid with cells of f pixels)\n"),
    "storm key with aggregate=7": (dict(storm="50", aggregate=7), [],
                                   "[rank 0] storm cannot be combined with aggregate (use --grid with cells of f "
                                   "pixels)\n"),
    "storm with --grid and --aggregate": ({}, ["--storm", "50", "--grid", GRID, "--aggregate", "25"],
                                          "[rank 0] storm cannot be combined with aggregate (use --grid with cells of "
                                          "f pixels)\n"),
    "storm with --verify": ({}, ["--storm", "50", "--verify"], "[rank 0] storm cannot be combined with --verify\n"),
    "storm with --grid and --verify": ({}, ["--storm", "50", "--grid", GRID, "--verify"],
                                       "[rank 0] storm cannot be combined with --verify\n"),
    "storm key with verify=1": (dict(storm="50", verify=1, grid=GRID), [],
                                "[rank 0] storm cannot be combined with --verify\n"),
    "bad --storm: empty": ({}, ["--storm", "", "--grid", GRID], "[rank 0] bad value for storm: '' " + BAD + "\n"),
    "bad --storm: text behind it": ({}, ["--storm", "50mm", "--grid", GRID],
                                    "[rank 0] bad value for storm: '50mm' " + BAD + "\n"),
    "bad --storm: 0": ({}, ["--storm", "0", "--grid", GRID], "[rank 0] bad value for storm: '0' " + BAD + "\n"),
    "bad --storm: 650.01": ({}, ["--storm", "650.01", "--grid", GRID],
                            "[rank 0] bad value for storm: '650.01' " + BAD + "\n"),
    "bad --storm: nan": ({}, ["--storm", "nan", "--zones", "{zones}"], "[rank 0] bad value for storm: 'nan' " + BAD + "\n"),
    "bad --storm: -1": ({}, ["--storm", "-1", "--grid", GRID], "[rank 0] bad value for storm: '-1' " + BAD + "\n"),
    "bad --storm: lambda = 1": ({}, ["--storm", "50,1", "--grid", GRID],
                                "[rank 0] bad value for storm: '50,1' " + BAD + "\n"),
    "bad --storm: three fields": ({}, ["--storm", "50,0.2,0.1", "--grid", GRID],
                                  "[rank 0] bad value for storm: '50,0.2,0.1' " + BAD + "\n"),
    "bad --storm over a good key": (dict(storm="50", grid=GRID), ["--storm", "x"],
                                    "[rank 0] bad value for storm: 'x' " + BAD + "\n"),
    "bad storm key": (dict(storm="50,1.5", grid=GRID), [], "bad value for storm: '50,1.5' " + BAD + "\n"),
    "bad storm key: empty": (dict(storm="", grid=GRID), [], "bad value for storm: '' " + BAD + "\n"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_before_any_gpu(tmp_path, zones, case):  # noqa: F811
    keys, args, stderr = REFUSALS[case]
    args = [a.format(zones=zones) for a in args]
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path)
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == stderr
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


# ---- a GPU library without the weighted entry points: the stub has none of the grid's -----------------------------------

@pytest.mark.parametrize("how", ["flag", "key", "flag over key"])
def test_a_gpu_library_without_the_weighted_entry_points_fails_at_start(tmp_path, stub, how):  # noqa: F811
    keys = dict(grid=GRID, storm="25.4,0.05") if how == "key" else dict(storm="1") if how == "flag over key" else {}
    args = [] if how == "key" else ["--grid", GRID, "--storm", "25.4,0.05"]
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_grid_sums_weighted (needed by storm=25.4,0.05)\n" % stub
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


def test_a_grid_run_without_a_storm_asks_for_the_plain_entry_points_only(tmp_path, stub):  # noqa: F811
    p = _gcn10(["-c", _config(tmp_path), "--grid", GRID], tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_grid_sums (needed by grid=%s)\n" % (stub, GRID)
    assert _nothing_written(tmp_path)

