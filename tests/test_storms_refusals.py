"""CPU: every way a run with several design storms (config key storms, --storms) stops before a GPU is opened: exit
status 1, the exact text on stderr, nothing created -- run the way tests/test_storm_refusals.py runs its table --; then
the start-up failure of a grid run with storms on a GPU library that lacks the entry points for several weight tables
(the stub of tests/stub_gpu), and what `--storm` goes on asking of that library."""
import pytest

from tests.test_grid_refusals import GRID, _config, _gcn10, _nothing_written, stub, zones  # noqa: F401

BAD = "(P1[:P2...][,lambda]: 1 to 8 rising depths, 0 < P <= 650 mm, 0 <= lambda < 1)"
AGG = "[rank 0] storms cannot be combined with aggregate (use --grid with cells of f pixels)\n"


def _bad(text, rank=True):
    return "%sbad value for storms: '%s' %s\n" % ("[rank 0] " if rank else "", text, BAD)


# name -> (config keys, arguments behind "-c <config>", stderr); "{zones}" stands for the zone file; a message without
# "[rank 0] " comes from the config parser, as it words it
REFUSALS = {
    "storms alone": ({}, ["--storms", "25:50"], "[rank 0] storms needs --grid or --zones\n"),
    "storms key alone": (dict(storms="25:50,0.05"), [], "[rank 0] storms needs --grid or --zones\n"),
    "storms with --aggregate": ({}, ["--storms", "25:50", "--aggregate", "25"], AGG),
    "storms key with aggregate=7": (dict(storms="50", aggregate=7), [], AGG),
    "storms with --grid and --aggregate": ({}, ["--storms", "25:50", "--grid", GRID, "--aggregate", "25"], AGG),
    "storms with --verify": ({}, ["--storms", "25:50", "--verify"], "[rank 0] storms cannot be combined with --verify\n"),
    "storms with --grid and --verify": ({}, ["--storms", "25:50", "--grid", GRID, "--verify"],
                                        "[rank 0] storms cannot be combined with --verify\n"),
    "storms key with verify=1": (dict(storms="25:50", verify=1, grid=GRID), [],
                                 "[rank 0] storms cannot be combined with --verify\n"),
    "storms with --storm": ({}, ["--storms", "25:50", "--storm", "50", "--grid", GRID],
                            "[rank 0] storms cannot be combined with storm\n"),
    "storms with the storm key": (dict(storm="50", grid=GRID), ["--storms", "25:50"],
                                  "[rank 0] storms cannot be combined with storm\n"),
    "storms key with --storm": (dict(storms="25:50"), ["--storm", "50", "--zones", "{zones}"],
                                "[rank 0] storms cannot be combined with storm\n"),
    "both keys": (dict(storms="25:50", storm="50", grid=GRID), [], "[rank 0] storms cannot be combined with storm\n"),
    "one depth with --storm all the same": ({}, ["--storms", "50", "--storm", "50", "--grid", GRID],
                                            "[rank 0] storms cannot be combined with storm\n"),
    "bad --storms: empty": ({}, ["--storms", "", "--grid", GRID], _bad("")),
    "bad --storms: nine depths": ({}, ["--storms", "1:2:3:4:5:6:7:8:9", "--grid", GRID], _bad("1:2:3:4:5:6:7:8:9")),
    "bad --storms: equal names": ({}, ["--storms", "50.001:50.004", "--grid", GRID], _bad("50.001:50.004")),
    "bad --storms: falling": ({}, ["--storms", "50:25", "--grid", GRID], _bad("50:25")),
    "bad --storms: an empty field": ({}, ["--storms", "25::50", "--grid", GRID], _bad("25::50")),
    "bad --storms: a trailing colon": ({}, ["--storms", "25:50:", "--zones", "{zones}"], _bad("25:50:")),
    "bad --storms: text behind it": ({}, ["--storms", "25:50mm", "--grid", GRID], _bad("25:50mm")),
    "bad --storms: nan": ({}, ["--storms", "25:nan", "--grid", GRID], _bad("25:nan")),
    "bad --storms: 650.01": ({}, ["--storms", "25:650.01", "--grid", GRID], _bad("25:650.01")),
    "bad --storms: lambda = 1": ({}, ["--storms", "25:50,1", "--grid", GRID], _bad("25:50,1")),
    "bad --storms over a good key": (dict(storms="25:50", grid=GRID), ["--storms", "x"], _bad("x")),
    "bad storms key": (dict(storms="25:50,1.5", grid=GRID), [], _bad("25:50,1.5", rank=False)),
    "bad storms key: empty": (dict(storms="", grid=GRID), [], _bad("", rank=False)),
    "bad storms key under a good flag": (dict(storms="50:25", grid=GRID), ["--storms", "25:50"],
                                         _bad("50:25", rank=False)),
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


# ---- a GPU library without the entry points for several tables: the stub has none of the grid's -------------------------

@pytest.mark.parametrize("how", ["flag", "key", "flag over key", "one depth"])
def test_a_gpu_library_without_the_storms_entry_points_fails_at_start(tmp_path, stub, how):  # noqa: F811
    text = "50" if how == "one depth" else "25.4:50,0.05"
    keys = dict(grid=GRID, storms=text) if how == "key" else dict(storms="1:2") if how == "flag over key" else {}
    args = [] if how == "key" else ["--grid", GRID, "--storms", text]
    p = _gcn10(["-c", _config(tmp_path, **keys)] + args, tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_grid_sums_storms (needed by storms=%s)\n" % (stub, text)
    assert p.stdout == ""
    assert _nothing_written(tmp_path)


def test_a_storm_goes_on_asking_for_the_weighted_entry_points(tmp_path, stub):  # noqa: F811
    p = _gcn10(["-c", _config(tmp_path), "--grid", GRID, "--storm", "50"], tmp_path, {"GCN10_GPU_LIB": stub})
    assert p.returncode == 1, p.stdout + p.stderr
    assert p.stderr == "[rank 0] %s lacks gcn10_gpu_grid_sums_weighted (needed by storm=50)\n" % stub
    assert _nothing_written(tmp_path)
