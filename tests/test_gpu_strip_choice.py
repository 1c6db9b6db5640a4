"""GPU: which strip kernel every gcn10_gpu_cn_strip request launches, and that the kernel is right.  Needs an MI355X.

A request is (W, cond_mask, table_mask, nontemporal, prefetch, ilp1 or ilp16, alignment of the pointers, compact_soil).
For each one, two things are asserted:

  * gcn10_gpu_last_kernel_name() is exactly the line of tests/golden/strip_kernel_choice.txt with the request's key.
    That file is our own record, made by running record_golden() of this module against the library BEFORE the
    strip-kernel table replaced the pick_by_* ladder and the snprintf that restated its choice;
  * every selected raster equals the oracle's (tests/soil_readers.ReaderTile, computed once per tile and shared),
    and the unselected rasters and the guard bytes around every raster are untouched.

Shapes: W = 1040 is kMinVectorW, the narrowest strip the vector kernels accept (a row end in every wave); 3 rows over
a soil window of 48 x 4.  The rows that must choose cn_strip_bytes: W = 1039, an output pointer or the landcover one
byte off 16-byte alignment, fewer than 16 pixels; and compact_soil = 0 at W = 1056, the code-bytes form of the vector
kernel.
"""
import itertools
import os

import numpy as np
import pytest

from tests import soil_readers as sr
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = sr.GUARD
POISON = 0xA5
ROWS, HSX, HSY = 3, 48, 4
GOLDEN_FILE = os.path.join(GOLDEN, "strip_kernel_choice.txt")
COND_MASKS = (1, 2, 3)
TABLE_MASKS = (0x004, 0x005, 0x1FF)     # one table; two tables (ALL_TABLES false); all nine


def vector_requests(cond_masks=COND_MASKS, table_masks=TABLE_MASKS):
    """The cross product of the module's docstring: dicts of the request's fields."""
    for cond, table in itertools.product(cond_masks, table_masks):
        single = bin(table).count("1") == 1
        for nt, pf, ilp in itertools.product((0, 1), (0, 1), (1, 2, 4) if single else (0, 1, 2)):
            yield dict(tile="1040", cond=cond, table=table, nt=nt, pf=pf, ilp=ilp)


# (tile, what is off): the five requests that do not reach the default vector kernel
BYTE_REQUESTS = (dict(tile="1039"), dict(tile="1040", out_shift=1), dict(tile="1040-esa+1"), dict(tile="5"),
                 dict(tile="1056", compact=0))
TILES = {"1040": dict(W=1040), "1040-esa+1": dict(W=1040, offsets=(1, 0, 0, 0)), "1039": dict(W=1039),
         "5": dict(W=5), "1056": dict(W=1056)}


def key_of(q):
    single = bin(q.get("table", 0x1FF)).count("1") == 1
    return "tile=%s cond=%d table=0x%03x nt=%d pf=%d %s=%d out_shift=%d compact_soil=%d" % (
        q["tile"], q.get("cond", 3), q.get("table", 0x1FF), q.get("nt", 1), q.get("pf", 1),
        "ilp1" if single else "ilp16", q.get("ilp", 2 if single else 0), q.get("out_shift", 0), q.get("compact", 1))


def read_golden():
    with open(GOLDEN_FILE) as f:
        return dict(line.rstrip("\n").split("\t") for line in f if line.strip() and not line.startswith("#"))


class Strips:
    """The tiles of the requests on one engine, and one arena of 18 raster slots with guard bytes."""

    def __init__(self, eng, tables):
        self.eng, self.tables, self.tiles = eng, tables, {}
        self.slot = (1056 * ROWS + 2 * GUARD + 1 + 255) & ~255
        self.arena = eng.alloc(18 * self.slot)

    def tile(self, name):
        if name not in self.tiles:
            spec = TILES[name]
            # (the shifted tile draws what "1040" draws: one oracle result serves both)
            self.tiles[name] = sr.ReaderTile(self.eng, self.tables, seed=spec["W"], W=spec["W"], H=ROWS, hsx=HSX,
                                             hsy=HSY, key="choice-%d" % spec["W"], offsets=spec.get("offsets"))
        return self.tiles[name]

    def run(self, q):
        """Launches request q (the options it names are set; the others are the defaults) and checks every byte of the
        arena; returns the kernel's name."""
        eng, t = self.eng, self.tile(q["tile"])
        cond, table, shift = q.get("cond", 3), q.get("table", 0x1FF), q.get("out_shift", 0)
        single = bin(table).count("1") == 1
        eng.set_option("defaults", 0)
        eng.set_option("nontemporal", q.get("nt", 1))
        eng.set_option("prefetch", q.get("pf", 1))
        eng.set_option("compact_soil", q.get("compact", 1))
        if "ilp" in q:
            eng.set_option("ilp1" if single else "ilp16", q["ilp"])
        t.prepare()
        n = t.W * ROWS
        sel = sr.selected(cond, table)
        eng.memset(self.arena.ptr, POISON, 18 * self.slot)
        # every raster gets a pointer; only the first selected one is shifted off 16-byte alignment
        at = [GUARD + (shift if r == sel[0] else 0) for r in range(18)]
        eng.cn_strip(t.bufs[0].ptr, t.W, ROWS, t.bufs[3].ptr, cond, table,
                     [self.arena.at(r * self.slot + at[r]) for r in range(18)])
        name = eng.last_kernel_name()
        img = eng.download(self.arena.ptr, (18, self.slot))
        what = "%s (%s)" % (key_of(q), name)
        for r in range(18):
            if r not in sel:
                assert (img[r] == POISON).all(), "%s: raster %d is not selected and was written" % (what, r)
                continue
            got = img[r, at[r]:at[r] + n].reshape(ROWS, t.W)
            bad = np.argwhere(got != t.want(r))
            assert bad.size == 0, "%s: raster %d differs in %d pixels, first at (row, column) %s" % (
                what, r, len(bad), tuple(bad[0]))
            assert (img[r, :at[r]] == POISON).all() and (img[r, at[r] + n:] == POISON).all(), \
                "%s: raster %d wrote outside its pixels" % (what, r)
        return name

    def close(self):
        self.eng.sync()
        for t in self.tiles.values():
            t.close()
        self.arena.close()
        self.eng.set_option("defaults", 0)


@pytest.fixture(scope="module")
def strips(engine, tables):
    engine.set_tables(tables)
    s = Strips(engine, tables)
    yield s
    s.close()


def record_golden(eng, tables, path):
    """Writes the table of names as the library behind `eng` chooses them (every raster checked as in the tests)."""
    eng.set_tables(tables)
    s = Strips(eng, tables)
    try:
        with open(path, "w") as f:
            f.write("# request of tests/test_gpu_strip_choice.py <TAB> gcn10_gpu_last_kernel_name() after it\n")
            for q in itertools.chain(vector_requests(), BYTE_REQUESTS):
                f.write("%s\t%s\n" % (key_of(q), s.run(q)))
    finally:
        s.close()


def test_the_golden_table_names_every_request():
    keys = [key_of(q) for q in itertools.chain(vector_requests(), BYTE_REQUESTS)]
    # 3 condition masks x 3 table masks x 2 x 2 x 3 chunk counts, and the five rows off the default vector kernel
    assert len(keys) == 108 + 5 and len(set(keys)) == len(keys)
    golden = read_golden()
    assert set(golden) == set(keys)
    # between them the requests launch every instantiation the library has
    assert len({v for v in golden.values() if v.startswith("cn_strip_kernel<")}) == 78


@pytest.mark.parametrize("table", TABLE_MASKS, ids=["one-table", "two-tables", "all-tables"])
@pytest.mark.parametrize("cond", COND_MASKS)
def test_vector_requests(strips, cond, table):
    golden = read_golden()
    for q in vector_requests((cond,), (table,)):
        assert strips.run(q) == golden[key_of(q)], key_of(q)


@pytest.mark.parametrize("q", BYTE_REQUESTS, ids=["W-1039", "out+1", "esa+1", "15-pixels", "code-bytes-W-1056"])
def test_requests_off_the_default_vector_kernel(strips, q):
    name = strips.run(q)
    assert name == read_golden()[key_of(q)], key_of(q)
    if q["tile"] == "1056":
        assert strips.eng.soil_words_state() == 0 and name.startswith("cn_strip_kernel<0, 3, true,")
    else:
        assert name == "cn_strip_bytes"


def test_ilp16_by_stream_count(strips):
    """ilp16 = 0: two sub-chunks per trip up to nine store streams, one beyond."""
    nine = strips.run(dict(tile="1040", cond=1, table=0x1FF))
    ten = strips.run(dict(tile="1040", cond=3, table=0x01F))
    assert nine == "cn_strip_kernel<0, 1, true, 2, true, true>"
    assert ten == "cn_strip_kernel<0, 3, false, 1, true, true>"
