"""tests/arena_model.py against layouts worked out by hand: the check that the model of the encoders' arena
contract is itself right (no GPU)."""
import numpy as np
import pytest

from tests import arena_model as am

NO = am.NO_ROOM
B_SIZES = [[100, 33], [1, 4000], [20, 16]]


def _table(lay):
    return [[tuple(e) for e in row] for row in lay.table.tolist()]


def test_one_tile_per_raster():
    lay = am.layout([[5], [16], [17]], None, 16, 1000)
    assert _table(lay) == [[(0, 5)], [(16, 16)], [(32, 17)]]
    assert (lay.cursor, lay.starts, lay.ends) == (64, [0, 16, 32], [16, 32, 64])
    assert sorted(lay.zeros) == [(5, 16), (49, 64)]
    assert sorted(lay.streams) == [(0, 5), (16, 32), (32, 49)]
    assert lay.unspecified == []


@pytest.mark.parametrize("seg_align, table, cursor, zeros", [
    (16, [[(0, 100), (112, 33)], [(160, 1), (176, 4000)], [(4176, 20), (4208, 16)]], 4224,
     [(100, 112), (145, 160), (161, 176), (4196, 4208)]),
    (512, [[(0, 100), (112, 33)], [(512, 1), (528, 4000)], [(4608, 20), (4640, 16)]], 4656,
     [(100, 112), (145, 160), (160, 512), (513, 528), (4528, 4608), (4628, 4640), (4656, 5120)]),
    (4096, [[(0, 100), (112, 33)], [(4096, 1), (4112, 4000)], [(8192, 20), (8224, 16)]], 8240,
     [(100, 112), (145, 160), (160, 4096), (4097, 4112), (8112, 8192), (8212, 8224), (8240, 12288)]),
])
def test_three_rasters_at_every_alignment(seg_align, table, cursor, zeros):
    lay = am.layout(B_SIZES, None, seg_align, 20000)
    assert _table(lay) == table
    assert lay.cursor == cursor
    assert sorted(lay.zeros) == zeros
    assert lay.starts == [row[0][0] for row in table]


def test_an_alias_in_the_middle_takes_no_room_and_carries_its_originals_entry():
    alias = [[None, None], [None, 0], [1, None]]
    lay = am.layout([[40, 50], [60, 70], [80, 90]], alias, 512, 4096)
    assert _table(lay) == [[(0, 40), (48, 50)], [(512, 60), (48, 50)], [(512, 60), (1024, 90)]]
    assert (lay.cursor, lay.starts, lay.ends) == (1120, [0, 512, 1024], [112, 576, 1120])
    assert sorted(lay.zeros) == [(40, 48), (98, 112), (112, 512), (572, 576), (576, 1024), (1114, 1120), (1120, 1536)]
    assert sorted(lay.streams) == [(0, 40), (48, 98), (512, 572), (1024, 1114)]


def test_a_raster_of_aliases_only_has_an_empty_extent():
    alias = [[None, None], [0, 0], [None, None]]
    lay = am.layout([[10, 20], [7, 7], [30, 40]], alias, 4096, 1 << 20)
    assert _table(lay) == [[(0, 10), (16, 20)], [(0, 10), (16, 20)], [(4096, 30), (4128, 40)]]
    assert (lay.starts, lay.ends, lay.cursor) == ([0, 4096, 4096], [48, 4096, 4176], 4176)
    assert sorted(lay.zeros) == [(10, 16), (36, 48), (48, 4096), (4126, 4128), (4168, 4176), (4176, 8192)]


def test_a_cap_on_a_slots_end_fits_and_one_byte_less_does_not():
    lay = am.layout(B_SIZES, None, 512, 4656)
    assert _table(lay)[2] == [(4608, 20), (4640, 16)] and lay.unspecified == []
    assert (4656, 5120) not in lay.zeros and max(b for _, b in lay.zeros) == 4640      # no room for the last pad
    lay = am.layout(B_SIZES, None, 512, 4655)
    assert _table(lay) == [[(0, 100), (112, 33)], [(512, 1), (528, 4000)], [(4608, 20), NO]]
    assert lay.cursor == 4656 and lay.unspecified == [(4640, 4656)]
    assert (4640, 4656) not in lay.streams
    # a cap that is no multiple of 16, inside a stream of the second raster
    lay = am.layout(B_SIZES, None, 512, 2001)
    assert _table(lay) == [[(0, 100), (112, 33)], [(512, 1), NO], [NO, NO]]
    assert lay.cursor == 4656 and sorted(lay.zeros) == [(100, 112), (145, 160), (160, 512), (513, 528)]


def test_a_cap_inside_a_pad_cuts_the_pad_to_whole_units():
    lay = am.layout(B_SIZES, None, 512, 300)
    assert _table(lay) == [[(0, 100), (112, 33)], [NO, NO], [NO, NO]]
    assert sorted(lay.zeros) == [(100, 112), (145, 160), (160, 288)]        # [288, 300) is not a whole unit
    assert lay.cursor == 4656
    lay = am.layout(B_SIZES, None, 512, 15)
    assert _table(lay) == [[NO, NO]] * 3 and lay.zeros == [] and lay.streams == [] and lay.cursor == 4656


def _paint(lay, cap, guard=64):
    """What a correct encoder leaves: stream bytes (here 0x11), zeros, poison everywhere else."""
    img = np.full(cap + guard, 0xA5, np.uint8)
    for a, b in lay.streams:
        img[a:b] = 0x11
    for a, b in lay.zeros:
        img[a:b] = 0
    return img


@pytest.mark.parametrize("cap", [20000, 4656, 4655, 2001, 300, 15])
def test_the_checker_accepts_a_correct_image_and_names_every_kind_of_stray_byte(cap):
    lay = am.layout(B_SIZES, None, 512, cap)
    img = _paint(lay, cap)
    am.check(lay, lay.table.copy(), lay.cursor, img, cap)
    # a stream's bytes may be anything, poison included; so may the slot of a stream that did not fit
    for a, b in lay.streams + [(a, min(b, cap)) for a, b in lay.unspecified if a < cap]:
        ok = img.copy()
        ok[a] = 0xA5
        ok[b - 1] = 0x00
        am.check_image(lay, ok, cap)
    wrong = []
    for a, b in lay.zeros:
        wrong += [a, b - 1]                              # a zero range that is not zero: first and last byte
    wrong += [cap, cap + 63]                             # the guard
    free = np.ones(cap, bool)
    for a, b in lay.streams + lay.zeros + lay.unspecified:
        free[a:b] = False
    if free.any():
        wrong += [int(np.flatnonzero(free)[0]), int(np.flatnonzero(free)[-1])]     # bytes nobody may touch
    assert len(wrong) >= 2
    for at in wrong:
        bad = img.copy()
        bad[at] ^= 0x40
        with pytest.raises(AssertionError, match="byte %d " % at):
            am.check_image(lay, bad, cap)


def test_the_checker_compares_table_and_cursor():
    lay = am.layout(B_SIZES, None, 512, 4655)
    t = lay.table.copy()
    am.check_table(lay, t, 4656)
    with pytest.raises(AssertionError, match="cursor"):
        am.check_table(lay, t, 4655)
    t[2, 1] = (4640, 16)
    with pytest.raises(AssertionError, match=r"raster 2, tile 1"):
        am.check_table(lay, t, 4656)
