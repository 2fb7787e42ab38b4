"""No GPU: the host arithmetic of the tail split-K of the RoI-pair Winograd launches (include/cmk.h cmk_wino6_tail_plan,
cmk_wino6_piece_bounds — the bounds function is the one the kernel itself calls)."""
import ctypes

import pytest


def _plan(lib, spatial_tiles, cout_tiles, chunk_pairs, slots):
    t, w = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.cmk_wino6_tail_plan(spatial_tiles, cout_tiles, chunk_pairs, slots, ctypes.byref(t), ctypes.byref(w)) == 0
    return t.value, w.value


def _bounds(lib, chunks, ways, piece):
    lo, hi = ctypes.c_int(-1), ctypes.c_int(-1)
    lib.cmk_wino6_piece_bounds(chunks, ways, piece, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def test_plan_bench_shape(cmk_lib):
    # 400 RoIs = 200 pairs x 8 cout tiles on 256 CUs x 2: 1600 = 3 x 512 + 64 -> 8 whole tiles, 8 x 8 x 8 = 512 short workgroups
    assert _plan(cmk_lib, 200, 8, 16, 512) == (8, 8)
    # the paired form: 4 cout-tile pairs, one workgroup per CU: 800 = 3 x 256 + 32
    assert _plan(cmk_lib, 200, 4, 16, 256) == (8, 8)


@pytest.mark.parametrize("args", [(416, 16, 16, 512), (4352, 2, 16, 512)])
def test_plan_exact_multiples_have_no_tail(cmk_lib, args):
    assert (args[0] * args[1]) % args[3] == 0
    assert _plan(cmk_lib, *args) == (0, 0)


def test_plan_under_one_round_has_no_tail(cmk_lib):
    assert _plan(cmk_lib, 30, 8, 16, 512) == (0, 0)            # 240 workgroups: ordinary split-K territory
    assert _plan(cmk_lib, 63, 8, 16, 512) == (0, 0)            # 504


def test_plan_tail_over_half_a_round_is_left_alone(cmk_lib):
    assert (230 * 8) % 512 == 304
    assert _plan(cmk_lib, 230, 8, 16, 512) == (0, 0)
    assert _plan(cmk_lib, 224, 8, 16, 512) == (32, 2)          # exactly half a round: 256 units x 2 ways fill it once


def test_plan_ways_follow_the_room_and_the_chunk_pairs(cmk_lib):
    assert _plan(cmk_lib, 200, 8, 17, 512) == (8, 8)           # the MaskIoU head's first conv: 272 channels = 17 pairs
    assert _plan(cmk_lib, 200, 8, 3, 512) == (8, 2)            # ways <= chunk pairs
    assert _plan(cmk_lib, 200, 8, 1, 512) == (0, 0)            # one pair cannot be split
    assert _plan(cmk_lib, 208, 8, 16, 512) == (16, 4)          # 128 units: 8 ways would need 1024 places
    assert _plan(cmk_lib, 193, 8, 16, 512) == (1, 8)
    assert _plan(cmk_lib, 200, 7, 16, 512) == (0, 0)           # 1400 = 2 x 512 + 376: over half a round
    # tail units are rounded DOWN to whole spatial tiles: 3 x 5 x 11 = 165 = 128 + 37 -> 7 tiles (35 units), 2 ways (70 <= 128, 140 > 128)
    assert _plan(cmk_lib, 33, 5, 16, 128) == (7, 2)
    assert _plan(cmk_lib, 0, 8, 16, 512) == (0, 0) and _plan(cmk_lib, 200, 8, 16, 0) == (0, 0)


# (the library refuses more ways than chunk pairs)
@pytest.mark.parametrize("chunks,ways", [(c, w) for c in (2, 4, 6, 12, 32, 34, 64, 96, 128) for w in (1, 2, 3, 4, 8) if w <= c // 2])
def test_piece_bounds_cover_every_chunk_pair_once(cmk_lib, chunks, ways):
    pieces = [_bounds(cmk_lib, chunks, ways, p) for p in range(ways)]
    assert pieces[0][0] == 0 and pieces[-1][1] == chunks
    for (lo, hi), nxt in zip(pieces, pieces[1:] + [None]):
        assert lo % 2 == 0 and hi % 2 == 0 and hi > lo           # whole pairs, never an empty piece
        if nxt is not None:
            assert hi == nxt[0]                                  # every pair exactly once
    sizes = [(hi - lo) // 2 for lo, hi in pieces]
    assert max(sizes) - min(sizes) <= 1
    if chunks % (2 * ways) == 0:                                 # where ordinary split-K's rule holds: its bounds
        assert pieces == [(p * chunks // ways, (p + 1) * chunks // ways) for p in range(ways)]


def test_piece_bounds_of_the_272_channel_conv(cmk_lib):
    assert [_bounds(cmk_lib, 34, 8, p) for p in range(8)] == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 20), (20, 24), (24, 28), (28, 34)]
    assert [_bounds(cmk_lib, 34, 4, p) for p in range(4)] == [(0, 8), (8, 16), (16, 24), (24, 34)]
    assert [_bounds(cmk_lib, 6, 2, p) for p in range(2)] == [(0, 2), (2, 6)]      # Cin 48: pieces of 1 + 2 pairs
