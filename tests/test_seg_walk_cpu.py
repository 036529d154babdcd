"""The segment walk without a device: the arithmetic that the copy, digest, unshuffle and undelta kernels share (csrc/brotli_seg_walk.h) through its
host hook -- BrotliAmdDebugSegWalkParts runs the very function the device walk runs, for every block of a grid, chunk after chunk of 1024
segments -- and as a program of its own under sanitizers.  A part is (block, tile, lo, hi): the units [lo, hi) that one chunk of segments holds
of one tile.  All comparisons are exact."""
import os

import pytest

import san_program
from conftest import ROOT

CHUNK = 1024   # segments whose prefix sum the device holds at a time (BROTLI_AMD_SEG_CHUNK_SEGS)
TILES = [4, 1024]   # units: a tiny tile, and the one of the copy, unshuffle and undelta kernels


def _units(at, length):
    return (at + length + 15) // 16 - at // 16 if length else 0


def _packed(lens, at=9):
    """the units of segments of these lengths in bytes, one behind the other from an odd address"""
    out = []
    for l in lens:
        out.append(_units(at, l))
        at += l
    return out


def _tables(tile_units):
    tile = 16 * tile_units   # bytes
    return {
        "a tile across empty segments": _packed([tile // 2 + 7] + [0] * 2500 + [tile + 9, 5, 0, 1] + [0] * 1100 + [3 * tile]),
        "1024 segments of one unit": [1] * 1024,
        "1025 segments of one unit": [1] * 1025,
        "3000 segments of one unit": [1] * 3000,
        "one segment of ten tiles and a unit": [10 * tile_units + 1],
        "all segments empty": [0] * 2100,
        "no segments": [],
    }


def _grids(units, tile_units):
    tiles = (sum(units) + tile_units - 1) // tile_units
    return [1, 2, 7, tiles + 3]


CASES = [(t, name) for t in TILES for name in _tables(t)]


def test_the_hook_and_the_header(pkg):
    lib = pkg.load_library()
    assert lib.BrotliAmdDebugSegWalkParts is not None and callable(pkg.seg_walk_parts)
    header = open(os.path.join(ROOT, "rust-brotli-decompressor_amd", "csrc", "brotli_seg_walk.h")).read()
    assert "#define BROTLI_AMD_SEG_CHUNK_SEGS %du" % CHUNK in header
    # the table of the GPU tests' shape does what its name says: a tile that begins in the first chunk and ends in the third
    for t in TILES:
        units = _tables(t)["a tile across empty segments"]
        assert len(units) > 3 * CHUNK and 0 < units[0] < t and sum(units[1:2 * CHUNK]) == 0 and units[2501] > t


@pytest.mark.parametrize("tile_units,name", CASES)
def test_the_parts_tile_the_units(pkg, tile_units, name):
    """for grids of 1, 2, 7 and more blocks than tiles: the parts are pairwise disjoint and cover [0, units) exactly; every part lies inside
    its tile and inside one chunk of segments; a tile's parts all belong to block tile % grid; and the parts do not depend on the grid"""
    units = _tables(tile_units)[name]
    total = sum(units)
    chunk_ends = [sum(units[:c + CHUNK]) for c in range(0, len(units), CHUNK)]
    sets = []
    for grid in _grids(units, tile_units):
        parts = pkg.seg_walk_parts(units, tile_units, grid)
        at = 0
        for block, tile, lo, hi in sorted(parts, key=lambda p: p[2]):
            assert lo == at and lo < hi, (grid, block, tile, lo, hi, at)   # disjoint, no unit left out
            at = hi
            assert tile * tile_units <= lo and hi <= (tile + 1) * tile_units, (grid, tile, lo, hi)
            assert block == tile % grid, (grid, block, tile)
            end = next(e for e in chunk_ends if lo < e)   # the chunk that holds lo
            assert hi <= end, (grid, tile, lo, hi, end)
        assert at == total, (grid, at, total)
        # a block takes its tiles in rising order, a tile's parts in rising order
        for b in range(grid):
            mine = [(tile, lo) for block, tile, lo, _ in parts if block == b]
            assert mine == sorted(mine), (grid, b)
        sets.append(sorted((tile, lo, hi) for _, tile, lo, hi in parts))
    assert all(s == sets[0] for s in sets)
    if not total:
        assert sets[0] == []


def test_a_tile_in_three_chunks_has_a_part_for_each_chunk_with_units(pkg):
    """the shape of test_a_tile_that_spans_a_stretch_of_empty_segments: tile 0 has a part in the first chunk, none in the second, which has no
    units, and one in the third"""
    for t in TILES:
        units = _tables(t)["a tile across empty segments"]
        first = [p for p in pkg.seg_walk_parts(units, t, 2) if p[1] == 0]
        assert first == [(0, 0, 0, units[0]), (0, 0, units[0], t)], first


def test_a_table_beyond_2_to_the_29_units(pkg):
    """short segments, one of 2^28 + 3 units -- 4 GiB and 48 bytes --, short segments, and one more of 2^28 + 1 units, so that the units sum
    beyond 2^29 and the bytes beyond 2^33: the same disjoint cover as above, with tiles of 1024 units and two grids (numpy does the comparing:
    there are more than half a million parts)"""
    import numpy as np
    tile_units = 1024
    units = [1, 3, 0, 7, 2] * 20 + [(1 << 28) + 3] + [2, 0, 5, 1, 9] * 20 + [(1 << 28) + 1]
    total = sum(units)
    tiles = (total + tile_units - 1) // tile_units
    assert len(units) < CHUNK and sum(units[:101]) > 1 << 28 and total > 1 << 29
    sets = []
    for grid in (7, tiles + 3):
        p = np.array(pkg.seg_walk_parts(units, tile_units, grid), dtype=np.uint64)
        for b in (0, 3, grid - 1):   # a block takes its tiles in rising order, a tile's parts in rising order
            mine = p[p[:, 0] == b]
            assert np.array_equal(mine, mine[np.lexsort((mine[:, 2], mine[:, 1]))]), (grid, b)
        p = p[np.argsort(p[:, 2], kind="stable")]
        block, tile, lo, hi = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
        assert lo[0] == 0 and hi[-1] == total and np.array_equal(lo[1:], hi[:-1]) and (lo < hi).all(), grid   # disjoint, no unit left out
        assert (tile * tile_units <= lo).all() and (hi <= (tile + 1) * tile_units).all(), grid
        assert np.array_equal(block, tile % grid), grid
        assert len(p) >= tiles and int(tile[-1]) == tiles - 1
        sets.append(p[:, 1:])
    assert np.array_equal(sets[0], sets[1])


def test_the_walk_under_sanitizers(tmp_path):
    """tests/tools/seg_walk_san.cpp: the same enumeration over the same tables under ASan and UBSan, as a program of its own"""
    r = san_program.run("seg_walk_san", tmp_path)
    assert r.stdout.count("parts") == len(CASES) * 4
