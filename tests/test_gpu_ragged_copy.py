"""The ragged copy kernel (csrc/brotli_copy_kernels.hip) through its test hook BrotliAmdDebugRaggedCopy: n independent segments of any
alignment and length in one launch.  Every case is a destination arena filled with a known pattern -- 64 guard bytes in front, behind, and
wherever the case leaves a gap between neighbours; most neighbours lie back to back, so that a store one byte too wide lands in another
segment or in a guard -- and the WHOLE arena is compared with a numpy restatement afterwards."""
import ctypes
import random

import numpy as np
import pytest

GUARD = 64


def _pattern(n):
    i = np.arange(n, dtype=np.uint32)
    return ((i * 7 + (i >> 8) * 13 + 0x5A) & 0xFF).astype(np.uint8)


@pytest.fixture(scope="module")
def source():
    """16 MiB + 64 of seeded bytes: computed once, never changed"""
    a = np.random.default_rng(20260).integers(0, 256, size=(16 << 20) + 64, dtype=np.uint8)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def dev_source(source):
    import torch
    return torch.from_numpy(source.copy()).cuda()


def _copy(pkg, dev_source, source, segs, dst_size):
    """segs: [(source offset, destination offset, length)] -> asserts the arena"""
    import torch
    L = pkg.load_library()
    before = _pattern(dst_size)
    dst = torch.from_numpy(before.copy()).cuda()
    n = len(segs)
    a_src = (ctypes.c_void_p * max(1, n))(*[dev_source.data_ptr() + s for s, _, _ in segs])
    a_dst = (ctypes.c_void_p * max(1, n))(*[dst.data_ptr() + d for _, d, _ in segs])
    a_len = (ctypes.c_size_t * max(1, n))(*[l for _, _, l in segs])
    torch.cuda.synchronize()
    assert L.BrotliAmdDebugRaggedCopy(n, a_src, a_dst, a_len) == 0, pkg.last_error()
    got = dst.cpu().numpy()
    want = before
    for s, d, l in segs:
        assert GUARD <= d and d + l <= dst_size - GUARD and s + l <= len(source)
        want[d:d + l] = source[s:s + l]
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        owner = next((k for k, (s, d, l) in enumerate(segs) if d <= at < d + l), None)
        raise AssertionError(("first wrong byte", at, "of segment", owner, segs[owner] if owner is not None else "a guard",
                              int(got[at]), int(want[at]), int((got != want).sum())))


def _packed(rnd, lens, src_limit, gaps=False):
    """destinations back to back from GUARD on (gaps: now and then up to 70 guard bytes between), sources anywhere"""
    segs, at = [], GUARD
    for l in lens:
        if gaps and rnd.random() < 0.1:
            at += rnd.randrange(1, 70)
        segs.append((rnd.randrange(0, src_limit - l), at, l))
        at += l
    return segs, at + GUARD


@pytest.mark.gpu
def test_every_alignment_pair(pkg, dev_source, source):
    """source offset 0..15 x destination offset 0..15 x lengths {0, 1, 2, 15, 16, 17, 31, 33, 255, 256, 257}: one launch of 2816 segments.  The
    destinations follow each other without a gap wherever the walk through the alignments allows it (a length that is odd visits all
    sixteen on its own); where the next alignment wanted is not the one reached, fewer than sixteen guard bytes lie between."""
    rnd = random.Random(1)
    segs, at = [], GUARD
    for so in range(16):
        for l in (0, 1, 2, 15, 16, 17, 31, 33, 255, 256, 257):
            left = set(range(16))
            while left:
                while at % 16 not in left:
                    at += 1
                left.discard(at % 16)
                segs.append((16 * rnd.randrange(1, 60000) + so, at, l))
                at += l
    assert len(segs) == 16 * 16 * 11
    rnd.shuffle(segs)   # (the table's order is not the arena's)
    _copy(pkg, dev_source, source, segs, at + GUARD)


@pytest.mark.gpu
def test_one_segment_and_none(pkg, dev_source, source):
    for segs in ([], [(5, GUARD + 3, 1)], [(5, GUARD + 3, 0)], [(0, GUARD, 1)], [(len(source) - 1, GUARD + 15, 1)],
                 [(0, GUARD + 1, 0), (7, GUARD + 1, 0)]):
        _copy(pkg, dev_source, source, segs, 2 * GUARD + 32)


@pytest.mark.gpu
def test_tile_edges(pkg, dev_source, source):
    """segments of tile - 1, tile, tile + 1 and 3 tile + 5 bytes at odd alignments, back to back, and the first and last bytes of the source"""
    tile = pkg.load_library().BrotliAmdDebugRaggedCopyTile()
    rnd = random.Random(2)
    lens = [tile - 1, tile, tile + 1, 3 * tile + 5]
    segs, at = [], GUARD + 5
    for so, l in [(3, l) for l in lens] + [(11, l) for l in reversed(lens)] + [(16, tile), (0, 3 * tile + 5)]:
        segs.append((16 * rnd.randrange(0, 1000) + so if so else 0, at, l))
        at += l
        if l == tile:
            at += 1   # (a guard byte, so that what follows a whole tile starts at another alignment)
    segs.append((len(source) - (tile + 1), at, tile + 1))   # ends where the source ends
    at += tile + 1
    # the same lengths with every word of the destination aligned, and the source not
    at = (at + 15) & ~15
    for l in lens:
        segs.append((16 * rnd.randrange(0, 1000) + 9, at, l))
        at = (at + l + 15) & ~15
    _copy(pkg, dev_source, source, segs, at + GUARD)


@pytest.mark.gpu
def test_one_long_segment_among_a_thousand_short_ones(pkg, dev_source, source):
    rnd = random.Random(3)
    lens = [rnd.randrange(1, 301) for _ in range(1000)]
    lens.insert(500, (8 << 20) + 3)
    segs, size = _packed(rnd, lens, len(source))
    _copy(pkg, dev_source, source, segs, size)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 257, 5000])
def test_more_segments_than_a_wave_or_a_block_covers(pkg, dev_source, source, n):
    rnd = random.Random(n)
    lens = [rnd.choice([0, 1, 3, 16, rnd.randrange(0, 41), rnd.randrange(0, 41), rnd.randrange(0, 700)]) for _ in range(n)]
    segs, size = _packed(rnd, lens, len(source), gaps=True)
    _copy(pkg, dev_source, source, segs, size)


@pytest.mark.gpu
def test_a_tile_that_spans_a_stretch_of_empty_segments(pkg, dev_source, source):
    """the kernel takes the segment table in pieces (a prefix sum of a thousand-odd segments at a time): a tile that begins in one piece, finds
    nothing in the next -- 1500 empty segments and more -- and ends in the one after"""
    rnd = random.Random(4)
    tile = pkg.load_library().BrotliAmdDebugRaggedCopyTile()
    lens = [tile // 2 + 7] + [0] * 2500 + [tile + 9, 5, 0, 1] + [0] * 1100 + [3 * tile]
    segs, size = _packed(rnd, lens, len(source))
    _copy(pkg, dev_source, source, segs, size)
