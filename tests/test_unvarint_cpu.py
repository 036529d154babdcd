"""Unvarint without a device: the unit and tile functions of csrc/brotli_unvarint.h through their host hook (BrotliAmdDebugUnvarintHost runs all
three phases over segments placed at given skews, with a given tile size and order of the tiles) against numpy (varint_ref.py), the new names of
batch.h, and the argument failures that need no device.  Every comparison is exact and over the WHOLE destination buffer, which starts as a
sentinel pattern: a byte written outside a segment's elements fails the test (and the hook itself, which returns -2)."""
import os
import random
import re

import numpy as np
import pytest

import san_program
import varint_ref as ref
from conftest import ROOT

WIDTHS = [1, 2, 4, 8]
NEW_SYMBOLS = ["BrotliAmdBatchUnvarintSegments", "BrotliAmdBatchUnvarintOutputs", "BrotliAmdBatchLastUnvarintMs", "BrotliAmdBatchLastUnvarintPhaseMs",
               "BrotliAmdDebugUnvarintTile", "BrotliAmdDebugUnvarintHost"]


@pytest.fixture(scope="module")
def data():
    """seeded bytes, computed once: about half of them end a varint, and some five hundred varints a MiB are overlong"""
    return np.random.default_rng(20271).integers(0, 256, size=1 << 19, dtype=np.uint8).tobytes()


def sentinel(size):
    return ((np.arange(size, dtype=np.uint64) % 251 + 3).astype(np.uint8)).tobytes()


def check(pkg, src, segs, dst_size, **kw):
    """segs: [(source offset, source length, destination offset, cap, width, flags)] -> the results; the whole destination and every result are
    compared with the reference"""
    want, want_res = bytearray(sentinel(dst_size)), []
    for s, l, d, cap, w, f in segs:
        elems, res = ref.elements_bytes(src[s:s + l], w, f, cap)
        assert d + len(elems) <= dst_size
        want[d:d + len(elems)] = elems
        want_res.append(res)
    got, res = pkg.unvarint_host(src, segs, dst_size, fill=sentinel(dst_size), **kw)
    assert res == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(res, want_res)) if a != b][:3]
    if got != bytes(want):
        at = next(i for i in range(dst_size) if got[i] != want[i])
        raise AssertionError("byte %d of the destination is %#x, not %#x; segment %r" % (at, got[at], want[at], [s for s in segs if s[2] <= at < s[2] + s[3] * s[4]][:1]))
    return res


def pack(lens, widths, flags, src_len, rnd, caps=None, src_gap=True):
    """segments of lens[i] bytes one after the other in a source of src_len bytes, here and there a gap; destinations with room for every varint
    (or caps[i] elements), back to back at whatever alignment that gives -> (segs, destination size)"""
    segs, s_at, d_at = [], 3, 5
    for i, l in enumerate(lens):
        if src_gap and rnd.random() < 0.3:
            s_at += rnd.randrange(1, 20); d_at += rnd.randrange(1, 20)
        assert s_at + l <= src_len
        cap = l if caps is None else caps[i]
        segs.append((s_at, l, d_at, cap, widths[i], flags[i]))
        s_at += l; d_at += min(cap, l) * widths[i]
    return segs, d_at + 64


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("unvarint_segments", "unvarint_outputs", "count_varints_outputs", "last_unvarint_ms"):
        assert callable(getattr(pkg.Batch, name))
    for name in ("unvarint_host", "unvarint_tile"):
        assert callable(getattr(pkg, name))
    assert pkg.unvarint_tile() % 16 == 0 and pkg.UNVARINT_ZIGZAG == ref.ZIGZAG
    assert "BROTLI_AMD_UNVARINT_ZIGZAG 1u" in header and "OVERLONG" in header and "typedef struct BrotliAmdUnvarintResult" in header


def test_the_reference(data):
    """the pinned examples, and the vectorised decoder against the serial one; the encoder round trip"""
    for src, w, f, elems, res in ref.EXAMPLES:
        vals, got = ref.unvarint(src, w, f)
        assert (list(map(int, vals)), got) == (elems, res), src.hex()
        assert ref.unvarint_serial(src, w, f) == (elems, res), src.hex()
    for w in WIDTHS:
        for f in (0, ref.ZIGZAG):
            for n in list(range(0, 40)) + [1000, 4099]:
                x = data[7:7 + n]
                vals, res = ref.unvarint(x, w, f)
                assert (list(map(int, vals)), res) == ref.unvarint_serial(x, w, f), (w, f, n)
    assert ref.unvarint(data[:1 << 16])[1][2] > 10   # overlong varints occur in random bytes
    values = [0, 1, 127, 128, 300, (1 << 63) - 1, (1 << 64) - 1]
    assert list(map(int, ref.unvarint(ref.varint(values))[0])) == values
    signed = [0, -1, 1, -2, 2147483647, -(1 << 63), (1 << 63) - 1]
    assert list(map(int, ref.unvarint(ref.varint(signed, True), 8, ref.ZIGZAG)[0].astype(np.int64))) == signed


def test_pinned_examples(pkg):
    for src, w, f, elems, res in ref.EXAMPLES:
        for ss, ds in ((0, 0), (5, 3), (15, 9)):
            got, results = pkg.unvarint_host(src, [(0, len(src), 0, len(elems), w, f)], len(elems) * w, src_skew=ss, dst_skew=ds, tile_units=1)
            assert results == [res], src.hex()
            assert got == b"".join(e.to_bytes(w, "little") for e in elems), src.hex()


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("flags", [0, ref.ZIGZAG])
def test_lengths_at_every_width(pkg, data, w, flags):
    """lengths 0 .. 70 and the lengths around 16, 64, one tile and two tiles, each at a skew of its own; one call, the kernel's tile"""
    tile = pkg.unvarint_tile()
    lens = list(range(71)) + [t + d for t in (tile, 2 * tile) for d in (-17, -1, 0, 1, 15, 16, 17)] + [63, 64, 65, 4095, 4097]
    rnd = random.Random(w * 2 + flags)
    segs, size = pack(lens, [w] * len(lens), [flags] * len(lens), len(data), rnd)
    assert len({s[0] % 16 for s in segs}) > 8 and len({s[2] % 16 for s in segs}) > 8
    check(pkg, data, segs, size, src_skew=rnd.randrange(16), dst_skew=rnd.randrange(16))


def test_every_pair_of_skews(pkg, data):
    """all 16 x 16 pairs of (source skew, destination skew) at one short length that has overlong varints in it, for every width, and a
    handful of pairs at a tile + 100 bytes"""
    x = data[100:137] + b"\x80" * 11 + data[200:203] + b"\x05"
    assert ref.unvarint(x)[1][2] >= 1
    for ss in range(16):
        for ds in range(16):
            w = WIDTHS[(ss + ds) % 4]
            check(pkg, x, [(0, len(x), 0, len(x), w, (ss ^ ds) & 1)], len(x) * w + 16, src_skew=ss, dst_skew=ds, tile_units=1 + (ss + ds) % 3)
    y = data[:pkg.unvarint_tile() + 100]
    for ss, ds, w in ((0, 0, 4), (1, 15, 8), (15, 1, 2), (7, 8, 8), (9, 3, 1)):
        check(pkg, y, [(0, len(y), 0, len(y), w, 1)], len(y) * w + 16, src_skew=ss, dst_skew=ds)


@pytest.mark.parametrize("boundary", [16, 64, 4096, "tile"])
def test_varints_across_boundaries(pkg, boundary):
    """a unit boundary (16), a thread's (64), a wave's (4096) and a tile's: a varint that ends in a tile's first bytes and begins in the tile
    before; with the kernel's tile, and the unit and thread boundaries with tiles of 1 and 4 units as well"""
    tile = pkg.unvarint_tile()
    b = tile if boundary == "tile" else boundary
    src, places, overlong = ref.boundary_segments(b, 2 * b if b >= 4096 else 128, 20272 + b)
    segs, d_at = [], 1
    for i, (s, l) in enumerate(places):
        segs.append((s, l, d_at, l, WIDTHS[i % 4], (i // 4) & 1))
        d_at += l * WIDTHS[i % 4] + i % 3
    for tu in ([0] if b >= 4096 else [0, 1, 4]):
        res = check(pkg, src, segs, d_at + 16, tile_units=tu, order_seed=tu)
    assert sum(r[2] for r in res) == overlong > 20   # the varints of 11 and 12 bytes


def test_small_tiles_in_shuffled_orders(pkg, data):
    """tiles of 1, 2 and 3 units taken in shuffled orders: the results and the bytes do not depend on it"""
    rnd = random.Random(6)
    lens = [rnd.choice([0, 1, 15, 16, 17, 33, 100, 250]) for _ in range(60)]
    segs, size = pack(lens, [rnd.choice(WIDTHS) for _ in lens], [rnd.randrange(2) for _ in lens], len(data), rnd)
    seen = set()
    for tu in (1, 2, 3):
        for seed in (0, 1, 2, 77):
            seen.add(tuple(check(pkg, data, segs, size, src_skew=tu, dst_skew=seed % 16, tile_units=tu, order_seed=seed)))
    assert len(seen) == 1


def test_segments_without_ends_and_with_trailing_bytes(pkg, data):
    """no end at all; only ends; a segment that ends in 1 .. 11 continuation bytes; 20 KiB of 0x80 in front of one end -- overlong across more
    than a whole tile --; a tenth byte with high bits set"""
    tile = pkg.unvarint_tile()
    no_ends = bytes(b | 0x80 for b in data[:300])
    assert check(pkg, no_ends, [(0, 300, 0, 10, 4, 0)], 64, tile_units=2) == [(0, 0, 0)]
    only_ends = bytes(b & 0x7F for b in data[:300])
    assert check(pkg, only_ends, [(0, 300, 3, 300, 2, 1)], 700) == [(300, 300, 0)]
    for t in range(1, 12):
        x = data[1000:1050] + b"\x07" + b"\xff" * t
        res = check(pkg, x, [(0, len(x), 1, len(x), 8, 0)], 8 * len(x) + 8, src_skew=t, tile_units=1)
        assert res[0][1] == 51 and len(x) - res[0][1] == t
    long_run = b"\x03" + b"\x80" * (20 << 10) + b"\x01\x02" + b"\x80" * 5
    assert len(long_run) > tile + 4000
    for tu, seed in ((0, 0), (0, 3), (5, 9)):
        assert check(pkg, long_run, [(0, len(long_run), 2, 10, 4, 0)], 64, src_skew=9, tile_units=tu, order_seed=seed) == [(3, (20 << 10) + 3, 1)]
    tenth = b"\xff" * 9 + b"\x7f" + b"\x80" * 9 + b"\x7e" + b"\x81" * 9 + b"\x03"
    check(pkg, tenth, [(0, len(tenth), 0, 3, 8, 0), (0, len(tenth), 24, 3, 8, 1), (0, len(tenth), 48, 3, 4, 1)], 64)
    assert list(map(int, ref.unvarint(tenth)[0])) == [(1 << 64) - 1, 0, (1 << 63) | sum(1 << (7 * j) for j in range(9))]


def test_a_varint_never_reaches_back_across_a_segment(pkg, data):
    """two segments back to back in memory, the first ending in continuation bytes: the second's first varint begins at the second's first byte;
    at every position of the boundary in its word"""
    for skew in range(16):
        for t in (1, 3, 9, 10, 12):
            first = data[50:60] + b"\x01" + b"\xc1" * t
            second = b"\x85\x86\x07" + data[70:90]
            src = first + second
            segs = [(0, len(first), 0, 30, 4, 0), (len(first), len(second), 200, 30, 8, 0)]
            res = check(pkg, src, segs, 512, src_skew=skew, tile_units=1 + skew % 3)
            assert res[0][1] == 11 and res[1][1] >= 3


def test_three_thousand_short_segments(pkg, data):
    """0 .. 300 bytes each, mixed widths and flags, empty ones among them: more than two chunks of the walk's prefix sum"""
    segs, size = ref.short_table(len(data))
    assert len(segs) > 2 * 1024
    res = check(pkg, data, segs, size, src_skew=5, dst_skew=11)
    assert sum(r[2] for r in res) > 50 and sum(1 for r in res if r == (0, 0, 0)) > 100
    assert check(pkg, data, segs, size, src_skew=5, dst_skew=11, tile_units=3, order_seed=5) == res


def test_capacities(pkg, data):
    """cap = 0, m - 1, m and m + 5: exactly min(m, cap) elements are written -- with m + 5 the bytes behind stay the sentinel's --, and the
    results are the same at every cap and every order of the tiles"""
    tile = pkg.unvarint_tile()
    for l, w in ((0, 4), (1, 8), (40, 2), (300, 8), (tile + 77, 4)):
        x = data[11:11 + l]
        m = ref.unvarint(x)[1][0]
        seen = set()
        for cap in sorted({0, max(m - 1, 0), m, m + 5}):
            for tu, seed in ((0, 0), (2, 4)):
                seen.add(check(pkg, x, [(0, l, 9, cap, w, 1)], 9 + (m + 5) * w + 32, src_skew=3, dst_skew=l % 16, tile_units=tu, order_seed=seed)[0])
        assert len(seen) == 1 and seen.pop()[0] == m


def test_refused_arguments(pkg, data):
    x = data[:64]
    for w in (0, 3, 5, 16, 255):
        with pytest.raises(RuntimeError, match=r"unvarint segment 1: width is not 1, 2, 4 or 8 \(width %d," % w):
            pkg.unvarint_host(x, [(0, 64, 0, 4, 4, 0), (0, 64, 0, 4, w, 0)], 512)
    for f in (2, 4, 3, 128):
        with pytest.raises(RuntimeError, match=r"unvarint segment 0: unknown flag bits \(width 4, flags %d," % f):
            pkg.unvarint_host(x, [(0, 64, 0, 4, 4, f)], 512)
    with pytest.raises(RuntimeError, match=r"unvarint segment 0: a capacity above 2\^56 elements"):
        pkg.unvarint_host(x, [(0, 64, 0, (1 << 56) + 1, 1, 0)], 512)
    for seg in ((60, 5, 0, 1, 1, 0), (0, 64, 500, 64, 1, 0), (0, 64, 0, 64, 8, 0), (1 << 63, 1 << 63, 0, 0, 1, 0)):
        with pytest.raises(RuntimeError, match="outside its buffer"):
            pkg.unvarint_host(x, [seg], 511)
    for kw in ({"src_skew": 16}, {"dst_skew": 16}):
        with pytest.raises(RuntimeError, match="invalid unvarint arguments"):
            pkg.unvarint_host(x, [(0, 64, 0, 4, 4, 0)], 512, **kw)
    L = pkg.load_library()
    assert L.BrotliAmdBatchUnvarintSegments(None, 0, None, None, None, None, None, None, None, None) < 0 and "invalid unvarint arguments" in pkg.last_error()
    assert L.BrotliAmdBatchUnvarintOutputs(None, None, None, None, None, None) < 0 and "invalid unvarint arguments" in pkg.last_error()
    assert L.BrotliAmdBatchLastUnvarintMs(None) == 0.0 and L.BrotliAmdBatchLastUnvarintPhaseMs(None, 1) == 0.0
    assert pkg.unvarint_host(b"", [], 0) == (b"", [])


def test_header_under_sanitizers(tmp_path):
    """tests/tools/unvarint_san.cpp: the header's functions over seeded segments at all skews, in heap blocks of exactly the words they may
    touch, under AddressSanitizer and UBSan, as a program of its own"""
    r = san_program.run("unvarint_san", tmp_path)
    assert re.search(r"\d+ segments", r.stdout)
