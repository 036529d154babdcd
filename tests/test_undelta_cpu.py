"""Undelta without a device: the unit and tile functions of csrc/brotli_undelta.h through their host hook (BrotliAmdDebugUndeltaHost runs all three
phases over segments placed at given skews, with a given tile size and order of the tiles) against numpy (delta_ref.py), the new names of
batch.h, and the argument failures that need no device.  All comparisons are exact."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import delta_ref as ref
import san_program
from conftest import ROOT

WIDTHS = [1, 2, 4, 8]
NEW_SYMBOLS = ["BrotliAmdBatchUndeltaSegments", "BrotliAmdBatchUndeltaOutputs", "BrotliAmdBatchLastUndeltaMs", "BrotliAmdBatchLastUndeltaPhaseMs",
               "BrotliAmdDebugUndeltaTile", "BrotliAmdDebugUndeltaCarrySpan", "BrotliAmdDebugUndeltaHost"]
FILL = 0xEE


@pytest.fixture(scope="module")
def data():
    """seeded bytes, computed once: room for a tile + 9 and for the tables of many segments"""
    return np.random.default_rng(20267).integers(0, 256, size=1 << 16, dtype=np.uint8).tobytes()


def _one(pkg, x, w, ss, ds, tile_units=0, seed=0, in_place=False):
    """one segment of all of x -> the hook's destination"""
    return pkg.undelta_host(x, [(0, 0, len(x), w)], src_skew=ss, dst_skew=ds, tile_units=tile_units, order_seed=seed, in_place=in_place, fill=FILL)


def _many(pkg, data, segs, size, **kw):
    """segs: [(source offset, destination offset, length, width)] into a destination of `size` bytes -> (got, want): what no segment covers stays FILL"""
    want = bytearray(bytes([FILL]) * size)
    for s, d, l, w in segs:
        want[d:d + l] = ref.undelta(data[s:s + l], w)
    return pkg.undelta_host(data, segs, dst_size=size, fill=FILL, **kw), bytes(want)


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("undelta_outputs", "undelta_segments", "last_undelta_ms"):
        assert callable(getattr(pkg.Batch, name))
    for name in ("undelta_host", "undelta_tile", "undelta_carry_span"):
        assert callable(getattr(pkg, name))
    assert pkg.undelta_carry_span() >= 1
    assert "Out of scope" in header and "UNDEFINED" in header


def test_the_reference_inverts_itself(data):
    for w in WIDTHS:
        for n in list(range(0, 70)) + [1023, 4099]:
            x = data[5:5 + n]
            assert ref.undelta(ref.delta(x, w), w) == x
            assert ref.delta(ref.undelta(x, w), w) == x
    # the definition, elementwise, once for every width; the sums wrap
    for w in WIDTHS:
        x = bytes([0xF0 + i for i in range(w)]) * 5 + b"\x01\x02\x03"[:w - 1]
        m = len(x) // w
        elems = [int.from_bytes(x[k * w:(k + 1) * w], "little") for k in range(m)]
        assert sum(elems) >= 1 << (8 * w)
        want = b"".join((sum(elems[:k + 1]) % (1 << (8 * w))).to_bytes(w, "little") for k in range(m)) + x[w * m:]
        assert ref.undelta(x, w) == want


@pytest.mark.parametrize("w", WIDTHS)
def test_short_lengths_at_every_pair_of_skews(pkg, data, w):
    """every length 0..80 x every (source skew, destination skew) in 16 x 16 x tiles of 1, 2 and 3 units: a carry passes through several whole
    tiles; the tiles in a shuffled order"""
    for n in range(81):
        x = data[3:3 + n]
        want = ref.undelta(x, w)
        for ss in range(16):
            for ds in range(16):
                for tu in (1, 2, 3):
                    assert _one(pkg, x, w, ss, ds, tu, seed=1 + ss * 16 + ds) == want, (w, n, ss, ds, tu)


@pytest.mark.parametrize("w", WIDTHS)
def test_short_lengths_in_place(pkg, data, w):
    """every length 0..80 in place at every element-aligned skew, tiles of 1, 2 and 3 units"""
    for n in range(81):
        x = data[7:7 + n]
        want = ref.undelta(x, w)
        for tu in (1, 2, 3):
            for ds in range(0, 16, w):
                assert _one(pkg, x, w, 0, ds, tu, seed=ds + 1, in_place=True) == want, (w, n, ds, tu)


def _pairs(seed):
    """the 16 diagonal pairs of skews and 16 seeded ones"""
    rnd = random.Random(seed)
    return [(k, k) for k in range(16)] + [(rnd.randrange(16), rnd.randrange(16)) for _ in range(16)]


@pytest.mark.parametrize("w", WIDTHS)
def test_longer_lengths(pkg, data, w):
    """every length 81..160, every 16 w k + d (k in 1..5, d in -1..w), 1023, 1024, 1025 and the tile's edges, at 32 pairs of skews each, with the
    kernel's own tile size"""
    tile = pkg.undelta_tile()
    lens = set(range(81, 161)) | {16 * w * k + d for k in range(1, 6) for d in range(-1, w + 1)} | {1023, 1024, 1025, tile - 1, tile, tile + w + 1}
    assert tile + w + 1 + 11 <= len(data)
    for n in sorted(lens):
        x = data[11:11 + n]
        want = ref.undelta(x, w)
        for ss, ds in _pairs(n * 8 + w):
            assert _one(pkg, x, w, ss, ds, 0, seed=n) == want, (w, n, ss, ds)


def _table(seed):
    """many segments back to back with tiny gaps here and there: a long one among two hundred short ones, zero-length ones between others,
    mixed widths -> (segs in buffer order, bytes of destination)"""
    rnd = random.Random(seed)
    items = [(rnd.choice([0, 0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 33, 47, 64, 100]), rnd.choice(WIDTHS)) for _ in range(200)]
    items.insert(100, (5003, rnd.choice(WIDTHS)))
    segs, s_at, d_at = [], 2, 5
    for l, w in items:
        if rnd.random() < 0.15:
            s_at += rnd.randrange(1, 20); d_at += rnd.randrange(1, 20)
        segs.append((s_at, d_at, l, w))
        s_at += l; d_at += l
    return segs, d_at + 7


@pytest.mark.parametrize("tile_units", [1, 2, 3, 5])
def test_many_segments_with_tiny_tiles(pkg, data, tile_units):
    """the table shuffled; several orders of the tiles give identical bytes, the right ones"""
    segs, size = _table(tile_units)
    random.Random(9).shuffle(segs)
    for ds in (0, 9):
        outs = []
        for seed in (0, 1, 2, 77):
            got, want = _many(pkg, data, segs, size, src_skew=3, dst_skew=ds, tile_units=tile_units, order_seed=seed)
            assert got == want, (tile_units, ds, seed)
            outs.append(got)
        assert len(set(outs)) == 1


def _units(d, l):
    return (d + l + 15) // 16 - d // 16 if l else 0


def test_segment_boundaries_inside_tiles(pkg, data):
    """tiles of 2 units at destination skew 0: a segment that ends mid-tile followed by one that starts there; zero-length segments between
    others; a segment that begins in a tile's last unit and runs through three more tiles; every width in every role"""
    for wa in WIDTHS:
        for wb in WIDTHS:
            segs = [(0, 0, 10, wa),            # one unit: ends in the middle of tile 0 ...
                    (100, 10, 0, wb),
                    (200, 10, 30, wb),         # ... and the next starts there: units 1 .. 3
                    (300, 40, 0, wa), (300, 40, 0, wb),
                    (400, 42, 8, wa),          # behind a gap of two bytes that stay what they were: units 4, 5
                    (450, 50, 5, wb),          # unit 6
                    (500, 55, 101, wb),        # units 7 .. 13: begins in the last unit of tile 3 and runs through tiles 4, 5 and 6
                    (700, 156, 1, wa)]
            pre = [0]
            for _, d, l, _ in segs:
                pre.append(pre[-1] + _units(d, l))
            assert pre[1] % 2 == 1 and pre[7] % 2 == 1 and pre[8] - pre[7] == 7 and pre[-1] == 15
            for seed in (0, 3):
                got, want = _many(pkg, data, segs, 256, src_skew=7, dst_skew=0, tile_units=2, order_seed=seed)
                assert got == want, (wa, wb, seed)


def test_in_place_among_tiles_and_the_round_trip(pkg, data):
    """in place: many element-aligned segments of mixed widths in one buffer, tiny tiles; and undelta(delta(x)) == x through the hook"""
    rnd = random.Random(11)
    segs, at = [], 0
    for _ in range(120):
        w = rnd.choice(WIDTHS)
        at = (at + rnd.randrange(0, 12) + w - 1) // w * w
        l = rnd.choice([0, 1, w, 3 * w + 1, 40, 41, 333])
        segs.append((0, at, l, w))
        at += l
    size = at + 3
    x = data[:size]
    want = bytearray(bytes([FILL]) * size)   # (the hook gives the segments' bytes back, nothing else)
    for _, d, l, w in segs:
        want[d:d + l] = ref.undelta(x[d:d + l], w)
    for ds in (0, 8):   # (a multiple of every width: the segments stay element-aligned)
        for tu in (1, 3, 0):
            assert pkg.undelta_host(x, segs, dst_skew=ds, tile_units=tu, order_seed=tu + 1, in_place=True, fill=FILL) == bytes(want), (ds, tu)
    for w in WIDTHS:
        for n in (0, 1, w - 1, w, 5 * w + 3, 4096 + w - 1):
            y = data[100:100 + n]
            assert _one(pkg, ref.delta(y, w), w, 5, 9, 3) == y, (w, n)


def _raw_host(pkg, n, src, dst, segs, ss=0, ds=0, tu=0, seed=0, in_place=0):
    L = pkg.load_library()
    a = [(ctypes.c_uint64 * max(1, n))(*[s[i] for s in segs]) for i in range(3)]
    a_w = (ctypes.c_uint8 * max(1, n))(*[s[3] for s in segs])
    return L.BrotliAmdDebugUndeltaHost(n, ctypes.addressof(src), len(src), ctypes.addressof(dst), len(dst), a[0], a[1], a[2], a_w, ss, ds, tu, seed, in_place)


def test_bad_widths_and_arguments(pkg, data):
    L = pkg.load_library()
    src = ctypes.create_string_buffer(data[:64], 64)
    for w in (0, 3, 16, 255):
        dst = ctypes.create_string_buffer(b"\x77" * 64, 64)
        assert _raw_host(pkg, 2, src, dst, [(0, 0, 16, 4), (16, 16, 48, w)]) < 0 and "width" in pkg.last_error()
        assert dst.raw == b"\x77" * 64
        with pytest.raises(RuntimeError, match="width"):
            pkg.undelta_host(data[:64], [(0, 0, 64, w)])
    dst = ctypes.create_string_buffer(b"\x77" * 64, 64)
    for ss, ds in ((16, 0), (0, 16)):
        assert _raw_host(pkg, 1, src, dst, [(0, 0, 64, 4)], ss=ss, ds=ds) < 0 and pkg.last_error()
    assert _raw_host(pkg, 1, src, dst, [(0, 1, 64, 4)]) < 0 and "outside" in pkg.last_error()   # a segment that leaves its buffer
    # in place at an address that is no multiple of the width: by the skew, and by the offset
    for w in (2, 4, 8):
        assert _raw_host(pkg, 1, src, dst, [(0, 0, 32, w)], ds=w // 2, in_place=1) < 0 and "in place" in pkg.last_error()
        assert _raw_host(pkg, 2, src, dst, [(0, 0, 8, w), (0, 8 + w - 1, 16, w)], ds=0, in_place=1) < 0 and "in place" in pkg.last_error()
        assert _raw_host(pkg, 1, src, dst, [(0, w, 32, w)], ds=0, in_place=1) == 0
        assert dst.raw[:w] == b"\x77" * w and dst.raw[w:w + 32] == ref.undelta(data[w:w + 32], w) and dst.raw[w + 32:] == b"\x77" * (32 - w)
        dst = ctypes.create_string_buffer(b"\x77" * 64, 64)
    assert dst.raw == b"\x77" * 64
    # the device calls: a NULL batch, NULL arrays (no device is touched)
    one_ptr, one_len, one_w = (ctypes.c_void_p * 1)(16), (ctypes.c_size_t * 1)(0), (ctypes.c_uint8 * 1)(4)
    assert L.BrotliAmdBatchUndeltaSegments(None, 1, one_ptr, one_ptr, one_len, one_w, None) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchUndeltaSegments(None, 0, None, None, None, None, None) < 0
    assert L.BrotliAmdBatchUndeltaOutputs(None, one_ptr, one_w) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchLastUndeltaMs(None) == 0.0
    assert L.BrotliAmdBatchLastUndeltaPhaseMs(None, 1) == 0.0


def test_the_tile_hook_is_the_headers_constant(pkg):
    abi = open(os.path.join(ROOT, "rust-brotli-decompressor_amd", "csrc", "brotli_device_abi.h")).read()
    m = re.search(r"#define\s+BROTLI_AMD_UNDELTA_TILE_BYTES\s+(\d+)u", abi)
    assert m and pkg.undelta_tile() == int(m.group(1)) and int(m.group(1)) % 16 == 0


def test_unit_and_tile_functions_under_sanitizers(tmp_path):
    """tests/tools/undelta_san.cpp: csrc/brotli_undelta.h against an elementwise loop, every source and destination in a heap block of exactly
    the sixteen-byte words its span touches, all three phases with small tiles, under ASan and UBSan, as a program of its own"""
    r = san_program.run("undelta_san", tmp_path)
    assert "segments" in r.stdout
