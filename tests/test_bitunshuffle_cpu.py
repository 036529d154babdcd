"""Bit-unshuffle without a device: the functions of csrc/brotli_bitunshuffle.h through their host hook (BrotliAmdDebugBitUnshuffleHost takes the
words of a segment placed at given skews as the kernel's lanes would) against numpy (bitshuffle_ref.py), the pinned vectors of the transform,
the new names of batch.h, and the argument failures that need no device."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import bitshuffle_ref as ref
import san_program
from conftest import ROOT

WIDTHS = [1, 2, 4, 8]
NEW_SYMBOLS = ["BrotliAmdBatchBitUnshuffleSegments", "BrotliAmdBatchBitUnshuffleOutputs", "BrotliAmdBatchLastBitUnshuffleMs",
               "BrotliAmdDebugBitUnshuffleTile", "BrotliAmdDebugBitUnshuffleHost"]
GUARD = bytes((0x3C ^ (11 * i)) & 0xFF for i in range(16))   # sixteen bytes of a fixed pattern on either side of a destination
OFF = 13   # where the tests' inputs begin in the seeded bytes


@pytest.fixture(scope="module")
def data():
    """seeded bytes, computed once: room for two tiles + 8 w + 1"""
    return np.random.default_rng(20270).integers(0, 256, size=1 << 18, dtype=np.uint8).tobytes()


def _blocks_for(n, w):
    """the block sizes every length runs under; the last is larger than the number of elements"""
    return [0, 8, 24, 32, 40, 2048, (n // w) // 8 * 8 + 16]


def _host(pkg, x, w, block, src_skew, dst_skew):
    """the hook into a destination between two guards -> (the destination's bytes, the fast items); the guards are asserted"""
    L = pkg.load_library()
    n = len(x)
    src = ctypes.create_string_buffer(x, max(1, n))
    room = ctypes.create_string_buffer(GUARD + b"\xEE" * n + GUARD, n + 32)
    fast = ctypes.c_uint64(0)
    rc = L.BrotliAmdDebugBitUnshuffleHost(w, block, ctypes.addressof(src), n, ctypes.addressof(room) + 16, src_skew, dst_skew, ctypes.byref(fast))
    assert rc == 0, (rc, pkg.last_error())
    raw = room.raw
    assert raw[:16] == GUARD and raw[16 + n:32 + n] == GUARD, (w, block, n, src_skew, dst_skew)
    return raw[16:16 + n], fast.value


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("bitunshuffle_outputs", "bitunshuffle_segments", "last_bitunshuffle_ms"):
        assert callable(getattr(pkg.Batch, name))
    assert callable(pkg.bitunshuffle_host) and callable(pkg.bitunshuffle_tile)


def test_the_pinned_vectors(pkg):
    ones = bytes.fromhex("ff00000000000000")
    diag = bytes.fromhex("0102040810204080")
    assert ref.bitunshuffle(ones, 1) == bytes.fromhex("0101010101010101") == ref.bitunshuffle_loop(ones, 1)
    assert ref.bitunshuffle(diag, 1) == diag == ref.bitunshuffle_loop(diag, 1)
    assert ref.bitshuffle(bytes(range(16)), 2) == bytes.fromhex("00aaccf000000000ffaaccf000000000")
    assert pkg.bitunshuffle_host(ones, 1)[0] == bytes.fromhex("0101010101010101")
    assert pkg.bitunshuffle_host(diag, 1)[0] == diag
    assert pkg.bitunshuffle_host(bytes.fromhex("00aaccf000000000ffaaccf000000000"), 2)[0] == bytes(range(16))
    # 100 elements of width 1 in blocks of 24: four blocks of 24 and 4 copied bytes
    assert ref._blocks(100, 1, 24) == [(0, 24), (24, 24), (48, 24), (72, 24), (96, 0)]
    x = bytes((37 * i + 11) & 0xFF for i in range(100))
    want = b"".join(ref.bitunshuffle(x[o:o + 24], 1) for o in range(0, 96, 24)) + x[96:]
    assert ref.bitunshuffle(x, 1, 24) == want
    assert pkg.bitunshuffle_host(x, 1, 24)[0] == want


def test_the_references_invert_each_other(data):
    for w in WIDTHS:
        for n in list(range(0, 70)) + [1023, 4099]:
            x = data[5:5 + n]
            for block in (0, 8, 24, 64):
                assert ref.bitunshuffle(ref.bitshuffle(x, w, block), w, block) == x
                assert ref.bitshuffle(ref.bitunshuffle(x, w, block), w, block) == x


def test_the_reference_is_the_formula(data):
    for w in WIDTHS:
        for n in (0, 1, 7, 8 * w - 1, 8 * w, 8 * w + 1, 24 * w + 3, 200 * w + 5):
            for block in (0, 8, 24, 64):
                x = data[9:9 + n]
                assert ref.bitunshuffle(x, w, block) == ref.bitunshuffle_loop(x, w, block), (w, n, block)


@pytest.mark.parametrize("w", WIDTHS)
def test_short_lengths_at_every_pair_of_skews(pkg, data, w):
    """every length 0..80 x every block size x every (source skew, destination skew) in 16 x 16"""
    for n in range(81):
        x = data[OFF:OFF + n]
        for block in _blocks_for(n, w):
            want = ref.bitunshuffle(x, w, block)
            for ss in range(16):
                for ds in range(16):
                    got, fast = _host(pkg, x, w, block, ss, ds)
                    assert got == want, (w, n, block, ss, ds)
                    assert fast == 0 or (n // w >= 32 and block != 8), (w, n, block, ss, ds, fast)


def _pairs(seed):
    """the 16 diagonal pairs of skews and 16 seeded ones, four of them with the destination at skew 0"""
    rnd = random.Random(seed)
    return [(k, k) for k in range(16)] + [(rnd.randrange(16), 0 if i < 4 else rnd.randrange(16)) for i in range(16)]


def _longer_lengths(w, tile):
    lens = set(range(81, 161)) | {8 * w * q + d for q in (1, 3, 4, 5, 8, 33) for d in (0, 1, w, 8 * w - 1)} | {1023, 1024, 1025}
    return sorted(l for l in lens if l > 80), [tile - 1, tile, tile + 1, 2 * tile + 8 * w + 1]


@pytest.mark.parametrize("w", WIDTHS)
def test_longer_lengths(pkg, data, w):
    """every length 81..160, every 8 w q + d, 1023 .. 1025 at 32 pairs of skews each, under every block size"""
    lens, _ = _longer_lengths(w, pkg.bitunshuffle_tile())
    for n in lens:
        x = data[OFF:OFF + n]
        for block in _blocks_for(n, w):
            want = ref.bitunshuffle(x, w, block)
            for ss, ds in _pairs(n * 8 + w):
                got, fast = _host(pkg, x, w, block, ss, ds)
                assert got == want, (w, n, block, ss, ds)
                if ds == 0 and block in (0, 32, 2048) and n >= 64 * w:
                    assert fast > 0, (w, n, block, ss)
                if block == 8 or n // w < 32:
                    assert fast == 0, (w, n, block, ss, ds)


@pytest.mark.parametrize("w", WIDTHS)
def test_the_tiles_edges(pkg, data, w):
    """tile - 1, tile, tile + 1 and 2 tile + 8 w + 1 bytes at 32 pairs of skews each, under every block size"""
    tile = pkg.bitunshuffle_tile()
    _, lens = _longer_lengths(w, tile)
    assert OFF + lens[-1] <= len(data)
    for n in lens:
        x = data[OFF:OFF + n]
        for block in _blocks_for(n, w):
            want = ref.bitunshuffle(x, w, block)
            for ss, ds in _pairs(n * 8 + w):
                got, fast = _host(pkg, x, w, block, ss, ds)
                assert got == want, (w, n, block, ss, ds)
                if ds == 0 and block in (0, 32, 2048):
                    assert fast > 0, (w, n, block, ss)
                if block == 8:
                    assert fast == 0, (w, n, block, ss, ds)
            if block in (0, 32, 2048):   # all whole groups of 32 of every block go the fast way where the destination is aligned
                m = n // w
                groups = m // 32 if block == 0 else (m // block) * (block // 32) + (m % block) // 32
                assert _host(pkg, x, w, block, 7, 0)[1] == groups, (w, n, block)


def test_the_python_helper_and_the_round_trip(pkg, data):
    for w in WIDTHS:
        for n in (0, 1, 8 * w - 1, 8 * w, 40 * w + 3, 4096 + w - 1):
            for block in (0, 8, 64):
                x = data[100:100 + n]
                got, fast = pkg.bitunshuffle_host(ref.bitshuffle(x, w, block), w, block, 5, 9)
                assert got == x and fast == 0, (w, n, block)
                assert pkg.bitunshuffle_host(ref.bitshuffle(x, w, block), w, block)[0] == x


def test_bad_arguments(pkg, data):
    L = pkg.load_library()
    src = ctypes.create_string_buffer(data[:64], 64)

    def hook(w, block, ss, ds):
        dst = ctypes.create_string_buffer(b"\x77" * 64, 64)
        rc = L.BrotliAmdDebugBitUnshuffleHost(w, block, ctypes.addressof(src), 64, ctypes.addressof(dst), ss, ds, None)
        assert dst.raw == b"\x77" * 64
        return rc

    for w in (0, 3, 16, 255):
        assert hook(w, 0, 0, 0) < 0 and "width" in pkg.last_error()
        with pytest.raises(RuntimeError, match="width"):
            pkg.bitunshuffle_host(data[:64], w)
    for block in (1, 4, 7, 12, 2049, (1 << 32) - 1):
        assert hook(4, block, 0, 0) < 0 and "block" in pkg.last_error()
        with pytest.raises(RuntimeError, match="block"):
            pkg.bitunshuffle_host(data[:64], 4, block)
    for ss, ds in ((16, 0), (0, 16)):
        assert hook(4, 0, ss, ds) < 0 and pkg.last_error()
    # the device calls: a NULL batch, NULL arrays (no device is touched)
    one_ptr, one_len, one_w = (ctypes.c_void_p * 1)(16), (ctypes.c_size_t * 1)(0), (ctypes.c_uint8 * 1)(4)
    assert L.BrotliAmdBatchBitUnshuffleSegments(None, 1, one_ptr, one_ptr, one_len, one_w, None, None) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchBitUnshuffleSegments(None, 0, None, None, None, None, None, None) < 0
    assert L.BrotliAmdBatchBitUnshuffleOutputs(None, one_ptr, one_w, None) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchLastBitUnshuffleMs(None) == 0.0


def test_the_tile_hook_is_the_headers_constant(pkg):
    abi = open(os.path.join(ROOT, "rust-brotli-decompressor_amd", "csrc", "brotli_device_abi.h")).read()
    m = re.search(r"#define\s+BROTLI_AMD_BITUNSHUFFLE_TILE_BYTES\s+(\d+)u", abi)
    assert m and pkg.bitunshuffle_tile() == int(m.group(1)) and int(m.group(1)) % 16 == 0


def test_functions_under_sanitizers(tmp_path):
    """tests/tools/bitunshuffle_san.cpp: csrc/brotli_bitunshuffle.h against a bit-by-bit loop, every source and destination in a heap block of
    exactly the sixteen-byte words its span touches, under ASan and UBSan, as a program of its own"""
    r = san_program.run("bitunshuffle_san", tmp_path)
    assert "segments" in r.stdout and "fast items" in r.stdout
