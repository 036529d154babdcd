"""Unshuffle without a device: the unit function of csrc/brotli_unshuffle.h through its host hook (BrotliAmdDebugUnshuffleHost runs it over every
16-byte unit of a segment placed at given skews) against numpy, the new names of batch.h, and the argument failures that need no device."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import shuffle_ref as ref
import san_program
from conftest import ROOT

WIDTHS = [1, 2, 4, 8]
NEW_SYMBOLS = ["BrotliAmdBatchUnshuffleSegments", "BrotliAmdBatchUnshuffleOutputs", "BrotliAmdBatchLastUnshuffleMs",
               "BrotliAmdDebugUnshuffleTile", "BrotliAmdDebugUnshuffleHost"]
GUARD = bytes((0xC3 ^ (7 * i)) & 0xFF for i in range(16))   # sixteen bytes of a fixed pattern on either side of a destination


@pytest.fixture(scope="module")
def data():
    """seeded bytes, computed once: room for a tile + 9"""
    return np.random.default_rng(20263).integers(0, 256, size=1 << 16, dtype=np.uint8).tobytes()


def _host(pkg, data, w, src_skew, dst_skew):
    """the hook into a destination between two guards -> the destination's bytes (the guards are asserted)"""
    L = pkg.load_library()
    n = len(data)
    src = ctypes.create_string_buffer(bytes(data), max(1, n))
    room = ctypes.create_string_buffer(GUARD + b"\xEE" * n + GUARD, n + 32)
    rc = L.BrotliAmdDebugUnshuffleHost(w, ctypes.addressof(src), n, ctypes.addressof(room) + 16, src_skew, dst_skew)
    assert rc == 0, (rc, pkg.last_error())
    raw = room.raw
    assert raw[:16] == GUARD and raw[16 + n:32 + n] == GUARD, (w, n, src_skew, dst_skew)
    return raw[16:16 + n]


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("unshuffle_outputs", "unshuffle_segments", "last_unshuffle_ms"):
        assert callable(getattr(pkg.Batch, name))
    assert callable(pkg.unshuffle_host)


def test_the_references_invert_each_other(data):
    for w in WIDTHS:
        for n in list(range(0, 70)) + [1023, 4099]:
            x = data[5:5 + n]
            assert ref.unshuffle(ref.shuffle(x, w), w) == x
            assert ref.shuffle(ref.unshuffle(x, w), w) == x
    # the definition, bytewise, once
    x, w = data[:23], 4
    m = len(x) // w
    assert ref.unshuffle(x, w) == bytes(x[(p % w) * m + p // w] if p < w * m else x[p] for p in range(len(x)))


@pytest.mark.parametrize("w", WIDTHS)
def test_short_lengths_at_every_pair_of_skews(pkg, data, w):
    """every length 0..80 x every (source skew, destination skew) in 16 x 16"""
    for n in range(81):
        want = ref.unshuffle(data[3:3 + n], w)
        for ss in range(16):
            for ds in range(16):
                got = _host(pkg, data[3:3 + n], w, ss, ds)
                assert got == want, (w, n, ss, ds)


def _pairs(seed):
    """the 16 diagonal pairs of skews and 16 seeded ones"""
    rnd = random.Random(seed)
    return [(k, k) for k in range(16)] + [(rnd.randrange(16), rnd.randrange(16)) for _ in range(16)]


@pytest.mark.parametrize("w", WIDTHS)
def test_longer_lengths(pkg, data, w):
    """every length 81..160, every 16 w k + d (k in 1..5, d in -1..w), 1023, 1024, 1025 and the tile's edges, at 32 pairs of skews each"""
    tile = pkg.unshuffle_tile()
    lens = set(range(81, 161)) | {16 * w * k + d for k in range(1, 6) for d in range(-1, w + 1)} | {1023, 1024, 1025, tile - 1, tile, tile + w + 1}
    assert tile + w + 1 + 11 <= len(data)
    for n in sorted(lens):
        want = ref.unshuffle(data[11:11 + n], w)
        for ss, ds in _pairs(n * 8 + w):
            assert _host(pkg, data[11:11 + n], w, ss, ds) == want, (w, n, ss, ds)


def test_the_python_helper_and_the_round_trip(pkg, data):
    for w in WIDTHS:
        for n in (0, 1, w - 1, w, 5 * w + 3, 4096 + w - 1):
            x = data[100:100 + n]
            assert pkg.unshuffle_host(ref.shuffle(x, w), w, 5, 9) == x, (w, n)


def test_bad_widths_and_arguments(pkg, data):
    L = pkg.load_library()
    src = ctypes.create_string_buffer(data[:64], 64)
    for w in (0, 3, 16, 255):
        dst = ctypes.create_string_buffer(b"\x77" * 64, 64)
        assert L.BrotliAmdDebugUnshuffleHost(w, ctypes.addressof(src), 64, ctypes.addressof(dst), 0, 0) < 0 and "width" in pkg.last_error()
        assert dst.raw == b"\x77" * 64
        with pytest.raises(RuntimeError, match="width"):
            pkg.unshuffle_host(data[:64], w)
    dst = ctypes.create_string_buffer(b"\x77" * 64, 64)
    for ss, ds in ((16, 0), (0, 16)):
        assert L.BrotliAmdDebugUnshuffleHost(4, ctypes.addressof(src), 64, ctypes.addressof(dst), ss, ds) < 0 and pkg.last_error()
    assert dst.raw == b"\x77" * 64
    # the device calls: a NULL batch, NULL arrays (no device is touched)
    one_ptr, one_len, one_w = (ctypes.c_void_p * 1)(16), (ctypes.c_size_t * 1)(0), (ctypes.c_uint8 * 1)(4)
    assert L.BrotliAmdBatchUnshuffleSegments(None, 1, one_ptr, one_ptr, one_len, one_w, None) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchUnshuffleSegments(None, 0, None, None, None, None, None) < 0
    assert L.BrotliAmdBatchUnshuffleOutputs(None, one_ptr, one_w) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchLastUnshuffleMs(None) == 0.0


def test_the_tile_hook_is_the_headers_constant(pkg):
    abi = open(os.path.join(ROOT, "rust-brotli-decompressor_amd", "csrc", "brotli_device_abi.h")).read()
    m = re.search(r"#define\s+BROTLI_AMD_UNSHUFFLE_TILE_BYTES\s+(\d+)u", abi)
    assert m and pkg.unshuffle_tile() == int(m.group(1)) and int(m.group(1)) % 16 == 0


def test_unit_function_under_sanitizers(tmp_path):
    """tests/tools/unshuffle_san.cpp: csrc/brotli_unshuffle.h against a bytewise loop, every source and destination in a heap block of exactly
    the sixteen-byte words its span touches, under ASan and UBSan, as a program of its own"""
    r = san_program.run("unshuffle_san", tmp_path)
    assert "segments" in r.stdout
