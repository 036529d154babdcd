"""Bit-unpack without a device: the functions of csrc/brotli_bitunpack.h through their host hook (BrotliAmdDebugBitUnpackHost takes the words of
a segment placed at given skews as the kernel's lanes would) against numpy (bitpack_ref.py), the pinned vectors of the transform, the new names
of batch.h, and the argument failures that need no device."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import bitpack_ref as ref
import san_program
from conftest import ROOT

WIDTHS = [1, 2, 4, 8]
ALL_FLAGS = [0, ref.MSB_FIRST, ref.SIGNED, ref.MSB_FIRST | ref.SIGNED]
NEW_SYMBOLS = ["BrotliAmdBatchBitUnpackSegments", "BrotliAmdBatchBitUnpackOutputs", "BrotliAmdBatchLastBitUnpackMs", "BrotliAmdDebugBitUnpackTile",
               "BrotliAmdDebugBitUnpackHost"]
GUARD = bytes((0x3C ^ (11 * i)) & 0xFF for i in range(16))   # sixteen bytes of a fixed pattern on either side of a destination
OFF = 13   # where the tests' inputs begin in the seeded bytes
SKEW_KS = [1, 3, 7, 8, 13, 31, 32, 33, 63, 64]   # the field widths that run at all 16 x 16 pairs of skews


@pytest.fixture(scope="module")
def data():
    """seeded bytes, computed once: room for the fields of two tiles and a few elements"""
    return np.random.default_rng(20271).integers(0, 256, size=(1 << 18) + 4096, dtype=np.uint8).tobytes()


def _host(pkg, x, m, k, w, flags, src_skew, dst_skew):
    """the hook into a destination between two guards -> (the destination's bytes, the fast items); the guards are asserted"""
    L = pkg.load_library()
    n = m * w
    src = ctypes.create_string_buffer(x, max(1, len(x)))
    room = ctypes.create_string_buffer(GUARD + b"\xEE" * n + GUARD, n + 32)
    fast = ctypes.c_uint64(0)
    rc = L.BrotliAmdDebugBitUnpackHost(k, w, flags, ctypes.addressof(src), len(x), m, ctypes.addressof(room) + 16, src_skew, dst_skew, ctypes.byref(fast))
    assert rc == 0, (rc, pkg.last_error())
    raw = room.raw
    assert raw[:16] == GUARD and raw[16 + n:32 + n] == GUARD, (w, k, flags, m, src_skew, dst_skew)
    return raw[16:16 + n], fast.value


def _pairs(seed, count=4):
    """seeded pairs of skews, the first with the destination at skew 0"""
    rnd = random.Random(seed)
    return [(rnd.randrange(16), 0 if i == 0 else rnd.randrange(1, 16)) for i in range(count)]


def _check(pkg, data, w, k, flags, m, pairs):
    x = data[OFF:OFF + ref.src_bytes(m, k)]
    want = ref.unpack(x, m, k, w, flags)
    for ss, ds in pairs:
        got, fast = _host(pkg, x, m, k, w, flags, ss, ds)
        assert got == want, (w, k, flags, m, ss, ds)
        assert fast == (m // 32 if ds == 0 else 0), (w, k, flags, m, ss, ds, fast)


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("bitunpack_outputs", "bitunpack_segments", "last_bitunpack_ms"):
        assert callable(getattr(pkg.Batch, name))
    assert callable(pkg.bitunpack_host) and callable(pkg.bitunpack_tile)
    assert (pkg.BITUNPACK_MSB_FIRST, pkg.BITUNPACK_SIGNED) == (1, 2) == (ref.MSB_FIRST, ref.SIGNED)
    for name, value in (("BROTLI_AMD_BITUNPACK_MSB_FIRST", 1), ("BROTLI_AMD_BITUNPACK_SIGNED", 2)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), header), name


def test_the_pinned_vectors(pkg):
    assert ref.pack(ref.PINNED_VALUES, 3) == ref.PINNED_LSB
    assert ref.pack(ref.PINNED_VALUES, 3, ref.MSB_FIRST) == ref.PINNED_MSB
    plain = bytes(ref.PINNED_VALUES)
    for fn in (ref.unpack, ref.unpack_loop, lambda *a: pkg.bitunpack_host(*a)[0]):
        assert fn(ref.PINNED_LSB, 8, 3, 1, 0) == plain
        assert fn(ref.PINNED_MSB, 8, 3, 1, ref.MSB_FIRST) == plain
        assert fn(ref.PINNED_MSB, 8, 3, 2, ref.MSB_FIRST | ref.SIGNED) == ref.PINNED_MSB_SIGNED_W2
    assert len(ref.valid_shapes()) == 120


def test_the_reference_is_the_definition(data):
    """numpy against the bit-by-bit loop, and pack against both"""
    for w, k in ref.valid_shapes():
        for flags in ALL_FLAGS:
            for m in (0, 1, 2, 7, 8, 9, 33):
                x = data[9:9 + ref.src_bytes(m, k)]
                y = ref.unpack(x, m, k, w, flags)
                assert y == ref.unpack_loop(x, m, k, w, flags), (w, k, flags, m)
                again = ref.pack(np.frombuffer(y, dtype="<u%d" % w), k, flags)
                pad = (-m * k) % 8   # the pad bits of the last byte are zero in `again`
                if m:
                    keep = (0xFF << pad) & 0xFF if flags & ref.MSB_FIRST else 0xFF >> pad
                    assert again == x[:-1] + bytes([x[-1] & keep]), (w, k, flags, m)
    # numpy.packbits' own layout is the MSB-first one at k = 1
    bits = np.frombuffer(data[:100], dtype=np.uint8) & 1
    assert ref.unpack(np.packbits(bits).tobytes(), 100, 1, 1, ref.MSB_FIRST) == bits.tobytes()


@pytest.mark.parametrize("w", WIDTHS)
def test_every_shape_at_short_counts(pkg, data, w):
    """every k of the width x both orders x both extensions x the counts 0 .. 80 and those round multiples of 32, at four seeded pairs of skews"""
    counts = list(range(81)) + [95, 96, 97, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
    for k in range(1, 8 * w + 1):
        for flags in ALL_FLAGS:
            for m in counts:
                _check(pkg, data, w, k, flags, m, _pairs((w * 64 + k) * 4096 + m * 4 + flags))


@pytest.mark.parametrize("w", WIDTHS)
def test_every_pair_of_skews(pkg, data, w):
    """all 16 x 16 pairs of skews at the field widths of SKEW_KS that the element holds, both orders and both extensions"""
    every = [(ss, ds) for ss in range(16) for ds in range(16)]
    for k in [k for k in SKEW_KS if k <= 8 * w]:
        for flags in ALL_FLAGS:
            for m in (1, 31, 32, 33, 70):
                _check(pkg, data, w, k, flags, m, every)


@pytest.mark.parametrize("w", WIDTHS)
def test_the_tiles_edges(pkg, data, w):
    """destinations that end an element short of, on and an element behind a tile's edge, and two tiles and a few elements"""
    tile = pkg.bitunpack_tile() // w   # elements of a tile
    assert OFF + ref.src_bytes(2 * tile + 33, 8 * w) <= len(data)
    for k in range(1, 8 * w + 1):
        for flags in ALL_FLAGS:
            for m in (tile - 1, tile, tile + 1, 2 * tile + 33):
                if m == 2 * tile + 33 and (k + flags) % 4:   # (the two-tile count at a quarter of the shapes)
                    continue
                _check(pkg, data, w, k, flags, m, _pairs(k * 8 + flags, 2))


def test_source_bytes_behind_the_fields_are_ignored(pkg, data):
    for w, k, flags, m in ((1, 3, 0, 21), (2, 11, 1, 37), (4, 20, 2, 64), (8, 40, 3, 5)):
        need = ref.src_bytes(m, k)
        want = ref.unpack(data[:need], m, k, w, flags)
        assert pkg.bitunpack_host(data[:need + 9], m, k, w, flags, 3, 0)[0] == want
        flipped = bytearray(data[:need])
        pad = (-m * k) % 8
        if pad:   # the pad bits of the last byte too
            flipped[-1] ^= ((0xFF >> (8 - pad)) if flags & ref.MSB_FIRST else (0xFF << (8 - pad))) & 0xFF
        assert pkg.bitunpack_host(bytes(flipped), m, k, w, flags, 0, 5)[0] == want


def test_bad_arguments(pkg, data):
    L = pkg.load_library()
    src = ctypes.create_string_buffer(data[:64], 64)

    def hook(k, w, flags, count, ss=0, ds=0, src_len=64):
        dst = ctypes.create_string_buffer(b"\x77" * 1024, 1024)
        rc = L.BrotliAmdDebugBitUnpackHost(k, w, flags, ctypes.addressof(src), src_len, count, ctypes.addressof(dst), ss, ds, None)
        assert rc == 0 or dst.raw == b"\x77" * 1024   # what is refused writes nothing
        return rc

    assert hook(3, 1, 0, 8) == 0
    for k, w in ((0, 1), (0, 8), (9, 1), (17, 2), (33, 4), (65, 8), (255, 8)):
        assert hook(k, w, 0, 8) < 0 and "field" in pkg.last_error(), (k, w)
        with pytest.raises(RuntimeError, match="field"):
            pkg.bitunpack_host(data[:64], 4, k, w)
    for w in (0, 3, 5, 16, 255):
        assert hook(1, w, 0, 8) < 0 and "width" in pkg.last_error()
        with pytest.raises(RuntimeError, match="width"):
            pkg.bitunpack_host(data[:64], 4, 1, w)
    for flags in (4, 8, 128, 255, 1 << 31):
        assert hook(3, 1, flags, 8) < 0 and "flag" in pkg.last_error()
        with pytest.raises(RuntimeError, match="flag"):
            pkg.bitunpack_host(data[:64], 4, 3, 1, flags)
    # a count beyond the source: 64 bytes hold 170 fields of 3 bits
    assert hook(3, 1, 0, 170) == 0
    assert hook(3, 1, 0, 171) < 0 and "source bytes" in pkg.last_error()
    assert hook(8, 1, 0, 1, src_len=0) < 0 and "source bytes" in pkg.last_error()
    with pytest.raises(RuntimeError, match="source bytes"):
        pkg.bitunpack_host(data[:64], 171, 3, 1)
    for count in ((1 << 56) + 1, (1 << 63), (1 << 64) - 1):
        assert hook(1, 1, 0, count) < 0 and "2^56" in pkg.last_error()
        with pytest.raises(RuntimeError, match="2\\^56"):
            pkg.bitunpack_host(data[:64], count, 1, 1)
    for ss, ds in ((16, 0), (0, 16), (255, 3)):
        assert hook(3, 1, 0, 8, ss, ds) < 0 and pkg.last_error()
    # the device calls: a NULL batch, NULL arrays (no device is touched)
    one_ptr, one_len, one_cnt, one_b = (ctypes.c_void_p * 1)(16), (ctypes.c_size_t * 1)(0), (ctypes.c_uint64 * 1)(0), (ctypes.c_uint8 * 1)(4)
    assert L.BrotliAmdBatchBitUnpackSegments(None, 1, one_ptr, one_len, one_ptr, one_cnt, one_b, one_b, None, None) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchBitUnpackSegments(None, 0, None, None, None, None, None, None, None, None) < 0
    assert L.BrotliAmdBatchBitUnpackOutputs(None, one_ptr, None, one_b, one_b, None) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchLastBitUnpackMs(None) == 0.0


class _Sizes:
    """what outputs_as_tensors asks of a batch object in front of everything that needs a device"""
    def __init__(self, sizes):
        self.out_sizes = sizes


def _tensors():
    """the package's tensors module, loaded as the GPU tests load it"""
    import importlib.util
    import sys
    name = "rust_brotli_decompressor_amd.tensors"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "rust-brotli-decompressor_amd", "tensors.py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


def test_outputs_as_tensors_refuses_without_a_device(pkg):
    import torch
    tensors = _tensors()
    assert "bitpack" in tensors.FILTERS
    t = tensors.outputs_as_tensors
    for spec, size, text in (
            ((torch.int16, (8,), (("bitpack", 12), "shuffle")), 12, "stream 1.*bitpack"),
            ((torch.int16, (8,), ("bitshuffle", ("bitpack", 12))), 12, "stream 1.*bitpack"),
            ((torch.int16, (8,), (("bitpack", 0),)), 0, "stream 1.*1 .. 16"),
            ((torch.int16, (8,), (("bitpack", 17),)), 17, "stream 1.*1 .. 16"),
            ((torch.int8, (8,), (("bitpack", 9),)), 9, "stream 1.*1 .. 8"),
            ((torch.int16, (8,), (("bitpack", 12, "little"),)), 12, "stream 1.*option"),
            ((torch.int16, (8,), (("bitpack", 12, "signed", "huge"),)), 12, "stream 1.*option"),
            ((torch.int16, (8,), (("bitpack",),)), 12, "stream 1"),
            ((torch.int16, (8,), (("bitpack", 12),)), 11, "stream 1.*12"),
            ((torch.int16, (8,), (("bitpack", 12),)), 13, "stream 1.*12"),
            ((torch.int16, (8,), (("bitpack", 12), "delta")), 16, "stream 1.*12")):
        with pytest.raises(ValueError, match=text):
            t(_Sizes([4, size]), [None, spec])


def test_the_tile_hook_is_the_headers_constant(pkg):
    abi = open(os.path.join(ROOT, "rust-brotli-decompressor_amd", "csrc", "brotli_device_abi.h")).read()
    m = re.search(r"#define\s+BROTLI_AMD_BITUNPACK_TILE_BYTES\s+(\d+)u", abi)
    assert m and pkg.bitunpack_tile() == int(m.group(1)) and int(m.group(1)) % 16 == 0


def test_functions_under_sanitizers(tmp_path):
    """tests/tools/bitunpack_san.cpp: csrc/brotli_bitunpack.h against a bit-by-bit loop, every source and destination in a heap block of exactly
    the sixteen-byte words its span touches, under ASan and UBSan, as a program of its own"""
    r = san_program.run("bitunpack_san", tmp_path)
    assert "segments" in r.stdout and "fast items" in r.stdout
