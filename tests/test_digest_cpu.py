"""Digests without a device: the arithmetic of csrc/brotli_crc.h through its host hooks (BrotliAmdDebugDigestHost cuts a segment the way the
kernel does: skew, 16-byte units, pieces of run_units units, a multiplication each, XOR) against zlib and a table-driven CRC-32C, the shift
against square and multiply, the new names of batch.h, and the argument failures that need no device."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import digest_ref as ref
import san_program
from conftest import ROOT

KINDS = [ref.CRC32, ref.CRC32C]
NEW_SYMBOLS = ["BrotliAmdBatchDigestSegments", "BrotliAmdBatchDigestOutputs", "BrotliAmdBatchLastDigestMs", "BrotliAmdDebugDigestTile",
               "BrotliAmdDebugDigestHost", "BrotliAmdDebugDigestShift"]


@pytest.fixture(scope="module")
def data():
    """seeded bytes, computed once: room for 3 tiles + 5"""
    return np.random.default_rng(20261).integers(0, 256, size=1 << 18, dtype=np.uint8).tobytes()


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    assert re.search(r"#define\s+BROTLI_AMD_DIGEST_CRC32\s+1u", header) and re.search(r"#define\s+BROTLI_AMD_DIGEST_CRC32C\s+2u", header)
    assert (pkg.DIGEST_CRC32, pkg.DIGEST_CRC32C) == (1, 2)
    for name in ("digest_outputs", "digest_segments", "last_digest_ms"):
        assert callable(getattr(pkg.Batch, name))


@pytest.mark.parametrize("kind", KINDS)
def test_check_values_and_the_empty_input(pkg, kind):
    assert ref.crc(kind, b"123456789") == ref.CHECK[kind]   # (the references themselves)
    for skew in (0, 7):
        for run_units in (0, 1, 3):
            assert pkg.digest_host(b"123456789", kind, skew, run_units) == ref.CHECK[kind]
            assert pkg.digest_host(b"", kind, skew, run_units) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_every_length_skew_and_run(pkg, data, kind):
    """every length 0..300 x every skew x pieces of 1, 2, 3, 4, 7 units and the kernel's own"""
    want = [ref.crc(kind, data[:n]) for n in range(301)]
    for n in range(301):
        for skew in range(16):
            for run_units in (1, 2, 3, 4, 7, 0):
                got = pkg.digest_host(data[:n], kind, skew, run_units)
                assert got == want[n], (n, skew, run_units, hex(got), hex(want[n]))


@pytest.mark.parametrize("kind", KINDS)
def test_tile_edges(pkg, data, kind):
    tile = pkg.load_library().BrotliAmdDebugDigestTile()
    assert tile % 16 == 0 and 3 * tile + 5 <= len(data)
    for n in (tile - 1, tile, tile + 1, 3 * tile + 5):
        want = ref.crc(kind, data[7:7 + n])
        for skew in (0, 1, 15):
            for run_units in (1, 2, 3, 4, 7, 0):
                assert pkg.digest_host(data[7:7 + n], kind, skew, run_units) == want, (n, skew, run_units)


@pytest.mark.parametrize("kind", KINDS)
def test_shift_combines_two_digests(pkg, data, kind):
    """crc(A B) == shift(crc(A), |B|) ^ crc(B): 200 random pairs of lengths, 0 included"""
    rnd = random.Random(kind)
    pairs = [(0, 0), (0, 5), (5, 0), (1, 1)] + [(rnd.randrange(0, 3000), rnd.randrange(0, 3000)) for _ in range(196)]
    for la, lb in pairs:
        at = rnd.randrange(0, len(data) - la - lb)
        a, b = data[at:at + la], data[at + la:at + la + lb]
        assert pkg.digest_shift(ref.crc(kind, a), lb, kind) ^ ref.crc(kind, b) == ref.crc(kind, a + b), (la, lb)


@pytest.mark.parametrize("kind", KINDS)
def test_shift_by_more_than_four_gib(pkg, kind):
    """multiplication by x^(8 n) mod P for n of 33 and 41 bits, against square and multiply in Python"""
    rnd = random.Random(100 + kind)
    for n in (0, 1, 4, (1 << 32) + 5, 1 << 40, (1 << 63) + 12345):
        power = ref.xpow(kind, 8 * n)
        assert pkg.digest_shift(0x80000000, n, kind) == power, n   # (x^0 shifted is the power itself)
        for crc in (0, 1, 0xFFFFFFFF, rnd.getrandbits(32), rnd.getrandbits(32)):
            assert pkg.digest_shift(crc, n, kind) == ref.mulmod(kind, crc, power), (hex(crc), n)


def test_argument_failures_without_a_device(pkg):
    L = pkg.load_library()
    one_ptr, one_len, out = (ctypes.c_void_p * 1)(16), (ctypes.c_size_t * 1)(0), (ctypes.c_uint32 * 1)()
    # a NULL batch
    assert L.BrotliAmdBatchDigestSegments(None, 1, 1, one_ptr, one_len, out, None) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchDigestSegments(None, 1, 0, None, None, None, None) < 0
    assert L.BrotliAmdBatchDigestOutputs(None, 1, out) < 0 and pkg.last_error()
    assert L.BrotliAmdBatchLastDigestMs(None) == 0.0
    # NULL arrays
    assert L.BrotliAmdBatchDigestSegments(None, 2, 1, None, None, None, None) < 0
    assert L.BrotliAmdBatchDigestOutputs(None, 2, None) < 0
    # a kind that is neither
    for kind in (0, 3):
        assert L.BrotliAmdBatchDigestSegments(None, kind, 1, one_ptr, one_len, out, None) < 0 and "kind" in pkg.last_error()
        assert L.BrotliAmdBatchDigestOutputs(None, kind, out) < 0 and "kind" in pkg.last_error()
        assert pkg.digest_host(b"abc", kind) == 0 and "kind" in pkg.last_error()
        assert pkg.digest_shift(1, 1, kind) == 0 and "kind" in pkg.last_error()


def test_arithmetic_under_sanitizers(tmp_path):
    """tests/tools/digest_san.cpp: csrc/brotli_crc.h against a bitwise loop, every segment in a heap block of exactly the sixteen-byte words
    it touches, under ASan and UBSan, as a program of its own"""
    r = san_program.run("digest_san", tmp_path)
    assert "digests" in r.stdout
