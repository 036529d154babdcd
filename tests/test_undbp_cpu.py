"""Undbp without a device: the varint, header, block, group and item functions of csrc/brotli_undbp.h through their host hook
(BrotliAmdDebugUndbpHost runs every segment's walk, then the items' sums, the carries and the items' stores, with items of a given size and in
a given order, over segments placed at given skews) against the reference (dbp_ref.py), the new names of batch.h, and the argument failures that
need no device.  Every comparison is exact and over the WHOLE destination buffer, which starts as a sentinel pattern: a byte written outside a
segment's elements fails the test (and the hook itself, which returns -2)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import dbp_ref as ref
import san_program
from conftest import ROOT

NEW_SYMBOLS = ["BrotliAmdBatchUndbpSegments", "BrotliAmdBatchUndbpOutputs", "BrotliAmdBatchLastUndbpMs", "BrotliAmdBatchLastUndbpPhaseMs",
               "BrotliAmdDebugUndbpItemDeltas", "BrotliAmdDebugUndbpWalkChunk", "BrotliAmdDebugUndbpHost"]
SHAPES = [(128, 1), (128, 4), (256, 4), (1024, 8), (1024, 32), (65536, 4)]


def sentinel(size):
    return ((np.arange(size, dtype=np.uint64) % 251 + 3).astype(np.uint8)).tobytes()


def check(pkg, src, segs, dst_size, **kw):
    """segs: [(source offset, source length, destination offset, cap, width)] -> the results; the whole destination and every result are
    compared with the reference"""
    want, want_res = bytearray(sentinel(dst_size)), []
    for s, l, d, cap, w in segs:
        elems, res = ref.elements_bytes(src[s:s + l], w, cap)
        assert d + len(elems) <= dst_size
        want[d:d + len(elems)] = elems
        want_res.append(res)
    got, res = pkg.undbp_host(src, segs, dst_size, fill=sentinel(dst_size), **kw)
    assert res == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(res, want_res)) if a != b][:3]
    if got != bytes(want):
        at = next(i for i in range(dst_size) if got[i] != want[i])
        raise AssertionError("byte %d of the destination is %#x, not %#x; segment %r" % (at, got[at], want[at], [s for s in segs if s[2] <= at < s[2] + s[3] * s[4]][:1]))
    return res


def one(pkg, data, w, cap=None, **kw):
    """one segment with room for cap elements (None: all of them) -> its result"""
    count = ref.decode(data, w, 0)[1][0]
    cap = count if cap is None else cap
    return check(pkg, b"\x99\x99\x99" + data + b"\x99", [(3, len(data), 5, cap, w)], 5 + min(cap, count) * w + 40, **kw)[0]


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("undbp_segments", "undbp_outputs", "count_dbp_outputs", "last_undbp_ms"):
        assert callable(getattr(pkg.Batch, name))
    for name in ("undbp_host", "undbp_item_deltas", "undbp_walk_chunk"):
        assert callable(getattr(pkg, name))
    assert pkg.undbp_item_deltas() % (64 * 32) == 0 and pkg.undbp_walk_chunk() % 16 == 0
    assert (pkg.UNDBP_OK, pkg.UNDBP_BAD_HEADER, pkg.UNDBP_BAD_WIDTH, pkg.UNDBP_TRUNCATED) == (ref.OK, ref.BAD_HEADER, ref.BAD_WIDTH, ref.TRUNCATED)
    for name, value in (("OK", 0), ("BAD_HEADER", 1), ("BAD_WIDTH", 2), ("TRUNCATED", 3)):
        assert "BROTLI_AMD_UNDBP_%s %du" % (name, value) in header
    assert "typedef struct BrotliAmdUndbpResult" in header
    assert ctypes.sizeof(pkg.UndbpResult) == 48


def test_the_reference():
    """the pinned vectors by hand, the numpy decoder against the serial one, and the encoder's round trip"""
    for data, values, consumed in ref.PINNED:
        vals = [v & ref.M64 for v in values]
        res = (len(vals), consumed, len(vals), 1 if len(vals) > 1 else 0, ref.OK, 128, 4)
        assert ref.decode_serial(data) == (vals, res), data.hex()
        got, r = ref.decode(data)
        assert (list(map(int, got)), r) == (vals, res), data.hex()
    assert ref.encode([7, 8, 9, 10, 11], junk=0) == ref.PINNED[0][0] and ref.encode([7, 5, 3, 1, 2, 3, 4, 5], junk=0) == ref.PINNED[1][0]
    assert ref.encode([-1]) == ref.PINNED[2][0] and ref.encode([0, -(1 << 63)], vlen=lambda p: 10 if p == ("min", 0) else 0) == ref.PINNED[3][0]
    assert ref.varint(3, 3) == b"\x83\x80\x00" and ref.varint(300) == b"\xac\x02" and ref.unzigzag(ref.zigzag(-5)) == (-5) & ref.M64
    rnd = random.Random(5)
    for B, M in SHAPES[:5]:
        for bits in (0, 9, 33, 64):
            values = ref.random_values(rnd, B + B // M + 3, bits)
            data = ref.encode(values, B, M, widen=lambda b, j, k: min(64, k + j % 3))
            for w in ref.WIDTHS:
                res = (len(values), len(data), len(values), (len(values) - 1 + B - 1) // B, ref.OK, B, M)
                assert ref.decode_serial(data, w) == ([v & ((1 << (8 * w)) - 1) for v in values], res), (B, M, bits, w)
            for cut in (len(data), len(data) - 1, len(data) // 2, 5, 1):
                for cap in (None, 7):
                    got, r = ref.decode(data[:cut], 4, cap)
                    assert (list(map(int, got)), r) == ref.decode_serial(data[:cut], 4, cap), (B, M, bits, cut, cap)


def test_pinned_vectors(pkg):
    for data, values, consumed in ref.PINNED:
        for w in ref.WIDTHS:
            assert one(pkg, data, w) == (len(values), consumed, len(values), 1 if len(values) > 1 else 0, ref.OK, 128, 4)
    dst, res = pkg.undbp_host(ref.PINNED[0][0], [(0, 10, 0, 5, 2)], 10)
    assert dst == b"".join(v.to_bytes(2, "little") for v in (7, 8, 9, 10, 11)) and res == [(5, 10, 5, 1, 0, 128, 4)]
    # OK with bytes behind the last block: consumed says where they begin
    assert one(pkg, ref.PINNED[1][0] + b"abcdef", 8) == (8, 18, 8, 1, ref.OK, 128, 4)


@pytest.mark.parametrize("B,M", SHAPES)
def test_counts_around_every_edge(pkg, B, M):
    """N around a group, a miniblock, a block and an item, of the device's size and of small ones, in shuffled orders"""
    V, rnd = B // M, random.Random(B + M)
    for item in (64, 96, 0):
        C = item or pkg.undbp_item_deltas()
        ns = sorted({0, 1, 2, 33, 34, V + 1, V + 2, B + 1, B + 2, C, C + 1, C + 2, 2 * C + 1})
        if B == 65536:
            ns = [n for n in ns if n <= 2 * V + 2 or n in (B + 1, B + 2)][:9 if item else 12]
        for n in ns:
            values = ref.random_values(rnd, n, rnd.choice([0, 1, 7, 12, 30]))
            w = rnd.choice(ref.WIDTHS)
            res = one(pkg, ref.encode(values, B, M), w, item_deltas=item, order_seed=n % 3, src_skew=n % 16, dst_skew=(3 * n) % 16)
            assert res[0] == n and res[4] == ref.OK and res[3] == (max(n, 1) - 1 + B - 1) // B


def test_mixed_widths_and_wrapping_sums(pkg):
    """one block whose miniblocks have the widths 0, 1, 7, 8, 31, 32, 33, 63 and 64; sums that wrap at 64 bits; a min_delta of -2^63"""
    rnd = random.Random(3)
    values, B, M, widths = ref.mixed_width_block(rnd)
    data = ref.encode(values, B, M, mins=lambda b, lo: 0)
    at = len(ref.varint(B) + ref.varint(M) + ref.varint(len(values)) + ref.varint(ref.zigzag(values[0]))) + 1   # (a min_delta of one byte)
    assert list(data[at:at + M]) == widths and max(values) > 1 << 63 and any(values[i + 1] < values[i] for i in range(len(values) - 1))
    for w in ref.WIDTHS:
        for item in (64, 96, 0):
            assert one(pkg, data, w, item_deltas=item, order_seed=w)[0] == len(values)
    values = [0, -(1 << 63), 5, 5 - (1 << 63), (1 << 64) - 1, 0, 1 << 63] * 30
    for w in ref.WIDTHS:
        assert one(pkg, ref.encode(values, 128, 4), w, item_deltas=64, order_seed=2)[0] == len(values)
    # widths written above the needed ones
    values = ref.random_values(rnd, 700, 9)
    assert one(pkg, ref.encode(values, 256, 8, widen=lambda b, j, k: [k, 64, k + 1, 33][(b + j) % 4]), 8, item_deltas=96, order_seed=1)[0] == 700


def test_varints_of_every_length(pkg):
    """1 to 10 bytes in every place of the header and in a block's min_delta"""
    rnd = random.Random(4)
    values = ref.random_values(rnd, 300, 11)
    for place in ("B", "M", "N", "first", ("min", 0), ("min", 2)):
        for length in range(1, 11):
            data = ref.encode(values, 128, 4, vlen=lambda p: length if p == place else 0)
            assert one(pkg, data, 8, item_deltas=64, src_skew=length) == (300, len(data), 300, 3, ref.OK, 128, 4)
    big = [(1 << 64) - 3, 5]   # a first value and a min_delta of ten bytes by themselves
    assert one(pkg, ref.encode(big, declared=2), 8)[0] == 2
    # eleven bytes in every place of the header
    for place in range(4):
        parts = [ref.varint(128), ref.varint(4), ref.varint(2), ref.varint(0)]
        parts[place] = b"\x80" * 10 + b"\x00"
        assert one(pkg, b"".join(parts) + bytes(40), 4) == (0, 0, 0, 0, ref.BAD_HEADER, 0, 0)


def test_header_rules(pkg):
    for B, M, ok in [(0, 4, 0), (64, 2, 0), (192, 2, 0), (65536 + 128, 4, 0), (128, 0, 0), (128, 3, 0), (128, 8, 0), (256, 16, 0), (128, 4, 1), (65536, 2048, 1),
                     (1 << 40, 4, 0), (128, 1 << 33, 0)]:
        data = ref.varint(B) + ref.varint(M) + ref.varint(1) + ref.varint(ref.zigzag(-9))
        rep = (min(B, ref.U32), min(M, ref.U32))
        assert one(pkg, data, 4) == ((1, len(data), 1, 0, ref.OK) + rep if ok else (0, 0, 1, 0, ref.BAD_HEADER) + rep), (B, M)
    hdr = ref.varint(128, 3) + ref.varint(4, 2) + ref.varint(0) + ref.varint(0, 4)
    assert one(pkg, hdr + b"junk", 4) == (0, len(hdr), 0, 0, ref.OK, 128, 4)
    for cut in range(len(hdr)):
        assert one(pkg, hdr[:cut], 4) == (0, 0, 0, 0, ref.TRUNCATED, 0, 0)


def test_all_skews(pkg):
    """segments of 0 .. 70 bytes and a few longer ones at every pair of skews"""
    rnd = random.Random(7)
    datas = []
    for n in list(range(71)) + [200, 333]:
        w = rnd.choice(ref.WIDTHS)
        data = ref.encode(ref.random_values(rnd, 400, rnd.choice([3, 10, 40])), *rnd.choice(SHAPES[:3]))[:n]
        datas.append((data, w, ref.decode(data, w)[1][0]))
    for ss in range(16):
        for ds in range(16):
            segs, src, d_at = [], bytearray(), 3
            for data, w, count in datas:
                segs.append((len(src), len(data), d_at, count, w))
                src += data
                d_at += count * w + 1
            check(pkg, bytes(src), segs, d_at + 16, src_skew=ss, dst_skew=ds, item_deltas=32 * (1 + (ss + ds) % 3), order_seed=ss * 16 + ds)


@pytest.mark.parametrize("item", [64, 96, 0])
def test_blocks_across_item_edges(pkg, item):
    """blocks that span three items, and items that span many blocks, in shuffled orders"""
    C = item or pkg.undbp_item_deltas()
    rnd = random.Random(C)
    for B, M in [(128, 4), (256, 4), (1024, 32)] + ([(65536, 4)] if item == 0 else []):
        Bs = max(B, 128 * ((3 * C + 127) // 128)) if B < 3 * C and item else B
        n = max(3 * Bs + 5, 3 * C + 5)
        values = ref.random_values(rnd, n, 13)
        for B2, M2 in {(B, M), (Bs, M)}:
            if (B2 // M2) % 32 == 0 and B2 <= 65536:
                data = ref.encode(values, B2, M2)
                for seed in (0, 1, 2):
                    assert one(pkg, data, rnd.choice(ref.WIDTHS), item_deltas=item, order_seed=seed, dst_skew=seed + 1, src_skew=5 * seed)[0] == n


def test_capacities(pkg):
    """0, below, equal to and above count: the result does not depend on it, and nothing is written beyond it"""
    rnd = random.Random(8)
    for w in ref.WIDTHS:
        data = ref.encode(ref.random_values(rnd, 500, 17), 128, 4)
        results = {one(pkg, data, w, cap=cap, item_deltas=64, order_seed=cap) for cap in (0, 1, 2, 64, 65, 66, 499, 500, 501, 600, 1 << 56)}
        assert len(results) == 1 and results.pop()[0] == 500


def test_every_stop(pkg):
    """every row of the stop table at the first, a middle and the last block: what lies in front of the stop is delivered"""
    rnd = random.Random(9)
    for B, M in [(128, 4), (256, 2)]:
        V = B // M
        values = ref.random_values(rnd, 1 + 4 * B, 9)
        for name, tail, status, gives, used in ref.stops(B, M):
            for front in (0, 2, 4):
                head = ref.encode(values[:1 + front * B], B, M, declared=1 + (front + 1) * B)
                res = one(pkg, head + tail, rnd.choice(ref.WIDTHS), item_deltas=64, order_seed=front + 1)
                consumed = len(head) + (len(tail) if used is None else used)
                assert res == (1 + front * B + gives, consumed, 1 + (front + 1) * B, front + (1 if gives else 0), status, B, M), (name, B, M, front)
        # a width above 64 in an unneeded miniblock is not looked at; in a needed one it stops the block although a payload in front is cut
        data = ref.encode(values[:1 + B + V], B, M, junk=0xFF)
        assert one(pkg, data, 8)[4] == ref.OK
        bad = bytearray(ref.encode(values[:1 + 2 * B], B, M))
        first_block = len(ref.encode(values[:1 + B], B, M))
        nb = ref.read_varint(bytes(bad), first_block)[1]   # (the second block's min_delta)
        bad[first_block + nb + (M - 1)] = 65
        assert one(pkg, bytes(bad[:first_block + nb + M + 3]), 8) == (1 + B, first_block, 1 + 2 * B, 1, ref.BAD_WIDTH, B, M)
        # a cut last padding: the values are all there
        values2 = values[:1 + B + 3]
        k_last = ref.encode(values2, B, M)[first_block + nb]
        if k_last:
            cut = (V - 3) * k_last // 8
            data = ref.encode(values2, B, M, cut=cut)
            assert one(pkg, data, 8) == (len(values2), len(data), len(values2), 2, ref.TRUNCATED, B, M)


def test_three_thousand_segments(pkg):
    src, segs, size = ref.short_table()
    assert len(segs) == 3000 and sum(1 for s in segs if s[1] == 0) > 100
    res = check(pkg, src, segs, size, src_skew=5, dst_skew=11, order_seed=4)
    assert {r[4] for r in res} == {ref.OK, ref.BAD_HEADER, ref.BAD_WIDTH, ref.TRUNCATED}


def test_bad_arguments(pkg):
    data = ref.PINNED[0][0]
    good = (0, len(data), 0, 5, 4)
    for bad_w in (3, 0, 16):
        with pytest.raises(RuntimeError, match="undbp segment 1: width is not 1, 2, 4 or 8"):
            pkg.undbp_host(data, [good, good[:4] + (bad_w,)], 64)
    for flag in (1, 2, 128):
        with pytest.raises(RuntimeError, match="undbp segment 0: unknown flag bits"):
            pkg.undbp_host(data, [good + (flag,)], 64)
    with pytest.raises(RuntimeError, match=r"undbp segment 0: a capacity above 2\^56"):
        pkg.undbp_host(data, [(0, len(data), 0, (1 << 56) + 1, 4)], 64)
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.undbp_host(data, [(1, len(data), 0, 5, 4)], 64)
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.undbp_host(data, [(0, len(data), 50, 5, 4)], 64)   # 5 elements of 4 bytes from 50 on
    with pytest.raises(RuntimeError, match="invalid undbp arguments"):
        pkg.undbp_host(data, [good], 64, src_skew=16)
    with pytest.raises(RuntimeError, match="no multiple of 32"):
        pkg.undbp_host(data, [good], 64, item_deltas=48)
    assert pkg.undbp_host(b"", [], 8, fill=1) == (b"\x01" * 8, [])


def test_sanitizer_program(tmp_path):
    r = san_program.run("undbp_san", tmp_path)
    assert re.search(r"^\d+ segments$", r.stdout.strip())
