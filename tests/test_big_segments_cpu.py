"""The closed forms of big_segments.py against the established whole-array references on materialised bytes, at small totals (3 P + 17, P - 1,
2 P) and source offsets, before test_gpu_big_segments.py trusts them at 4 GiB: every window reference must equal a slice of what shuffle_ref,
delta_ref, bitshuffle_ref, bitpack_ref, varint_ref, rle_ref, dict_ref and dlba_ref give, and the folded digests what zlib and digest_ref give.
The windows: the whole destination in one piece, its first and last bytes, pieces around every multiple of the period and of a plane, odd
pieces of one and of a few bytes, and seeded random ones.  All comparisons are exact.  No device and no library is needed."""
import zlib

import numpy as np
import pytest

import big_segments as B
import bitpack_ref
import bitshuffle_ref
import delta_ref
import dict_ref
import digest_ref
import dlba_ref
import rle_ref
import shuffle_ref
import varint_ref

P = B.P
TOTALS = [3 * P + 17, P - 1, 2 * P]
STARTS = [0, 5, P - 3]
PER = B.period(20261)


def _windows(n, marks=(), seed=0):
    """the whole, the edges, around every mark, one byte, a few bytes, random ones"""
    marks = [t for t in list(marks) + [P, 2 * P, 3 * P] if 0 < t < n]
    out = [(0, n)] + B.windows(n, marks, seed, count=8, size=300)
    out += [(t, t + 1) for t in marks] + [(t - 1, min(n, t + 6)) for t in marks] + [(n - 1, n), (0, 1), (n // 2, n // 2)]
    return [w for w in out if 0 <= w[0] <= w[1] <= n]


def _check(window, whole, n, marks=(), seed=0):
    """window(a, b) against whole[a:b] at every window of a destination of n bytes"""
    whole = np.frombuffer(bytes(whole), dtype=np.uint8)
    assert len(whole) == n
    for a, b in _windows(n, marks, seed):
        got = window(a, b)
        assert got.dtype == np.uint8 and len(got) == b - a and np.array_equal(got, whole[a:b]), (a, b)


def test_the_period():
    assert B.is_prime(P) and P % 2 == 1 and abs(P - (1 << 18)) < 16 and not B.is_prime(P + 2) and not B.is_prime(1 << 18)
    assert len(PER) == P and not PER.flags.writeable
    assert np.array_equal(B.materialise(PER, 5, 2 * P + 3), np.tile(PER, 4)[5:5 + 2 * P + 3])
    # the condition on the inputs that the GPU tests assert on their windows, here over a whole period of positions
    for k in (29, 31, 32):
        assert B.equal_share(PER, 3, 1 << k, (1 << k) + P, k) < 0.01
        assert B.equal_share(PER, 3, 0, 1 << k, k) == 0.0
    B.assert_distinct(PER, 3, B.windows((1 << 32) + (1 << 20) + 5, [1 << 29, 1 << 31, 1 << 32], 1))
    with pytest.raises(AssertionError):
        B.assert_distinct(np.zeros(P, dtype=np.uint8), 0, [((1 << 32), (1 << 32) + 100)])
    wins = B.windows(10 * P, [P, 7 * P, 11 * P], 3)
    assert wins[0] == (0, 4096) and wins[1] == (10 * P - 4096, 10 * P) and (P - 2048, P + 2048) in wins and len(wins) == 4 + 32
    assert all(0 <= a < b <= 10 * P for a, b in wins) and B.windows(10 * P, [P], 3) == B.windows(10 * P, [P], 3)


@pytest.mark.parametrize("n", TOTALS)
@pytest.mark.parametrize("s0", STARTS)
def test_copy_unshuffle_and_undelta_windows(n, s0):
    src = B.materialise(PER, s0, n)
    _check(lambda a, b: B.copy_window(PER, s0, a, b), src, n)
    for w in (1, 2, 4, 8):
        m = n // w
        _check(lambda a, b: B.unshuffle_window(PER, s0, n, w, a, b), shuffle_ref.unshuffle(src, w), n, [w * m] + [j * m for j in range(1, w)], w)
        _check(lambda a, b: B.undelta_window(PER, s0, n, w, a, b), delta_ref.undelta(src, w), n, [w * m, P * w, 2 * P * w], w)


@pytest.mark.parametrize("n", TOTALS)
@pytest.mark.parametrize("s0", STARTS[:2])
def test_bitunshuffle_windows(n, s0):
    src = B.materialise(PER, s0, n)
    for w, block in ((1, 0), (4, 0), (4, 2048), (8, 1024), (2, 8), (1, 8192), (2, 1 << 20)):
        m = n // w
        marks = [w * m, m // 8 * 8 * w] + ([m // block * block * w, block * w, 2 * block * w] if block else [])
        _check(lambda a, b: B.bitunshuffle_window(PER, s0, n, w, block, a, b), bitshuffle_ref.bitunshuffle(src, w, block), n, marks, w + block)


@pytest.mark.parametrize("n", TOTALS)
@pytest.mark.parametrize("k,w,flags", [(3, 1, 0), (31, 4, 0), (1, 1, 3), (7, 2, 1), (12, 2, 2), (64, 8, 0), (33, 8, 3)])
def test_bitunpack_windows(n, k, w, flags):
    s0 = 5
    src = B.materialise(PER, s0, n)
    count = n * 8 // k
    _check(lambda a, b: B.bitunpack_window(PER, s0, count, k, w, flags, a, b), bitpack_ref.unpack(src, count, k, w, flags), count * w, [P * 8 // k * w], k)


@pytest.mark.parametrize("n", TOTALS)
@pytest.mark.parametrize("w,flags", [(1, 0), (1, 1), (4, 1), (8, 0)])
def test_unvarint_windows(n, w, flags):
    per = B.varint_period(20262)
    assert per[-1] < 0x80 and 0.86 < (per < 0x80).mean() < 0.89
    src = B.materialise(per, 0, n)
    vals, res = varint_ref.unvarint(src, w, flags)
    assert B.unvarint_result(per, n) == res and res[2] >= 3 * (n // P)
    assert B.unvarint_length(per, res[0]) == res[1] and B.unvarint_result(per, res[1] - 1)[0] == res[0] - 1
    for cap in (res[0], res[0] // 2 + 1, res[0] + 9):
        want, _ = varint_ref.elements_bytes(src, w, flags, cap)
        _check(lambda a, b: B.unvarint_window(per, n, w, flags, cap, a, b), want, min(cap, res[0]) * w, [], w)


def _plans(n):
    """the shapes of the GPU cases at small counts: an RLE giant, a packed giant, and three runs of which the middle one is packed"""
    return [(7, [("rle", 5 * n + 3, 0x55)]), (1, [("packed", n // 8 * 8, PER, 11)]),
            (7, [("rle", n + 5, 0x2A), ("packed", 4096, PER, 3), ("rle", 77, 0x7F)]), (0, [("rle", 9, 0), ("packed", 16, PER, 0)]),
            (13, [("packed", 8, PER, 1), ("rle", 3, 0x1ABC), ("packed", n // 16 * 8, PER, 9)])]


@pytest.mark.parametrize("n", TOTALS[1:])
def test_unrle_windows(n):
    for k, plan in _plans(n):
        data = B.rle_materialise(plan, k)
        for w in (1, 2, 8):
            if k > 8 * w:
                continue
            count = B.rle_result(plan, k)[0]
            for cap in (count, count - 5, count + 5, 3):
                want, res = rle_ref.elements_bytes(data, k, w, 0, cap)
                assert res == B.rle_result(plan, k) and res[1] == len(data)
                _check(lambda a, b: B.rle_window(plan, k, w, cap, a, b), want, min(cap, count) * w, [(n + 5) * w, (n + 5 + 4096) * w], k)


@pytest.mark.parametrize("n", TOTALS[1:])
def test_undict_windows(n):
    rng = np.random.default_rng(5)
    for k, plan in _plans(n)[:4] + [(2, [("rle", n + 3, 1), ("packed", 8, np.array([0x0C, 0x00], dtype=np.uint8), 0), ("rle", 5, 2)])]:
        for w, entries in ((8, 2), (1, 3), (2, 200)):
            table = rng.integers(1, 1 << (8 * w - 1), size=max(entries, 1), dtype=np.uint64)
            count = B.rle_result(plan, k)[0]
            data = B.rle_materialise(plan, k)
            for cap in (count, count - 7):
                want, res = dict_ref.elements_bytes(data, k, w, 0, dict_ref.dictionary_bytes(table, w), entries, cap)
                assert res == B.undict_result(plan, k, entries, cap), (k, w, entries, cap)
                _check(lambda a, b: B.undict_window(plan, k, w, table, entries, cap, a, b), want, min(cap, count) * w, [(n + 3) * w], w)
    # the one bad index of the GPU case: field 1 of the packed run is 3, with three entries
    assert B.undict_result([("rle", n + 3, 1), ("packed", 8, np.array([0x0C, 0x00], dtype=np.uint8), 0), ("rle", 5, 2)], 2, 3, 1 << 40)[5:] == (1, n + 3 + 1)


@pytest.mark.parametrize("count,length", [(1, 7), (129, 3), (128, 0), (1000, 4099), (257, 1)])
def test_undlba_page(count, length):
    """the lengths stream of a page of equal lengths, its result and its offsets against dlba_ref.column over a materialised page"""
    head = B.dlba_lengths(count, length)
    for avail, cap, data_cap in ((count * length, count, None), (count * length + 9, count - 1 or 1, None), (count * length, count + 4, count * length // 2 + 1)):
        page = head + B.materialise(PER, 4, avail).tobytes()
        for flags, base in ((0, 0), (B.OFFSETS64, 0), (0, (1 << 32) - 5), (B.OFFSETS64 | B.ENDS_ONLY, (1 << 33) + 1), (B.ENDS_ONLY, 9)):
            offsets, data, res = dlba_ref.column(page, cap, base, data_cap)
            assert res == B.dlba_result(count, length, avail, cap), (res, B.dlba_result(count, length, avail, cap))
            assert data == page[len(head):len(head) + min(res[10], avail, data_cap if data_cap is not None else avail)]
            want = dlba_ref.offsets_bytes(offsets, flags)
            _check(lambda a, b: B.dlba_offsets_window(count, length, cap, base, flags, a, b), want, len(want), [], count)


@pytest.mark.parametrize("kind", [digest_ref.CRC32, digest_ref.CRC32C])
def test_folded_digests(kind):
    """the CRC of one period folded over the repeats and a remainder: zlib on materialised repeats at small totals, digest_ref.crc32c on a period
    of 101 bytes, and the fold's own rules"""
    if kind == digest_ref.CRC32:
        for n in TOTALS + [0, 1, P, 40 * P + 1]:
            for s0 in STARTS:
                assert B.crc_periodic(kind, PER, s0, n) == zlib.crc32(B.materialise(PER, s0, n).tobytes()) & 0xFFFFFFFF, (n, s0)
    short = B.period(7, 101)
    for n, s0 in ((705, 0), (7 * 101 + 13, 40), (100, 99), (0, 0)):
        assert B.crc_periodic(kind, short, s0, n) == digest_ref.crc(kind, B.materialise(short, s0, n).tobytes()), (n, s0)
    one = (B.crc_one(kind, b"123456789"), 9)
    assert one[0] == digest_ref.CHECK[kind] and B.crc_repeat(kind, one, 0) == (0, 0) and B.crc_repeat(kind, one, 1) == one
    assert B.crc_repeat(kind, one, 5) == (B.crc_one(kind, b"123456789" * 5), 45)
    # 5 GiB of repeats folds without the bytes: two ways round give one answer
    n = 5 << 30
    q, r = divmod(n - P, P)
    head = (B.crc_one(kind, PER), P)
    rest = B.crc_join(kind, B.crc_repeat(kind, head, q), (B.crc_one(kind, PER[:r]), r))
    assert B.crc_join(kind, head, rest)[0] == B.crc_periodic(kind, PER, 0, n)
