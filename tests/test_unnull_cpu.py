"""Unnull without a device: the prefix, mask, rank and validity functions of csrc/brotli_unnull.h on unrle's walk, through their host hook
(BrotliAmdDebugUnnullHost runs every segment's walk, then the items' counts, the carries and the items' expansion, with items of a given size in
given orders, over a source, a destination, a values buffer and a bitmap buffer placed at given skews) against the reference (null_ref.py), the
new names of batch.h, and the argument failures that need no device.  Every comparison is exact and over the WHOLE destination buffer and the
WHOLE bitmap buffer, which start as sentinel patterns: a byte written outside a segment's slots or validity bytes fails the test (and the hook
itself, which returns -2)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import null_ref as ref
import rle_ref
import san_program
from conftest import ROOT

NEW_SYMBOLS = ["BrotliAmdBatchUnnullSegments", "BrotliAmdBatchUnnullOutputs", "BrotliAmdBatchLastUnnullMs", "BrotliAmdBatchLastUnnullPhaseMs",
               "BrotliAmdDebugUnnullHost"]
KS = [0, 1, 2, 3, 8, 9, 32]
PF = ref.LENGTH_PREFIX | ref.VALUES_FOLLOW


def sentinel(size, mul=1):
    return (((np.arange(size, dtype=np.uint64) * mul) % 251 + 3).astype(np.uint8)).tobytes()


def levels_of(k):
    top = (1 << k) - 1
    return sorted({0, top, top // 2})


def check(pkg, src, values, segs, dst_size, valid_size, **kw):
    """segs: [(source offset, source length, destination offset, cap, bits, width, flags, level, values offset, values count, validity offset)]
    -> the results; the whole destination, the whole bitmap buffer and every result are compared with the reference"""
    want, want_bits, want_res = bytearray(sentinel(dst_size)), bytearray(sentinel(valid_size, 7)), []
    for s, l, d, cap, k, w, f, level, v, V, b in segs:
        slots, bits, res = ref.outputs(src[s:s + l], k, level, w, f, values[v:], V, cap)
        assert d + len(slots) <= dst_size
        want[d:d + len(slots)] = slots
        if b != ref.NO_BITMAP:
            assert b + len(bits) <= valid_size
            want_bits[b:b + len(bits)] = bits
        want_res.append(res)
    got, got_bits, res = pkg.unnull_host(src, values, segs, dst_size, valid_size, fill=sentinel(dst_size), valid_fill=sentinel(valid_size, 7), **kw)
    assert res == want_res, [(i, a, b, segs[i]) for i, (a, b) in enumerate(zip(res, want_res)) if a != b][:3]
    if got != bytes(want):
        at = next(i for i in range(dst_size) if got[i] != want[i])
        raise AssertionError("byte %d of the destination is %#x, not %#x; segment %r" % (at, got[at], want[at], [s for s in segs if s[2] <= at < s[2] + s[3] * s[5]][:1]))
    if got_bits != bytes(want_bits):
        at = next(i for i in range(valid_size) if got_bits[i] != want_bits[i])
        raise AssertionError("byte %d of the bitmaps is %#x, not %#x" % (at, got_bits[at], want_bits[at]))
    return res


def one(pkg, data, k, level, w, values=b"", V=0, flags=0, cap=None, bitmap=True, **kw):
    """one segment with room for cap slots (None: all of them) -> its result"""
    count = ref.decode(data, k, level, w, flags, values, V, 0)[2][0]
    cap = count if cap is None else cap
    m = min(cap, count)
    return check(pkg, b"\x99\x99\x99" + bytes(data) + b"\x99", values, [(3, len(data), 5, cap, k, w, flags, level, 0, V, 2 if bitmap else ref.NO_BITMAP)], 5 + m * w + 40,
                 2 + (m + 7) // 8 + 20, **kw)[0]


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("unnull_segments", "unnull_outputs", "count_levels_outputs", "last_unnull_ms"):
        assert callable(getattr(pkg.Batch, name))
    assert callable(pkg.unnull_host)
    assert ctypes.sizeof(pkg.UnnullResult) == 56
    assert [f[0] for f in pkg.UnnullResult._fields_] == ["count", "consumed", "runs", "status", "bits", "present", "missing", "values"]
    assert (pkg.UNNULL_LENGTH_PREFIX, pkg.UNNULL_VALUES_FOLLOW, pkg.UNNULL_BAD_LENGTH) == (ref.LENGTH_PREFIX, ref.VALUES_FOLLOW, ref.BAD_LENGTH) == (1, 2, 5)
    assert pkg.UNNULL_NO_BITMAP == ref.NO_BITMAP
    for text in ("BROTLI_AMD_UNNULL_LENGTH_PREFIX 1u", "BROTLI_AMD_UNNULL_VALUES_FOLLOW 2u", "BROTLI_AMD_UNNULL_BAD_LENGTH 5u", "typedef struct BrotliAmdUnnullResult"):
        assert text in header, text


def test_pinned_vectors(pkg):
    for k, level, flags, data, w, values, cap, slots, bits, (count, consumed, present, missing, V) in ref.PINNED:
        table = b"" if values is None else ref.values_bytes(values, w)
        n = 0 if values is None else len(values)
        got, got_bits, res = ref.decode(data, k, level, w, flags, table, n, cap)
        assert list(map(int, got)) == slots and got_bits == bits and res[:2] + res[5:] == (count, consumed, present, missing, V), data.hex()
        out, out_bits, results = pkg.unnull_host(data, table, [(0, len(data), 0, len(slots), k, w, flags, level, 0, n, 0)], len(slots) * w, len(bits))
        assert out == np.array(slots, dtype="<u%d" % w).tobytes() and out_bits == bits, data.hex()
        assert results == [res] and res[3] == ref.OK and res[4] == k, data.hex()
    for data in (ref.V1_EXAMPLE[:3], b"\x0b" + ref.V1_EXAMPLE[1:]):   # the prefix is cut; L is one above the room
        assert pkg.unnull_host(data, b"", [(0, len(data), 0, 8, 1, 2, PF, 1, 0, 0, 0)], 16, 1, fill=9, valid_fill=9) == (b"\x09" * 16, b"\x09", [(0, 0, 0, ref.BAD_LENGTH, 1, 0, 0, 0)])


def test_every_width_field_width_and_level(pkg):
    """every w with every k of KS and level 0, 2^k - 1 and a middle value; levels above and below `level`; both kinds of run"""
    rnd = random.Random(51)
    for w in ref.WIDTHS:
        for k in KS:
            for level in levels_of(k):
                plan = ref.level_plan(rnd, k, level, 150, 0.4)
                data = rle_ref.encode(plan, k)
                present = ref.present_of(plan, level)
                values = ref.random_values(rnd, present + 2, w)
                res = one(pkg, data, k, level, w, values, present, item_elems=24, order_seed=k + 1)
                assert res == (len(rle_ref.plan_values(plan)), len(data), len(plan), ref.OK, k, present, 0, present), (w, k, level)


def test_unmasked_rle_value(pkg):
    """an RLE run's value is not masked: 0xFF under k = 3 is level 255, not 7"""
    data = rle_ref.encode([("rle", 2, 0xFF), ("rle", 3, 7)], 3)
    vals = ref.values_bytes([5, 6, 7, 8, 9], 4)
    assert one(pkg, data, 3, 7, 4, vals, 5)[5:] == (3, 0, 5)
    assert one(pkg, data, 3, 255, 4, vals, 5)[5:] == (2, 0, 5)
    data = rle_ref.encode([("rle", 4, 0xFFFFFFFF), ("packed", [0xFFFFFFFF, 1, 2, 3, 4, 5, 6, 7])], 32)
    assert one(pkg, data, 32, 0xFFFFFFFF, 1, vals, 5)[5:] == (5, 0, 5)


@pytest.mark.parametrize("item", [8, 24, 1024])
def test_patterns_across_lanes_bytes_and_items(pkg, item):
    """all null, none null, alternating, and long null and present runs that straddle a lane's 16, a byte's 8 and an item's edge; m % 8 in
    0 .. 7; items in shuffled orders"""
    rnd = random.Random(52)
    k, w = 1, 4
    alt = [i & 1 for i in range(2 * item + 16)]
    plans = {
        "all null": [("rle", 2 * item + 5, 0)],
        "none null": [("rle", item + 3, 1), ("packed", [1] * 24)],
        "alternating": [("packed", alt)],
        "long runs": [("rle", 13, 1), ("rle", item - 7, 0), ("rle", item + 9, 1), ("packed", alt[:16]), ("rle", 2 * item + 1, 0), ("rle", 7, 1), ("rle", 17, 0), ("rle", 15, 1)],
        "many short runs": [("rle", 1 + i % 3, i & 1) for i in range(200)],
    }
    for name, plan in plans.items():
        data = rle_ref.encode(plan, k)
        n, present = len(rle_ref.plan_values(plan)), ref.present_of(plan, 1)
        values = ref.random_values(rnd, present, w)
        for cut in range(8):
            for seed in (0, 3):
                res = one(pkg, data, k, 1, w, values, present, cap=n - cut, item_elems=item, order_seed=seed)
                assert res[0] == n and res[6] == 0, (name, cut)
        assert one(pkg, data, k, 1, w, values, present, item_elems=item, order_seed=9)[5] == present, name


def test_all_skews(pkg):
    """every skew of the levels, of the values, of the destination and of the bitmap, independently and together, at every w"""
    rnd = random.Random(53)
    for w in ref.WIDTHS:
        plans = [ref.level_plan(rnd, 2, 3, n, 0.3, runs=(1, 9), packed=(8, 16)) for n in (1, 9, 70)]
        values = ref.random_values(rnd, 200, w)
        for skew in range(16):
            segs, src, d_at, b_at, v_at = [], bytearray(), 3, 1, 0
            for j, plan in enumerate(plans):
                data = rle_ref.encode(plan, 2)
                count, present = len(rle_ref.plan_values(plan)), ref.present_of(plan, 3)
                segs.append((len(src), len(data), d_at, count, 2, w, 0, 3, v_at, present, b_at))
                src += data
                d_at += count * w + 1
                b_at += (count + 7) // 8 + (j & 1)
                v_at += present * w + j
            for ss, ds, vs, bs in ((skew, 0, 0, 0), (0, skew, 0, 0), (0, 0, skew, 0), (0, 0, 0, skew), (skew, (skew * 7 + 3) % 16, (skew * 5 + 1) % 16, (skew * 3 + 2) % 16)):
                res = check(pkg, bytes(src), values, segs, d_at + 16, b_at + 16, src_skew=ss, dst_skew=ds, values_skew=vs, valid_skew=bs, item_elems=8 * (1 + skew % 3),
                            order_seed=skew)
                assert all(r[6] == 0 and r[5] == r[7] for r in res)


def test_capacities_and_value_counts(pkg):
    """cap below, at and above count; V at present - 1 with the missing slot first, middle and last; V = 0 and V above present; no bitmap"""
    rnd = random.Random(54)
    k, w, level = 2, 8, 2
    for plan in ([("rle", 1, 2), ("rle", 40, 0), ("packed", [2, 1, 2, 3, 0, 2, 2, 1] * 5), ("rle", 9, 3)],       # the last present slot in the middle
                 [("rle", 30, 1), ("packed", [2, 2, 0, 0, 2, 2, 2, 2] * 4), ("rle", 1, 2)],                        # ... is the last slot
                 [("rle", 1, 2), ("rle", 50, 1)]):                                                                # ... is the first slot
        data = rle_ref.encode(plan, k)
        n, present = len(rle_ref.plan_values(plan)), ref.present_of(plan, level)
        values = ref.random_values(rnd, present + 4, w)
        for V, missing in [(present, 0), (present - 1, 1), (0, present), (present + 4, 0)]:
            for bitmap in (True, False):
                assert one(pkg, data, k, level, w, values, V, bitmap=bitmap, item_elems=8, order_seed=V + 1) == (n, len(data), len(plan), ref.OK, k, present, missing, V)
        for cap in (0, 1, n // 2, n - 1, n, n + 5, 1 << 56):
            res = one(pkg, data, k, level, w, values, present, cap=cap, item_elems=24, order_seed=cap % 5)
            assert res[:5] == (n, len(data), len(plan), ref.OK, k) and res[7] == present and (cap != 0 or res[5:7] == (0, 0)), cap


def test_every_stop(pkg):
    """every unrle stop at the first, a middle and the last run: what lies in front of the stop is delivered; with the prefix too"""
    rnd = random.Random(55)
    for k, w in [(1, 4), (3, 1), (9, 2), (32, 8), (0, 1)]:
        level = (1 << k) - 1
        plan = ref.level_plan(rnd, k, level, 100, 0.3, runs=(1, 30), packed=(8, 24))
        present = ref.present_of(plan, level)
        values = ref.random_values(rnd, present, w)
        for name, tail, status in rle_ref.stops(k):
            for front in (0, len(plan) // 2, len(plan)):
                head = rle_ref.encode(plan[:front], k)
                res = one(pkg, head + tail, k, level, w, values, present, item_elems=8, order_seed=front + 1)
                assert res[3] == status and res[4] == k, (name, k, w, front)
                res = one(pkg, ref.v1_body(head + tail, values), k, level, w, flags=PF, item_elems=8)
                assert res[3] == status and res[7] == 0 and res[6] == res[5], (name, k, w, front)   # (V = 0 where the status is not OK: every present slot is missing)
    assert one(pkg, b"", 3, 1, 4) == (0, 0, 0, ref.OK, 3, 0, 0, 0)


def test_length_prefix(pkg):
    """len 0 .. 4; L one above the room; L that cuts a run; L short of len with 0 .. w left-over bytes under VALUES_FOLLOW"""
    rnd = random.Random(56)
    for w in ref.WIDTHS:
        plan = [("rle", 5, 1), ("packed", [1, 0, 1, 1, 0, 0, 1, 0] * 3), ("rle", 11, 0), ("rle", 3, 1)]
        levels = rle_ref.encode(plan, 1)
        n, present = len(rle_ref.plan_values(plan)), ref.present_of(plan, 1)
        values = ref.random_values(rnd, present, w)
        body = ref.v1_body(levels, values)
        for cut in range(5):
            for flags in (ref.LENGTH_PREFIX, PF):
                want = (0, 0, 0, ref.BAD_LENGTH, 1, 0, 0, 0) if cut < 4 else (0, 4, 0, ref.OK, 1, 0, 0, 0)
                assert one(pkg, (b"\0" * 4)[:cut], 1, 1, w, flags=flags, cap=3) == want, cut
        for flags in (ref.LENGTH_PREFIX, PF):
            bad = (len(levels) + 1).to_bytes(4, "little") + levels
            assert one(pkg, bad, 1, 1, w, values, present, flags=flags, cap=n)[:4] == (0, 0, 0, ref.BAD_LENGTH)
        for extra in range(w + 1):   # left-over bytes: a whole further value at `extra` == w
            res = one(pkg, body + bytes(extra), 1, 1, w, flags=PF, item_elems=8, order_seed=extra)
            assert res == (n, 4 + len(levels), len(plan), ref.OK, 1, present, 0, present + extra // w), extra
        assert one(pkg, body, 1, 1, w, values, present, flags=ref.LENGTH_PREFIX) == (n, 4 + len(levels), len(plan), ref.OK, 1, present, 0, present)
        for L in range(len(levels)):   # an L that cuts the runs: judged as unrle judges a segment of that length
            cut = L.to_bytes(4, "little") + body[4:]
            res = one(pkg, cut, 1, 1, w, flags=PF, item_elems=8)
            r = rle_ref.decode(levels[:L], 1, 8)[1]
            assert res[:5] == (r[0], 4 + r[1], r[2], r[3], r[4]), L


def test_three_thousand_segments(pkg):
    src, values, segs, size, bsize = ref.short_table()
    assert len(segs) == 3000
    res = check(pkg, src, values, segs, size, bsize, src_skew=5, dst_skew=11, values_skew=3, valid_skew=9, order_seed=4)
    assert {r[3] for r in res} == {ref.OK, ref.BAD_HEADER, ref.ZERO_RUN, ref.TRUNCATED, ref.BAD_LENGTH}
    assert sum(1 for r in res if r[6]) > 100 and sum(1 for r in res if r[5] and not r[6]) > 300
    check(pkg, src, values, segs, size, bsize, item_elems=8, order_seed=77)


def test_bad_arguments(pkg):
    values = bytes(64)
    good = (0, 2, 0, 8, 3, 4, 0, 5, 0, 8, 0)
    src = b"\x10\x05"
    for bad_w in (3, 0, 16):
        with pytest.raises(RuntimeError, match="unnull segment 1: width is not 1, 2, 4 or 8"):
            pkg.unnull_host(src, values, [good, good[:5] + (bad_w,) + good[6:]], 64, 8)
    with pytest.raises(RuntimeError, match="unnull segment 0: unknown flag bits"):
        pkg.unnull_host(src, values, [good[:6] + (4,) + good[7:]], 64, 8)
    with pytest.raises(RuntimeError, match="unnull segment 0: values that follow the levels without a length prefix"):
        pkg.unnull_host(src, values, [good[:6] + (ref.VALUES_FOLLOW,) + good[7:]], 64, 8)
    with pytest.raises(RuntimeError, match=r"unnull segment 0: field of more than 32 bits \(bits 33, level 5, width 4"):
        pkg.unnull_host(src, values, [good[:4] + (33,) + good[5:]], 64, 8)
    with pytest.raises(RuntimeError, match=r"unnull segment 0: a capacity above 2\^56"):
        pkg.unnull_host(src, values, [good[:3] + ((1 << 56) + 1,) + good[4:]], 64, 8)
    with pytest.raises(RuntimeError, match=r"unnull segment 2: more than 2\^56 values \(.*values 72057594037927937\)"):
        pkg.unnull_host(src, values, [good, good, good[:9] + ((1 << 56) + 1, 0)], 64, 8)
    with pytest.raises(RuntimeError, match="values outside their buffer"):
        pkg.unnull_host(src, values, [good[:8] + (40, 8, 0)], 64, 8)   # 8 values of 4 bytes from 40 on
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.unnull_host(src, values, [(1, 2) + good[2:]], 64, 8)
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.unnull_host(src, values, [(0, 2, 40) + good[3:]], 64, 8)   # 8 slots of 4 bytes from 40 on
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.unnull_host(src, values, [good[:10] + (8,)], 64, 8)       # a validity byte from 8 on
    for item in (4, 12, 1023):
        with pytest.raises(RuntimeError, match="an item that is no multiple of 8 slots"):
            pkg.unnull_host(src, values, [good], 64, 8, item_elems=item)
    for kw in ({"src_skew": 16}, {"dst_skew": 16}, {"values_skew": 16}, {"valid_skew": 16}):
        with pytest.raises(RuntimeError, match="invalid unnull arguments"):
            pkg.unnull_host(src, values, [good], 64, 8, **kw)
    assert pkg.unnull_host(b"", b"", [], 8, 2, fill=1, valid_fill=2) == (b"\x01" * 8, b"\x02" * 2, [])
    # no values need no bytes: every present slot is missing
    assert pkg.unnull_host(src, b"", [(0, 2, 0, 8, 3, 2, 0, 5, 0, 0, 0)], 16, 1) == (bytes(16), b"\xff", [(8, 2, 1, ref.OK, 3, 8, 8, 0)])


def test_the_hooks_own_check(pkg):
    """the hook's -2: a destination and a bitmap that the hook is told are smaller than what the slots need is refused in front of any store
    (-1), so what -2 guards -- a store outside -- cannot be provoked through the functions themselves: the rooms' comparison is exercised by
    every test above, whose sentinels around the slots and the validity bytes all passed through it"""
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.unnull_host(b"\x10\x05", bytes(8), [(0, 2, 0, 8, 3, 1, 0, 5, 0, 8, 0)], 7, 1)
    out, bits, res = pkg.unnull_host(b"\x10\x05", bytes(range(1, 9)), [(0, 2, 1, 8, 3, 1, 0, 5, 0, 8, 1)], 10, 3, fill=0x77, valid_fill=0x66)
    assert out == b"\x77" + bytes(range(1, 9)) + b"\x77" and bits == b"\x66\xff\x66" and res[0][5:] == (8, 0, 8)


def test_sanitizer_program(tmp_path):
    r = san_program.run("unnull_san", tmp_path)
    assert re.search(r"^\d+ segments$", r.stdout.strip())
