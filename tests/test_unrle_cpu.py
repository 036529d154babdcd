"""Unrle without a device: the run, element and item functions of csrc/brotli_unrle.h through their host hook (BrotliAmdDebugUnrleHost runs every
segment's walk and then the items, of a given size and in a given order, over segments placed at given skews) against the reference
(rle_ref.py), the new names of batch.h, and the argument failures that need no device.  Every comparison is exact and over the WHOLE destination
buffer, which starts as a sentinel pattern: a byte written outside a segment's elements fails the test (and the hook itself, which returns -2)."""
import os
import random
import re

import numpy as np
import pytest

import rle_ref as ref
import san_program
from conftest import ROOT

NEW_SYMBOLS = ["BrotliAmdBatchUnrleSegments", "BrotliAmdBatchUnrleOutputs", "BrotliAmdBatchLastUnrleMs", "BrotliAmdBatchLastUnrlePhaseMs",
               "BrotliAmdDebugUnrleItemElems", "BrotliAmdDebugUnrleWalkChunk", "BrotliAmdDebugUnrleHost"]


def sentinel(size):
    return ((np.arange(size, dtype=np.uint64) % 251 + 3).astype(np.uint8)).tobytes()


def check(pkg, src, segs, dst_size, **kw):
    """segs: [(source offset, source length, destination offset, cap, bits, width, flags)] -> the results; the whole destination and every
    result are compared with the reference"""
    want, want_res = bytearray(sentinel(dst_size)), []
    for s, l, d, cap, k, w, f in segs:
        elems, res = ref.elements_bytes(src[s:s + l], k, w, f, cap)
        assert d + len(elems) <= dst_size
        want[d:d + len(elems)] = elems
        want_res.append(res)
    got, res = pkg.unrle_host(src, segs, dst_size, fill=sentinel(dst_size), **kw)
    assert res == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(res, want_res)) if a != b][:3]
    if got != bytes(want):
        at = next(i for i in range(dst_size) if got[i] != want[i])
        raise AssertionError("byte %d of the destination is %#x, not %#x; segment %r" % (at, got[at], want[at], [s for s in segs if s[2] <= at < s[2] + s[3] * s[5]][:1]))
    return res


def one(pkg, data, k, w, flags=0, cap=None, **kw):
    """one segment with room for cap elements (None: all of them) -> its result"""
    count = ref.decode(data, k, w, flags, 0)[1][0]
    cap = count if cap is None else cap
    return check(pkg, b"\x99\x99\x99" + data + b"\x99", [(3, len(data), 5, cap, k, w, flags)], 5 + min(cap, count) * w + 40, **kw)[0]


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("unrle_segments", "unrle_outputs", "count_rle_outputs", "last_unrle_ms"):
        assert callable(getattr(pkg.Batch, name))
    for name in ("unrle_host", "unrle_item_elems", "unrle_walk_chunk"):
        assert callable(getattr(pkg, name))
    assert pkg.unrle_item_elems() % 64 == 0 and pkg.unrle_walk_chunk() % 16 == 0 and pkg.UNRLE_WIDTH_BYTE == ref.WIDTH_BYTE
    assert (pkg.UNRLE_OK, pkg.UNRLE_BAD_HEADER, pkg.UNRLE_ZERO_RUN, pkg.UNRLE_TRUNCATED, pkg.UNRLE_BAD_WIDTH) == (ref.OK, ref.BAD_HEADER, ref.ZERO_RUN, ref.TRUNCATED, ref.BAD_WIDTH)
    for name, value in (("OK", 0), ("BAD_HEADER", 1), ("ZERO_RUN", 2), ("TRUNCATED", 3), ("BAD_WIDTH", 4)):
        assert "BROTLI_AMD_UNRLE_%s %du" % (name, value) in header
    assert "BROTLI_AMD_UNRLE_WIDTH_BYTE 1u" in header and "typedef struct BrotliAmdUnrleResult" in header
    import ctypes
    assert ctypes.sizeof(pkg.UnrleResult) == 32


def test_the_reference():
    """the pinned vectors, the numpy decoder against the serial one, and the encoder's round trip"""
    for k, data, values in ref.PINNED:
        assert ref.decode_serial(data, k, 4) == (values, (len(values), len(data), 1, ref.OK, k)), data.hex()
        vals, res = ref.decode(data, k, 4)
        assert (list(map(int, vals)), res) == (values, (len(values), len(data), 1, ref.OK, k)), data.hex()
    assert ref.encode([("packed", list(range(8)))], 3) == ref.PINNED[0][1] and ref.encode([("rle", 200, 7)], 3) == ref.PINNED[3][1]
    assert ref.header(3, 3) == b"\x83\x80\x00" and ref.header(300) == b"\xac\x02"
    rnd = random.Random(5)
    for k, w in ref.shapes():
        plan = ref.random_plan(rnd, k, 60, packed=(8, 24), repeated=(1, 30), hlen=True)
        for wb in (False, True):
            data = ref.encode(plan, k, wb)
            values = [v & ((1 << (8 * w)) - 1) for v in ref.plan_values(plan)]
            res = (len(values), len(data), len(plan), ref.OK, k)
            assert ref.decode_serial(data, k, w, int(wb)) == (values, res), (k, w)
            for cut in (len(data), len(data) - 1, len(data) // 2, 1):
                for cap in (None, 7):
                    vals, got = ref.decode(data[:cut], k, w, int(wb), cap)
                    assert (list(map(int, vals)), got) == ref.decode_serial(data[:cut], k, w, int(wb), cap), (k, w, cut, cap)
        for _, tail, status in ref.stops(k):
            vals, got = ref.decode(ref.encode(plan[:2], k) + tail, k, w)
            assert (list(map(int, vals)), got) == ref.decode_serial(ref.encode(plan[:2], k) + tail, k, w) and got[3] == status, (k, w, tail)


def test_pinned_vectors(pkg):
    for k, data, values in ref.PINNED:
        for w in ref.WIDTHS:
            if k <= 8 * w:
                assert one(pkg, data, k, w) == (len(values), len(data), 1, ref.OK, k)
    dst, res = pkg.unrle_host(ref.PINNED[2][1], [(0, 3, 0, 3, 9, 2, 0)], 6)
    assert dst == (300).to_bytes(2, "little") * 3 and res == [(3, 3, 1, 0, 9)]
    # an RLE value is not masked to k bits, and is truncated to the element
    assert pkg.unrle_host(b"\x04\xff\x01", [(0, 3, 0, 2, 9, 2, 0)], 4)[0] == b"\xff\x01" * 2
    assert pkg.unrle_host(b"\x04\xff\x01", [(0, 3, 0, 2, 9, 4, 0)], 8)[0] == b"\xff\x01\x00\x00" * 2
    assert pkg.unrle_host(b"\x04\xff\xff", [(0, 3, 0, 2, 12, 2, 0)], 4)[0] == b"\xff\xff" * 2


def test_every_shape_and_header_length(pkg):
    """every k 0 .. 32 with every width that takes it: both kinds of run, headers of 1 .. 5 bytes, with and without the width byte"""
    rnd = random.Random(6)
    for k, w in ref.shapes():
        top = (1 << k) - 1
        plan = []
        for hl in range(1, 6):
            plan.append(("packed", [rnd.randint(0, top) for _ in range(8 * rnd.randrange(1, 4))], hl))
            plan.append(("rle", rnd.randrange(1, 40), rnd.randint(0, top), hl))
        plan.append(("packed", [top] * 8 + [0] * 8))
        for wb in (0, 1):
            data = ref.encode(plan, k, bool(wb))
            res = one(pkg, data, 99 if wb else k, w, wb, item_elems=24, order_seed=k + 1)
            assert res == (len(ref.plan_values(plan)), len(data), len(plan), ref.OK, k)


def test_all_skews(pkg):
    """segments of 0 .. 70 bytes at every pair of skews"""
    rnd = random.Random(7)
    datas = []
    for n in range(71):
        k, w = rnd.choice(ref.shapes())
        data = ref.encode(ref.random_plan(rnd, k, 3000, packed=(8, 16), repeated=(1, 9)), k)[:n]
        assert len(data) == n
        datas.append((data, k, w, ref.decode(data, k, w)[1][0]))
    for ss in range(16):
        for ds in range(16):
            segs, src, d_at = [], bytearray(), 3
            for data, k, w, count in datas:
                segs.append((len(src), len(data), d_at, count, k, w, 0))
                src += data
                d_at += count * w + 1
            check(pkg, bytes(src), segs, d_at + 16, src_skew=ss, dst_skew=ds, item_elems=8 * (1 + (ss + ds) % 3), order_seed=ss * 16 + ds)


@pytest.mark.parametrize("item", [8, 24, 0])
def test_runs_across_item_edges(pkg, item):
    """a repeated run and a packed run that each span three items; packed groups that are not aligned to the items, behind an RLE run of 1, 3 or 5
    values; more than 64 runs in one item; the items in shuffled orders"""
    C = item or pkg.unrle_item_elems()
    for k, w in [(3, 1), (12, 2), (12, 4), (17, 4), (32, 8), (0, 1), (1, 8)]:
        for lead in (1, 3, 5):
            plan = ref.straddling_plans(k, C, lead)
            data = ref.encode(plan, k)
            for seed in (0, 1, 2):
                res = one(pkg, data, k, w, item_elems=item, order_seed=seed, dst_skew=lead, src_skew=seed)
                assert res[0] == len(ref.plan_values(plan)) > 5 * C and res[2] == len(plan)
        plan = ref.many_runs_plan(k, max(200, C + C // 2), k)
        for seed in (0, 3):
            assert one(pkg, ref.encode(plan, k), k, w, item_elems=item, order_seed=seed)[2] == len(plan)


def test_capacities(pkg):
    """0, below, equal to and above count: the result does not depend on it, and nothing is written beyond it"""
    rnd = random.Random(8)
    for k, w in [(5, 1), (12, 4), (20, 8), (0, 2)]:
        data = ref.encode(ref.random_plan(rnd, k, 300, packed=(8, 80), repeated=(1, 90)), k)
        count = ref.decode(data, k, w)[1][0]
        results = {one(pkg, data, k, w, cap=cap, item_elems=24, order_seed=cap) for cap in (0, 1, 23, 24, 25, count - 1, count, count + 1, count + 100, 1 << 56)}
        assert len(results) == 1 and results.pop()[0] == count


def test_every_stop(pkg):
    """every status at the first run, a middle run and the last run: what lies in front of the stop is delivered"""
    rnd = random.Random(9)
    for k, w in [(3, 1), (9, 2), (12, 4), (32, 4), (0, 1), (1, 8)]:
        plan = ref.random_plan(rnd, k, 100, packed=(8, 24), repeated=(1, 30))
        assert len(plan) >= 3
        for name, tail, status in ref.stops(k):
            for front in (0, len(plan) // 2, len(plan)):
                head = ref.encode(plan[:front], k)
                res = one(pkg, head + tail, k, w, item_elems=8, order_seed=front + 1)
                in_front = len(ref.plan_values(plan[:front]))
                assert res[3] == status and res[4] == k, (name, k, w, front)
                if name == "payload cut":   # the whole values of the bytes that are there are counted and delivered
                    assert res == (in_front + (2 * k - 1) * 8 // k, len(head) + len(tail), front + 1, status, k)
                elif name == "all 35 bits":
                    assert res == (in_front, len(head) + len(tail), front, status, k)
                else:
                    assert res == (in_front, len(head), front, status, k), (name, k, w, front)
    # the width byte: good, bad for the element, bad for the format, and an empty segment
    body = ref.encode([("rle", 5, 1), ("packed", [1, 0, 1, 1, 0, 0, 0, 1])], 1)
    assert one(pkg, b"\x01" + body, 0, 1, ref.WIDTH_BYTE) == (13, len(body) + 1, 2, ref.OK, 1)
    assert one(pkg, b"\x09" + body, 0, 1, ref.WIDTH_BYTE) == (0, 0, 0, ref.BAD_WIDTH, 9)
    assert one(pkg, b"\x21" + body, 0, 8, ref.WIDTH_BYTE) == (0, 0, 0, ref.BAD_WIDTH, 33)
    assert one(pkg, b"", 3, 4, ref.WIDTH_BYTE) == (0, 0, 0, ref.BAD_WIDTH, 0)
    assert one(pkg, b"", 3, 4) == (0, 0, 0, ref.OK, 3)
    assert one(pkg, b"\x00", 0, 4, ref.WIDTH_BYTE) == (0, 1, 0, ref.OK, 0)


def test_three_thousand_segments(pkg):
    src, segs, size = ref.short_table()
    assert len(segs) == 3000 and sum(1 for s in segs if s[1] == 0) > 100
    res = check(pkg, src, segs, size, src_skew=5, dst_skew=11, order_seed=4)
    assert {r[3] for r in res} == {ref.OK, ref.BAD_HEADER, ref.ZERO_RUN, ref.TRUNCATED, ref.BAD_WIDTH}


def test_bad_arguments(pkg):
    good = (0, 2, 0, 8, 3, 4, 0)
    for bad_w in (3, 0, 16):
        with pytest.raises(RuntimeError, match="unrle segment 1: width is not 1, 2, 4 or 8"):
            pkg.unrle_host(b"\x10\x05", [good, good[:5] + (bad_w, 0)], 64)
    with pytest.raises(RuntimeError, match="unrle segment 0: unknown flag bits"):
        pkg.unrle_host(b"\x10\x05", [good[:6] + (2,)], 64)
    with pytest.raises(RuntimeError, match="unrle segment 0: field of more than 32 bits"):
        pkg.unrle_host(b"\x10\x05", [(0, 2, 0, 8, 33, 8, 0)], 64)
    with pytest.raises(RuntimeError, match=r"unrle segment 2: field is wider than the element \(bits 9, width 1"):
        pkg.unrle_host(b"\x10\x05", [good, good, (0, 2, 0, 8, 9, 1, 0)], 64)
    with pytest.raises(RuntimeError, match=r"unrle segment 0: a capacity above 2\^56"):
        pkg.unrle_host(b"\x10\x05", [(0, 2, 0, (1 << 56) + 1, 3, 4, 0)], 64)
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.unrle_host(b"\x10\x05", [(1, 2, 0, 8, 3, 4, 0)], 64)
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.unrle_host(b"\x10\x05", [(0, 2, 40, 8, 3, 4, 0)], 64)   # 8 elements of 4 bytes from 40 on
    with pytest.raises(RuntimeError, match="invalid unrle arguments"):
        pkg.unrle_host(b"\x10\x05", [good], 64, src_skew=16)
    assert pkg.unrle_host(b"", [], 8, fill=1) == (b"\x01" * 8, [])


def test_sanitizer_program(tmp_path):
    r = san_program.run("unrle_san", tmp_path)
    assert re.search(r"^\d+ segments$", r.stdout.strip())
