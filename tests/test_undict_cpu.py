"""Undict without a device: the lookup and item functions of csrc/brotli_undict.h on unrle's walk, through their host hook
(BrotliAmdDebugUndictHost runs every segment's walk and then the items, of a given size and in a given order, over a source, a destination and a
dictionary placed at given skews) against the reference (dict_ref.py), the new names of batch.h, and the argument failures that need no device.
Every comparison is exact and over the WHOLE destination buffer, which starts as a sentinel pattern: a byte written outside a segment's elements
fails the test (and the hook itself, which returns -2)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import dict_ref as ref
import rle_ref
import san_program
from conftest import ROOT

NEW_SYMBOLS = ["BrotliAmdBatchUndictSegments", "BrotliAmdBatchUndictOutputs", "BrotliAmdBatchLastUndictMs", "BrotliAmdBatchLastUndictPhaseMs",
               "BrotliAmdDebugUndictHost"]
KS = [0, 1, 3, 8, 9, 16, 17, 24, 31, 32]


def sentinel(size):
    return ((np.arange(size, dtype=np.uint64) % 251 + 3).astype(np.uint8)).tobytes()


def check(pkg, src, dictionary, segs, dst_size, **kw):
    """segs: [(source offset, source length, destination offset, cap, bits, width, flags, dictionary offset, entries)] -> the results; the whole
    destination and every result are compared with the reference"""
    want, want_res = bytearray(sentinel(dst_size)), []
    for s, l, d, cap, k, w, f, t, entries in segs:
        elems, res = ref.elements_bytes(src[s:s + l], k, w, f, dictionary[t:], entries, cap)
        assert d + len(elems) <= dst_size
        want[d:d + len(elems)] = elems
        want_res.append(res)
    got, res = pkg.undict_host(src, dictionary, segs, dst_size, fill=sentinel(dst_size), **kw)
    assert res == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(res, want_res)) if a != b][:3]
    if got != bytes(want):
        at = next(i for i in range(dst_size) if got[i] != want[i])
        raise AssertionError("byte %d of the destination is %#x, not %#x; segment %r" % (at, got[at], want[at], [s for s in segs if s[2] <= at < s[2] + s[3] * s[5]][:1]))
    return res


def one(pkg, data, k, w, dictionary, entries, flags=0, cap=None, t_at=0, **kw):
    """one segment with room for cap elements (None: all of them) -> its result"""
    count = rle_ref.decode(data, k, 8, flags, 0)[1][0]
    cap = count if cap is None else cap
    return check(pkg, b"\x99\x99\x99" + data + b"\x99", dictionary, [(3, len(data), 5, cap, k, w, flags, t_at, entries)], 5 + min(cap, count) * w + 40, **kw)[0]


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("undict_segments", "undict_outputs", "last_undict_ms"):
        assert callable(getattr(pkg.Batch, name))
    assert callable(pkg.undict_host)
    assert ctypes.sizeof(pkg.UndictResult) == 48
    assert [f[0] for f in pkg.UndictResult._fields_] == ["count", "consumed", "runs", "status", "bits", "bad", "first_bad"]
    assert pkg.UNDICT_WIDTH_BYTE == ref.WIDTH_BYTE == 1 and pkg.UNDICT_NO_STREAM == ref.NO_STREAM == 0xFFFFFFFF and pkg.UNDICT_NONE == ref.NONE
    assert "BROTLI_AMD_UNDICT_WIDTH_BYTE 1u" in header and "BROTLI_AMD_UNDICT_NO_STREAM 0xFFFFFFFFu" in header
    assert "typedef struct BrotliAmdUndictResult" in header
    assert "the dictionary gather;" not in header   # (unrle's out of scope now points here)


def test_pinned_vectors(pkg):
    for k, flags, data, w, entries, values, (bad, first_bad) in ref.PINNED:
        dictionary = ref.dictionary_bytes(entries, w)
        vals, res = ref.decode(data, k, w, flags, dictionary, len(entries))
        assert list(map(int, vals)) == values and res[0] == len(values) and res[5:] == (bad, first_bad), data.hex()
        got, results = pkg.undict_host(data, dictionary, [(0, len(data), 0, len(values), k, w, flags, 0, len(entries))], len(values) * w)
        assert got == np.array(values, dtype="<u%d" % w).tobytes(), data.hex()
        assert results == [(len(values), len(data), 1, ref.OK, 3 if flags else k, bad, first_bad)], data.hex()


def test_every_width_and_field_width(pkg):
    """every w with k in KS -- the index width is not bound by w --, both kinds of run, with and without the width byte"""
    rnd = random.Random(41)
    for w in ref.WIDTHS:
        for k in KS:
            entries = min(1 << k, 600)
            dictionary = ref.random_dictionary(rnd, entries + 3, w)
            top = entries - 1
            plan = []
            for hl in (1, 3, 5):
                plan.append(("packed", [rnd.randint(0, top) for _ in range(8 * rnd.randrange(1, 4))], hl))
                plan.append(("rle", rnd.randrange(1, 40), rnd.randint(0, top), hl))
            for wb in (0, 1):
                data = rle_ref.encode(plan, k, bool(wb))
                res = one(pkg, data, 99 if wb else k, w, dictionary, entries, wb, t_at=w % 3, item_elems=24, order_seed=k + 1)
                assert res == (len(rle_ref.plan_values(plan)), len(data), len(plan), ref.OK, k, 0, ref.NONE), (w, k, wb)


def test_all_skews(pkg):
    """every skew of the source, of the destination AND of the dictionary at every w: an entry is one load where the dictionary is a multiple of
    w, and single bytes elsewhere"""
    rnd = random.Random(42)
    for w in ref.WIDTHS:
        dictionary = ref.random_dictionary(rnd, 40, w)
        datas = [rle_ref.encode(rle_ref.random_plan(rnd, 5, n, packed=(8, 16), repeated=(1, 9)), 5) for n in (1, 9, 40)]
        for skew in range(16):
            segs, src, d_at = [], bytearray(), 3
            for j, data in enumerate(datas):
                count = rle_ref.decode(data, 5, 8)[1][0]
                segs.append((len(src), len(data), d_at, count, 5, w, 0, j, 32 + j))
                src += data
                d_at += count * w + 1
            for ss, ds, ts in ((skew, 0, 0), (0, skew, 0), (0, 0, skew), (skew, (skew * 7 + 3) % 16, (skew * 5 + 1) % 16)):
                res = check(pkg, bytes(src), dictionary, segs, d_at + 16, src_skew=ss, dst_skew=ds, dict_skew=ts, item_elems=8 * (1 + skew % 3), order_seed=skew)
                assert all(r[5] == 0 for r in res)


def test_dictionary_edges(pkg):
    """D in {0, 1, the largest index, the largest index + 1, 2^k}: all, all but the zeros, exactly one, none and none of the elements are bad"""
    rnd = random.Random(43)
    for k, w in [(3, 1), (9, 2), (12, 4), (17, 8)]:
        top = (1 << k) - 1
        big = top - 2   # the largest index, once, in a packed group in the middle
        values = [rnd.randint(1, big - 1) for _ in range(64)]
        plan = [("rle", 7, 0), ("packed", values[:32]), ("rle", 5, big - 1), ("packed", values[32:40] + [big] + values[41:48]), ("rle", 3, 1)]
        flat = rle_ref.plan_values(plan)
        data = rle_ref.encode(plan, k)
        dictionary = ref.random_dictionary(rnd, 1 << k, w)
        n, at = len(flat), flat.index(big)
        assert flat.count(big) == 1
        for D, bad, first in [(0, n, 0), (1, n - 7, 7), (big, 1, at), (big + 1, 0, ref.NONE), (1 << k, 0, ref.NONE)]:
            for seed in (0, 5):
                res = one(pkg, data, k, w, dictionary, D, item_elems=8, order_seed=seed)
                assert res[5:] == (bad, first), (k, w, D)


def test_unmasked_rle_value(pkg):
    """an RLE run's value is not masked to k bits: 0xFFFFFFFF under k = 32, and 0xFF under k = 3, against a small dictionary are out of range,
    are never made an address, and give zeros"""
    dictionary = ref.dictionary_bytes(list(range(100, 110)), 4)
    data = rle_ref.encode([("rle", 4, 2), ("rle", 6, 0xFFFFFFFF), ("rle", 1, 9)], 32)
    assert one(pkg, data, 32, 4, dictionary, 10) == (11, len(data), 3, ref.OK, 32, 6, 4)
    data = rle_ref.encode([("rle", 2, 0xFF), ("rle", 3, 7)], 3)
    assert one(pkg, data, 3, 4, dictionary, 10) == (5, len(data), 2, ref.OK, 3, 2, 0)
    got, _ = pkg.undict_host(data, dictionary, [(0, len(data), 0, 5, 3, 4, 0, 0, 10)], 20)
    assert got == b"\0" * 8 + (107).to_bytes(4, "little") * 3


@pytest.mark.parametrize("item", [8, 24, 1024])
def test_bad_indices_across_items_in_any_order(pkg, item):
    """bad indices in three different items, the items taken in shuffled orders: bad and first_bad do not depend on the order"""
    rnd = random.Random(44)
    k, w, D = 9, 2, 300
    n = 5 * item + 3
    values = [rnd.randint(0, D - 1) for _ in range((n + 7) // 8 * 8)]
    where = [item + 1, item + 2, 2 * item + item // 2, 4 * item + 3]
    for at in where:
        values[at] = D + rnd.randint(0, 200)
    lead = 3
    plan = [("rle", lead, 5), ("packed", values)]
    data = rle_ref.encode(plan, k)
    dictionary = ref.random_dictionary(rnd, D + 250, w)
    seen = {one(pkg, data, k, w, dictionary, D, item_elems=item, order_seed=seed, dict_skew=seed % 16) for seed in (0, 1, 2, 3, 17)}
    assert seen == {(lead + len(values), len(data), 2, ref.OK, k, len(where), lead + where[0])}


@pytest.mark.parametrize("item", [64, 0])
def test_more_than_64_runs_in_one_item(pkg, item):
    """the plan of the device's test of the same name -- at the default item size, three items of several batches of runs each --, at every width
    and at destination skews 0 and 1, the items in a shuffled order"""
    k, D = 9, 400
    plan = ref.many_runs_plan(61)
    assert max(ref.runs_per_item(plan, pkg.unrle_item_elems())) > 64
    data = rle_ref.encode(plan, k)
    dictionary = ref.random_dictionary(random.Random(62), D, 8)
    segs, d_at = [], 0
    for skew in (0, 1):
        for w in ref.WIDTHS:
            d_at += (skew - d_at) % 16
            segs.append((2, len(data), d_at, 2880, k, w, 0, 0, D))
            d_at += 2880 * w
    res = check(pkg, b"\x99\x99" + data + b"\x99", dictionary, segs, d_at + 40, item_elems=item, order_seed=7)
    assert all(r[:4] == (2880, len(data), len(plan), ref.OK) and r[5] > 0 for r in res)


def test_capacities(pkg):
    """a capacity that cuts in front of the only bad index (bad 0) and behind it; counting alone: 0 and none"""
    rnd = random.Random(45)
    k, w, D = 7, 4, 100
    values = [rnd.randint(0, D - 1) for _ in range(200)]
    values[77] = 120
    data = rle_ref.encode([("packed", values)], k)
    dictionary = ref.random_dictionary(rnd, 128, w)
    for cap, bad in [(0, (0, ref.NONE)), (1, (0, ref.NONE)), (77, (0, ref.NONE)), (78, (1, 77)), (200, (1, 77)), (1 << 56, (1, 77))]:
        res = one(pkg, data, k, w, dictionary, D, cap=cap, item_elems=24, order_seed=cap % 7)
        assert res == (200, len(data), 1, ref.OK, k) + bad, cap


def test_every_stop(pkg):
    """every status behind a few runs: what lies in front of the stop is delivered, through the dictionary"""
    rnd = random.Random(46)
    for k, w in [(3, 1), (9, 2), (12, 8), (32, 4), (0, 1), (17, 1)]:
        D = min(1 << k, 500)
        dictionary = ref.random_dictionary(rnd, D, w)
        plan = [r[:2] + (r[2] % D,) if r[0] == "rle" else ("packed", [v % D for v in r[1]])
                for r in rle_ref.random_plan(rnd, k, 100, packed=(8, 24), repeated=(1, 30))]
        for name, tail, status in rle_ref.stops(k):
            for front in (0, len(plan)):
                head = rle_ref.encode(plan[:front], k)
                res = one(pkg, head + tail, k, w, dictionary, D, item_elems=8, order_seed=front + 1)
                assert res[3] == status and res[4] == k, (name, k, w, front)
    body = rle_ref.encode([("rle", 5, 1)], 1)
    dictionary = b"\x07\x08"
    assert one(pkg, b"\x01" + body, 0, 1, dictionary, 2, ref.WIDTH_BYTE) == (5, len(body) + 1, 1, ref.OK, 1, 0, ref.NONE)
    assert one(pkg, b"\x09" + rle_ref.encode([("rle", 5, 1)], 9), 0, 1, dictionary, 2, ref.WIDTH_BYTE)[3:5] == (ref.OK, 9)   # (9 bits into bytes: legal here)
    assert one(pkg, b"\x21" + body, 0, 8, dictionary * 4, 1, ref.WIDTH_BYTE) == (0, 0, 0, ref.BAD_WIDTH, 33, 0, ref.NONE)
    assert one(pkg, b"", 3, 4, dictionary * 2, 1, ref.WIDTH_BYTE) == (0, 0, 0, ref.BAD_WIDTH, 0, 0, ref.NONE)
    assert one(pkg, b"", 3, 4, dictionary * 2, 1) == (0, 0, 0, ref.OK, 3, 0, ref.NONE)


def test_three_thousand_segments(pkg):
    src, dictionary, segs, size = ref.short_table()
    assert len(segs) == 3000 and sum(1 for s in segs if s[1] == 0) > 100
    res = check(pkg, src, dictionary, segs, size, src_skew=5, dst_skew=11, dict_skew=3, order_seed=4)
    assert {r[3] for r in res} == {ref.OK, ref.BAD_HEADER, ref.ZERO_RUN, ref.TRUNCATED, ref.BAD_WIDTH}
    assert sum(1 for r in res if r[5]) > 300 and sum(1 for r in res if r[0] and not r[5]) > 300


def test_bad_arguments(pkg):
    dictionary = bytes(64)
    good = (0, 2, 0, 8, 3, 4, 0, 0, 8)
    for bad_w in (3, 0, 16):
        with pytest.raises(RuntimeError, match="undict segment 1: width is not 1, 2, 4 or 8"):
            pkg.undict_host(b"\x10\x05", dictionary, [good, good[:5] + (bad_w,) + good[6:]], 64)
    with pytest.raises(RuntimeError, match="undict segment 0: unknown flag bits"):
        pkg.undict_host(b"\x10\x05", dictionary, [good[:6] + (2,) + good[7:]], 64)
    with pytest.raises(RuntimeError, match=r"undict segment 0: field of more than 32 bits \(bits 33, width 8"):
        pkg.undict_host(b"\x10\x05", dictionary, [(0, 2, 0, 8, 33, 8, 0, 0, 8)], 64)
    pkg.undict_host(b"\x10\x05\x00", dictionary, [(0, 3, 0, 8, 12, 1, 0, 0, 8)], 64)   # 12-bit fields into a uint8 dictionary: legal
    with pytest.raises(RuntimeError, match=r"undict segment 0: a capacity above 2\^56"):
        pkg.undict_host(b"\x10\x05", dictionary, [(0, 2, 0, (1 << 56) + 1, 3, 4, 0, 0, 8)], 64)
    with pytest.raises(RuntimeError, match=r"undict segment 2: a dictionary of more than 2\^56 entries \(.*dictionary entries 72057594037927937\)"):
        pkg.undict_host(b"\x10\x05", dictionary, [good, good, good[:8] + ((1 << 56) + 1,)], 64)
    with pytest.raises(RuntimeError, match="a dictionary outside its buffer"):
        pkg.undict_host(b"\x10\x05", dictionary, [good[:7] + (40, 8)], 64)   # 8 entries of 4 bytes from 40 on
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.undict_host(b"\x10\x05", dictionary, [(1, 2) + good[2:]], 64)
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        pkg.undict_host(b"\x10\x05", dictionary, [(0, 2, 40) + good[3:]], 64)   # 8 elements of 4 bytes from 40 on
    for kw in ({"src_skew": 16}, {"dst_skew": 16}, {"dict_skew": 16}):
        with pytest.raises(RuntimeError, match="invalid undict arguments"):
            pkg.undict_host(b"\x10\x05", dictionary, [good], 64, **kw)
    assert pkg.undict_host(b"", b"", [], 8, fill=1) == (b"\x01" * 8, [])
    # a dictionary of no entries needs no bytes
    assert pkg.undict_host(b"\x10\x05", b"", [(0, 2, 0, 8, 3, 2, 0, 0, 0)], 16) == (bytes(16), [(8, 2, 1, ref.OK, 3, 8, 0)])


def test_sanitizer_program(tmp_path):
    r = san_program.run("undict_san", tmp_path)
    assert re.search(r"^\d+ segments$", r.stdout.strip())
