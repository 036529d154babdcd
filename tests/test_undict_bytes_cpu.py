"""Undict for byte arrays without a device: the functions of csrc/brotli_undict_bytes.h on unrle's walk, through their host hook
(BrotliAmdDebugUndictBytesHost runs every distinct dictionary's walk, every segment's walk and then the items, of a given size and in given
orders, over a source, an offsets, a data and a dictionary buffer placed at given skews) against the reference (dict_bytes_ref.py), the new names
of batch.h, and the argument failures that need no device.  Every comparison is exact and over the WHOLE offsets and data buffers, which start as
sentinel patterns: a byte written outside a segment's offsets or bytes fails the test (and the hook itself, which returns -2)."""
import ctypes
import os
import random
import re

import pytest

import dict_bytes_ref as ref
import rle_ref
import san_program
from conftest import ROOT

NEW_SYMBOLS = ["BrotliAmdBatchUndictBytesSegments", "BrotliAmdBatchUndictBytesOutputs", "BrotliAmdBatchLastUndictBytesMs", "BrotliAmdBatchLastUndictBytesPhaseMs",
               "BrotliAmdDebugUndictBytesHost"]


def check(pkg, src, dictionary, segs, offsets_size, data_size, **kw):
    """-> (the results, the dictionaries walked); both whole buffers and every result are compared with the reference"""
    want_o, want_d, want_res = ref.expected(src, dictionary, segs, offsets_size, data_size)
    got_o, got_d, res, walks = pkg.undict_bytes_host(src, dictionary, segs, offsets_size, data_size, offsets_fill=ref.sentinel(offsets_size),
                                                     data_fill=ref.sentinel(data_size, 7), **kw)
    assert res == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(res, want_res)) if a != b][:3]
    assert got_o == want_o, ("offsets", ref.first_difference(got_o, want_o))
    assert got_d == want_d, ("data", ref.first_difference(got_d, want_d))
    return res, walks


def one(pkg, data, k, entries, flags=0, cap=None, data_cap=None, bound=ref.ALL, base=0, dictionary=None, **kw):
    """one segment with room for what it delivers -> its result"""
    dictionary = ref.dictionary_bytes(entries) if dictionary is None else dictionary
    blob = b"\x11" + dictionary + b"\x22"
    src, segs, o_size, d_size = ref.layout(random.Random(1), [data], 1, len(dictionary), k, flags, None if cap is None else [cap], None if data_cap is None else [data_cap],
                                           bound, base, dictionary=blob)
    return check(pkg, src, blob, segs, o_size, d_size, **kw)[0][0]


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("undict_bytes_segments", "undict_bytes_outputs", "measure_dict_bytes_outputs", "last_undict_bytes_ms"):
        assert callable(getattr(pkg.Batch, name))
    assert callable(pkg.undict_bytes_host)
    assert ctypes.sizeof(pkg.UndictBytesResult) == 80
    assert [f[0] for f in pkg.UndictBytesResult._fields_] == ["count", "consumed", "runs", "status", "bits", "bad", "first_bad", "bytes", "dict_entries", "dict_consumed",
                                                              "dict_status", "reserved"]
    assert (pkg.UNDICT_BYTES_WIDTH_BYTE, pkg.UNDICT_BYTES_OFFSETS64, pkg.UNDICT_BYTES_ENDS_ONLY, pkg.UNDICT_BYTES_SKIP) == (ref.WIDTH_BYTE, ref.OFFSETS64, ref.ENDS_ONLY, ref.SKIP)
    assert pkg.UNDICT_BYTES_ALL == ref.ALL and (pkg.UNDICT_BYTES_DICT_OK, pkg.UNDICT_BYTES_DICT_CUT) == (ref.DICT_OK, ref.DICT_CUT) == (0, 1)
    for text in ("BROTLI_AMD_UNDICT_BYTES_WIDTH_BYTE 1u", "BROTLI_AMD_UNDICT_BYTES_OFFSETS64 2u", "BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY 4u", "BROTLI_AMD_UNDICT_BYTES_DICT_CUT 1u",
                 "typedef struct BrotliAmdUndictBytesResult"):
        assert text in header, text
    assert "OUT OF SCOPE: BYTE_ARRAY" not in header   # (undict's out of scope now points here)


def test_pinned_vectors(pkg):
    for k, flags, data, dictionary, bound, (elements, bad, first_bad, nbytes, D, dict_status) in ref.PINNED:
        offsets, body, res = ref.column(data, k, flags, dictionary, bound)
        assert body == b"".join(elements) and offsets == [sum(len(e) for e in elements[:i]) for i in range(len(elements) + 1)], data.hex()
        assert res[0] == len(elements) and res[5:9] == (bad, first_bad, nbytes, D) and res[10] == dict_status, data.hex()
        m = len(elements)
        got_o, got_d, results, walks = pkg.undict_bytes_host(data, dictionary, [(0, len(data), 0, 0, 1 << 40, m, 0, 0, len(dictionary), bound, k, flags)], 4 * (m + 1), nbytes)
        assert got_o == ref.offsets_bytes(offsets, 0) and got_d == body and results == [res] and walks == 1, data.hex()


def test_entry_lengths(pkg):
    """entries of 0, 1, 3, 15, 16, 17, 31, 33 and 4096 bytes, each alone and mixed, under packed and repeated runs"""
    rnd = random.Random(51)
    for lengths in ([0], [1], [3], [15], [16], [17], [31], [33], [4096], [0, 1, 3, 15, 16, 17, 31, 33, 4096]):
        entries = ref.random_entries(rnd, 16, lengths)
        plan = [("packed", [rnd.randrange(16) for _ in range(24)]), ("rle", 5, rnd.randrange(16)), ("packed", [rnd.randrange(16) for _ in range(8)]), ("rle", 2, 15)]
        data = rle_ref.encode(plan, 4)
        for seed in (0, 3):
            res = one(pkg, data, 4, entries, item_elems=8, order_seed=seed, word_seed=seed, data_skew=seed)
            assert res[:7] == (39, len(data), 4, ref.OK, 4, 0, ref.NONE) and res[8:] == (16, len(ref.dictionary_bytes(entries)), ref.DICT_OK)


def test_all_skews(pkg):
    """every pair of skews of the source, the data and the dictionary, and every skew of the offsets at both widths, at one small shape"""
    rnd = random.Random(52)
    entries = ref.random_entries(rnd, 32, [0, 1, 2, 5, 16, 17, 23])
    dictionary = b"\x11" + ref.dictionary_bytes(entries)
    datas = [rle_ref.encode(rle_ref.random_plan(rnd, 5, n, packed=(8, 16), repeated=(1, 9)), 5) for n in (1, 9, 40)]
    tables = {f: ref.layout(rnd, datas, 1, len(dictionary) - 1, 5, f, dictionary=dictionary) for f in (0, ref.OFFSETS64)}
    for a in range(16):
        for b in range(16):
            src, segs, o_size, d_size = tables[ref.OFFSETS64 if (a + b) & 1 else 0]
            for kw in ({"src_skew": a, "data_skew": b}, {"src_skew": a, "dict_skew": b}, {"data_skew": a, "dict_skew": b}):
                check(pkg, src, dictionary, segs, o_size, d_size, offsets_skew=(a * 5 + b) % 16, item_elems=8 * (1 + a % 3), order_seed=a, word_seed=b, **kw)
    for flags in (0, ref.OFFSETS64, ref.ENDS_ONLY, ref.OFFSETS64 | ref.ENDS_ONLY):
        src, segs, o_size, d_size = ref.layout(rnd, datas, 1, len(dictionary) - 1, 5, flags, dictionary=dictionary)
        for skew in range(16):
            check(pkg, src, dictionary, segs, o_size, d_size, offsets_skew=skew, item_elems=8, word_seed=skew)


def test_ends_only_and_offset_base(pkg):
    """ENDS_ONLY: m entries from offsets[1] on; a base that is not 0, one that wraps a 4-byte offset, and one that does not wrap 8 bytes"""
    rnd = random.Random(53)
    entries = ref.random_entries(rnd, 8, [0, 3, 9])
    data = rle_ref.encode([("packed", [rnd.randrange(8) for _ in range(40)]), ("rle", 9, 2)], 3)
    for flags in (0, ref.ENDS_ONLY, ref.OFFSETS64, ref.OFFSETS64 | ref.ENDS_ONLY):
        for base in (0, 12345, (1 << 32) - 7, (1 << 63) + 5):
            res = one(pkg, data, 3, entries, flags, base=base, item_elems=24, word_seed=1)
            assert res[0] == 49 and res[7] == sum(len(entries[int(v)]) for v in rle_ref.decode(data, 3, 8)[0])
    # two pages appended into one offsets array and one data buffer: the second with ENDS_ONLY and the first's bytes as its base
    d2 = rle_ref.encode([("rle", 11, 5), ("packed", [rnd.randrange(8) for _ in range(8)])], 3)
    dictionary = ref.dictionary_bytes(entries)
    o1, b1, r1 = ref.column(data, 3, 0, dictionary)
    o2, b2, r2 = ref.column(d2, 3, 0, dictionary, offset_base=len(b1))
    segs = [(0, len(data), 0, 0, 1 << 40, 49, 0, 0, len(dictionary), ref.ALL, 3, 0), (len(data), len(d2), 4 * 50, len(b1), 1 << 40, 19, len(b1), 0, len(dictionary), ref.ALL, 3, ref.ENDS_ONLY)]
    got_o, got_d, res, walks = pkg.undict_bytes_host(data + d2, dictionary, segs, 4 * 69, len(b1) + len(b2), item_elems=8, order_seed=2)
    assert got_o == ref.offsets_bytes(o1 + o2[1:], 0) and got_d == b1 + b2 and res == [r1, r2] and walks == 1


def test_dictionary_sizes(pkg):
    """D of 0, 1, 2^k - 1, 2^k and 2^k + 1 under indices that cover all of 2^k"""
    rnd = random.Random(54)
    k = 4
    values = list(range(16)) + [rnd.randrange(16) for _ in range(16)]
    data = rle_ref.encode([("rle", 3, 0), ("packed", values), ("rle", 2, 15)], k)
    flat = [0] * 3 + values + [15] * 2
    for D in (0, 1, 15, 16, 17):
        bad = sum(1 for v in flat if v >= D)
        first = next((e for e, v in enumerate(flat) if v >= D), ref.NONE)
        assert (bad, first) == {0: (37, 0), 1: (bad, 4), 15: (bad, 18), 16: (0, ref.NONE), 17: (0, ref.NONE)}[D]
        entries = ref.random_entries(rnd, D, [0, 1, 4, 18])
        for seed in (0, 5):
            res = one(pkg, data, k, entries, item_elems=8, order_seed=seed, word_seed=seed)
            assert res[5:7] == (bad, first) and res[8] == D, (D, res)
    # no dictionary at all: no bytes, a pointer that is not looked at
    assert one(pkg, data, k, [], dictionary=b"")[5:9] == (37, 0, 0, 0)


def test_unmasked_rle_value(pkg):
    """an RLE run's value is not masked to k bits: 0xFFFFFFFF under k = 32, and 0xFF under k = 3, against a small dictionary are out of range,
    are never made an address, and give empty elements"""
    entries = [b"zero", b"one", b"two!!"]
    data = rle_ref.encode([("rle", 4, 2), ("rle", 6, 0xFFFFFFFF), ("rle", 1, 1)], 32)
    assert one(pkg, data, 32, entries)[:8] == (11, len(data), 3, ref.OK, 32, 6, 4, 4 * 5 + 3)
    data = rle_ref.encode([("rle", 2, 0xFF), ("rle", 3, 1)], 3)
    assert one(pkg, data, 3, entries)[:8] == (5, len(data), 2, ref.OK, 3, 2, 0, 9)


@pytest.mark.parametrize("item", [8, 24, 1024])
def test_bad_indices_across_items_in_any_order(pkg, item):
    """bad indices in three different items, the items and an item's words taken in shuffled orders: bad, first_bad and bytes do not depend on
    the orders.  The runs span three items."""
    rnd = random.Random(55)
    k, D = 9, 300
    n = 5 * item + 3
    values = [rnd.randint(0, D - 1) for _ in range((n + 7) // 8 * 8)]
    where = [item + 1, item + 2, 2 * item + item // 2, 4 * item + 3]
    for at in where:
        values[at] = D + rnd.randint(0, 200)
    lead = 3
    data = rle_ref.encode([("rle", lead, 5), ("packed", values), ("rle", 2 * item + 5, 7)], k)
    entries = ref.random_entries(rnd, D, [0, 1, 2, 3, 9])
    seen = {one(pkg, data, k, entries, item_elems=item, order_seed=seed, word_seed=(seed * 3) % 5, dict_skew=seed % 16) for seed in (0, 1, 2, 3, 17)}
    assert len(seen) == 1 and next(iter(seen))[:7] == (lead + len(values) + 2 * item + 5, len(data), 3, ref.OK, k, len(where), lead + where[0])


@pytest.mark.parametrize("item", [64, 0])
def test_more_than_64_runs_in_one_item(pkg, item):
    rnd = random.Random(56)
    k = 6
    plan = rle_ref.many_runs_plan(k, 2500, 57)
    data = rle_ref.encode(plan, k)
    entries = ref.random_entries(rnd, 60, [0, 1, 2, 7])
    res = one(pkg, data, k, entries, item_elems=item, order_seed=7, word_seed=2)
    assert res[:4] == (2500, len(data), 2500, ref.OK) and res[5] > 0


def test_data_capacities_and_capacities(pkg):
    """data_cap at 0, inside the first element, exactly at an element's end, inside a 16-byte word, at bytes - 1, at bytes and above; cap below
    and above count.  bytes does not depend on data_cap."""
    rnd = random.Random(58)
    entries = ref.random_entries(rnd, 8, [5, 11, 16, 3])
    values = [rnd.randrange(8) for _ in range(48)]
    data = rle_ref.encode([("packed", values)], 3)
    ends = [0]
    for v in values:
        ends.append(ends[-1] + len(entries[v]))
    total = ends[-1]
    for data_cap in (0, 2, ends[1], ends[7], ends[7] + 5, 100, total - 1, total, total + 20):
        for skew in (0, 9):
            assert one(pkg, data, 3, entries, data_cap=data_cap, item_elems=8, word_seed=3, data_skew=skew)[7] == total
    for cap in (0, 1, 17, 47, 48, 49, 1 << 56):
        res = one(pkg, data, 3, entries, cap=cap, item_elems=8, order_seed=1)
        assert res[0] == 48 and res[7] == ends[min(cap, 48)], cap


def test_measuring_call(pkg):
    """no destinations: nothing is written, and the result is that of the call that writes"""
    rnd = random.Random(59)
    entries = ref.random_entries(rnd, 30, [0, 4, 21])
    data = rle_ref.encode(rle_ref.random_plan(rnd, 5, 200, packed=(8, 40), repeated=(1, 30)), 5)
    dictionary = ref.dictionary_bytes(entries)
    count = rle_ref.decode(data, 5, 8)[1][0]
    _, body, want = ref.column(data, 5, 0, dictionary)
    for o_at, d_at, data_cap in ((ref.NONE, ref.NONE, 0), (0, ref.NONE, 0), (ref.NONE, 0, 1 << 40)):
        (res,), walks = check(pkg, data, dictionary, [(0, len(data), o_at, d_at, data_cap, count, 0, 0, len(dictionary), ref.ALL, 5, 0)], 4 * (count + 1) + 8, len(body) + 8,
                              item_elems=24, order_seed=3)
        assert res == want and res[7] == len(body)


def test_empty_items_and_one_long_element(pkg):
    """an item whose elements are all empty between two that are not; an element longer than the rest of its item's bytes together"""
    rnd = random.Random(60)
    entries = [b"", rnd.randbytes(7), rnd.randbytes(3000), b"q"]
    plan = [("packed", [1] * 8), ("packed", [0] * 8), ("rle", 8, 0), ("packed", [3, 3, 3, 2, 3, 3, 3, 3]), ("rle", 8, 1)]
    data = rle_ref.encode(plan, 2)
    for seed in range(4):
        res = one(pkg, data, 2, entries, item_elems=8, order_seed=seed, word_seed=seed, data_skew=3 * seed)
        assert res[7] == 56 + 7 + 3000 + 56


def test_cut_dictionaries(pkg):
    """a dictionary cut at every byte of its last entry -- inside the length prefix and inside the bytes --; dict_entries below, at and above what
    the bytes hold, and ALL"""
    entries = [b"ab", b"", b"cdefg", b"hi"]
    whole = ref.dictionary_bytes(entries)
    data = rle_ref.encode([("packed", [0, 1, 2, 3, 3, 2, 1, 0])], 2)
    for cut in range(len(whole) + 1):
        parsed = ref.parse_dictionary(whole[:cut])
        res = one(pkg, data, 2, None, dictionary=whole[:cut], item_elems=8, dict_skew=cut % 16)
        assert res[8:] == (len(parsed[0]), parsed[1], parsed[2]), cut
    assert [ref.parse_dictionary(whole[:cut])[2] for cut in (0, 1, 4, 6, 7, 10, 14, 19, 20, 24, 25, 26)] == [0, 1, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0]
    for bound, D, consumed, bad in ((0, 0, 0, 8), (3, 3, 19, 2), (4, 4, 25, 0), (5, 4, 25, 0), (ref.ALL, 4, 25, 0)):
        res = one(pkg, data, 2, None, dictionary=whole + b"\xff", bound=bound) if bound <= 4 else one(pkg, data, 2, None, dictionary=whole, bound=bound)
        assert res[5] == bad and res[8:] == (D, consumed, ref.DICT_OK), bound
    # bytes left over behind dict_entries whole entries are no error; without the bound they are a cut
    assert one(pkg, data, 2, None, dictionary=whole + b"\xff", bound=ref.ALL)[8:] == (4, 25, ref.DICT_CUT)


def test_every_stop(pkg):
    rnd = random.Random(61)
    for k in (0, 3, 9, 17, 32):
        D = min(1 << k, 50)
        entries = ref.random_entries(rnd, D, [0, 2, 6])
        plan = [r[:2] + (r[2] % D,) if r[0] == "rle" else ("packed", [v % D for v in r[1]]) for r in rle_ref.random_plan(rnd, k, 60, packed=(8, 24), repeated=(1, 30))]
        for name, tail, status in rle_ref.stops(k):
            for front in (0, len(plan)):
                res = one(pkg, rle_ref.encode(plan[:front], k) + tail, k, entries, item_elems=8, order_seed=front + 1)
                assert res[3] == status and res[4] == k, (name, k, front)
    body = rle_ref.encode([("rle", 5, 1)], 1)
    assert one(pkg, b"\x01" + body, 0, [b"x", b"yz"], ref.WIDTH_BYTE)[:8] == (5, len(body) + 1, 1, ref.OK, 1, 0, ref.NONE, 10)
    assert one(pkg, b"\x21" + body, 0, [b"x"], ref.WIDTH_BYTE)[:8] == (0, 0, 0, ref.BAD_WIDTH, 33, 0, ref.NONE, 0)
    assert one(pkg, b"", 3, [b"x"])[:8] == (0, 0, 0, ref.OK, 3, 0, ref.NONE, 0)


def test_two_hundred_segments_share_one_dictionary(pkg):
    """the pages of a chunk: the dictionary is walked once, and every segment's dictionary fields are the same"""
    rnd = random.Random(62)
    entries = ref.random_entries(rnd, 64, [0, 1, 5, 12, 30])
    dictionary = b"\x11\x22" + ref.dictionary_bytes(entries)
    datas = [rle_ref.encode(rle_ref.random_plan(rnd, 6, rnd.randrange(1, 80), packed=(8, 24), repeated=(1, 30)), 6) for _ in range(200)]
    src, segs, o_size, d_size = ref.layout(rnd, datas, 2, len(dictionary) - 2, 6, dictionary=dictionary)
    res, walks = check(pkg, src, dictionary, segs, o_size, d_size, item_elems=24, order_seed=9, word_seed=4)
    assert walks == 1 and {r[8:] for r in res} == {(64, len(dictionary) - 2, ref.DICT_OK)}
    # another bound is another dictionary
    segs[7] = segs[7][:9] + (64,) + segs[7][10:]
    assert check(pkg, src, dictionary, segs, o_size, d_size, item_elems=24)[1] == 2


def test_three_thousand_segments(pkg):
    src, dictionary, segs, o_size, d_size = ref.short_table()
    assert len(segs) == 3000 and sum(1 for s in segs if s[1] == 0) > 100
    res, walks = check(pkg, src, dictionary, segs, o_size, d_size, src_skew=5, offsets_skew=11, data_skew=7, dict_skew=3, order_seed=4, word_seed=6)
    assert {r[3] for r in res} >= {ref.OK, ref.BAD_HEADER, ref.ZERO_RUN, ref.TRUNCATED} and {r[10] for r in res} == {ref.DICT_OK, ref.DICT_CUT}
    assert sum(1 for r in res if r[5]) > 300 and sum(1 for r in res if r[0] and not r[5]) > 300 and 40 < walks <= 160


def test_bad_arguments(pkg):
    dictionary = ref.dictionary_bytes(ref.EIGHT)
    good = (0, 2, 0, 0, 64, 8, 0, 0, len(dictionary), ref.ALL, 3, 0)
    run = lambda segs, **kw: pkg.undict_bytes_host(b"\x10\x05", dictionary, segs, 64, 64, **kw)
    for flags in (8, 16, 128):   # (SKIP is the outputs call's)
        with pytest.raises(RuntimeError, match=r"undict-bytes segment 1: unknown flag bits \(bits 3, flags %d, capacity 8, data capacity 64, dictionary bytes 60\)" % flags):
            run([good, good[:11] + (flags,)])
    with pytest.raises(RuntimeError, match="undict-bytes segment 0: field of more than 32 bits"):
        run([good[:10] + (33, 0)])
    run([good[:10] + (33, ref.WIDTH_BYTE)])   # (with the width byte the argument is not looked at)
    with pytest.raises(RuntimeError, match=r"undict-bytes segment 2: a capacity above 2\^56 elements"):
        run([good, good, good[:5] + ((1 << 56) + 1,) + good[6:]])
    with pytest.raises(RuntimeError, match="undict-bytes segment 0: no data destination for a data capacity that is not 0"):
        run([good[:3] + (ref.NONE, 5) + good[5:]])
    with pytest.raises(RuntimeError, match=r"undict-bytes segment 0: a dictionary of 2\^32 bytes or more"):
        run([good[:8] + (1 << 32,) + good[9:]])
    with pytest.raises(RuntimeError, match="a dictionary outside its buffer"):
        run([good[:7] + (1,) + good[8:]])
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        run([(1, 2) + good[2:]])
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        run([good[:2] + (40,) + good[3:]])   # nine offsets of 4 bytes from 40 on
    with pytest.raises(RuntimeError, match="a segment outside its buffer"):
        run([good[:3] + (30,) + good[4:]])   # 40 bytes from 30 on
    for kw in ({"src_skew": 16}, {"offsets_skew": 16}, {"data_skew": 16}, {"dict_skew": 16}):
        with pytest.raises(RuntimeError, match="invalid undict-bytes arguments"):
            run([good], **kw)
    assert pkg.undict_bytes_host(b"", b"", [], 8, 4, offsets_fill=1, data_fill=2) == (b"\x01" * 8, b"\x02" * 4, [], 0)
    # the device calls refuse in front of everything that touches the device: no batch object is needed for the NULL checks
    lib = pkg.load_library()
    assert lib.BrotliAmdBatchUndictBytesSegments(None, 0, None, None, None, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert "invalid undict-bytes arguments" in pkg.last_error()
    assert lib.BrotliAmdBatchLastUndictBytesMs(None) == 0.0 and lib.BrotliAmdBatchLastUndictBytesPhaseMs(None, 1) == 0.0


def test_sanitizer_program(tmp_path):
    r = san_program.run("undict_bytes_san", tmp_path)
    assert re.search(r"^\d+ segments$", r.stdout.strip())
