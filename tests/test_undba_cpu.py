"""Undba without a device: undbp's walk and items and the functions of csrc/brotli_undba.h, through their host hook (BrotliAmdDebugUndbaHost runs
every segment's two walks and then the items, of a given size and in given orders, over a source, an offsets and a data buffer placed at given
skews) against the reference (dba_ref.py), the new names of batch.h, and the argument failures that need no device.  Every comparison is exact
and over the WHOLE offsets and data buffers, which start as sentinel patterns: a byte written outside a segment's offsets or bytes fails the test
(and the hook itself, which returns -2)."""
import ctypes
import os
import random
import re

import pytest

import dba_ref as ref
import dbp_ref
import san_program
from conftest import ROOT

NEW_SYMBOLS = ["BrotliAmdBatchUndbaSegments", "BrotliAmdBatchUndbaOutputs", "BrotliAmdBatchLastUndbaMs", "BrotliAmdBatchLastUndbaPhaseMs", "BrotliAmdDebugUndbaHost"]
R = ref


def check(pkg, src, segs, offsets_size, data_size, **kw):
    """-> the results; both whole buffers and every result are compared with the reference"""
    want_o, want_d, want_res = ref.expected(src, segs, offsets_size, data_size)
    got_o, got_d, res = pkg.undba_host(src, segs, offsets_size, data_size, offsets_fill=ref.sentinel(offsets_size), data_fill=ref.sentinel(data_size, 7), **kw)
    assert res == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(res, want_res)) if a != b][:3]
    assert got_o == want_o, ("offsets", ref.first_difference(got_o, want_o))
    assert got_d == want_d, ("data", ref.first_difference(got_d, want_d))
    return res


def one(pkg, body, flags=0, cap=None, data_cap=None, base=0, **kw):
    """one segment with room for what it delivers -> its result"""
    src, segs, o_size, d_size = ref.layout(random.Random(1), [body], flags, None if cap is None else [cap], None if data_cap is None else [data_cap], base)
    return check(pkg, src, segs, o_size, d_size, **kw)[0]


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("undba_segments", "undba_outputs", "count_dba_outputs", "measure_dba_outputs", "last_undba_ms"):
        assert callable(getattr(pkg.Batch, name))
    assert callable(pkg.undba_host)
    assert ctypes.sizeof(pkg.UndbaResult) == 128 and len(pkg.UndbaResult._fields_) == 20
    assert (pkg.UNDBA_OFFSETS64, pkg.UNDBA_ENDS_ONLY, pkg.UNDBA_SKIP) == (ref.OFFSETS64, ref.ENDS_ONLY, ref.SKIP)
    assert (pkg.UNDBA_DATA_OK, pkg.UNDBA_DATA_SHORT, pkg.UNDBA_DATA_BAD, pkg.UNDBA_DATA_COUNTS_DIFFER) == (0, 1, 2, 4) and pkg.UNDBA_NONE == ref.NONE
    for text in ("BROTLI_AMD_UNDBA_OFFSETS64 2u", "BROTLI_AMD_UNDBA_ENDS_ONLY 4u", "BROTLI_AMD_UNDBA_SKIP 8u", "BROTLI_AMD_UNDBA_DATA_SHORT 1u", "BROTLI_AMD_UNDBA_DATA_BAD 2u",
                 "BROTLI_AMD_UNDBA_DATA_COUNTS_DIFFER 4u", "BROTLI_AMD_UNDBA_BAD_PREFIX_LONG 3u", "typedef struct BrotliAmdUndbaResult",
                 "BROTLI_AMD_UNDBA_LDS_STRING %du" % pkg.UNDBA_LDS_STRING, "BROTLI_AMD_UNDBA_LDS_CARRY %du" % pkg.UNDBA_LDS_CARRY):
        assert text in header, text
    assert "DELTA_BYTE_ARRAY's prefix copies" not in header   # (out of scope no longer)


def test_pinned_examples(pkg):
    """batch.h's examples, against values written down by hand, in the reference and through the hook"""
    for body, offsets, data, res in ref.PINNED:
        assert ref.column(body) == (offsets, data, res), body.hex()
        assert dbp_ref.decode(body)[1] == res[:7] and dbp_ref.decode(body[res[1]:])[1] == res[8:15], body.hex()
        m = min(res[0], res[8])
        got_o, got_d, results = pkg.undba_host(body, [(0, len(body), 0, 0, 1 << 40, max(m, 1), 0, 0)], 4 * (m + 1), len(data), data_fill=0x77)
        assert got_o == ref.offsets_bytes(offsets, 0) and got_d == data and results == [res], body.hex()
    # the last: offset_base alone, at both widths; nothing with ENDS_ONLY
    empty = ref.PINNED[-1][0]
    assert pkg.undba_host(empty, [(0, 10, 0, ref.NONE, 0, 7, 1234, ref.OFFSETS64)], 8, 0)[0] == (1234).to_bytes(8, "little")
    assert pkg.undba_host(empty, [(0, 10, 0, ref.NONE, 0, 7, 1234, ref.ENDS_ONLY)], 8, 0, offsets_fill=0x11)[0] == b"\x11" * 8
    # all in one call
    src, segs, o_size, d_size = ref.layout(random.Random(2), [p[0] for p in ref.PINNED], caps=[5] * len(ref.PINNED))
    assert check(pkg, src, segs, o_size, d_size) == [p[3] for p in ref.PINNED]


def test_the_encoder_and_the_reference():
    rnd = random.Random(3)
    strings = ref.sorted_strings(rnd, 300, b"stem/")
    offsets, data, res = ref.column(ref.encode(strings))
    assert data == b"".join(strings) and offsets[-1] == len(data) and res[R.R_STATUS] == ref.DATA_OK and res[R.R_SUFFIX] == res[R.R_AVAIL] < len(data)
    shorter = [0] + [rnd.randrange(0, ref.common_prefix(strings[x - 1], strings[x]) + 1) for x in range(1, 300)]
    assert ref.column(ref.encode(strings, shorter))[:2] == (offsets, data)
    assert ref.column(ref.encode([]))[2] == ref.PINNED[-1][3]


@pytest.mark.parametrize("flags", [0, ref.OFFSETS64, ref.ENDS_ONLY, ref.OFFSETS64 | ref.ENDS_ONLY])
def test_skews(pkg, flags):
    """every skew 0..15 of source, offsets and data, each varied with the other two fixed, and 16 mixed triples, at item_deltas 32 and 64"""
    rnd = random.Random(31 + flags)
    bodies = [ref.encode(ref.sorted_strings(rnd, n, b"k/")) for n in (70, 1, 133)]
    src, segs, o_size, d_size = ref.layout(rnd, bodies, flags, base=7)
    triples = [(s, 3, 5) for s in range(16)] + [(2, s, 9) for s in range(16)] + [(11, 6, s) for s in range(16)] + [(rnd.randrange(16), rnd.randrange(16), rnd.randrange(16)) for _ in range(16)]
    for x, (a, b, c) in enumerate(triples):
        check(pkg, src, segs, o_size, d_size, src_skew=a, offsets_skew=b, data_skew=c, item_deltas=32 + 32 * (x & 1), order_seed=a + 16 * b + c)


@pytest.mark.parametrize("item", [32, 64, 0])
def test_item_edges_and_orders(pkg, item):
    rnd = random.Random(41 + item)
    C = item or pkg.undbp_item_deltas()
    counts = (0, 1, 2, C, C + 1, C + 2, 2 * C + 1)
    bodies = [ref.encode(ref.sorted_strings(rnd, n, b"shared/")) for n in counts]
    for flags in (0, ref.OFFSETS64 | ref.ENDS_ONLY):
        src, segs, o_size, d_size = ref.layout(rnd, bodies, flags)
        first = check(pkg, src, segs, o_size, d_size, item_deltas=item)
        for seed in (1, 7):
            assert check(pkg, src, segs, o_size, d_size, item_deltas=item, order_seed=seed, offsets_skew=seed, data_skew=3) == first
        assert [r[0] for r in first] == list(counts)


@pytest.mark.parametrize("item", [32, 64])
def test_first_bad_by_each_rule_and_capacities_around_it(pkg, item):
    rnd = random.Random(47 + item)
    n = 5 * item + 9
    strings = ref.sorted_strings(rnd, n, b"p/")
    good_p = [0] + [ref.common_prefix(strings[x - 1], strings[x]) for x in range(1, n)]
    good_s = [len(v) - p for v, p in zip(strings, good_p)]
    for rule in (ref.BAD_PREFIX_NEGATIVE, ref.BAD_SUFFIX_NEGATIVE, ref.BAD_PREFIX_LONG):
        for at in (0, 1, item, item + 1, 2 * item + 5, n - 1):
            p, s = list(good_p), list(good_s)
            for e in (at, min(at + 40, n - 1)):
                if rule == ref.BAD_PREFIX_NEGATIVE:
                    p[e] = -1 - rnd.randrange(1 << 20)
                elif rule == ref.BAD_SUFFIX_NEGATIVE:
                    s[e] = (1 << 31) + rnd.randrange(1 << 20) + (7 << 32)
                else:
                    p[e] = (len(strings[e - 1]) if e else 0) + 1 + (3 << 32)
            body = ref.encode(strings, p, s)
            for cap in (None, at + 1) + ((at,) if at else ()):
                res = one(pkg, body, cap=cap, item_deltas=item, order_seed=at + 1)
                bad = cap is None or cap > at
                assert (res[R.R_FIRST_BAD], res[R.R_KIND]) == ((at, rule) if bad else (ref.NONE, 0)) and res[R.R_BYTES] == sum(len(v) for v in strings[:at])


def test_long_strings_beyond_both_running_strings(pkg):
    """prefixes longer than the 4096 bytes that phase A keeps -- the walk back through the item -- and than the 32768 that phase B keeps --
    the far bytes from the items in front, through three items that share them --, with a data capacity that cuts a far copy"""
    rnd = random.Random(53)
    stem5, stem40 = rnd.randbytes(5000), rnd.randbytes(40000)
    strings = ref.sorted_strings(rnd, 20, b"a/") + [stem5 + rnd.randbytes(40) for _ in range(6)] + [stem5[:4500]] + [stem5 + b"x", stem5 + b"x", stem5 + b"xy"]
    strings += ref.sorted_strings(rnd, 3, b"b/") + [stem40 + rnd.randbytes(20) for _ in range(100)]   # (items of 32: three of them share 40000 bytes)
    body = ref.encode(strings)
    total = sum(len(v) for v in strings)
    for seed in (0, 3):
        assert one(pkg, body, item_deltas=32, order_seed=seed)[R.R_BYTES] == total
    one(pkg, body, item_deltas=32, data_cap=total - 100000)
    shorter = [0] + [rnd.randrange(0, ref.common_prefix(strings[x - 1], strings[x]) + 1) for x in range(1, len(strings))]
    assert one(pkg, ref.encode(strings, shorter), item_deltas=64)[R.R_BYTES] == total


def test_declared_lengths_of_two_gib_over_ten_bytes_of_source(pkg):
    """elements that declare 2^31 - 1 bytes and more, through three items: the work follows min(bytes, data_cap), and the results and the cut
    output are what they are for any page"""
    body, n = ref.huge_page(70)
    big = (1 << 31) - 1
    want = None
    for data_cap in (0, 1, 10, 64, 100000):
        for item, seed in ((32, 0), (64, 3)):
            res = one(pkg, body, flags=ref.OFFSETS64, cap=n, data_cap=data_cap, item_deltas=item, order_seed=seed)
            assert want in (None, res)
            want = res
    assert want[R.R_STATUS] == ref.DATA_SHORT and want[R.R_FIRST_BAD] == ref.NONE and want[R.R_AVAIL] == 10 and want[R.R_SUFFIX] == 3 * big + 5
    assert want[R.R_BYTES] == big + 2 * big + (big + 3) + (5 + big) + 70 * big + 9
    assert ref.column(body, n, 0, 40)[1] == b"0123456789" + bytes(30)
    # 4-byte offsets wrap, as they do for any column of more than 4 GiB
    one(pkg, body, cap=n, data_cap=17, item_deltas=32)


def test_repeats_empty_strings_and_item_starts(pkg):
    rnd = random.Random(59)
    strings = ref.sorted_strings(rnd, 33, b"aa/") + [b"zz-repeat"] * 64 + [b""] + ref.sorted_strings(rnd, 30, b"zz/") + [b"", b"", b"x"]
    body = ref.encode(strings)
    for item in (32, 64):
        assert one(pkg, body, item_deltas=item, order_seed=item)[R.R_BYTES] == sum(len(v) for v in strings)


def test_data_capacity_short_data_and_left_over(pkg):
    rnd = random.Random(61)
    strings = ref.sorted_strings(rnd, 80, b"k/")
    body = ref.encode(strings)
    whole = one(pkg, body, item_deltas=32)
    total, suffixes = whole[R.R_BYTES], whole[R.R_SUFFIX]
    for skew in (0, 9):
        for data_cap in [0, 1, 15, 16, 17] + list(range(28, 52)) + [total - 1, total, total + 1, 1 << 60]:
            assert one(pkg, body, data_cap=data_cap, item_deltas=32, data_skew=skew) == whole
    for cut in (1, suffixes):
        res = one(pkg, body[:len(body) - cut], item_deltas=32, flags=ref.OFFSETS64)
        assert res[R.R_STATUS] == ref.DATA_SHORT and (res[R.R_BYTES], res[R.R_SUFFIX], res[R.R_AVAIL]) == (total, suffixes, suffixes - cut)
    res = one(pkg, body + b"left over", item_deltas=32)
    assert res[R.R_STATUS] == ref.DATA_OK and res[R.R_AVAIL] == suffixes + 9


def test_streams_of_other_blocks_and_counts_and_stops(pkg):
    rnd = random.Random(67)
    strings = ref.sorted_strings(rnd, 700, b"k/")
    res = one(pkg, ref.encode(strings, p_knobs=dict(B=256, M=8), s_knobs=dict(B=1024, M=8)), item_deltas=64, order_seed=2)
    assert (res[5], res[6], res[13], res[14]) == (256, 8, 1024, 8)
    p = [0] + [ref.common_prefix(strings[x - 1], strings[x]) for x in range(1, 700)]
    s = [len(v) - q for v, q in zip(strings, p)]
    tail = b"".join(v[q:] for v, q in zip(strings, p))
    for np_, ns in ((700, 650), (600, 700)):
        res = one(pkg, dbp_ref.encode(p[:np_]) + dbp_ref.encode(s[:ns]) + tail, item_deltas=32)
        assert (res[0], res[8], res[R.R_STATUS]) == (np_, ns, ref.DATA_COUNTS_DIFFER)
    # every undbp stop in P and in S: S is read from P's consumed whatever the status is
    front_p, front_s = dbp_ref.encode(p[:129], declared=329), dbp_ref.encode(s[:129], declared=329)
    for name, stop, status, more, _ in dbp_ref.stops():
        a = one(pkg, front_p + stop + dbp_ref.encode(s[:129]) + tail, item_deltas=32)
        b = one(pkg, dbp_ref.encode(p[:129]) + front_s + stop + tail, item_deltas=32)
        assert a[:7] == dbp_ref.decode(front_p + stop + dbp_ref.encode(s[:129]) + tail)[1] and b[12] == dbp_ref.decode(front_s + stop + tail)[1][4], name


def test_counting_and_measuring_write_nothing(pkg):
    rnd = random.Random(71)
    bodies = [ref.encode(ref.sorted_strings(rnd, n, b"k/")) for n in (0, 1, 40, 100)]
    src, segs, o_size, d_size = ref.layout(rnd, bodies)
    full = check(pkg, src, segs, o_size, d_size, item_deltas=32)
    counting = [(s, l, o, d, 0, 0, base, flags) for s, l, o, d, _, _, base, flags in segs]
    got = check(pkg, src, counting, o_size, d_size, item_deltas=32)
    assert [r[:15] + (0, ref.NONE, 0, 0, r[19]) for r in full] == got
    measuring = [(s, l, ref.NONE, ref.NONE, 0, cap, base, flags) for s, l, _, _, _, cap, base, flags in segs]
    assert check(pkg, src, measuring, o_size, d_size, item_deltas=32) == full
    check(pkg, src, [(s, l, o, ref.NONE, 0, cap, base, flags) for s, l, o, _, _, cap, base, flags in segs], o_size, d_size, item_deltas=32)
    check(pkg, src, [(s, l, ref.NONE, d, dc, cap, base, flags) for s, l, _, d, dc, cap, base, flags in segs], o_size, d_size, item_deltas=32)


def test_table_of_3000_segments(pkg):
    src, segs, o_size, d_size = ref.short_table(3000)
    first = check(pkg, src, segs, o_size, d_size, item_deltas=32)
    assert check(pkg, src, segs, o_size, d_size, item_deltas=64, order_seed=9, src_skew=5, offsets_skew=10, data_skew=15) == first
    every = {ref.OK, ref.BAD_HEADER, ref.BAD_WIDTH, ref.TRUNCATED}
    assert {r[4] for r in first} == every and {r[12] for r in first} == every
    assert all(any(r[R.R_STATUS] & bit for r in first) for bit in (1, 2, 4)) and {r[R.R_KIND] for r in first} == {0, 1, 2, 3}


def test_refusals(pkg):
    """every host refusal, with its text; nothing is written"""
    body = ref.PINNED[1][0]

    def refused(seg, text, **kw):
        with pytest.raises(RuntimeError) as e:
            pkg.undba_host(body, [seg], 64, 64, **kw)
        assert text in str(e.value), str(e.value)

    refused((0, len(body), 0, 0, 64, 4, 0, 1), "undba segment 0: unknown flag bits")
    refused((0, len(body), 0, 0, 64, 4, 0, 16), "undba segment 0: unknown flag bits")
    refused((0, len(body), 0, 0, 64, 4, 0, ref.SKIP), "undba segment 0: BROTLI_AMD_UNDBA_SKIP is for the outputs of a decode call")
    refused((0, len(body), 0, 0, 64, (1 << 56) + 1, 0, 0), "undba segment 0: a capacity above 2^56 elements")
    refused((0, len(body), 0, ref.NONE, 64, 4, 0, 0), "undba segment 0: no data destination for a data capacity that is not 0")
    refused((0, len(body) + 1, 0, 0, 64, 4, 0, 0), "a segment outside its buffer")
    refused((0, len(body), 60, 0, 64, 4, 0, 0), "a segment outside its buffer")      # (no room for three offsets)
    refused((0, len(body), 0, 60, 64, 4, 0, 0), "a segment outside its buffer")      # (no room for six bytes)
    refused((0, len(body), 0, 0, 64, 4, 0, 0), "invalid undba arguments", src_skew=16)
    refused((0, len(body), 0, 0, 64, 4, 0, 0), "an item that is no multiple of 32 deltas", item_deltas=48)
    lib = pkg.load_library()
    assert lib.BrotliAmdBatchUndbaSegments(None, 0, None, None, None, None, None, None, None, None, None, None) != 0
    assert "invalid undba arguments" in pkg.last_error()
    assert lib.BrotliAmdBatchUndbaOutputs(None, None, None, None, None, None, None, None) != 0
    assert lib.BrotliAmdBatchLastUndbaMs(None) == 0.0 and lib.BrotliAmdBatchLastUndbaPhaseMs(None, 1) == 0.0


def test_host_phases_under_sanitizers(tmp_path):
    """the header's host phases over a seeded table under AddressSanitizer and UBSan, in a program of its own"""
    r = san_program.run("undba_san", tmp_path)
    assert "undba_san: ok" in r.stdout
