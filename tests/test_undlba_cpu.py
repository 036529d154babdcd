"""Undlba without a device: undbp's walk and items and the functions of csrc/brotli_undlba.h, through their host hook (BrotliAmdDebugUndlbaHost
runs every segment's walk and then the items, of a given size and in given orders, over a source, an offsets and a data buffer placed at given
skews) against the reference (dlba_ref.py), the new names of batch.h, and the argument failures that need no device.  Every comparison is exact
and over the WHOLE offsets and data buffers, which start as sentinel patterns: a byte written outside a segment's offsets or bytes fails the test
(and the hook itself, which returns -2)."""
import ctypes
import os
import random
import re

import pytest

import dbp_ref
import dlba_ref as ref
import san_program
from conftest import ROOT

NEW_SYMBOLS = ["BrotliAmdBatchUndlbaSegments", "BrotliAmdBatchUndlbaOutputs", "BrotliAmdBatchLastUndlbaMs", "BrotliAmdBatchLastUndlbaPhaseMs", "BrotliAmdDebugUndlbaHost"]


def check(pkg, src, segs, offsets_size, data_size, **kw):
    """-> the results; both whole buffers and every result are compared with the reference"""
    want_o, want_d, want_res = ref.expected(src, segs, offsets_size, data_size)
    got_o, got_d, res = pkg.undlba_host(src, segs, offsets_size, data_size, offsets_fill=ref.sentinel(offsets_size), data_fill=ref.sentinel(data_size, 7), **kw)
    assert res == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(res, want_res)) if a != b][:3]
    assert got_o == want_o, ("offsets", ref.first_difference(got_o, want_o))
    assert got_d == want_d, ("data", ref.first_difference(got_d, want_d))
    return res


def one(pkg, body, flags=0, cap=None, data_cap=None, base=0, **kw):
    """one segment with room for what it delivers -> its result"""
    src, segs, o_size, d_size = ref.layout(random.Random(1), [body], flags, None if cap is None else [cap], None if data_cap is None else [data_cap], base)
    return check(pkg, src, segs, o_size, d_size, **kw)[0]


def strings_of(rnd, n, lengths=(0, 1, 2, 3, 7, 16, 17, 40)):
    return ref.random_strings(rnd, n, list(lengths))


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    for name in ("undlba_segments", "undlba_outputs", "count_dlba_outputs", "measure_dlba_outputs", "last_undlba_ms"):
        assert callable(getattr(pkg.Batch, name))
    assert callable(pkg.undlba_host)
    assert ctypes.sizeof(pkg.UndlbaResult) == 80
    assert [f[0] for f in pkg.UndlbaResult._fields_] == ["count", "consumed", "declared", "blocks", "status", "block_values", "miniblocks", "data_status", "bad", "first_bad",
                                                         "bytes", "data_avail"]
    assert (pkg.UNDLBA_OFFSETS64, pkg.UNDLBA_ENDS_ONLY, pkg.UNDLBA_SKIP) == (ref.OFFSETS64, ref.ENDS_ONLY, ref.SKIP)
    assert (pkg.UNDLBA_DATA_OK, pkg.UNDLBA_DATA_SHORT) == (ref.DATA_OK, ref.DATA_SHORT) == (0, 1) and pkg.UNDLBA_NONE == ref.NONE
    for text in ("BROTLI_AMD_UNDLBA_OFFSETS64 2u", "BROTLI_AMD_UNDLBA_ENDS_ONLY 4u", "BROTLI_AMD_UNDLBA_SKIP 8u", "BROTLI_AMD_UNDLBA_DATA_SHORT 1u",
                 "typedef struct BrotliAmdUndlbaResult"):
        assert text in header, text
    assert "the byte part of DELTA_LENGTH_BYTE_ARRAY" not in header   # (undbp's out of scope now points here)


def test_reference_decoders_agree():
    """the numpy decoder against the serial one, over the table's segments of every kind and a few capacities"""
    src, segs, _, _ = ref.short_table(400, seed=5)
    for s, l, _, _, data_cap, cap, base, _ in segs:
        for c in (None, cap, 1):
            assert ref.column(src[s:s + l], c, base, data_cap) == ref.column_serial(src[s:s + l], c, base, data_cap), (s, l, c)


def test_pinned_examples(pkg):
    """batch.h's five examples, against values written down by hand, in the reference and through the hook"""
    for body, offsets, data, res in ref.PINNED:
        assert ref.column_serial(body) == (offsets, data, res) and ref.column(body) == (offsets, data, res), body.hex()
        assert dbp_ref.decode(body)[1] == res[:7], body.hex()
        m = res[0]
        got_o, got_d, results = pkg.undlba_host(body, [(0, len(body), 0, 0, 1 << 40, max(m, 1), 0, 0)], 4 * (m + 1), len(data), data_fill=0x77)
        assert got_o == ref.offsets_bytes(offsets, 0) and got_d == data and results == [res], body.hex()
    # the fifth: offset_base alone, at both widths; nothing with ENDS_ONLY
    empty = ref.PINNED[4][0]
    assert pkg.undlba_host(empty, [(0, 5, 0, ref.NONE, 0, 7, 1234, ref.OFFSETS64)], 8, 0)[0] == (1234).to_bytes(8, "little")
    assert pkg.undlba_host(empty, [(0, 5, 0, ref.NONE, 0, 7, 1234, ref.ENDS_ONLY)], 8, 0, offsets_fill=0x11)[0] == b"\x11" * 8
    # all five in one call
    src, segs, o_size, d_size = ref.layout(random.Random(2), [p[0] for p in ref.PINNED], caps=[5] * 5)
    assert check(pkg, src, segs, o_size, d_size) == [p[3] for p in ref.PINNED]


@pytest.mark.parametrize("flags", [0, ref.OFFSETS64, ref.ENDS_ONLY, ref.OFFSETS64 | ref.ENDS_ONLY])
def test_skews(pkg, flags):
    """every skew 0..15 of source, offsets and data, each varied with the other two fixed, and 16 mixed triples"""
    rnd = random.Random(31 + flags)
    bodies = [ref.encode(strings_of(rnd, n)) for n in (70, 1, 33)]
    src, segs, o_size, d_size = ref.layout(rnd, bodies, flags, base=7)
    triples = [(s, 3, 5) for s in range(16)] + [(2, s, 9) for s in range(16)] + [(11, 6, s) for s in range(16)] + [(rnd.randrange(16), rnd.randrange(16), rnd.randrange(16)) for _ in range(16)]
    for a, b, c in triples:
        check(pkg, src, segs, o_size, d_size, src_skew=a, offsets_skew=b, data_skew=c, item_deltas=32, order_seed=a + 16 * b + c)


def test_offset_base_wraps(pkg):
    """4-byte offsets on a base that makes them wrap; 8-byte ones on the same base do not"""
    rnd = random.Random(33)
    body = ref.encode(strings_of(rnd, 90, (0, 5, 200)))
    for flags in (0, ref.ENDS_ONLY, ref.OFFSETS64):
        res = one(pkg, body, flags, base=(1 << 32) - 100, item_deltas=32)
        assert res[10] > 100


@pytest.mark.parametrize("item", [32, 64, 0])
def test_item_edges_and_orders(pkg, item):
    """N of 0, 1, 2, item, item + 1, item + 2 and 2 x item + 1 at item sizes of 32, 64 and the device's, in shuffled orders"""
    rnd = random.Random(41 + item)
    C = item or pkg.undbp_item_deltas()
    bodies = [ref.encode(strings_of(rnd, n, (0, 1, 2, 3))) for n in (0, 1, 2, C, C + 1, C + 2, 2 * C + 1)]
    for flags in (0, ref.OFFSETS64 | ref.ENDS_ONLY):
        src, segs, o_size, d_size = ref.layout(rnd, bodies, flags)
        first = check(pkg, src, segs, o_size, d_size, item_deltas=item)
        for seed in (1, 7):
            assert check(pkg, src, segs, o_size, d_size, item_deltas=item, order_seed=seed, offsets_skew=seed, data_skew=3) == first
        assert [r[0] for r in first] == [0, 1, 2, C, C + 1, C + 2, 2 * C + 1]


@pytest.mark.parametrize("B,M", [(128, 4), (256, 4)])
def test_length_widths(pkg, B, M):
    """lengths whose fields are 0, 1, 7, 20 and 31 bits wide, by widened fields over short strings and by the lengths themselves"""
    rnd = random.Random(43)
    for bits in (0, 1, 7, 20, 31):
        strings = [b"ab"] * 300 if bits == 0 else strings_of(rnd, 300, (0, 1, 2, 3))
        body = ref.encode(strings, B=B, M=M, widen=lambda b, j, k: bits)
        assert max(body[dbp_ref.block_offsets(body)[0] + 1:][:M]) >= bits
        for item in (32, 0):
            res = one(pkg, body, item_deltas=item, order_seed=bits + 1)
            assert res[0] == 300 and res[7] == ref.DATA_OK and res[10] == res[11]
    # wide lengths for real: the data is short by far, and the offsets follow the lengths
    lengths = [rnd.getrandbits(b) for b in (20, 31, 7, 1, 0, 20) * 20]
    res = one(pkg, ref.encode([b"x"] * len(lengths), lengths, B=B, M=M), ref.OFFSETS64, item_deltas=32)
    assert res[7] == ref.DATA_SHORT and res[10] == sum(lengths) and res[11] == len(lengths)


def test_negative_lengths(pkg):
    """negative lengths in a segment's first, a middle and its last item: empty elements, counted, the first one named"""
    rnd = random.Random(47)
    n = 5 * 32 + 9
    strings = strings_of(rnd, n, (1, 2, 3))
    for bad_at in ([0], [1], [2 * 32 + 5], [n - 1], [0, 40, 100, n - 1], list(range(60, 70))):
        lengths = [len(s) for s in strings]
        for e in bad_at:
            lengths[e] = -1 - rnd.randrange(1 << 20)
        body = ref.encode(strings, lengths)
        for seed in (0, 5):
            res = one(pkg, body, item_deltas=32, order_seed=seed)
            assert res[8:10] == (len(bad_at), bad_at[0])
            assert res[10] == sum(v for v in lengths if v >= 0) and res[11] == sum(len(s) for s in strings)
    # a length whose upper 32 bits are set is its lower 32 bits: INT32 arithmetic
    lengths = [len(s) for s in strings]
    lengths[7] += 5 << 32
    lengths[9] = (1 << 31) + 3      # negative as an int32
    res = one(pkg, ref.encode(strings, lengths), item_deltas=64)
    assert res[8:10] == (1, 9)


def test_capacity_around_the_bad_length(pkg):
    """cap below and above count, in front of and behind the only bad length: only bad, first_bad and bytes depend on cap"""
    rnd = random.Random(53)
    strings = strings_of(rnd, 100, (1, 2, 3))
    lengths = [len(s) for s in strings]
    lengths[50] = -7
    body = ref.encode(strings, lengths)
    seen = {}
    for cap in (1, 50, 51, 52, 99, 100, 101, 1 << 56):
        res = one(pkg, body, cap=cap, item_deltas=32)
        assert res[8:10] == ((1, 50) if cap > 50 else (0, ref.NONE)), cap
        assert res[10] == sum(v for v in lengths[:cap] if v >= 0)
        seen[res[:7] + (res[11],)] = cap
    assert len(seen) == 1   # (the walk's part is cap's own)


def test_data_capacity(pkg):
    """data_cap at every byte offset around a 16-byte word of the data, and 0: the cut is exact to the byte, and nothing else changes"""
    rnd = random.Random(59)
    body = ref.encode(strings_of(rnd, 40, (0, 3, 5)))
    whole = one(pkg, body, item_deltas=32)
    for skew in (0, 9):
        for data_cap in [0] + list(range(28, 52)) + [whole[10] - 1, whole[10], whole[10] + 1, 1 << 60]:
            assert one(pkg, body, data_cap=data_cap, item_deltas=32, data_skew=skew) == whole


def test_data_short_and_left_over(pkg):
    rnd = random.Random(61)
    strings = strings_of(rnd, 50, (1, 2, 3))
    body = ref.encode(strings)
    total = sum(len(s) for s in strings)
    # short by 1 byte and by everything: the offsets follow the lengths, the data is what there is
    for cut in (1, total):
        res = one(pkg, body[:len(body) - cut], item_deltas=32, flags=ref.OFFSETS64)
        assert res[4] == ref.OK and res[7] == ref.DATA_SHORT and (res[10], res[11]) == (total, total - cut)
    # left-over bytes: no error, both numbers in the result; with cap < count they are the later elements'
    res = one(pkg, body + b"left over", item_deltas=32)
    assert res[7] == ref.DATA_OK and (res[10], res[11]) == (total, total + 9)
    res = one(pkg, body, cap=10, item_deltas=32)
    assert res[7] == ref.DATA_OK and res[10] == sum(len(s) for s in strings[:10]) and res[11] == total


def test_stops_with_bytes_behind(pkg):
    """every undbp stop behind a whole block, alone and with bytes behind it: undbp's seven fields, and the data begins at `consumed` whatever
    the status is"""
    rnd = random.Random(67)
    for B, M in ((128, 4), (256, 4)):
        strings = strings_of(rnd, B + 1, (0, 1, 2))
        front = dbp_ref.encode([len(s) for s in strings], B, M, declared=B + 1 + 200)
        for name, stop, status, more, _ in dbp_ref.stops(B, M):
            for tail in (b"", b"".join(strings)):
                body = front + stop + tail
                res = one(pkg, body, item_deltas=32, order_seed=3)
                assert res[:7] == dbp_ref.decode(body)[1], name
                if not tail:
                    assert res[4] == status and res[0] == B + 1 + more, name
    # a header that is none: nothing is consumed, and a capacity still has its offsets[0]
    res = one(pkg, b"\x40\x04\x05\x00" + b"abc", cap=4)
    assert res[:5] == (0, 0, 5, 0, ref.BAD_HEADER) and res[11] == 7


def test_counting_and_measuring_write_nothing(pkg):
    rnd = random.Random(71)
    bodies = [ref.encode(strings_of(rnd, n)) for n in (0, 1, 40, 100)]
    src, segs, o_size, d_size = ref.layout(rnd, bodies)
    full = check(pkg, src, segs, o_size, d_size, item_deltas=32)
    counting = [(s, l, o, d, 0, 0, base, flags) for s, l, o, d, _, _, base, flags in segs]
    got = check(pkg, src, counting, o_size, d_size, item_deltas=32)
    assert [r[:8] + (0, ref.NONE, 0, r[11]) for r in full] == got
    measuring = [(s, l, ref.NONE, ref.NONE, 0, cap, base, flags) for s, l, _, _, _, cap, base, flags in segs]
    assert check(pkg, src, measuring, o_size, d_size, item_deltas=32) == full
    # one destination alone
    check(pkg, src, [(s, l, o, ref.NONE, 0, cap, base, flags) for s, l, o, _, _, cap, base, flags in segs], o_size, d_size, item_deltas=32)
    check(pkg, src, [(s, l, ref.NONE, d, dc, cap, base, flags) for s, l, _, d, dc, cap, base, flags in segs], o_size, d_size, item_deltas=32)


def test_table_of_3000_segments(pkg):
    src, segs, o_size, d_size = ref.short_table(3000)
    first = check(pkg, src, segs, o_size, d_size, item_deltas=32)
    assert check(pkg, src, segs, o_size, d_size, item_deltas=64, order_seed=9, src_skew=5, offsets_skew=10, data_skew=15) == first
    statuses = {r[4] for r in first}
    assert statuses == {ref.OK, ref.BAD_HEADER, ref.BAD_WIDTH, ref.TRUNCATED}
    assert any(r[7] == ref.DATA_SHORT for r in first) and any(r[8] for r in first)


def test_refusals(pkg):
    """every host refusal, with its text; nothing is written"""
    body = ref.PINNED[0][0]

    def refused(seg, text, **kw):
        with pytest.raises(RuntimeError) as e:
            pkg.undlba_host(body, [seg], 64, 64, **kw)
        assert text in str(e.value), str(e.value)

    refused((0, len(body), 0, 0, 64, 4, 0, 1), "undlba segment 0: unknown flag bits")
    refused((0, len(body), 0, 0, 64, 4, 0, 16), "undlba segment 0: unknown flag bits")
    refused((0, len(body), 0, 0, 64, 4, 0, ref.SKIP), "undlba segment 0: BROTLI_AMD_UNDLBA_SKIP is for the outputs of a decode call")
    refused((0, len(body), 0, 0, 64, (1 << 56) + 1, 0, 0), "undlba segment 0: a capacity above 2^56 elements")
    refused((0, len(body), 0, ref.NONE, 64, 4, 0, 0), "undlba segment 0: no data destination for a data capacity that is not 0")
    refused((0, len(body) + 1, 0, 0, 64, 4, 0, 0), "a segment outside its buffer")
    refused((0, len(body), 60, 0, 64, 4, 0, 0), "a segment outside its buffer")      # (no room for five offsets)
    refused((0, len(body), 0, 60, 64, 4, 0, 0), "a segment outside its buffer")      # (no room for six bytes)
    refused((0, len(body), 0, 0, 64, 4, 0, 0), "invalid undlba arguments", src_skew=16)
    refused((0, len(body), 0, 0, 64, 4, 0, 0), "an item that is no multiple of 32 deltas", item_deltas=48)
    # the entry points refuse without a device: a NULL batch
    lib = pkg.load_library()
    assert lib.BrotliAmdBatchUndlbaSegments(None, 0, None, None, None, None, None, None, None, None, None, None) != 0
    assert "invalid undlba arguments" in pkg.last_error()
    assert lib.BrotliAmdBatchUndlbaOutputs(None, None, None, None, None, None, None, None) != 0
    assert lib.BrotliAmdBatchLastUndlbaMs(None) == 0.0 and lib.BrotliAmdBatchLastUndlbaPhaseMs(None, 1) == 0.0


def test_host_phases_under_sanitizers(tmp_path):
    """the header's host phases over the five examples and a seeded table under AddressSanitizer and UBSan, in a program of its own"""
    r = san_program.run("undlba_san", tmp_path)
    assert "undlba_san: ok" in r.stdout
