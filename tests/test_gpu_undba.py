"""Undba on the device (needs a real MI355X): the kernels (csrc/brotli_undba_kernels.hip) through BrotliAmdBatchUndbaSegments,
BrotliAmdBatchUndbaOutputs after the three kinds of decode call, and tensors.outputs_as_strings, against the reference (dba_ref.py) AND against
the host hook.  Offsets and data each come from a buffer prefilled with a sentinel pattern, and the WHOLE buffers are compared with the
expectation: a byte written outside a segment's offsets or bytes fails the test.  Bad inputs are lengths and bounds that the contract answers
with a status, never with an address.  All comparisons are exact."""
import random

import numpy as np
import pytest

import dba_ref as ref
import dbp_ref
import seg_filter_harness as H
from seg_filter_harness import stream as _stream, upload as _upload

pytestmark = pytest.mark.gpu
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT
ZERO = (0,) * 16 + (ref.NONE, 0, 0, 0)   # a skipped stream's result
R = ref


@pytest.fixture(scope="module")
def batch(pkg):
    b = pkg.Batch(1)   # (the number of segments is not bound by max_streams)
    yield b
    b.close()


def _device(raw):
    import torch
    t = torch.frombuffer(bytearray(raw) + bytearray(16), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _run(pkg, batch, src, segs, o_size, d_size, hook=True, **hook_kw):
    """one undba_segments call over the hook's kind of table into fresh sentinel buffers: results and both WHOLE buffers against the reference,
    and against the host hook -> the results"""
    want_o, want_d, want_res = ref.expected(src, segs, o_size, d_size)
    d_src, d_o, d_d = _upload(src), _device(ref.sentinel(o_size)), _device(ref.sentinel(d_size, 7))
    sp, op, dp = d_src.data_ptr(), d_o.data_ptr(), d_d.data_ptr()
    got = batch.undba_segments([sp + s[0] for s in segs], [s[1] for s in segs], [None if s[2] == ref.NONE else op + s[2] for s in segs],
                               [None if s[3] == ref.NONE else dp + s[3] for s in segs], [s[4] for s in segs], [s[5] for s in segs], [s[7] for s in segs], [s[6] for s in segs])
    got_o, got_d = d_o[:o_size].cpu().numpy().tobytes(), d_d[:d_size].cpu().numpy().tobytes()
    assert got == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(got, want_res)) if a != b][:3]
    assert got_o == want_o, ("offsets", ref.first_difference(got_o, want_o))
    assert got_d == want_d, ("data", ref.first_difference(got_d, want_d))
    if hook:
        hook_o, hook_d, hook_res = pkg.undba_host(src, segs, o_size, d_size, offsets_fill=ref.sentinel(o_size), data_fill=ref.sentinel(d_size, 7), **hook_kw)
        assert (hook_res, hook_o, hook_d) == (got, got_o, got_d)
    return got


def _sorted(rnd, n, stem=b"key/", **kw):
    return ref.sorted_strings(rnd, n, stem, **kw)


def test_the_pinned_examples_in_one_call(pkg, batch):
    src, segs, o_size, d_size = ref.layout(random.Random(2), [p[0] for p in ref.PINNED], caps=[5] * len(ref.PINNED))
    assert _run(pkg, batch, src, segs, o_size, d_size) == [p[3] for p in ref.PINNED]
    for (body, offsets, data, _), s in zip(ref.PINNED, segs):   # (what _run compared, said once more by hand)
        want_o, want_d, _ = ref.expected(src, segs, o_size, d_size)
        assert want_o[s[2]:s[2] + 4 * len(offsets)] == ref.offsets_bytes(offsets, 0) and want_d[s[3]:s[3] + len(data)] == data


def test_item_edges(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(81)
    counts = (1, 2, C, C + 1, C + 2, 2 * C + 1)
    bodies = [ref.encode(_sorted(rnd, n)) for n in counts]
    for flags in (0, ref.OFFSETS64 | ref.ENDS_ONLY):
        got = _run(pkg, batch, *ref.layout(rnd, bodies, flags), order_seed=3)
        assert [r[R.R_COUNT_P] for r in got] == [r[R.R_COUNT_S] for r in got] == list(counts)
    # capacities at the edges too: only first_bad, bad_kind, bytes, suffix_bytes and two bits of data_status depend on them
    got = _run(pkg, batch, *ref.layout(rnd, [bodies[5]] * 6, caps=[1, 2, C, C + 1, C + 2, 2 * C + 9]))
    assert len({r[:15] + r[19:] for r in got}) == 1 and [r[R.R_BYTES] for r in got] == sorted(r[R.R_BYTES] for r in got) and got[0][R.R_BYTES] < got[4][R.R_BYTES] < got[5][R.R_BYTES]


def test_all_skews_of_source_offsets_and_data_at_both_widths(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(83)
    count = C + 300
    body = ref.encode(_sorted(rnd, count))
    data_len = len(ref.column(body, count)[1])
    src, segs, o_at, d_at = bytearray(), [], 0, 0
    for skew in range(16):
        for flags in (0, ref.OFFSETS64, ref.ENDS_ONLY, ref.OFFSETS64 | ref.ENDS_ONLY):
            src += b"\xc3" * (H.next_at(len(src), skew) - len(src))
            o_at = H.next_at(o_at, (3 * skew + flags) % 16)
            d_at = H.next_at(d_at, (5 * skew + flags // 2) % 16)
            segs.append((len(src), len(body), o_at, d_at, data_len, count, 100 * skew, flags))
            src += body
            o_at += 8 * (count + 1); d_at += data_len + 1
    assert {s[0] % 16 for s in segs} == set(range(16)) and {s[2] % 16 for s in segs} == set(range(16)) and {s[3] % 16 for s in segs} == set(range(16))
    _run(pkg, batch, bytes(src), segs, o_at + 64, d_at + 64)


def test_two_pages_appended_with_ends_only(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(84)
    n1, n2 = C + 77, 500
    p1, p2 = ref.encode(_sorted(rnd, n1)), ref.encode(_sorted(rnd, n2, b"later/"))
    o1, b1, _ = ref.column(p1, n1)
    o2, b2, _ = ref.column(p2, n2, len(b1))
    segs = [(0, len(p1), 4, 1, len(b1), n1, 0, 0), (len(p1), len(p2), 4 + 4 * (n1 + 1), 1 + len(b1), len(b2), n2, len(b1), ref.ENDS_ONLY)]
    o_size, d_size = 4 + 4 * (n1 + n2 + 1) + 32, 1 + len(b1) + len(b2) + 32
    _run(pkg, batch, p1 + p2, segs, o_size, d_size)
    want_o, want_d, _ = ref.expected(p1 + p2, segs, o_size, d_size)
    assert want_o[4:4 + 4 * (n1 + n2 + 1)] == ref.offsets_bytes(o1 + o2[1:], 0) and want_d[1:1 + len(b1) + len(b2)] == b1 + b2   # one Arrow array


def test_three_thousand_segments(pkg, batch):
    src, segs, o_size, d_size = ref.short_table(3000)
    got = _run(pkg, batch, src, segs, o_size, d_size, item_deltas=64, order_seed=4)
    every = {ref.OK, ref.BAD_HEADER, ref.BAD_WIDTH, ref.TRUNCATED}
    assert {r[4] for r in got} == every and {r[12] for r in got} == every   # every status of both walks
    for bit in (ref.DATA_SHORT, ref.DATA_BAD, ref.DATA_COUNTS_DIFFER):
        assert any(r[R.R_STATUS] & bit for r in got), bit
    assert {r[R.R_KIND] for r in got} == {0, 1, 2, 3}
    assert batch.last_undba_ms() > 0.0
    assert all(batch.last_undba_ms(p) >= 0.0 for p in range(1, 10)) and batch.last_undba_ms(10) == 0.0 and batch.last_undba_ms(0) == 0.0
    assert all(batch.last_undba_ms(p) > 0.0 for p in (1, 2, 4, 6, 7, 8, 9))
    assert abs(sum(batch.last_undba_ms(p) for p in range(1, 10)) - batch.last_undba_ms()) < 0.05 * batch.last_undba_ms() + 0.01


def test_data_short_and_data_capacities(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(88)
    strings = _sorted(rnd, C + 40)
    body = ref.encode(strings)
    total, suffixes = sum(len(s) for s in strings), ref.column(body)[2][R.R_SUFFIX]
    # the suffix data short by a byte and by everything (the missing bytes read as 0), and bytes left over
    bodies = [body[:-1], body[:len(body) - suffixes], body + b"left over"]
    got = _run(pkg, batch, *ref.layout(rnd, bodies, ref.OFFSETS64))
    assert [(r[R.R_STATUS], r[R.R_BYTES], r[R.R_SUFFIX], r[R.R_AVAIL]) for r in got] == [(ref.DATA_SHORT, total, suffixes, suffixes - 1), (ref.DATA_SHORT, total, suffixes, 0),
                                                                                       (ref.DATA_OK, total, suffixes, suffixes + 9)]
    # data capacities: the cut is exact to the byte, and nothing in the result depends on it
    data_caps = [0, 1, 15, 16, 17, 100, total - 1, total, total + 20]
    got = _run(pkg, batch, *ref.layout(rnd, [body] * len(data_caps), data_caps=data_caps))
    assert len(set(got)) == 1


def test_measuring_and_counting_calls(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(89)
    bodies = [ref.encode(_sorted(rnd, n)) for n in (5, C + 9, 3 * C)]
    src, segs, o_size, d_size = ref.layout(rnd, bodies)
    measuring = [s[:2] + (ref.NONE, ref.NONE, 0) + s[5:] for s in segs]
    measured = _run(pkg, batch, src, measuring, o_size, d_size)   # (nothing is written: both buffers are the sentinels)
    assert all(batch.last_undba_ms(p) > 0.0 for p in (1, 2, 4, 6))   # (the same launches)
    sized = [s[:4] + (m[R.R_BYTES],) + s[5:] for s, m in zip(segs, measured)]
    assert _run(pkg, batch, src, sized, o_size, d_size) == measured
    counting = [s[:4] + (0, 0) + s[6:] for s in segs]
    counted = _run(pkg, batch, src, counting, o_size, d_size)
    assert [c[:15] + c[19:] for c in counted] == [m[:15] + m[19:] for m in measured] and all(c[15:19] == (0, ref.NONE, 0, 0) for c in counted)
    assert batch.last_undba_ms(1) > 0.0 and all(batch.last_undba_ms(p) == 0.0 for p in range(2, 10)) and batch.last_undba_ms() == batch.last_undba_ms(1)
    # without any array of destinations
    d_src = _upload(src)
    assert batch.undba_segments([d_src.data_ptr() + s[0] for s in segs], [s[1] for s in segs], None, None, None, [0] * 3) == counted
    assert batch.undba_segments([d_src.data_ptr() + s[0] for s in segs], [s[1] for s in segs], None, None, None, [s[5] for s in segs]) == measured


def test_bad_arguments_launch_nothing(pkg, batch):
    d = _device(ref.sentinel(4096))
    p = d.data_ptr()
    args = lambda **kw: [kw.get(k, v) for k, v in (("src", [p]), ("lens", [10]), ("offsets", [p + 1024]), ("data", [p + 2048]), ("data_caps", [100]), ("caps", [8]), ("flags", [0]),
                                                  ("bases", None))]
    for kw, text in (({"flags": [16]}, "undba segment 0: unknown flag bits"), ({"flags": [1]}, "undba segment 0: unknown flag bits"),
                     ({"flags": [ref.SKIP]}, "undba segment 0: BROTLI_AMD_UNDBA_SKIP is for the outputs of a decode call"),
                     ({"caps": [(1 << 56) + 1]}, r"undba segment 0: a capacity above 2\^56"),
                     ({"data": [None]}, "undba segment 0: no data destination for a data capacity that is not 0"),
                     ({"data": None}, "undba segment 0: no data destination for a data capacity that is not 0")):
        with pytest.raises(RuntimeError, match=text):
            batch.undba_segments(*args(**kw))
        assert batch.last_undba_ms() == 0.0   # (nothing was launched)
    assert d.cpu().numpy().tobytes() == ref.sentinel(4096) + bytes(16)
    assert batch.undba_segments([], [], [], [], [], []) == []


# ------------------------------------------------------------------ the prefix phases
def test_a_prefix_shared_by_every_element_of_three_items(pkg, batch):
    """no element of items 1 and 2 has r_e == 0: phases B and C carry byte 0 from element 0"""
    C = pkg.undbp_item_deltas()
    rnd = random.Random(92)
    strings = _sorted(rnd, 3 * C + 50, b"a prefix that every element shares/", tail=(1, 2, 5, 12))
    body = ref.encode(strings)
    pv = dbp_ref.decode(body, 8)[0]
    assert int(min(pv[1:])) >= 35
    got = _run(pkg, batch, *ref.layout(rnd, [body, body], caps=[3 * C + 50, 2 * C + 1]), order_seed=5)
    assert got[0][R.R_BYTES] == sum(len(s) for s in strings) and got[0][R.R_STATUS] == ref.DATA_OK


def test_forty_items_whose_shared_prefix_grows_and_shrinks_at_item_boundaries(pkg, batch):
    """the carry of phase B through about forty items and a second segment behind them; the hook is compared at its own, smaller shapes
    elsewhere"""
    C = pkg.undbp_item_deltas()
    rnd = random.Random(93)
    strings, stem = [], b"0123456789abcdefghij"
    for j in range(40):
        depth = 10 + (j % 7 if j % 2 else -(j % 5))   # (one byte more or less than the item in front, and more)
        n = C + 1 if j == 0 else C
        strings += [stem[:depth] + b"%05d" % (j * C + x) for x in range(n)]
    strings += [stem[:3] + b"tail%d" % x for x in range(77)]
    first = ref.encode(strings, B=1024, M=8)
    second = ref.encode(_sorted(rnd, 2 * C + 5), B=256, M=4)
    got = _run(pkg, batch, *ref.layout(rnd, [first, second], ref.OFFSETS64, gap=(0,)), hook=False)
    assert got[0][R.R_COUNT_P] == 40 * C + 78 and got[0][R.R_BYTES] == sum(len(s) for s in strings) and all(r[R.R_STATUS] == ref.DATA_OK for r in got)


def test_item_starts_repeats_and_empty_strings_at_item_edges(pkg, batch):
    """an item whose first element has p = 0, an item made only of repeats (s = 0, p = L), and empty strings at the items' edges"""
    C = pkg.undbp_item_deltas()
    rnd = random.Random(94)
    a = _sorted(rnd, C + 1, b"aa/")                    # item 0
    b_ = [b"zz-repeated-string"] * C                   # item 1: its first element has p = 0, every other one is a repeat
    c = [b"zz-repeated-string"] * C                    # item 2: repeats alone
    d = [b""] + _sorted(rnd, C - 2, b"zz/") + [b""]    # item 3: empty at both edges
    e = [b"", b"", b"x"]                               # item 4
    strings = a + b_ + c + d + e
    assert ref.common_prefix(a[-1], b_[0]) == 0
    body = ref.encode(strings)
    got = _run(pkg, batch, *ref.layout(rnd, [body] * 3, caps=[len(strings), 3 * C + 1, 3 * C + 2]), order_seed=6)
    assert got[0][R.R_BYTES] == sum(len(s) for s in strings)
    # any legal shorter prefix gives the same column
    prefixes = [0] + [rnd.randrange(0, ref.common_prefix(strings[x - 1], strings[x]) + 1) for x in range(1, len(strings))]
    assert _run(pkg, batch, *ref.layout(rnd, [ref.encode(strings, prefixes)]))[0][R.R_BYTES] == got[0][R.R_BYTES]


def test_long_strings_across_an_item_boundary_and_beyond_the_lds_lengths(pkg, batch):
    """strings of 4 KiB that share 4000 bytes across an item boundary, and strings of 70 KiB -- beyond both LDS lengths: phase A's walk back and
    phase B's far bytes -- that share 69 KiB inside an item and across a boundary, among short ones"""
    C = pkg.undbp_item_deltas()
    rnd = random.Random(95)
    assert pkg.UNDBA_LDS_STRING == 4096 and pkg.UNDBA_LDS_CARRY == 32768
    stem4, stem70 = rnd.randbytes(4000), rnd.randbytes(69 << 10)
    strings = _sorted(rnd, C - 3, b"a/")
    strings += [stem4 + rnd.randbytes(96) for _ in range(8)]          # elements C - 3 .. C + 4: items 0 and 1
    strings += _sorted(rnd, C - 10, b"b/")
    strings += [stem70 + rnd.randbytes(1 << 10) for _ in range(3)]    # elements 2C - 5 .. 2C - 3: inside item 1
    strings += [stem70[:40000] + b"shorter"]
    strings += [stem70 + rnd.randbytes(1 << 10) for _ in range(4)]    # elements 2C - 1 .. 2C + 2: items 1 and 2
    strings += _sorted(rnd, 40, b"d/")
    body = ref.encode(strings)
    pv = dbp_ref.decode(body, 8)[0]
    assert int(pv[C + 1]) >= 4000 and int(pv[2 * C + 1]) >= 69 << 10 and int(pv[2 * C - 3]) >= 69 << 10 and int(pv[2 * C - 1]) >= 40000
    # a segment whose last item is three such strings: its last element's r is 69 KiB, beyond what phase B keeps in LDS
    ending = _sorted(rnd, C - 1, b"e/") + [stem70 + rnd.randbytes(100) for _ in range(5)]
    body2 = ref.encode(ending)
    assert len(ending) == C + 4 and min(int(v) for v in dbp_ref.decode(body2, 8)[0][C + 1:]) >= 69 << 10 > pkg.UNDBA_LDS_CARRY
    got = _run(pkg, batch, *ref.layout(rnd, [_sorted_body(rnd, 30), body, body2, _sorted_body(rnd, 3)], gap=(1,)))
    assert got[1][R.R_BYTES] == sum(len(s) for s in strings) and got[2][R.R_BYTES] == sum(len(s) for s in ending) and got[1][R.R_STATUS] == got[2][R.R_STATUS] == ref.DATA_OK
    # cut in the middle of a far copy
    _run(pkg, batch, *ref.layout(rnd, [body, body2], data_caps=[got[1][R.R_BYTES] - 45 * (1 << 10), got[2][R.R_BYTES] - 20 * (1 << 10)]))


def test_declared_lengths_of_two_gib_over_ten_bytes_of_source(pkg, batch):
    """elements that declare 2^31 - 1 bytes and more, through three items, under small data capacities: every launch's work follows what is
    stored, and the results and the cut output are what they are for any page"""
    C = pkg.undbp_item_deltas()
    body, n = ref.huge_page(2 * C + 10)
    data_caps = [0, 1, 10, 64, 100000]
    got = _run(pkg, batch, *ref.layout(random.Random(98), [body] * len(data_caps), ref.OFFSETS64, caps=[n] * len(data_caps), data_caps=data_caps), item_deltas=64)
    assert len(set(got)) == 1 and got[0][R.R_STATUS] == ref.DATA_SHORT and got[0][R.R_BYTES] > (2 * C + 10) << 30 and got[0][R.R_AVAIL] == 10
    assert batch.last_undba_ms() < 1000.0


def _sorted_body(rnd, n):
    return ref.encode(_sorted(rnd, n))


def test_streams_in_different_blocks_and_of_different_counts(pkg, batch):
    """P in blocks of 256 values and 8 miniblocks against S in blocks of 1024 and 8; and counts that differ, either way round"""
    C = pkg.undbp_item_deltas()
    rnd = random.Random(96)
    strings = _sorted(rnd, 2 * C + 300)
    body = ref.encode(strings, p_knobs=dict(B=256, M=8), s_knobs=dict(B=1024, M=8))
    got = _run(pkg, batch, *ref.layout(rnd, [body], ref.OFFSETS64))
    assert (got[0][5], got[0][6], got[0][13], got[0][14]) == (256, 8, 1024, 8) and got[0][R.R_STATUS] == ref.DATA_OK
    prefixes = [0] + [ref.common_prefix(strings[x - 1], strings[x]) for x in range(1, len(strings))]
    lens = [len(v) - p for v, p in zip(strings, prefixes)]
    tail = b"".join(v[p:] for v, p in zip(strings, prefixes))
    fewer_s = dbp_ref.encode(prefixes, 256, 8) + dbp_ref.encode(lens[:C + 7], 1024, 8) + tail
    fewer_p = dbp_ref.encode(prefixes[:C - 9], 256, 8) + dbp_ref.encode(lens, 1024, 8) + tail
    got = _run(pkg, batch, *ref.layout(rnd, [fewer_s, fewer_p]))
    assert [(r[R.R_COUNT_P], r[R.R_COUNT_S], r[R.R_STATUS]) for r in got] == [(2 * C + 300, C + 7, ref.DATA_COUNTS_DIFFER), (C - 9, 2 * C + 300, ref.DATA_COUNTS_DIFFER)]
    assert [len(ref.column(b)[0]) - 1 for b in (fewer_s, fewer_p)] == [C + 7, C - 9]


@pytest.mark.parametrize("rule", [ref.BAD_PREFIX_NEGATIVE, ref.BAD_SUFFIX_NEGATIVE, ref.BAD_PREFIX_LONG])
def test_first_bad_by_each_rule(pkg, batch, rule):
    """first_bad at 0, at C, at C + 1 and in the last item, with upper value bits that are not looked at; everything behind it is empty and
    unwritten, whatever it holds -- later bad elements among it"""
    C = pkg.undbp_item_deltas()
    rnd = random.Random(97 + rule)
    strings = _sorted(rnd, 3 * C + 50)
    good_p = [0] + [ref.common_prefix(strings[x - 1], strings[x]) for x in range(1, len(strings))]
    good_s = [len(v) - p for v, p in zip(strings, good_p)]
    bodies, places = [], [0, C, C + 1, 3 * C + 49]
    for at in places:
        p, s = list(good_p), list(good_s)
        for e in (at, min(at + 700, len(strings) - 1)):   # (a second bad element behind the first)
            if rule == ref.BAD_PREFIX_NEGATIVE:
                p[e] = -1 - rnd.randrange(1 << 20)
            elif rule == ref.BAD_SUFFIX_NEGATIVE:
                s[e] = (1 << 31) + rnd.randrange(1 << 20) + (7 << 32)   # (negative as an int32)
            else:
                p[e] = (len(strings[e - 1]) if e else 0) + 1 + (3 << 32)
        p[5] += (at != 0) * (9 << 32)   # (a good element with upper bits)
        bodies.append(ref.encode(strings, p, s))
    got = _run(pkg, batch, *ref.layout(rnd, bodies), order_seed=8)
    assert [(r[R.R_FIRST_BAD], r[R.R_KIND], r[R.R_STATUS] & ref.DATA_BAD) for r in got] == [(at, rule, ref.DATA_BAD) for at in places]
    assert [r[R.R_BYTES] for r in got] == [sum(len(v) for v in strings[:at]) for at in places]
    # a capacity in front of it: no bad element
    got = _run(pkg, batch, *ref.layout(rnd, [bodies[1], bodies[2]], caps=[C, C + 1]))
    assert [(r[R.R_FIRST_BAD], r[R.R_KIND]) for r in got] == [(ref.NONE, ref.BAD_NONE)] * 2


# ------------------------------------------------------------------ the outputs of a decode call
class _Pages:
    """streams of one decode call: page bodies of several shapes, an empty one, one with a bad prefix, one cut, and streams that are no such
    pages"""

    def __init__(self, pkg):
        C = pkg.undbp_item_deltas()
        rnd = random.Random(90)
        strings = _sorted(rnd, 300)
        prefixes = [0] + [ref.common_prefix(strings[x - 1], strings[x]) for x in range(1, 300)]
        prefixes[250] = len(strings[249]) + 1
        self.raws = [ref.encode(_sorted(rnd, 5000)), b"not a page at all, just some bytes" * 40, ref.encode(_sorted(rnd, 1)), ref.encode([]),
                     ref.encode(_sorted(rnd, C + 9), B=256, M=8), ref.encode(strings, prefixes), ref.encode(_sorted(rnd, 700))[:-100], ref.encode(_sorted(rnd, 2 * C + 1, b"k"))]
        self.streams = [_stream(r) for r in self.raws]


@pytest.fixture(scope="module")
def pages(pkg):
    return _Pages(pkg)


def _check_outputs(b, pages, skip, delivered=None):
    """undba_outputs of the pages' streams into fresh sentinel buffers: offsets, bytes and results, the skipped streams' zeros; then a measuring
    call and a counting call, which write nothing; delivered: what the streams delivered, where that is not all of them"""
    n = len(pages.raws)
    raws = [(delivered or {}).get(i, raw) for i, raw in enumerate(pages.raws)]
    want_res, cols = [], []
    for i, raw in enumerate(raws):
        if i in skip:
            want_res.append(ZERO); cols.append(None)
            continue
        flags = (ref.OFFSETS64 if i & 1 else 0) | (ref.ENDS_ONLY if i & 2 else 0)
        offsets, data, res = ref.column(raw, max(max(ref.counts(raw)), 1), 7 * i)
        want_res.append(res); cols.append((ref.offsets_array(offsets, flags), data, flags))
    none = {i for i, c in enumerate(cols) if c is None}
    o_offs, o_size = H.slots([0 if c is None else len(c[0]) for c in cols], none)
    d_offs, d_size = H.slots([0 if c is None else len(c[1]) for c in cols], none, start=9)
    want_o, want_d = bytearray(ref.sentinel(o_size)), bytearray(ref.sentinel(d_size, 7))
    for c, o, d in zip(cols, o_offs, d_offs):
        if c is not None:
            want_o[o:o + len(c[0])] = c[0]; want_d[d:d + len(c[1])] = c[1]
    d_o, d_d = _device(ref.sentinel(o_size)), _device(ref.sentinel(d_size, 7))
    op, dp = d_o.data_ptr(), d_d.data_ptr()
    flags = [ref.SKIP if c is None else c[2] for c in cols]
    caps = [0 if c is None else max(max(r[R.R_COUNT_P], r[R.R_COUNT_S]), 1) for c, r in zip(cols, want_res)]
    got = b.undba_outputs([None if o is None else op + o for o in o_offs], [None if d is None else dp + d for d in d_offs], [0 if c is None else len(c[1]) for c in cols],
                          caps, flags, [7 * i for i in range(n)])
    assert got == want_res, [(i, a, c) for i, (a, c) in enumerate(zip(got, want_res)) if a != c][:3]
    both = lambda: (d_o[:o_size].cpu().numpy().tobytes(), d_d[:d_size].cpu().numpy().tobytes())
    assert both() == (bytes(want_o), bytes(want_d))
    assert b.measure_dba_outputs([None if c is None else k for c, k in zip(cols, caps)]) == want_res
    counted = b.count_dba_outputs()
    assert counted == [ref.column(raw, 0)[2] for raw in raws]
    assert b.count_dba_outputs(flags) == [ZERO if c is None else r for c, r in zip(cols, counted)]
    assert both() == (bytes(want_o), bytes(want_d))   # (measuring and counting write nothing)
    return got


def test_outputs_of_decode_device(pkg, pages):
    import torch
    datas, caps = pages.streams, [len(r) for r in pages.raws]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    offs = [sum(caps[:i]) + 3 for i in range(len(caps))]
    arena = torch.from_numpy(np.frombuffer(ref.sentinel(sum(caps) + 4096), dtype=np.uint8).copy()).cuda()   # the outputs back to back, at whatever alignment that gives
    torch.cuda.synchronize()
    n = len(datas)
    b = pkg.Batch(n)
    try:
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.count_dba_outputs()
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, c) for c in caps]
        got = _check_outputs(b, pages, skip={2})
        assert (got[5][R.R_FIRST_BAD], got[5][R.R_KIND]) == (250, ref.BAD_PREFIX_LONG) and got[6][R.R_STATUS] == ref.DATA_SHORT and got[3][0] == 0 and got[1][4] != ref.OK
        with pytest.raises(RuntimeError, match="undba stream 4: unknown flag bits"):
            b.undba_outputs(None, None, None, [0] * n, [0, 0, 0, 0, 1, 0, 0, 0])
    finally:
        b.close()


def test_outputs_of_decode_host_and_packed(pkg, pages):
    n = len(pages.raws)
    b = pkg.Batch(n)
    try:
        results, outs = b.decode_host(pages.streams, [len(r) for r in pages.raws], FLAGS)
        assert [r.result for r in results] == [1] * n and outs == pages.raws
        _check_outputs(b, pages, skip={1, 6})
        results, outs = b.decode_packed(pages.streams, flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(r)) for r in pages.raws]
        _check_outputs(b, pages, skip={4})
    finally:
        b.close()


def test_outputs_as_strings_on_the_pyarrow_pages(pkg):
    """the data page that pyarrow wrote for every DELTA_BYTE_ARRAY column (tests/golden/dba_pages/), each Brotli-compressed, in ONE decode
    call; outputs_as_strings gives the columns, and with pyarrow present an Arrow array over the buffers equals the column"""
    import torch
    import dba_pages
    tensors = H.tensors_module()
    pages = dba_pages.load()
    streams = [_stream(body) for _, body, _, _ in pages]
    specs = [("dba", e["values"]) + (("large",) if k & 1 else ()) for k, (e, _, _, _) in enumerate(pages)]
    b = pkg.Batch(len(streams))
    try:
        results, _ = b.decode_packed(streams, flags=FLAGS)
        assert [r.result for r in results] == [1] * len(streams)
        got = tensors.outputs_as_strings(b, specs)
        for k, ((e, _, offsets, data), (o, d)) in enumerate(zip(pages, got)):
            assert o.is_cuda and d.is_cuda and o.dtype == (torch.int64 if k & 1 else torch.int32) and d.dtype == torch.uint8 and o.data_ptr() % 64 == 0 and d.data_ptr() % 64 == 0
            assert o.cpu().tolist() == np.frombuffer(offsets, dtype="<i4").tolist() and d.cpu().numpy().tobytes() == data, e["label"]
        try:
            import pyarrow as pa
        except ImportError:
            pa = None
        if pa is not None:
            for k, ((e, _, offsets, data), (o, d)) in enumerate(zip(pages, got)):
                typ = {("string", 0): pa.string(), ("string", 1): pa.large_string(), ("binary", 0): pa.binary(), ("binary", 1): pa.large_binary()}[(e["type"], k & 1)]
                arr = pa.Array.from_buffers(typ, e["values"], [None, pa.py_buffer(o.cpu().numpy().tobytes()), pa.py_buffer(d.cpu().numpy().tobytes())])
                o32 = np.frombuffer(offsets, dtype="<i4")
                assert arr.to_pylist() == [(data[o32[r]:o32[r + 1]].decode() if e["type"] == "string" else data[o32[r]:o32[r + 1]]) for r in range(e["values"])], e["label"]
    finally:
        b.close()


def test_outputs_as_strings_with_the_other_specs_in_the_same_call(pkg):
    import dba_pages
    import dlba_pages
    import dlba_ref
    tensors = H.tensors_module()
    e1, body1, offsets1, data1 = dlba_pages.load()[2]
    e2, body2, offsets2, data2 = dba_pages.load()[2]
    b = pkg.Batch(3)
    try:
        results, _ = b.decode_packed([_stream(body2), _stream(body1), _stream(ref.encode([]))], flags=FLAGS)
        assert [r.result for r in results] == [1] * 3
        got = tensors.outputs_as_strings(b, [("dba", e2["values"], "large"), ("dlba", e1["values"]), ("dba", 0)])
        assert got[0][0].cpu().tolist() == np.frombuffer(offsets2, dtype="<i4").tolist() and got[0][1].cpu().numpy().tobytes() == data2
        assert got[1][0].cpu().tolist() == np.frombuffer(offsets1, dtype="<i4").tolist() and got[1][1].cpu().numpy().tobytes() == data1
        assert got[2][0].cpu().tolist() == [0] and got[2][1].numel() == 0
        assert len({t.untyped_storage().data_ptr() for pair in got for t in pair}) == 1   # ONE buffer
        assert dlba_ref.column(body1, e1["values"])[1] == data1
    finally:
        b.close()


def test_every_new_value_error_of_outputs_as_strings(pkg):
    tensors = H.tensors_module()
    rnd = random.Random(91)
    strings = _sorted(rnd, 20)
    prefixes = [0] + [ref.common_prefix(strings[x - 1], strings[x]) for x in range(1, 20)]
    lens = [len(v) - p for v, p in zip(strings, prefixes)]
    suffixes = sum(lens)
    good = ref.encode(strings)
    at_s = dbp_ref.decode(good, 8, 0)[1][1]
    long_p, neg_p, neg_s = list(prefixes), list(prefixes), list(lens)
    long_p[5], neg_p[7], neg_s[11] = len(strings[4]) + 1, -2, -9
    raws = [good, good[:7], ref.encode(strings, long_p), good + b"xy", good[:-3], b"\x40\x04\x05\x00" + good, good[:at_s] + b"\x40\x04\x05\x00",
            dbp_ref.encode(prefixes) + dbp_ref.encode(lens[:19]) + b"x" * suffixes, ref.encode(strings, neg_p), ref.encode(strings, None, neg_s)]
    b = pkg.Batch(len(raws))
    try:
        results, _ = b.decode_packed([_stream(r) for r in raws], flags=FLAGS)
        assert [r.result for r in results] == [1] * len(raws)
        only = lambda i, spec: [spec if s == i else None for s in range(len(raws))]
        o, d = tensors.outputs_as_strings(b, only(0, ("dba", 20)))[0]
        assert o.cpu().tolist() == ref.column(good)[0] and d.cpu().numpy().tobytes() == b"".join(strings)
        for i, spec, text in ((1, ("dba", 20), r"stream 1: its prefix lengths: blocks that the stream's end cuts \(status 3\) after 1 lengths in 5 bytes, of 20 declared"),
                              (5, ("dba", 20), r"stream 5: its prefix lengths: a header that is none \(status 1\)"),
                              (6, ("dba", 20), r"stream 6: its suffix lengths: a header that is none \(status 1\)"),
                              (7, ("dba", 20), "stream 7: 20 prefix lengths and 19 suffix lengths"),
                              (0, ("dba", 21), "stream 0: 20 lengths in its streams, but the column has 21 rows"),
                              (0, ("dba", 19), "stream 0: 20 lengths in its streams, but the column has 19 rows"),
                              (2, ("dba", 20), "stream 2: element 5 of its 20 has a prefix longer than the element in front of it"),
                              (8, ("dba", 20), "stream 8: element 7 of its 20 has a negative prefix length"),
                              (9, ("dba", 20), "stream 9: element 11 of its 20 has a negative suffix length"),
                              (3, ("dba", 20), "stream 3: its suffix lengths add up to %d bytes and %d are there: bytes are left over" % (suffixes, suffixes + 2)),
                              (4, ("dba", 20), "stream 4: its suffix lengths add up to %d bytes and %d are there: the data is short" % (suffixes, suffixes - 3)),
                              (0, ("dba", 20, "big"), r"stream 0: a \"dba\" spec is"), (0, ("dba", -1), r"stream 0: a \"dba\" spec is"),
                              (0, ("dba",), r"stream 0: a \"dba\" spec is")):
            with pytest.raises(ValueError, match=text):
                tensors.outputs_as_strings(b, only(i, spec))
    finally:
        b.close()
