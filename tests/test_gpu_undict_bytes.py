"""Undict for byte arrays on the device (needs a real MI355X): the kernels (csrc/brotli_undict_bytes_kernels.hip) through
BrotliAmdBatchUndictBytesSegments, BrotliAmdBatchUndictBytesOutputs after the three kinds of decode call, and tensors.outputs_as_strings, against
the reference (dict_bytes_ref.py) AND against the host hook.  Offsets and data each come from a buffer prefilled with a sentinel pattern, and the
WHOLE buffers are compared with the expectation: a byte written outside a segment's offsets or bytes fails the test.  A dictionary lies inside
a larger allocation among other dictionaries' bytes, and an index outside it gives an empty element: a wrong bound check shows as bytes in the
data, not as a stray read.  All comparisons are exact."""
import random

import numpy as np
import pytest

import dict_bytes_ref as ref
import rle_ref
import seg_filter_harness as H
from seg_filter_harness import stream as _stream, upload as _upload

pytestmark = pytest.mark.gpu
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT
ZERO = (0, 0, 0, 0, 0, 0, ref.NONE, 0, 0, 0, 0)   # a skipped stream's result


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


def _run(pkg, batch, src, dictionary, segs, o_size, d_size, hook=True, **hook_kw):
    """one undict_bytes_segments call over the hook's kind of table into fresh sentinel buffers: results and both WHOLE buffers against the
    reference, and against the host hook -> the results"""
    want_o, want_d, want_res = ref.expected(src, dictionary, segs, o_size, d_size)
    d_src, d_dict, d_o, d_d = _upload(src), _upload(dictionary), _device(ref.sentinel(o_size)), _device(ref.sentinel(d_size, 7))
    sp, tp, op, dp = d_src.data_ptr(), d_dict.data_ptr(), d_o.data_ptr(), d_d.data_ptr()
    got = batch.undict_bytes_segments([sp + s[0] for s in segs], [s[1] for s in segs], [None if s[2] == ref.NONE else op + s[2] for s in segs],
                                      [None if s[3] == ref.NONE else dp + s[3] for s in segs], [s[4] for s in segs], [s[5] for s in segs], [s[10] for s in segs],
                                      [s[11] for s in segs], [s[6] for s in segs], [tp + s[7] for s in segs], [s[8] for s in segs], [s[9] for s in segs])
    got_o, got_d = d_o[:o_size].cpu().numpy().tobytes(), d_d[:d_size].cpu().numpy().tobytes()
    assert got == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(got, want_res)) if a != b][:3]
    assert got_o == want_o, ("offsets", ref.first_difference(got_o, want_o))
    assert got_d == want_d, ("data", ref.first_difference(got_d, want_d))
    if hook:
        hook_o, hook_d, hook_res, _ = pkg.undict_bytes_host(src, dictionary, segs, o_size, d_size, offsets_fill=ref.sentinel(o_size), data_fill=ref.sentinel(d_size, 7), **hook_kw)
        assert (hook_res, hook_o, hook_d) == (got, got_o, got_d)
    return got


def _table(rnd, datas, entries, k, flags=0, **kw):
    dictionary = b"\x11\x22\x33" + ref.dictionary_bytes(entries) + b"\x44" * 5
    src, segs, o_size, d_size = ref.layout(rnd, datas, 3, len(dictionary) - 8, k, flags, dictionary=dictionary, **kw)
    return src, dictionary, segs, o_size, d_size


def test_three_thousand_segments_over_forty_dictionaries(pkg, batch):
    src, dictionary, segs, o_size, d_size = ref.short_table()
    got = _run(pkg, batch, src, dictionary, segs, o_size, d_size)
    assert sum(1 for r in got if r[5]) > 300 and {r[10] for r in got} == {ref.DICT_OK, ref.DICT_CUT}
    assert batch.last_undict_bytes_ms() > 0.0
    assert all(batch.last_undict_bytes_ms(p) >= 0.0 for p in (1, 2, 3, 4, 5)) and batch.last_undict_bytes_ms(6) == 0.0 and batch.last_undict_bytes_ms(0) == 0.0
    assert batch.last_undict_bytes_ms(2) > 0.0 and batch.last_undict_bytes_ms(5) > 0.0


def test_item_edges(pkg, batch):
    """one element; 1023, 1024 and 1025 elements; an item edge inside an RLE run and inside a bit-packed group"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(71)
    entries = ref.random_entries(rnd, 32, [0, 1, 2, 5, 16, 17, 23])
    packed = lambda n: ("packed", [rnd.randrange(32) for _ in range(n)])
    plans = [[("rle", 1, 3)], [("rle", C - 1, 7)], [packed(C)], [packed(C - 8), ("rle", 9, 30)], [("rle", C - 4, 2), packed(16), ("rle", 2 * C, 9)],
             [("rle", 3, 1), packed(2 * C), ("rle", 5, 4)]]
    datas = [rle_ref.encode(p, 5) for p in plans]
    caps = [1, C - 1, C, C + 1, None, None]
    caps = [rle_ref.decode(d, 5, 8)[1][0] if c is None else c for d, c in zip(datas, caps)]
    got = _run(pkg, batch, *_table(rnd, datas, entries, 5, caps=caps))
    assert [min(r[0], c) for r, c in zip(got, caps)] == [1, C - 1, C, C + 1, 3 * C + 12, 2 * C + 8]


@pytest.mark.parametrize("length", [1, 5, 16, 17])
def test_item_boundaries_at_every_offset_within_a_word(pkg, batch, length):
    """entries of one length: with sixteen data skews the items' boundaries fall at every offset within a 16-byte word"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(72 + length)
    entries = ref.random_entries(rnd, 16, [length])
    data = rle_ref.encode([("packed", [rnd.randrange(16) for _ in range(2 * C + 8)]), ("rle", C // 2, 3)], 4)
    src, dictionary, segs, o_size, d_size = _table(rnd, [data] * 16, entries, 4, gap=(0,))
    segs = [s[:3] + (s[3] + j,) + s[4:] for j, s in enumerate(segs)]   # (the segments' bytes are a multiple of the length: j more each)
    assert {(s[3] + C * length * i) % 16 for s in segs for i in range(3)} == set(range(16)) or length == 16
    _run(pkg, batch, src, dictionary, segs, o_size, d_size + 16 * 16)


def test_all_skews_of_data_and_dictionary_and_both_offset_widths(pkg, batch):
    C = pkg.unrle_item_elems()
    rnd = random.Random(73)
    entries = ref.random_entries(rnd, 64, [0, 1, 3, 7, 15, 16, 17, 31, 33])
    data = rle_ref.encode(rle_ref.random_plan(rnd, 6, C + 300, packed=(8, 64), repeated=(1, 40)), 6)
    count = rle_ref.decode(data, 6, 8)[1][0]
    body = ref.column(data, 6, 0, ref.dictionary_bytes(entries))[1]
    blob = b"".join(b"\x55" * (1 + (16 - len(ref.dictionary_bytes(entries)) % 16)) + ref.dictionary_bytes(entries) for _ in range(16))
    step = len(blob) // 16
    assert step % 16 == 1
    segs, o_at, d_at = [], 0, 0
    for skew in range(16):
        flags = (ref.OFFSETS64 if skew & 1 else 0) | (ref.ENDS_ONLY if skew & 2 else 0)
        d_at = H.next_at(d_at, (5 - skew) % 16)
        o_at = H.next_at(o_at, (3 * skew) % 16)
        segs.append((0, len(data), o_at, d_at, len(body), count, 100 * skew, skew * step + step - len(ref.dictionary_bytes(entries)), len(ref.dictionary_bytes(entries)), ref.ALL, 6, flags))
        o_at += 8 * (count + 1); d_at += len(body)
    assert {s[7] % 16 for s in segs} == set(range(16))
    _run(pkg, batch, data, blob, segs, o_at + 64, d_at + 64)


def test_two_pages_appended_with_ends_only(pkg, batch):
    C = pkg.unrle_item_elems()
    rnd = random.Random(74)
    entries = ref.random_entries(rnd, 100, [0, 2, 9, 30])
    dictionary = ref.dictionary_bytes(entries)
    p1 = rle_ref.encode(rle_ref.random_plan(rnd, 7, C + 77, packed=(8, 64), repeated=(1, 40)), 7)
    p2 = rle_ref.encode(rle_ref.random_plan(rnd, 7, 500, packed=(8, 64), repeated=(1, 40)), 7)
    n1, n2 = rle_ref.decode(p1, 7, 8)[1][0], rle_ref.decode(p2, 7, 8)[1][0]
    o1, b1, _ = ref.column(p1, 7, 0, dictionary)
    o2, b2, _ = ref.column(p2, 7, 0, dictionary, offset_base=len(b1))
    segs = [(0, len(p1), 4, 1, len(b1), n1, 0, 0, len(dictionary), ref.ALL, 7, 0), (len(p1), len(p2), 4 + 4 * (n1 + 1), 1 + len(b1), len(b2), n2, len(b1), 0, len(dictionary), ref.ALL, 7, ref.ENDS_ONLY)]
    _run(pkg, batch, p1 + p2, dictionary, segs, 4 + 4 * (n1 + n2 + 1) + 32, 1 + len(b1) + len(b2) + 32)
    want_o = ref.offsets_bytes(o1 + o2[1:], 0)
    assert len(want_o) == 4 * (n1 + n2 + 1)   # (one Arrow array: what _run compared is exactly this behind byte 4)


def test_data_capacities_bad_indices_no_dictionary_and_a_cut_one(pkg, batch):
    C = pkg.unrle_item_elems()
    rnd = random.Random(75)
    entries = ref.random_entries(rnd, 50, [5, 11, 16, 3])
    values = [rnd.randrange(50) for _ in range(C + 40)]
    for at in (3, C - 1, C, C + 17):
        values[at] = 50 + rnd.randrange(14)
    data = rle_ref.encode([("packed", values), ("rle", 4, 0xFF)], 6)
    dictionary = ref.dictionary_bytes(entries)
    total = len(ref.column(data, 6, 0, dictionary)[1])
    first = len(entries[values[0]])
    datas, data_caps = [data] * 8, [0, 2, first, first + len(entries[values[1]]), 100, total - 1, total, total + 20]
    src, blob, segs, o_size, d_size = _table(rnd, datas, entries, 6, data_caps=data_caps)
    got = _run(pkg, batch, src, blob, segs, o_size, d_size)
    assert {r[5:8] for r in got} == {(8, 3, total)}
    # D = 0 -- no dictionary bytes --, and a dictionary cut inside an entry and inside a length
    for cut in (0, len(dictionary) - 1, len(dictionary) - len(entries[-1]) - 2):
        src, segs, o_size, d_size = ref.layout(rnd, [data], 0, cut, 6, dictionary=dictionary)
        got = _run(pkg, batch, src, dictionary, segs, o_size, d_size)
        assert got[0][8:] == ((0, 0, ref.DICT_OK) if cut == 0 else (49, len(dictionary) - len(entries[-1]) - 4, ref.DICT_CUT))


def test_a_segment_of_three_hundred_items_and_a_second_behind_it(pkg, batch):
    """the carry launch across items, blocks and segments; the hook is compared at its own, smaller shape elsewhere"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(76)
    entries = ref.random_entries(rnd, 4000, [0, 1, 2, 3, 4, 9])
    first = rle_ref.encode(rle_ref.random_plan(rnd, 12, 300 * C + 77, hlen=True), 12)
    second = rle_ref.encode(rle_ref.random_plan(rnd, 7, 9 * C + 5, packed=(8, 64), repeated=(1, 70)), 7, True)
    dictionary = ref.dictionary_bytes(entries)
    src, segs, o_size, d_size = ref.layout(rnd, [first], 0, len(dictionary), 12, ref.OFFSETS64, gap=(0,), dictionary=dictionary)
    src2, segs2, o2, d2 = ref.layout(rnd, [second], 0, len(dictionary), 7, ref.WIDTH_BYTE, gap=(0,), dictionary=dictionary)
    s = segs2[0]
    segs.append((len(src),) + s[1:2] + (o_size, d_size) + s[4:])
    got = _run(pkg, batch, src + second, dictionary, segs, o_size + o2, d_size + d2, hook=False)
    assert got[0][0] > 300 * C and got[0][5] > 0 and got[1][5] == 0 and got[1][4] == 7 and got[0][7] > 500000


def test_a_measuring_call_and_then_the_writing_call(pkg, batch):
    C = pkg.unrle_item_elems()
    rnd = random.Random(77)
    entries = ref.random_entries(rnd, 200, [0, 4, 21, 100])
    datas = [rle_ref.encode(rle_ref.random_plan(rnd, 8, n, packed=(8, 64), repeated=(1, 40)), 8) for n in (5, C + 9, 3 * C)]
    src, dictionary, segs, o_size, d_size = _table(rnd, datas, [e for e in entries], 8)
    measuring = [s[:2] + (ref.NONE, ref.NONE, 0) + s[5:] for s in segs]
    measured = _run(pkg, batch, src, dictionary, measuring, o_size, d_size)   # (nothing is written: both buffers are the sentinels)
    sized = [s[:4] + (m[7],) + s[5:] for s, m in zip(segs, measured)]
    assert _run(pkg, batch, src, dictionary, sized, o_size, d_size) == measured
    counted = batch.undict_bytes_segments([1] * 3, [0] * 3, None, None, None, [0] * 3, [3] * 3, None, None, None, None)
    assert counted == [(0, 0, 0, ref.OK, 3) + ZERO[5:]] * 3 and batch.last_undict_bytes_ms(1) == 0.0 and batch.last_undict_bytes_ms(5) == 0.0


def test_bad_arguments_launch_nothing(pkg, batch):
    d = _device(ref.sentinel(4096))
    p = d.data_ptr()
    args = lambda **kw: [kw.get(k, v) for k, v in (("src", [p]), ("lens", [10]), ("offsets", [p + 1024]), ("data", [p + 2048]), ("data_caps", [100]), ("caps", [8]), ("bits", [3]),
                                                  ("flags", [0]), ("bases", None), ("dicts", [p + 512]), ("dict_lens", [64]), ("dict_entries", None))]
    for kw, text in (({"flags": [16]}, "undict-bytes segment 0: unknown flag bits"), ({"flags": [ref.SKIP]}, "undict-bytes segment 0: unknown flag bits"),
                     ({"bits": [33]}, "undict-bytes segment 0: field of more than 32 bits"), ({"caps": [(1 << 56) + 1]}, r"undict-bytes segment 0: a capacity above 2\^56"),
                     ({"data": [None]}, "undict-bytes segment 0: no data destination for a data capacity that is not 0"),
                     ({"dicts": [None]}, "undict-bytes segment 0: no dictionary for bytes and a capacity that are not 0"),
                     ({"dict_lens": [1 << 32]}, r"undict-bytes segment 0: a dictionary of 2\^32 bytes or more"), ({"dicts": None, "dict_lens": None}, "invalid undict-bytes arguments")):
        with pytest.raises(RuntimeError, match=text):
            batch.undict_bytes_segments(*args(**kw))
        assert batch.last_undict_bytes_ms() == 0.0   # (nothing was launched)
    assert d.cpu().numpy().tobytes() == ref.sentinel(4096) + bytes(16)
    assert batch.undict_bytes_segments([], [], [], [], [], [], [], None, None, [], []) == []


# ------------------------------------------------------------------ the outputs of a decode call
class _Pages:
    """streams of one decode call: dictionary pages and the index page bodies that name them, and one dictionary outside the call"""

    def __init__(self):
        rnd = random.Random(78)
        self.dict_a, self.dict_b, self.outside = (ref.dictionary_bytes(ref.random_entries(rnd, n, lengths)) for n, lengths in ((300, [0, 1, 7, 20]), (70, [3, 40, 200]), (1000, [0, 2, 5])))

        def body(k, n, top):
            plan = [r[:2] + (r[2] % top,) if r[0] == "rle" else ("packed", [v % top for v in r[1]])
                    for r in rle_ref.random_plan(rnd, k, n, packed=(8, 504), repeated=(1, 2000))] if n else []
            return rle_ref.encode(plan, k, True)

        self.raws = [self.dict_a, body(9, 5000, 300), body(9, 1, 300), self.dict_b, body(7, 4096, 70), body(10, 3000, 1000), body(3, 0, 8), body(9, 20003, 310)]
        self.of = [None, 0, 0, None, 3, "outside", 0, 0]   # (the last one's indices reach 309: some are outside the dictionary)
        self.streams = [_stream(r) for r in self.raws]


@pytest.fixture(scope="module")
def pages():
    return _Pages()


def _check_outputs(pkg, b, pages, skip, delivered=None):
    """undict_bytes_outputs of the pages' streams into fresh sentinel buffers: offsets, bytes and results, the skipped streams' zeros; then a
    measuring call and a counting call, which write nothing; delivered: what the dictionary streams delivered, where that is not all of them"""
    n = len(pages.raws)
    delivered = delivered or {0: pages.dict_a, 3: pages.dict_b}
    d_out = _upload(pages.outside)
    want_res, cols = [], []
    for i, (raw, of) in enumerate(zip(pages.raws, pages.of)):
        if of is None or i in skip:
            want_res.append(ZERO); cols.append(None)
            continue
        count = rle_ref.decode(raw, 0, 8, 1)[1][0]
        offsets, body, res = ref.column(raw, 0, ref.WIDTH_BYTE | (ref.OFFSETS64 if i & 1 else 0), pages.outside if of == "outside" else delivered[of], ref.ALL, max(count, 1), 7 * i)
        want_res.append(res); cols.append((ref.offsets_bytes(offsets, ref.OFFSETS64 if i & 1 else 0), body))
    o_offs, o_size = H.slots([0 if c is None else len(c[0]) for c in cols], {i for i, c in enumerate(cols) if c is None})
    d_offs, d_size = H.slots([0 if c is None else len(c[1]) for c in cols], {i for i, c in enumerate(cols) if c is None}, start=9)
    want_o, want_d = bytearray(ref.sentinel(o_size)), bytearray(ref.sentinel(d_size, 7))
    for c, o, d in zip(cols, o_offs, d_offs):
        if c is not None:
            want_o[o:o + len(c[0])] = c[0]; want_d[d:d + len(c[1])] = c[1]
    d_o, d_d = _device(ref.sentinel(o_size)), _device(ref.sentinel(d_size, 7))
    op, dp = d_o.data_ptr(), d_d.data_ptr()
    flags = [ref.SKIP if c is None else ref.WIDTH_BYTE | (ref.OFFSETS64 if i & 1 else 0) for i, c in enumerate(cols)]
    caps = [0 if c is None else max(r[0], 1) for c, r in zip(cols, want_res)]
    dict_args = ([pkg.UNDICT_NO_STREAM if of in (None, "outside") else of for of in pages.of], [d_out.data_ptr() if of == "outside" else None for of in pages.of],
                 [len(pages.outside) if of == "outside" else 0 for of in pages.of])
    got = b.undict_bytes_outputs([None if o is None else op + o for o in o_offs], [None if d is None else dp + d for d in d_offs], [0 if c is None else len(c[1]) for c in cols],
                                 caps, [0] * n, flags, [7 * i for i in range(n)], *dict_args)
    assert got == want_res, [(i, a, c) for i, (a, c) in enumerate(zip(got, want_res)) if a != c][:3]
    both = lambda: (d_o[:o_size].cpu().numpy().tobytes(), d_d[:d_size].cpu().numpy().tobytes())
    assert both() == (bytes(want_o), bytes(want_d))
    assert b.measure_dict_bytes_outputs([None if c is None else k for c, k in zip(cols, caps)], [0] * n, *dict_args, flags=[ref.WIDTH_BYTE] * n) == want_res
    counted = b.undict_bytes_outputs(None, None, None, None, [0] * n, [ref.WIDTH_BYTE] * n)
    assert [r[:5] for r in counted[1:3]] == [rle_ref.decode(raw, 0, 8, 1)[1] for raw in pages.raws[1:3]] and all(r[5:] == ZERO[5:] for r in counted)
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
            b.undict_bytes_outputs(None, None, None, None, [0] * n)
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, c) for c in caps]
        got = _check_outputs(pkg, b, pages, skip={2})
        assert got[7][5] > 0 and got[1][5] == 0
        one = lambda i, j: b.undict_bytes_outputs(None, None, None, [1 if s == i else 0 for s in range(n)], [0] * n, [1] * n, None, [j if s == i else 0 for s in range(n)])
        with pytest.raises(RuntimeError, match="undict-bytes stream 1: its dictionary stream 1 is the stream itself"):
            one(1, 1)
        with pytest.raises(RuntimeError, match="undict-bytes stream 2: its dictionary stream 8 is none of the 8 streams"):
            one(2, 8)
    finally:
        b.close()


def test_outputs_of_decode_host_and_packed(pkg, pages):
    n = len(pages.raws)
    b = pkg.Batch(n)
    try:
        results, outs = b.decode_host(pages.streams, [len(r) for r in pages.raws], FLAGS)
        assert [r.result for r in results] == [1] * n and outs == pages.raws
        _check_outputs(pkg, b, pages, skip={1, 6})
        results, outs = b.decode_packed(pages.streams, flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(r)) for r in pages.raws]
        _check_outputs(pkg, b, pages, skip={4})
    finally:
        b.close()


def test_a_dictionary_stream_delivered_truncated(pkg, pages):
    """a dictionary stream given less room than it needs (with the eager limit): exactly its decoded_size bytes are the dictionary -- a shorter
    one, cut --, and the indices beyond it are bad"""
    import torch
    datas, caps = pages.streams, [len(r) for r in pages.raws]
    caps[0] = 1003
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    offs = [sum(caps[:i]) + 1 for i in range(len(caps))]
    arena = torch.from_numpy(np.frombuffer(ref.sentinel(sum(caps) + 4096), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS | EAGER)
        results = b.wait()
        assert [r.result for r in results] == [3] + [1] * (len(datas) - 1) and results[0].decoded_size == 1003
        got = _check_outputs(pkg, b, pages, skip=set(), delivered={0: pages.dict_a[:1003], 3: pages.dict_b})
        assert got[1][5] > 0 and got[1][8] < 300 and got[4][5] == 0
    finally:
        b.close()


def test_outputs_as_strings_on_the_pyarrow_pages(pkg):
    """the dictionary page and the data page that pyarrow wrote for every string column (tests/golden/string_pages/), each Brotli-compressed, in
    ONE decode call; outputs_as_strings gives the columns, and with pyarrow present an Arrow array over the buffers equals the column"""
    import torch
    import string_pages
    tensors = H.tensors_module()
    pages = string_pages.load()
    streams, specs = [], []
    for k, (e, dictionary, body, offsets, data) in enumerate(pages):
        streams += [_stream(dictionary), _stream(body)]
        specs += [None, (e["values"], len(streams) - 2) + (("large",) if k & 1 else ())]
    b = pkg.Batch(len(streams))
    try:
        results, _ = b.decode_packed(streams, flags=FLAGS)
        assert [r.result for r in results] == [1] * len(streams)
        got = tensors.outputs_as_strings(b, specs)
        assert all(g is None for g in got[0::2])
        for k, ((e, _, _, offsets, data), (o, d)) in enumerate(zip(pages, got[1::2])):
            assert o.is_cuda and d.is_cuda and o.dtype == (torch.int64 if k & 1 else torch.int32) and d.dtype == torch.uint8 and o.data_ptr() % 64 == 0 and d.data_ptr() % 64 == 0
            assert o.cpu().tolist() == np.frombuffer(offsets, dtype="<i4").tolist() and d.cpu().numpy().tobytes() == data, e["label"]
        try:
            import pyarrow as pa
        except ImportError:
            pa = None
        if pa is not None:
            for k, ((e, _, _, offsets, data), (o, d)) in enumerate(zip(pages, got[1::2])):
                typ = {("string", 0): pa.string(), ("string", 1): pa.large_string(), ("binary", 0): pa.binary(), ("binary", 1): pa.large_binary()}[(e["type"], k & 1)]
                arr = pa.Array.from_buffers(typ, e["values"], [None, pa.py_buffer(o.cpu().numpy().tobytes()), pa.py_buffer(d.cpu().numpy().tobytes())])
                o32 = np.frombuffer(offsets, dtype="<i4")
                assert arr.to_pylist() == [(data[o32[r]:o32[r + 1]].decode() if e["type"] == "string" else data[o32[r]:o32[r + 1]]) for r in range(e["values"])], e["label"]
        # the dictionary as a tensor of the caller's
        e, dictionary, body, offsets, data = pages[2]
        o, d = tensors.outputs_as_strings(b, [None] * 5 + [(e["values"], _upload(dictionary)[:len(dictionary)])] + [None] * (len(streams) - 6))[5]
        assert o.cpu().tolist() == np.frombuffer(offsets, dtype="<i4").tolist() and d.cpu().numpy().tobytes() == data
    finally:
        b.close()


def test_every_value_error_of_outputs_as_strings(pkg):
    tensors = H.tensors_module()
    rnd = random.Random(79)
    entries = ref.random_entries(rnd, 8, [0, 3, 9])
    dictionary = ref.dictionary_bytes(entries)
    good = rle_ref.encode([("packed", [0, 1, 2, 3, 4, 5, 6, 7]), ("rle", 12, 3)], 3, True)
    bad_index = rle_ref.encode([("rle", 5, 1), ("rle", 2, 9), ("rle", 13, 0)], 4, True)
    raws = [dictionary, good, good + b"\x82", b"\x21" + good[1:], bad_index, dictionary[:-2]]
    b = pkg.Batch(len(raws))
    try:
        results, _ = b.decode_packed([_stream(r) for r in raws], flags=FLAGS)
        assert [r.result for r in results] == [1] * len(raws)
        only = lambda i, spec: [spec if s == i else None for s in range(len(raws))]
        o, d = tensors.outputs_as_strings(b, only(1, (20, 0)))[1]
        assert o.cpu().tolist() == ref.column(good, 0, 1, dictionary)[0] and d.cpu().numpy().tobytes() == ref.column(good, 0, 1, dictionary)[1]
        assert tensors.outputs_as_strings(b, only(1, (17, 0)))[1][0].numel() == 18   # more values than rows: padding, not judged
        assert tensors.outputs_as_strings(b, only(1, (0, 0)))[1][0].cpu().tolist() == [0]
        for i, spec, text in ((2, (20, 0), r"stream 2: runs that the stream's end cuts \(status 3\)"), (3, (20, 0), r"stream 3: a width byte that is none \(status 4\)"),
                              (1, (21, 0), "stream 1: 20 values in its runs, but the column has 21 rows"), (1, (20, 5), "stream 1: its dictionary is cut: 7 whole entries in"),
                              (4, (20, 0), "stream 4: 2 of its 20 values have an index outside its dictionary of 8 entries, the first of them value 5"),
                              (1, (20, 1), "stream 1: its dictionary stream 1 is the stream itself"), (1, (20, 6), "stream 1: its dictionary stream 6 is none of the 6 streams"),
                              (1, (20, -1), "stream 1: its dictionary stream -1 is none of the 6 streams"), (1, (20, 0, "big"), "stream 1: a spec is"),
                              (1, (20, "0"), r"stream 1: \(rows, j\) names the stream")):
            with pytest.raises(ValueError, match=text):
                tensors.outputs_as_strings(b, only(i, spec))
        with pytest.raises(ValueError, match="specs: 2 entries for the 6 streams"):
            tensors.outputs_as_strings(b, [None, None])
    finally:
        b.close()


def test_more_bytes_than_int32_offsets_hold(pkg):
    """bytes > 2^31 - 1 without "large" is refused by the measuring call's result alone: nothing of that size is allocated"""
    tensors = H.tensors_module()
    dictionary = ref.dictionary_bytes([b"x" * 70000])
    body = rle_ref.encode([("rle", 31000, 0)], 0, True)   # 31 000 x 70 000 bytes
    b = pkg.Batch(2)
    try:
        results, _ = b.decode_packed([_stream(dictionary), _stream(body)], flags=FLAGS)
        assert [r.result for r in results] == [1, 1]
        assert b.measure_dict_bytes_outputs([None, 31000], [0, 0], [0, 0], flags=[0, 1])[1][7] == 31000 * 70000 > (1 << 31) - 1
        with pytest.raises(ValueError, match=r"stream 1: 2170000000 bytes of strings, more than int32 offsets hold: ask for \"large\""):
            tensors.outputs_as_strings(b, [None, (31000, 0)])
    finally:
        b.close()
