"""Undlba on the device (needs a real MI355X): the kernels (csrc/brotli_undlba_kernels.hip) through BrotliAmdBatchUndlbaSegments,
BrotliAmdBatchUndlbaOutputs after the three kinds of decode call, and tensors.outputs_as_strings, against the reference (dlba_ref.py) AND against
the host hook.  Offsets and data each come from a buffer prefilled with a sentinel pattern, and the WHOLE buffers are compared with the
expectation: a byte written outside a segment's offsets or bytes fails the test.  Bad inputs are lengths and bounds that the contract answers
with a status, never with an address.  All comparisons are exact."""
import random

import numpy as np
import pytest

import dbp_ref
import dlba_ref as ref
import seg_filter_harness as H
from seg_filter_harness import stream as _stream, upload as _upload

pytestmark = pytest.mark.gpu
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT
ZERO = (0, 0, 0, 0, 0, 0, 0, 0, 0, ref.NONE, 0, 0)   # a skipped stream's result


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
    """one undlba_segments call over the hook's kind of table into fresh sentinel buffers: results and both WHOLE buffers against the reference,
    and against the host hook -> the results"""
    want_o, want_d, want_res = ref.expected(src, segs, o_size, d_size)
    d_src, d_o, d_d = _upload(src), _device(ref.sentinel(o_size)), _device(ref.sentinel(d_size, 7))
    sp, op, dp = d_src.data_ptr(), d_o.data_ptr(), d_d.data_ptr()
    got = batch.undlba_segments([sp + s[0] for s in segs], [s[1] for s in segs], [None if s[2] == ref.NONE else op + s[2] for s in segs],
                                [None if s[3] == ref.NONE else dp + s[3] for s in segs], [s[4] for s in segs], [s[5] for s in segs], [s[7] for s in segs], [s[6] for s in segs])
    got_o, got_d = d_o[:o_size].cpu().numpy().tobytes(), d_d[:d_size].cpu().numpy().tobytes()
    assert got == want_res, [(i, a, b) for i, (a, b) in enumerate(zip(got, want_res)) if a != b][:3]
    assert got_o == want_o, ("offsets", ref.first_difference(got_o, want_o))
    assert got_d == want_d, ("data", ref.first_difference(got_d, want_d))
    if hook:
        hook_o, hook_d, hook_res = pkg.undlba_host(src, segs, o_size, d_size, offsets_fill=ref.sentinel(o_size), data_fill=ref.sentinel(d_size, 7), **hook_kw)
        assert (hook_res, hook_o, hook_d) == (got, got_o, got_d)
    return got


def _strings(rnd, n, lengths=(0, 1, 2, 3, 7, 16, 17, 40)):
    return ref.random_strings(rnd, n, list(lengths))


def test_the_five_examples_in_one_call(pkg, batch):
    src, segs, o_size, d_size = ref.layout(random.Random(2), [p[0] for p in ref.PINNED], caps=[5] * 5)
    assert _run(pkg, batch, src, segs, o_size, d_size) == [p[3] for p in ref.PINNED]
    for (body, offsets, data, _), s in zip(ref.PINNED, segs):   # (what _run compared, said once more by hand)
        assert ref.expected(src, segs, o_size, d_size)[0][s[2]:s[2] + 4 * len(offsets)] == ref.offsets_bytes(offsets, 0)


def test_item_edges(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(81)
    counts = (1, 2, C, C + 1, C + 2, 2 * C + 1)
    bodies = [ref.encode(_strings(rnd, n, (0, 1, 2, 3, 9))) for n in counts]
    for flags in (0, ref.OFFSETS64 | ref.ENDS_ONLY):
        got = _run(pkg, batch, *ref.layout(rnd, bodies, flags), order_seed=3)
        assert [r[0] for r in got] == list(counts)
    # capacities at the edges too: only bad, first_bad and bytes depend on them
    got = _run(pkg, batch, *ref.layout(rnd, [bodies[5]] * 6, caps=[1, 2, C, C + 1, C + 2, 2 * C + 9]))
    assert len({r[:8] + r[11:] for r in got}) == 1 and [r[10] for r in got] == sorted(r[10] for r in got) and got[0][10] < got[4][10] < got[5][10]


@pytest.mark.parametrize("length", [1, 5, 16, 17])
def test_item_boundaries_at_every_offset_within_a_word(pkg, batch, length):
    """values of one length under sixteen data skews: the copy's words and the items' offsets meet every offset within a 16-byte word"""
    C = pkg.undbp_item_deltas()
    rnd = random.Random(82 + length)
    body = ref.encode(_strings(rnd, 2 * C + 8, (length,)))
    src, segs, o_size, d_size = ref.layout(rnd, [body] * 16, gap=(0,))
    segs = [s[:3] + (s[3] + j,) + s[4:] for j, s in enumerate(segs)]   # (the segments' bytes are a multiple of the length: j more each)
    assert {s[3] % 16 for s in segs} == set(range(16)) or length == 16
    _run(pkg, batch, src, segs, o_size, d_size + 16 * 16)


def test_all_skews_of_source_and_offsets_at_both_widths(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(83)
    body = ref.encode(_strings(rnd, C + 300))
    count = C + 300
    data_len = len(ref.column(body, count)[1])
    src, segs, o_at, d_at = bytearray(), [], 0, 0
    for skew in range(16):
        for flags in (0, ref.OFFSETS64, ref.ENDS_ONLY, ref.OFFSETS64 | ref.ENDS_ONLY):
            src += b"\xc3" * (H.next_at(len(src), skew) - len(src))
            o_at = H.next_at(o_at, (3 * skew + flags) % 16)
            segs.append((len(src), len(body), o_at, d_at, data_len, count, 100 * skew, flags))
            src += body
            o_at += 8 * (count + 1); d_at += data_len + 1
    assert {s[0] % 16 for s in segs} == set(range(16)) and {s[2] % 16 for s in segs} == set(range(16))
    _run(pkg, batch, bytes(src), segs, o_at + 64, d_at + 64)


def test_two_pages_appended_with_ends_only(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(84)
    p1, p2 = ref.encode(_strings(rnd, C + 77)), ref.encode(_strings(rnd, 500))
    n1, n2 = C + 77, 500
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
    assert {r[4] for r in got} == {ref.OK, ref.BAD_HEADER, ref.BAD_WIDTH, ref.TRUNCATED}   # every status
    assert any(r[7] == ref.DATA_SHORT for r in got) and any(r[8] for r in got)
    assert batch.last_undlba_ms() > 0.0
    assert all(batch.last_undlba_ms(p) >= 0.0 for p in range(1, 8)) and batch.last_undlba_ms(8) == 0.0 and batch.last_undlba_ms(0) == 0.0
    assert all(batch.last_undlba_ms(p) > 0.0 for p in (1, 2, 4, 6, 7))
    assert abs(sum(batch.last_undlba_ms(p) for p in range(1, 8)) - batch.last_undlba_ms()) < 0.05 * batch.last_undlba_ms() + 0.01


def test_a_segment_of_three_hundred_items_and_a_second_behind_it(pkg, batch):
    """the carry launches' later passes, across items, blocks and segments; the hook is compared at its own, smaller shapes elsewhere"""
    C = pkg.undbp_item_deltas()
    rng = np.random.default_rng(85)
    lens = rng.integers(0, 4, size=300 * C + 77)
    first = dbp_ref.encode([int(v) for v in lens], 1024, 8) + rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
    rnd = random.Random(85)
    second = ref.encode(_strings(rnd, 9 * C + 5, (0, 1, 2, 3)), B=256, M=4)
    src, segs, o_size, d_size = ref.layout(rnd, [first, second], ref.OFFSETS64, gap=(0,))
    got = _run(pkg, batch, src, segs, o_size, d_size, hook=False)
    assert got[0][0] == 300 * C + 77 and got[1][0] == 9 * C + 5 and got[0][10] == int(lens.sum()) and all(r[7] == ref.DATA_OK and r[10] == r[11] for r in got)


def test_long_strings_among_short_ones(pkg, batch):
    """one segment of 2048 strings of 4 KiB among short ones: the data is the ragged copy's, spread over many blocks"""
    rng = np.random.default_rng(86)
    lens = [4096 if i % 3 == 1 else int(v) for i, v in enumerate(rng.integers(0, 6, size=3 * 2048))]
    assert lens.count(4096) == 2048
    body = dbp_ref.encode(lens) + rng.integers(0, 256, size=sum(lens), dtype=np.uint8).tobytes()
    rnd = random.Random(86)
    src, segs, o_size, d_size = ref.layout(rnd, [ref.encode(_strings(rnd, 40)), body, ref.encode(_strings(rnd, 3))], gap=(1,))
    got = _run(pkg, batch, src, segs, o_size, d_size, hook=False)
    assert got[1][10] == got[1][11] == sum(lens) > 8 << 20


def test_negative_lengths_in_three_items(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(87)
    strings = _strings(rnd, 3 * C + 50, (1, 2, 3))
    lengths = [len(s) for s in strings]
    bad_at = [0, 7, C, C + 1, 2 * C + 1000, 3 * C + 49]
    for e in bad_at:
        lengths[e] = -1 - rnd.randrange(1 << 20)
    lengths[C + 9] += 3 << 32   # (upper bits that are not looked at)
    body = ref.encode(strings, lengths)
    got = _run(pkg, batch, *ref.layout(rnd, [body] * 3, caps=[3 * C + 50, 2 * C, C + 1]))
    assert [r[8:10] for r in got] == [(6, 0), (4, 0), (3, 0)]
    assert got[0][10] == sum(v for v in lengths if v >= 0) - (3 << 32) and got[0][7] == ref.DATA_OK
    # the first bad one in a later item alone
    lengths[0], lengths[7] = len(strings[0]), len(strings[7])
    assert _run(pkg, batch, *ref.layout(rnd, [ref.encode(strings, lengths)]))[0][8:10] == (4, C)


def test_data_short_data_capacities_and_every_status(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(88)
    strings = _strings(rnd, C + 40, (0, 3, 5, 11))
    body = ref.encode(strings)
    total = sum(len(s) for s in strings)
    # the data short by a byte and by everything, and bytes left over
    bodies = [body[:-1], body[:len(body) - total], body + b"left over"]
    got = _run(pkg, batch, *ref.layout(rnd, bodies, ref.OFFSETS64))
    assert [(r[7], r[10], r[11]) for r in got] == [(ref.DATA_SHORT, total, total - 1), (ref.DATA_SHORT, total, 0), (ref.DATA_OK, total, total + 9)]
    # data capacities: the cut is exact to the byte, and nothing in the result depends on it
    data_caps = [0, 1, 15, 16, 17, 100, total - 1, total, total + 20]
    got = _run(pkg, batch, *ref.layout(rnd, [body] * len(data_caps), data_caps=data_caps))
    assert len(set(got)) == 1
    # every status, with the data at `consumed` whatever it is
    front = dbp_ref.encode([len(s) for s in strings[:129]], declared=129 + 200)
    stopped = [front + stop + b"".join(strings[:129]) for _, stop, _, _, _ in dbp_ref.stops()] + [front + stop for _, stop, _, _, _ in dbp_ref.stops()] + [b"\x40\x04\x05\x00abc", b"", body]
    got = _run(pkg, batch, *ref.layout(rnd, stopped, caps=[400] * len(stopped)))
    assert {r[4] for r in got} == {ref.OK, ref.BAD_HEADER, ref.BAD_WIDTH, ref.TRUNCATED}
    assert [r[4] for r in got[6:12]] == [status for _, _, status, _, _ in dbp_ref.stops()]


def test_measuring_and_counting_calls(pkg, batch):
    C = pkg.undbp_item_deltas()
    rnd = random.Random(89)
    bodies = [ref.encode(_strings(rnd, n)) for n in (5, C + 9, 3 * C)]
    src, segs, o_size, d_size = ref.layout(rnd, bodies)
    measuring = [s[:2] + (ref.NONE, ref.NONE, 0) + s[5:] for s in segs]
    measured = _run(pkg, batch, src, measuring, o_size, d_size)   # (nothing is written: both buffers are the sentinels)
    assert all(batch.last_undlba_ms(p) > 0.0 for p in (1, 2, 4, 6))   # (the same launches)
    sized = [s[:4] + (m[10],) + s[5:] for s, m in zip(segs, measured)]
    assert _run(pkg, batch, src, sized, o_size, d_size) == measured
    counting = [s[:4] + (0, 0) + s[6:] for s in segs]
    counted = _run(pkg, batch, src, counting, o_size, d_size)
    assert [c[:8] + c[11:] for c in counted] == [m[:8] + m[11:] for m in measured] and all(c[8:11] == (0, ref.NONE, 0) for c in counted)
    assert batch.last_undlba_ms(1) > 0.0 and all(batch.last_undlba_ms(p) == 0.0 for p in range(2, 8)) and batch.last_undlba_ms() == batch.last_undlba_ms(1)
    # without any array of destinations
    d_src = _upload(src)
    assert batch.undlba_segments([d_src.data_ptr() + s[0] for s in segs], [s[1] for s in segs], None, None, None, [0] * 3) == counted
    assert batch.undlba_segments([d_src.data_ptr() + s[0] for s in segs], [s[1] for s in segs], None, None, None, [s[5] for s in segs]) == measured


def test_bad_arguments_launch_nothing(pkg, batch):
    d = _device(ref.sentinel(4096))
    p = d.data_ptr()
    args = lambda **kw: [kw.get(k, v) for k, v in (("src", [p]), ("lens", [10]), ("offsets", [p + 1024]), ("data", [p + 2048]), ("data_caps", [100]), ("caps", [8]), ("flags", [0]),
                                                  ("bases", None))]
    for kw, text in (({"flags": [16]}, "undlba segment 0: unknown flag bits"), ({"flags": [1]}, "undlba segment 0: unknown flag bits"),
                     ({"flags": [ref.SKIP]}, "undlba segment 0: BROTLI_AMD_UNDLBA_SKIP is for the outputs of a decode call"),
                     ({"caps": [(1 << 56) + 1]}, r"undlba segment 0: a capacity above 2\^56"),
                     ({"data": [None]}, "undlba segment 0: no data destination for a data capacity that is not 0"),
                     ({"data": None}, "undlba segment 0: no data destination for a data capacity that is not 0")):
        with pytest.raises(RuntimeError, match=text):
            batch.undlba_segments(*args(**kw))
        assert batch.last_undlba_ms() == 0.0   # (nothing was launched)
    assert d.cpu().numpy().tobytes() == ref.sentinel(4096) + bytes(16)
    assert batch.undlba_segments([], [], [], [], [], []) == []


# ------------------------------------------------------------------ the outputs of a decode call
class _Pages:
    """streams of one decode call: page bodies of several shapes, an empty one, one with a negative length, one cut, and streams that are no
    such pages"""

    def __init__(self, pkg):
        C = pkg.undbp_item_deltas()
        rnd = random.Random(90)
        strings = _strings(rnd, 300, (1, 2, 3))
        lengths = [len(s) for s in strings]
        lengths[250] = -4
        self.raws = [ref.encode(_strings(rnd, 5000)), b"not a page at all, just some bytes" * 40, ref.encode(_strings(rnd, 1)), ref.encode([]),
                     ref.encode(_strings(rnd, C + 9, (0, 5, 9)), B=256, M=8), ref.encode(strings, lengths), ref.encode(_strings(rnd, 700))[:-100], ref.encode(_strings(rnd, 2 * C + 1, (0, 1, 40)))]
        self.streams = [_stream(r) for r in self.raws]


@pytest.fixture(scope="module")
def pages(pkg):
    return _Pages(pkg)


def _check_outputs(b, pages, skip, delivered=None):
    """undlba_outputs of the pages' streams into fresh sentinel buffers: offsets, bytes and results, the skipped streams' zeros; then a measuring
    call and a counting call, which write nothing; delivered: what the streams delivered, where that is not all of them"""
    n = len(pages.raws)
    raws = [(delivered or {}).get(i, raw) for i, raw in enumerate(pages.raws)]
    want_res, cols = [], []
    for i, raw in enumerate(raws):
        if i in skip:
            want_res.append(ZERO); cols.append(None)
            continue
        flags = (ref.OFFSETS64 if i & 1 else 0) | (ref.ENDS_ONLY if i & 2 else 0)
        count = dbp_ref.decode(raw, 8, 0)[1][0]
        offsets, data, res = ref.column(raw, max(count, 1), 7 * i)
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
    caps = [0 if c is None else max(r[0], 1) for c, r in zip(cols, want_res)]
    got = b.undlba_outputs([None if o is None else op + o for o in o_offs], [None if d is None else dp + d for d in d_offs], [0 if c is None else len(c[1]) for c in cols],
                           caps, flags, [7 * i for i in range(n)])
    assert got == want_res, [(i, a, c) for i, (a, c) in enumerate(zip(got, want_res)) if a != c][:3]
    both = lambda: (d_o[:o_size].cpu().numpy().tobytes(), d_d[:d_size].cpu().numpy().tobytes())
    assert both() == (bytes(want_o), bytes(want_d))
    assert b.measure_dlba_outputs([None if c is None else k for c, k in zip(cols, caps)]) == want_res
    counted = b.count_dlba_outputs()
    assert [r[:8] + r[11:] for r in counted] == [ref.column(raw, 0)[2][:8] + ref.column(raw, 0)[2][11:] for raw in raws] and all(r[8:11] == ZERO[8:11] for r in counted)
    assert b.count_dlba_outputs(flags) == [ZERO if c is None else r for c, r in zip(cols, counted)]
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
            b.count_dlba_outputs()
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, c) for c in caps]
        got = _check_outputs(b, pages, skip={2})
        assert got[5][8:10] == (1, 250) and got[6][7] == ref.DATA_SHORT and got[3][0] == 0 and got[1][4] != ref.OK
        with pytest.raises(RuntimeError, match="undlba stream 4: unknown flag bits"):
            b.undlba_outputs(None, None, None, [0] * n, [0, 0, 0, 0, 1, 0, 0, 0])
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


def test_a_stream_delivered_truncated(pkg, pages):
    """a page given less room than it needs (with the eager limit): exactly its decoded_size bytes are the segment -- its lengths are whole and
    its data is short"""
    import torch
    datas, caps = pages.streams, [len(r) for r in pages.raws]
    caps[0] = len(pages.raws[0]) - 1000
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    offs = [sum(caps[:i]) + 1 for i in range(len(caps))]
    arena = torch.from_numpy(np.frombuffer(ref.sentinel(sum(caps) + 4096), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS | EAGER)
        results = b.wait()
        assert [r.result for r in results] == [3] + [1] * (len(datas) - 1) and results[0].decoded_size == caps[0]
        got = _check_outputs(b, pages, skip=set(), delivered={0: pages.raws[0][:caps[0]]})
        assert got[0][0] == 5000 and got[0][7] == ref.DATA_SHORT and got[0][10] == got[0][11] + 1000
    finally:
        b.close()


def test_outputs_as_strings_on_the_pyarrow_pages(pkg):
    """the data page that pyarrow wrote for every DELTA_LENGTH_BYTE_ARRAY column (tests/golden/dlba_pages/), each Brotli-compressed, in ONE decode
    call; outputs_as_strings gives the columns, and with pyarrow present an Arrow array over the buffers equals the column"""
    import torch
    import dlba_pages
    tensors = H.tensors_module()
    pages = dlba_pages.load()
    streams = [_stream(body) for _, body, _, _ in pages]
    specs = [("dlba", e["values"]) + (("large",) if k & 1 else ()) for k, (e, _, _, _) in enumerate(pages)]
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


def test_outputs_as_strings_with_a_dictionary_spec_in_the_same_call(pkg):
    import dict_bytes_ref
    import dlba_pages
    import string_pages
    tensors = H.tensors_module()
    e1, dictionary, body1, offsets1, data1 = string_pages.load()[2]
    e2, body2, offsets2, data2 = dlba_pages.load()[2]
    b = pkg.Batch(4)
    try:
        results, _ = b.decode_packed([_stream(body2), _stream(dictionary), _stream(body1), _stream(ref.encode([]))], flags=FLAGS)
        assert [r.result for r in results] == [1] * 4
        got = tensors.outputs_as_strings(b, [("dlba", e2["values"], "large"), None, (e1["values"], 1), ("dlba", 0)])
        assert got[1] is None
        assert got[0][0].cpu().tolist() == np.frombuffer(offsets2, dtype="<i4").tolist() and got[0][1].cpu().numpy().tobytes() == data2
        assert got[2][0].cpu().tolist() == np.frombuffer(offsets1, dtype="<i4").tolist() and got[2][1].cpu().numpy().tobytes() == data1
        assert got[3][0].cpu().tolist() == [0] and got[3][1].numel() == 0
        assert len({t.untyped_storage().data_ptr() for pair in (got[0], got[2], got[3]) for t in pair}) == 1   # ONE buffer
        assert dict_bytes_ref.column(body1, 0, 1, dictionary, cap=e1["values"])[1] == data1
    finally:
        b.close()


def test_every_new_value_error_of_outputs_as_strings(pkg):
    tensors = H.tensors_module()
    rnd = random.Random(91)
    strings = _strings(rnd, 20, (1, 3, 9))
    total = sum(len(s) for s in strings)
    lengths = [len(s) for s in strings]
    negative = list(lengths)
    negative[5], negative[11] = -1, -9
    good = ref.encode(strings)
    raws = [good, good[:7], ref.encode(strings, negative), good + b"xy", good[:-3], b"\x40\x04\x05\x00" + good]
    b = pkg.Batch(len(raws))
    try:
        results, _ = b.decode_packed([_stream(r) for r in raws], flags=FLAGS)
        assert [r.result for r in results] == [1] * len(raws)
        only = lambda i, spec: [spec if s == i else None for s in range(len(raws))]
        o, d = tensors.outputs_as_strings(b, only(0, ("dlba", 20)))[0]
        assert o.cpu().tolist() == ref.column(good)[0] and d.cpu().numpy().tobytes() == b"".join(strings)
        for i, spec, text in ((1, ("dlba", 20), r"stream 1: blocks that the stream's end cuts \(status 3\) after 1 lengths in 5 of its 7 delivered bytes, of 20 declared"),
                              (5, ("dlba", 20), r"stream 5: a header that is none \(status 1\)"),
                              (0, ("dlba", 21), "stream 0: 20 lengths in its stream, but the column has 21 rows"),
                              (0, ("dlba", 19), "stream 0: 20 lengths in its stream, but the column has 19 rows"),
                              (2, ("dlba", 20), "stream 2: 2 of its 20 lengths are negative, the first of them value 5"),
                              (3, ("dlba", 20), "stream 3: its lengths add up to %d bytes and %d are there: bytes are left over" % (total, total + 2)),
                              (4, ("dlba", 20), "stream 4: its lengths add up to %d bytes and %d are there: the data is short" % (total, total - 3)),
                              (0, ("dlba", 20, "big"), r"stream 0: a \"dlba\" spec is"), (0, ("dlba", -1), r"stream 0: a \"dlba\" spec is"),
                              (0, ("dlba",), r"stream 0: a \"dlba\" spec is")):
            with pytest.raises(ValueError, match=text):
                tensors.outputs_as_strings(b, only(i, spec))
    finally:
        b.close()
