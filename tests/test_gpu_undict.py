"""Undict on the device (needs a real MI355X): the kernels (csrc/brotli_undict_kernels.hip) through BrotliAmdBatchUndictSegments,
BrotliAmdBatchUndictOutputs after the three kinds of decode call, and tensors.outputs_as_tensors, against the reference (dict_ref.py) and against
the host hook.  Destinations come from one buffer prefilled with a sentinel pattern, and the WHOLE destination buffer is compared with the
expectation: a byte written outside a segment's elements fails the test.  A dictionary is the FRONT of a larger allocation whose rest holds the
sentinel (or other dictionaries' seeded bytes), and every out-of-range index stays below that allocation's entries: a wrong bound check shows as
a value that is not 0 in the destination, not as a stray read.  All comparisons are exact."""
import random

import numpy as np
import pytest

import dict_ref as ref
import rle_ref
import seg_filter_harness as H
from seg_filter_harness import fresh_dst as _fresh_dst, pack as _pack, stream as _stream, upload as _upload

pytestmark = pytest.mark.gpu
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT
LAYOUT = ("src", "len", "dst", "cap", "bits", "w", "flags", "dict", "D")
ZERO = (0, 0, 0, 0, 0, 0, ref.NONE)   # a skipped stream's result


@pytest.fixture(scope="module")
def table():
    """the table of the tests without a device, with fields of up to 10 bits -> (source, dictionary buffer, segments, destination size)"""
    return ref.short_table(max_k=10)


@pytest.fixture(scope="module")
def sentinel():
    return H.sentinel(4 << 20)


@pytest.fixture(scope="module")
def dev(table, sentinel):
    return H.device_buffers(np.frombuffer(table[0], dtype=np.uint8), sentinel)


@pytest.fixture(scope="module")
def batch(pkg):
    b = pkg.Batch(1)   # (the number of segments is not bound by max_streams)
    yield b
    b.close()


def _room(dictionary, total, sentinel):
    """the dictionary's bytes as the front of an allocation of `total` bytes whose rest holds the sentinel -> (the bytes, the device's copy)"""
    assert len(dictionary) <= total
    room = bytes(dictionary) + sentinel[:total - len(dictionary)].tobytes()
    return room, _upload(room)


def _undict(batch, dev, src, sentinel, segs, size, room, d_src=None):
    """segs: [(source offset, source length, destination offset, cap, bits, width, flags, dictionary offset, entries)], the dictionaries at their
    offsets in room = (the bytes, the device's copy) -> one call into a fresh destination of `size` bytes, the whole destination and all
    results compared"""
    src, (room_bytes, d_room) = bytes(src), room
    assert all(t + max(D, 1 << min(k, 17) if not f else 0) * w <= len(room_bytes) for _, _, _, _, k, w, f, t, D in segs)
    tp = d_room.data_ptr()
    call = lambda sp, sl, dp, caps, bits, ws, flags, toffs, Ds: batch.undict_segments(sp, sl, dp, caps, bits, ws, flags, [tp + t for t in toffs], Ds)
    elements = lambda data, k, w, f, t, D, cap: ref.elements_bytes(data, k, w, f, room_bytes[t:], D, cap)
    return H.counted_call(call, elements, LAYOUT, dev, src, _upload(src) if d_src is None else d_src, sentinel, segs, size)


def test_three_thousand_short_segments_and_the_host_hook(pkg, batch, dev, table, sentinel):
    """more than two chunks of a thousand segments, every shape, every ending, every alignment of source, destination and dictionary, dictionaries
    larger and smaller than their indices; the kernels' results and bytes are the host hook's"""
    src, dictionary, segs, size = table
    assert {s[0] % 16 for s in segs} == set(range(16)) and {s[2] % 16 for s in segs} == set(range(16)) and {s[7] % 16 for s in segs} == set(range(16))
    got = _undict(batch, dev, src, sentinel, segs, size, (dictionary, _upload(dictionary)), d_src=dev["src"])
    assert sum(1 for r in got if r[5]) > 300 and sum(1 for r in got if r[0] and not r[5]) > 300
    assert batch.last_undict_ms() > 0.0
    assert all(batch.last_undict_ms(p) > 0.0 for p in (1, 2)) and batch.last_undict_ms(3) == 0.0
    hook_dst, hook_res = pkg.undict_host(src, dictionary, segs, size, fill=sentinel[:size].tobytes())
    assert hook_res == got
    assert hook_dst == dev["dst"][:size].cpu().numpy().tobytes()


def test_one_long_segment_and_a_second_behind_it(pkg, batch, dev, sentinel):
    """a segment of 300 items, which several blocks share, and a second one of another shape right behind it in the source and in the
    destination; then both at destinations that are no multiple of the width"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(51)
    first = rle_ref.encode(rle_ref.random_plan(rnd, 12, 300 * C + 77, hlen=True), 12)
    second = rle_ref.encode(rle_ref.random_plan(rnd, 7, 9 * C + 5, packed=(8, 64), repeated=(1, 70)), 7, True)
    src, offs = _pack([first, second], start=5, gap=lambda i: 0)
    counts = [rle_ref.decode(first, 12, 8)[1][0], rle_ref.decode(second, 0, 8, 1)[1][0]]
    assert counts[0] > 300 * C
    room = _room(ref.random_dictionary(rnd, 4000, 4) + ref.random_dictionary(rnd, 128, 1), 4096 * 4 + 256, sentinel)   # (96 of the 12-bit indices are bad)
    d1 = 12 + 4 * counts[0]
    for skew in (0, 1):
        segs = [(offs[0], len(first), 12 + skew, counts[0], 12, 4, 0, 0, 4000), (offs[1], len(second), d1 + skew, counts[1], 0, 1, ref.WIDTH_BYTE, 16000, 128)]
        got = _undict(batch, dev, src, sentinel, segs, d1 + counts[1] + 64, room)
        assert got[0][3] == got[1][3] == ref.OK and got[1][4] == 7 and got[0][5] > 0 and got[1][5] == 0


def test_more_than_64_runs_in_one_item(pkg, batch, dev, sentinel):
    """items of several batches of 64 runs, every batch's edge inside one lane's 16 elements, at every width and at destination skews 0 and 1;
    a dictionary of 400 entries under 9-bit indices: bad and first_bad come from more than one batch"""
    C, k, D = pkg.unrle_item_elems(), 9, 400
    plan = ref.many_runs_plan(61)
    assert max(ref.runs_per_item(plan, C)) > 64
    data = rle_ref.encode(plan, k)
    count = rle_ref.decode(data, k, 8)[1][0]
    assert count == len(rle_ref.plan_values(plan)) == 2880
    src, offs = _pack([data])
    d_src = _upload(src)
    room = _room(ref.random_dictionary(random.Random(62), D, 8), (1 << k) * 8 + 64, sentinel)
    segs, d_at = [], 0
    for skew in (0, 1):
        for w in ref.WIDTHS:
            d_at = H.next_at(d_at, skew)
            segs.append((offs[0], len(data), d_at, count, k, w, 0, 0, D))
            d_at += count * w
    got = _undict(batch, dev, src, sentinel, segs, d_at + 64, room, d_src=d_src)
    assert all(r[:4] == (count, len(data), len(plan), ref.OK) and r[5] > 0 for r in got)


def test_a_payload_across_the_walk_chunks(pkg, batch, dev, sentinel):
    """packed payloads that skip more than two of the walk's chunks, between short runs, at several skews of the source"""
    chunk = pkg.unrle_walk_chunk()
    rnd = random.Random(52)
    datas = []
    for skew in (0, 5, 15):
        plan = [("rle", 5, 7), ("packed", [rnd.randrange(1 << 16) for _ in range(8 * 200)], 2), ("rle", 3, 0xFFFF, 3),
                ("packed", [rnd.randrange(1 << 16) for _ in range(8 * (3 * chunk // 16))]), ("packed", [1, 2, 3, 4, 5, 6, 7, 8], 5), ("rle", 2, 60000)]
        datas.append(rle_ref.encode(plan, 16))
    src, offs = _pack(datas, start=16, gap=lambda i: [0, 5, 15][i] + (-len(datas[0]) * i) % 16)
    room = _room(ref.random_dictionary(rnd, 60001, 2), 2 << 16, sentinel)
    segs, d_at = [], 1
    for i, (d, o) in enumerate(zip(datas, offs)):
        count = rle_ref.decode(d, 16, 8)[1][0]
        segs.append((o, len(d), d_at, count, 16, 2, 0, 0, 60001))
        d_at += count * 2 + i
    got = _undict(batch, dev, src, sentinel, segs, d_at + 16, room)
    assert all(r[3] == ref.OK and r[5] > 0 for r in got)


def test_the_dictionary_at_all_skews(pkg, batch, dev, sentinel):
    """sixteen skews of the dictionary at every width, the destination's skew going the other way: an entry is one load where the dictionary is a
    multiple of the width, and single bytes elsewhere"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(53)
    data = rle_ref.encode(rle_ref.random_plan(rnd, 6, C + 200, packed=(8, 64), repeated=(1, 40)), 6)
    count = rle_ref.decode(data, 6, 8)[1][0]
    src, offs = _pack([data])
    d_src = _upload(src)
    room = _room(ref.random_dictionary(rnd, 80, 8), 1024, sentinel)
    segs, d_at = [], 0
    for w in ref.WIDTHS:
        for skew in range(16):
            d_at = H.next_at(d_at, (5 - skew) % 16)
            segs.append((offs[0], len(data), d_at, count, 6, w, 0, skew, 64 - skew % 3))
            d_at += count * w
    got = _undict(batch, dev, src, sentinel, segs, d_at + 64, room, d_src=d_src)
    assert {r[5] == 0 for r in got} == {True, False}


def test_a_large_dictionary_under_random_indices(pkg, batch, dev, sentinel):
    """70 000 entries of 8 bytes under uniformly random 17-bit indices: nearly half of them out of range, all inside the allocation"""
    rnd = np.random.default_rng(54)
    D, n = 70000, 40000
    idx = rnd.integers(0, 1 << 17, size=n).tolist()
    data = rle_ref.encode([("packed", idx[:20000]), ("rle", 9, 69999), ("rle", 4, 70000), ("packed", idx[20000:])], 17)
    dictionary = rnd.integers(1, 256, size=D * 8, dtype=np.uint8).tobytes()
    room = _room(dictionary, (1 << 17) * 8 + 3, sentinel)
    src, offs = _pack([data])
    got = _undict(batch, dev, src, sentinel, [(offs[0], len(data), 9, n + 13, 17, 8, 0, 0, D)], 9 + (n + 13) * 8 + 64, room)
    assert got[0][0] == n + 13 and n // 3 < got[0][5] < 2 * n // 3


def test_dictionary_edges_and_bad_indices_across_items(pkg, batch, dev, sentinel):
    """D in {0, 1, the largest index, the largest index + 1, 2^k}: all, all but the zeros, exactly one, none and none of the elements are bad; bad
    indices in three different items: their number, and the first of them"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(55)
    k, w = 11, 4
    big = (1 << k) - 3
    values = [rnd.randint(1, big - 1) for _ in range(4 * C)]
    at = 2 * C + 17
    values[at] = big
    plan = [("rle", 7, 0), ("packed", values), ("rle", 3, 1)]
    data = rle_ref.encode(plan, k)
    n = 7 + len(values) + 3
    wide = [rnd.randint(0, 499) for _ in range(5 * C)]
    where = [C + 1, C + 2, 2 * C + C // 2, 4 * C + 3]
    for p in where:
        wide[p] = 500 + rnd.randint(0, 1500)
    data2 = rle_ref.encode([("rle", 3, 5), ("packed", wide)], k)
    src, offs = _pack([data, data2])
    d_src = _upload(src)
    room = _room(ref.random_dictionary(rnd, big + 1, w), (1 << k) * w + 64, sentinel)
    segs, d_at, want = [], 3, []
    for D, bad, first in [(0, n, 0), (1, n - 7, 7), (big, 1, 7 + at), (big + 1, 0, ref.NONE), (1 << k, 0, ref.NONE)]:
        segs.append((offs[0], len(data), d_at, n, k, w, 0, 0, D)); want.append((bad, first))
        d_at += n * w + 1
    segs.append((offs[1], len(data2), d_at, 3 + len(wide), k, w, 0, 0, 500)); want.append((len(where), 3 + where[0]))
    d_at += (3 + len(wide)) * w
    got = _undict(batch, dev, src, sentinel, segs, d_at + 64, room, d_src=d_src)
    assert [r[5:] for r in got] == want


def test_counting_alone_and_small_capacities(pkg, batch, dev, sentinel):
    """a call whose capacities are all 0 needs no destination and no dictionary, and gives unrle's five fields with bad 0 and no first bad; cap <
    count writes cap elements and nothing behind them, and bad and first_bad are about those alone"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(56)
    shapes = [(5, 1), (12, 4), (20, 8), (0, 2), (9, 2)]
    datas = [rle_ref.encode(rle_ref.random_plan(rnd, k, n, packed=(8, 200), repeated=(1, 300)), k) for (k, _), n in zip(shapes, [0, 50, 5 * C + 3, 3 * C, C])]
    src, offs = _pack(datas)
    d_src = _upload(src)
    sp = d_src.data_ptr()
    full = [rle_ref.decode(d, k, 8)[1] + (0, ref.NONE) for d, (k, _) in zip(datas, shapes)]
    args = ([sp + o for o in offs], [len(d) for d in datas])
    bits, ws = [k for k, _ in shapes], [w for _, w in shapes]
    assert batch.undict_segments(*args, None, [0] * 5, bits, ws, None, None, None) == full
    assert batch.last_undict_ms(1) > 0.0 and batch.last_undict_ms(2) == 0.0   # (counting is the walk alone)
    assert batch.undict_segments(*args, [None] * 5, [0] * 5, bits, ws, [0] * 5, [None] * 5, [7] * 5) == full
    room = _room(ref.random_dictionary(rnd, 600, 8), (1 << 17) * 8, sentinel)   # (the 20-bit indices are kept below 2^17 by the capacity's segment alone)
    segs, d_at = [], 3
    for d, o, (k, w), res, cap in zip(datas, offs, shapes, full, [4, 17, 0, 10 ** 9, C - 1]):
        segs.append((o, len(d), d_at, cap, k, w, 0, 0, 600))
        d_at += min(cap, res[0]) * w + 1   # (the next one begins one byte behind: a store beyond cap would hit it, or the sentinel between)
    got = _undict(batch, dev, src, sentinel, segs, d_at + 64, room, d_src=d_src)
    assert [r[:5] for r in got] == [r[:5] for r in full] and got[2][5:] == (0, ref.NONE)


def test_every_status(pkg, batch, dev, sentinel):
    """every stop behind a few runs: the status, and the values in front of the stop"""
    rnd = random.Random(57)
    datas, shapes = [], []
    for k, w in [(3, 1), (12, 4), (16, 8)]:
        plan = rle_ref.random_plan(rnd, k, 2500, packed=(8, 24), repeated=(1, 300))
        for _, tail, _ in rle_ref.stops(k):
            datas.append(rle_ref.encode(plan, k) + tail); shapes.append((k, w, 0))
        datas.append(b"\x21" + rle_ref.encode(plan, k)); shapes.append((0, w, ref.WIDTH_BYTE))
    datas.append(b""); shapes.append((0, 4, ref.WIDTH_BYTE))
    src, offs = _pack(datas)
    room = _room(ref.random_dictionary(rnd, 3000, 8), (1 << 16) * 8, sentinel)
    segs, d_at = [], 6
    for d, o, (k, w, f) in zip(datas, offs, shapes):
        count = rle_ref.decode(d, k, 8, f, 0)[1][0]
        segs.append((o, len(d), d_at, count + 3, k, w, f, 0, 3000))
        d_at += count * w + 3
    got = _undict(batch, dev, src, sentinel, segs, d_at + 16, room)
    assert {r[3] for r in got} == {ref.BAD_HEADER, ref.ZERO_RUN, ref.TRUNCATED, ref.BAD_WIDTH} and sum(1 for r in got if r[0] > 2500) >= 15


def test_bad_arguments_launch_nothing(pkg, batch, dev, sentinel):
    _fresh_dst(dev, 4096)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    three = ([sp, sp + 100, sp + 200], [100] * 3, [dp, dp + 1000, dp + 2000], [10] * 3)
    dicts = ([sp, sp, sp], [8] * 3)
    for bad in (3, 0, 16, 255):
        with pytest.raises(RuntimeError, match="undict segment 1: width is not 1, 2, 4 or 8"):
            batch.undict_segments(*three, [3] * 3, [4, bad, 2], None, *dicts)
    with pytest.raises(RuntimeError, match="undict segment 2: unknown flag bits"):
        batch.undict_segments(*three, [3] * 3, [4, 8, 2], [0, 1, 2], *dicts)
    with pytest.raises(RuntimeError, match="undict segment 1: field of more than 32 bits"):
        batch.undict_segments(*three, [3, 33, 3], [4, 8, 2], None, *dicts)
    with pytest.raises(RuntimeError, match=r"undict segment 0: a capacity above 2\^56"):
        batch.undict_segments([sp], [100], [dp], [(1 << 56) + 1], [3], [1], None, [sp], [8])
    with pytest.raises(RuntimeError, match="undict segment 1: no destination"):
        batch.undict_segments([sp, sp + 100], [100] * 2, [dp, None], [10, 10], [3, 3], [4, 4], None, [sp, sp], [8, 8])
    with pytest.raises(RuntimeError, match="undict segment 1: no dictionary for entries and a capacity that are not 0"):
        batch.undict_segments([sp, sp + 100], [100] * 2, [dp, dp + 1000], [10, 10], [3, 3], [4, 4], None, [sp, None], [8, 8])
    with pytest.raises(RuntimeError, match=r"undict segment 0: a dictionary of more than 2\^56 entries"):
        batch.undict_segments([sp], [100], [dp], [10], [3], [1], None, [sp], [(1 << 56) + 1])
    with pytest.raises(RuntimeError, match="invalid undict arguments"):   # capacities that are not 0, and no dictionaries at all
        batch.undict_segments(*three, [3] * 3, [4, 8, 2], None, None, None)
    H.compare(dev, sentinel[:4096])
    assert batch.last_undict_ms() == 0.0   # (nothing was launched)
    assert batch.undict_segments([], [], [], [], [], [], None, [], []) == []
    assert batch.undict_segments([sp + 7, sp + 7], [0, 0], [dp, dp], [5, 5], [17, 40], [1, 8], [0, 1], [None, None], [0, 0]) == [(0, 0, 0, ref.OK, 17, 0, ref.NONE),
                                                                                                                                (0, 0, 0, ref.BAD_WIDTH, 0, 0, ref.NONE)]
    H.compare(dev, sentinel[:4096])


# ------------------------------------------------------------------ the outputs of a decode call
class _Pages:
    """streams of one decode call: dictionary pages and the dictionary-index page bodies that name them, and one dictionary outside the call
    -> raws, streams, and per stream (dictionary stream or None: the outside one, width, entries, the dictionary's bytes) -- None for a
    dictionary page itself"""

    def __init__(self, sentinel):
        rnd = random.Random(58)
        self.dict_a, self.dict_b, self.outside = ref.random_dictionary(rnd, 300, 4), ref.random_dictionary(rnd, 70, 8), ref.random_dictionary(rnd, 1000, 2)

        def body(k, n, top):
            plan = [r[:2] + (r[2] % top,) if r[0] == "rle" else ("packed", [v % top for v in r[1]])
                    for r in rle_ref.random_plan(rnd, k, n, packed=(8, 504), repeated=(1, 2000))] if n else []
            return rle_ref.encode(plan, k, True)

        self.raws = [self.dict_a, body(9, 5000, 300), body(9, 1, 300), self.dict_b, body(7, 4096, 70), body(10, 3000, 1000), body(3, 0, 8), body(9, 100003, 310)]
        self.of = [None, (0, 4, 300, self.dict_a), (0, 4, 300, self.dict_a), None, (3, 8, 70, self.dict_b), (None, 2, 1000, self.outside), (0, 4, 300, self.dict_a),
                   (0, 4, 300, self.dict_a)]   # (the last one's indices reach 309: some are outside, inside the arena all the same)
        self.streams = [_stream(r) for r in self.raws]
        self.room = _room(self.outside, 4096, sentinel)


@pytest.fixture(scope="module")
def pages(sentinel):
    return _Pages(sentinel)


def _check_outputs(pkg, b, dev, sentinel, pages, skip, dict_bytes=None):
    """undict_outputs of the pages' streams into a fresh destination: the values, their results, and sentinel in the slots that were skipped,
    whose results are zeros; dict_bytes: what the dictionary streams delivered, where that is not all of their bytes"""
    n = len(pages.raws)
    delivered = dict_bytes or {j: pages.raws[j] for j in (0, 3)}
    want_res, elems = [], []
    for i, (raw, of) in enumerate(zip(pages.raws, pages.of)):
        if of is None or i in skip:
            want_res.append(ZERO); elems.append(b"")
            continue
        j, w, D, table = of
        if j is not None:
            table, D = delivered[j], len(delivered[j]) // w
        count = rle_ref.decode(raw, 0, 8, 1)[1][0]
        e, res = ref.elements_bytes(raw, 0, w, 1, table, D, count)
        want_res.append(res); elems.append(e)
    offs, size = H.slots([len(e) for e in elems], {i for i, e in enumerate(pages.of) if e is None or i in skip})
    want = sentinel[:size].copy()
    for e, o in zip(elems, offs):
        if o is not None:
            want[o:o + len(e)] = np.frombuffer(e, dtype=np.uint8)
    _fresh_dst(dev, size)
    dp, tp = dev["dst"].data_ptr(), pages.room[1].data_ptr()
    widths = [1 if of is None else of[1] for of in pages.of]
    got = b.undict_outputs([None if o is None else dp + o for o in offs], [r[0] for r in want_res], [0] * n, widths, [1] * n,
                           [pkg.UNDICT_NO_STREAM if of is None or of[0] is None else of[0] for of in pages.of],
                           [tp if of is not None and of[0] is None else None for of in pages.of], [of[2] if of is not None and of[0] is None else 0 for of in pages.of])
    assert got == want_res, [(i, a, c) for i, (a, c) in enumerate(zip(got, want_res)) if a != c][:3]
    H.compare(dev, want)
    counted = b.undict_outputs(None, None, [0] * n, [4] * n, [1] * n)
    assert [r[:5] for r in counted[1:3]] == [rle_ref.decode(raw, 0, 8, 1)[1] for raw in pages.raws[1:3]] and all(r[5:] == (0, ref.NONE) for r in counted)
    H.compare(dev, want)   # (counting writes nothing)
    return got


def test_outputs_of_decode_device(pkg, dev, sentinel, pages):
    import torch
    datas, caps = pages.streams, [len(r) for r in pages.raws]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    offs = [sum(caps[:i]) + 3 for i in range(len(caps))]
    arena = torch.from_numpy(sentinel[:sum(caps) + 4096].copy()).cuda()   # the outputs back to back, at whatever alignment that gives
    torch.cuda.synchronize()
    n = len(datas)
    b = pkg.Batch(n)
    try:
        with pytest.raises(RuntimeError, match="no decode call"):
            b.out_n = n
            b.undict_outputs(None, None, [0] * n, [4] * n)
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.undict_outputs(None, None, [0] * n, [4] * n)
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, c) for c in caps]
        ms, digests = b.last_kernel_ms(), b.digest_outputs()
        got = _check_outputs(pkg, b, dev, sentinel, pages, skip={2})
        assert got[7][5] > 0 and got[1][5] == 0
        assert b.last_kernel_ms() == ms and b.digest_outputs() == digests   # (not a decode call: the accessors say what they said)
        dp = dev["dst"].data_ptr()
        one = lambda i, j, w=4: b.undict_outputs([dp if s == i else None for s in range(n)], [1] * n, [0] * n, [w] * n, [1] * n, [j if s == i else 0 for s in range(n)])
        with pytest.raises(RuntimeError, match="undict stream 1: its dictionary stream 1 is the stream itself"):
            one(1, 1)
        with pytest.raises(RuntimeError, match="undict stream 2: its dictionary stream 8 is none of the 8 streams"):
            one(2, 8)
        with pytest.raises(RuntimeError, match="undict stream 1: width"):
            one(1, 0, 3)
    finally:
        b.close()


def test_outputs_of_decode_host_and_packed(pkg, dev, sentinel, pages):
    n = len(pages.raws)
    b = pkg.Batch(n)
    try:
        results, outs = b.decode_host(pages.streams, [len(r) for r in pages.raws], FLAGS)
        assert [r.result for r in results] == [1] * n and outs == pages.raws
        _check_outputs(pkg, b, dev, sentinel, pages, skip={1, 6})
        results, outs = b.decode_packed(pages.streams, flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(r)) for r in pages.raws]
        view, launches = b._packed_view(n), b.last_packed_launches()
        _check_outputs(pkg, b, dev, sentinel, pages, skip={4})
        assert b._packed_view(n) == view and view[0] != 0 and b.last_packed_launches() == launches   # BrotliAmdBatchPackedOutput still returns the buffer
    finally:
        b.close()


def test_a_dictionary_stream_delivered_truncated(pkg, dev, sentinel, pages):
    """a dictionary stream given less room than it needs (with the eager limit): exactly its decoded_size bytes are the dictionary, D shrinks,
    and the indices beyond it are bad"""
    import torch
    datas, caps = pages.streams, [len(r) for r in pages.raws]
    caps[0] = 1003   # 250 entries and three bytes of the dictionary's 300
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    offs = [sum(caps[:i]) + 1 for i in range(len(caps))]
    arena = torch.from_numpy(sentinel[:sum(caps) + 4096].copy()).cuda()
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS | EAGER)
        results = b.wait()
        assert [r.result for r in results] == [3] + [1] * (len(datas) - 1) and results[0].decoded_size == 1003
        got = _check_outputs(pkg, b, dev, sentinel, pages, skip=set(), dict_bytes={0: pages.dict_a[:1003], 3: pages.dict_b})
        assert got[1][5] > 0 and got[1][6] < 5000 and got[4][5] == 0
    finally:
        b.close()


def test_outputs_as_tensors(pkg, dev):
    import torch
    tensors = H.tensors_module()
    g = torch.Generator().manual_seed(59)
    rnd = random.Random(60)

    def body(idx, k):
        """seeded runs over the indices: repeats as RLE runs, the rest in packed groups, the last one padded; the width byte in front"""
        plan, i = [], 0
        while i < len(idx):
            j = i
            while j < len(idx) and idx[j] == idx[i]:
                j += 1
            if j - i >= 4 or rnd.random() < 0.1:
                plan.append(("rle", j - i, idx[i])); i = j
            else:
                take = idx[i:i + 8 * rnd.randrange(1, 5)]
                plan.append(("packed", take + [0] * (-len(take) % 8))); i += len(take)
        return rle_ref.encode(plan, k, True)

    d32 = torch.randn(200, generator=g)                                       # a float32 dictionary, a stream of the call
    d64 = torch.randint(-1 << 40, 1 << 40, (5000,), generator=g)              # an int64 dictionary, a tensor of the caller's
    i32 = torch.randint(0, 200, (33, 7), generator=g)
    i32b = torch.repeat_interleave(torch.randint(0, 200, (40,), generator=g), 50)
    i64 = torch.randint(0, 5000, (4096,), generator=g)
    plain = torch.randn((3, 5), generator=g)
    import shuffle_ref
    raws = [d32.numpy().tobytes(), body(i32.flatten().tolist(), 8), body(i32b.tolist(), 8), body(i64.tolist(), 13),
            shuffle_ref.shuffle(plain.numpy().tobytes(), 4)]
    d64_dev = d64.cuda()
    b = pkg.Batch(len(raws))
    try:
        results, _ = b.decode_packed([_stream(r) for r in raws], flags=FLAGS)
        assert [r.result for r in results] == [1] * len(raws)
        specs = [None, (torch.float32, (33, 7), (("dict", 0),)), (torch.float32, (2000,), (("dict", 0),)), (torch.int64, (4096,), (("dict", d64_dev),)),
                 (torch.float32, (3, 5))]
        got = tensors.outputs_as_tensors(b, specs)
        assert got[0] is None
        for t, o in zip(got[1:], [d32[i32], d32[i32b], d64[i64], plain]):
            assert t.is_cuda and t.dtype == o.dtype and tuple(t.shape) == tuple(o.shape) and t.data_ptr() % 64 == 0
            assert torch.equal(t.cpu().view(torch.uint8), o.contiguous().view(torch.uint8))
        # the dictionary stream with a spec of its own: unshuffled bytes as they are
        own = tensors.outputs_as_tensors(b, [(torch.float32, (200,), ())] + specs[1:])
        assert torch.equal(own[0].cpu(), d32) and torch.equal(own[1].cpu(), d32[i32])

        def wrong(i, spec):
            return [spec if k == i else s for k, s in enumerate(specs)]

        with pytest.raises(ValueError, match=r"stream 1: 2\d\d values in its runs, but shape"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.float32, (300,), (("dict", 0),))))
        tensors.outputs_as_tensors(b, wrong(1, (torch.float32, (225,), (("dict", 0),))))   # more values than numel: padding, not judged
        for other in ("shuffle", "delta", ("rle", 8), "dbp"):
            with pytest.raises(ValueError, match="stream 1: \"dict\" stands alone"):
                tensors.outputs_as_tensors(b, wrong(1, (torch.float32, (33, 7), (("dict", 0), other))))
        with pytest.raises(ValueError, match="stream 1: \"dict\" without its dictionary"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.float32, (33, 7), ("dict",))))
        with pytest.raises(ValueError, match=r"stream 1: \(\"dict\", j\) names the stream"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.float32, (33, 7), (("dict", 0, 1),))))
        with pytest.raises(ValueError, match="stream 1: its dictionary stream 1 is the stream itself"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.float32, (33, 7), (("dict", 1),))))
        with pytest.raises(ValueError, match="stream 1: its dictionary stream 5 is none of the 5 streams"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.float32, (33, 7), (("dict", 5),))))
        with pytest.raises(ValueError, match="stream 3: its dictionary is a torch.int32 tensor"):
            tensors.outputs_as_tensors(b, wrong(3, (torch.int64, (4096,), (("dict", d64_dev.to(torch.int32)),))))
        with pytest.raises(ValueError, match="stream 3: its dictionary is .* on the host"):
            tensors.outputs_as_tensors(b, wrong(3, (torch.int64, (4096,), (("dict", d64),))))
        # an index outside the dictionary: a dictionary tensor cut short, and float64 elements of the stream's 800 bytes
        with pytest.raises(ValueError, match=r"stream 3: \d+ of its 4096 values have an index outside its dictionary of 3000 entries, the first of them value \d+"):
            tensors.outputs_as_tensors(b, wrong(3, (torch.int64, (4096,), (("dict", d64_dev[:3000]),))))
        with pytest.raises(ValueError, match=r"stream 1: \d+ of its 231 values have an index outside its dictionary of 100 entries"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.float64, (33, 7), (("dict", 0),))))
        # runs that do not end well
        results, _ = b.decode_packed([_stream(raws[0]), _stream(raws[1] + b"\x82"), _stream(b"\x21" + raws[2][1:])], flags=FLAGS)
        with pytest.raises(ValueError, match=r"stream 1: runs that the stream's end cuts \(status 3\)"):
            tensors.outputs_as_tensors(b, [None, (torch.float32, (33, 7), (("dict", 0),)), None])
        with pytest.raises(ValueError, match=r"stream 2: a width byte that is none \(status 4\)"):
            tensors.outputs_as_tensors(b, [None, None, (torch.float32, (2000,), (("dict", 0),))])
    finally:
        b.close()


def test_pyarrow_pages_from_decode_call_to_tensor(pkg, dev):
    """the dictionary page and the data page that pyarrow wrote for every column (tests/golden/dict_pages/), each Brotli-compressed, in ONE decode
    call; outputs_as_tensors with ("dict", j) gives the columns"""
    import torch
    import dict_pages
    tensors = H.tensors_module()
    pages = dict_pages.load()
    assert len(pages) == 32
    dtypes = {"int32": torch.int32, "int64": torch.int64, "float32": torch.float32, "float64": torch.float64}
    streams, specs = [], []
    for e, dictionary, body, column in pages:
        streams += [_stream(dictionary), _stream(body)]
        specs += [None, (dtypes[e["type"]], (e["values"],), (("dict", len(streams) - 2),))]
    b = pkg.Batch(len(streams))
    try:
        results, _ = b.decode_packed(streams, flags=FLAGS)
        assert [r.result for r in results] == [1] * len(streams)
        got = tensors.outputs_as_tensors(b, specs)
        for (e, _, _, column), t in zip(pages, got[1::2]):
            assert t.is_cuda and t.numel() == e["values"] and t.cpu().numpy().tobytes() == column, e["label"]
    finally:
        b.close()
