"""Unnull on the device (needs a real MI355X): the kernels (csrc/brotli_unnull_kernels.hip) through BrotliAmdBatchUnnullSegments,
BrotliAmdBatchUnnullOutputs after the three kinds of decode call, and tensors.outputs_as_tensors, against the reference (null_ref.py) and against
the host hook.  Destinations come from one buffer and bitmaps from another, each prefilled with a sentinel pattern, and the WHOLE destination
buffer AND the WHOLE bitmap buffer are compared with the expectation: a byte written outside a segment's slots or validity bytes fails the
test.  All comparisons are exact."""
import random

import numpy as np
import pytest

import null_ref as ref
import rle_ref
import seg_filter_harness as H
from seg_filter_harness import pack as _pack, stream as _stream, upload as _upload

pytestmark = pytest.mark.gpu
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT
PF = ref.LENGTH_PREFIX | ref.VALUES_FOLLOW
ZERO = (0,) * 8  # a skipped stream's result


@pytest.fixture(scope="module")
def table():
    return ref.short_table()


@pytest.fixture(scope="module")
def sentinel():
    return H.sentinel(12 << 20)


@pytest.fixture(scope="module")
def dev(table, sentinel):
    """the harness's buffers, and one more for the bitmaps with a sentinel of its own"""
    import torch
    d = H.device_buffers(np.frombuffer(table[0], dtype=np.uint8), sentinel)
    vs = ((np.arange(2 << 20, dtype=np.uint64) * 7) % 251 + 3).astype(np.uint8)
    d["vsentinel_host"] = vs
    d["vsentinel"] = torch.from_numpy(vs.copy()).cuda()
    d["valid"] = torch.empty(len(vs), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def batch(pkg):
    b = pkg.Batch(1)   # (the number of segments is not bound by max_streams)
    yield b
    b.close()


def _fresh(dev, size, bsize):
    import torch
    H.fresh_dst(dev, size)
    dev["valid"][:bsize].copy_(dev["vsentinel"][:bsize])
    torch.cuda.synchronize()


def _compare(dev, want, want_bits):
    H.compare(dev, want)
    got = dev["valid"][:len(want_bits)].cpu().numpy()
    if not np.array_equal(got, want_bits):
        at = int(np.flatnonzero(got != want_bits)[0])
        raise AssertionError("byte %d of the bitmaps is %#x, not %#x" % (at, got[at], want_bits[at]))


def _expect(dev, sentinel, src, values, segs, size, bsize):
    want, want_bits, results = sentinel[:size].copy(), dev["vsentinel_host"][:bsize].copy(), []
    for s, l, d, cap, k, w, f, level, v, V, b in segs:
        slots, bits, res = ref.outputs(src[s:s + l], k, level, w, f, values[v:], V, cap)
        assert d + len(slots) <= size
        want[d:d + len(slots)] = np.frombuffer(slots, dtype=np.uint8)
        if b != ref.NO_BITMAP:
            assert b + len(bits) <= bsize
            want_bits[b:b + len(bits)] = np.frombuffer(bits, dtype=np.uint8)
        results.append(res)
    return want, want_bits, results


def _unnull(batch, dev, sentinel, src, values, segs, size, bsize, d_src=None, d_values=None):
    """segs: [(source offset, source length, destination offset, cap, bits, width, flags, level, values offset, values count, validity offset or
    NO_BITMAP)] -> one call into a fresh destination of `size` bytes and fresh bitmaps of `bsize`, both buffers and all results compared"""
    src, values = bytes(src), bytes(values)
    want, want_bits, results = _expect(dev, sentinel, src, values, segs, size, bsize)
    d_src = _upload(src) if d_src is None else d_src
    d_values = _upload(values) if d_values is None else d_values
    _fresh(dev, size, bsize)
    sp, vp, dp, bp = d_src.data_ptr(), d_values.data_ptr(), dev["dst"].data_ptr(), dev["valid"].data_ptr()
    got = batch.unnull_segments([sp + s[0] for s in segs], [s[1] for s in segs], [vp + s[8] for s in segs], [s[9] for s in segs], [dp + s[2] for s in segs],
                                [None if s[10] == ref.NO_BITMAP else bp + s[10] for s in segs], [s[3] for s in segs], [s[4] for s in segs], [s[7] for s in segs],
                                [s[5] for s in segs], [s[6] for s in segs])
    assert got == results, [(i, a, b, segs[i]) for i, (a, b) in enumerate(zip(got, results)) if a != b][:3]
    _compare(dev, want, want_bits)
    return got


def _layout(cases, start=3, bstart=1, gap=1):
    """cases: [(levels or body, k, level, w, flags, values, V, cap or None, bitmap)] -> (src, values buffer, segs, size, bsize)"""
    datas = [c[0] for c in cases]
    src, offs = _pack(datas)
    vals, segs, d_at, b_at = bytearray(b"\x11" * 3), [], start, bstart
    for (data, k, level, w, f, values, V, cap, bitmap), o in zip(cases, offs):
        count = ref.decode(data, k, level, w, f, values, V, 0)[2][0]
        cap = count if cap is None else cap
        m = min(cap, count)
        segs.append((o, len(data), d_at, cap, k, w, f, level, len(vals), V, b_at if bitmap else ref.NO_BITMAP))
        vals += bytes(values) + b"\x22" * (len(segs) % 3)
        d_at += m * w + gap
        b_at += ((m + 7) // 8 + gap) if bitmap else 0
    return src, bytes(vals), segs, d_at + 64, b_at + 64


def test_three_thousand_short_segments_and_the_host_hook(pkg, batch, dev, table, sentinel):
    """more than two chunks of a thousand segments: every shape, flag, ending and value count, every alignment of levels, values, destination and
    bitmap; the kernels' results and bytes are the host hook's"""
    src, values, segs, size, bsize = table
    assert {s[0] % 16 for s in segs} == set(range(16)) and {s[2] % 16 for s in segs} == set(range(16)) and {s[8] % 16 for s in segs} == set(range(16))
    assert {s[10] % 16 for s in segs if s[10] != ref.NO_BITMAP} == set(range(16))
    got = _unnull(batch, dev, sentinel, src, values, segs, size, bsize, d_src=dev["src"])
    assert {r[3] for r in got} == {ref.OK, ref.BAD_HEADER, ref.ZERO_RUN, ref.TRUNCATED, ref.BAD_LENGTH}   # every status
    assert sum(1 for r in got if r[6]) > 100 and sum(1 for r in got if r[5] and not r[6]) > 300
    assert batch.last_unnull_ms() > 0.0
    assert all(batch.last_unnull_ms(p) > 0.0 for p in (1, 2, 3, 4)) and batch.last_unnull_ms(5) == 0.0
    hook_dst, hook_bits, hook_res = pkg.unnull_host(src, values, segs, size, bsize, fill=sentinel[:size].tobytes(), valid_fill=dev["vsentinel_host"][:bsize].tobytes())
    assert hook_res == got
    assert hook_dst == dev["dst"][:size].cpu().numpy().tobytes() and hook_bits == dev["valid"][:bsize].cpu().numpy().tobytes()


def test_every_width_field_width_and_level(pkg, batch, dev, sentinel):
    """every w with k in 0 .. 3, 8, 9 and 32 and level 0, 2^k - 1 and a middle value, levels above and below it; more than one item each"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(61)
    cases = []
    for w in ref.WIDTHS:
        for k in (0, 1, 2, 3, 8, 9, 32):
            top = (1 << k) - 1
            for level in sorted({0, top, top // 2}):
                plan = ref.level_plan(rnd, k, level, C + 100 + 8 * k, 0.4, runs=(1, 60), packed=(8, 64))
                present = ref.present_of(plan, level)
                cases.append((rle_ref.encode(plan, k), k, level, w, 0, ref.random_values(rnd, present, w), present, None, True))
    got = _unnull(batch, dev, sentinel, *_layout(cases))
    assert all(r[3] == ref.OK and r[6] == 0 and r[5] == r[7] for r in got) and sum(1 for r in got if 0 < r[5] < r[0]) > 40


def test_patterns_and_every_tail(pkg, batch, dev, sentinel):
    """all null, none null, alternating, long null and present runs that straddle a lane's 16, a byte's 8 and an item's edge, many runs in one
    item; every m % 8 and every m % 16 behind an item's edge; with and without a bitmap"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(62)
    alt = [i & 1 for i in range(2 * C + 16)]
    plans = [[("rle", 2 * C + 5, 0)], [("rle", C + 3, 1), ("packed", [1] * 24)], [("packed", alt)],
             [("rle", 13, 1), ("rle", C - 7, 0), ("rle", C + 9, 1), ("packed", alt[:16]), ("rle", 2 * C + 1, 0), ("rle", 7, 1), ("rle", 17, 0), ("rle", 15, 1)],
             [("rle", 1 + i % 3, i & 1) for i in range(1500)]]   # (more than 64 runs in one item, and in one lane's neighbourhood several)
    cases = []
    for j, plan in enumerate(plans):
        data, n, present = rle_ref.encode(plan, 1), ref.rows_of(plan), ref.present_of(plan, 1)
        values = ref.random_values(rnd, present, 4)
        cases.append((data, 1, 1, 4, 0, values, present, None, j != 1))
        for cut in range(1, 17):
            cases.append((data, 1, 1, 1 << (cut & 3), 0, values, present // 8, C + cut, cut != 5))   # (V below the present slots: missing ones too)
    got = _unnull(batch, dev, sentinel, *_layout(cases, gap=0))
    assert got[0][5] == 0 and got[17][5] == got[17][0] and sum(1 for r in got if r[6]) > 20


def test_all_skews(pkg, batch, dev, sentinel):
    """sixteen skews of the bitmap against sixteen of the destination at every width, the levels' and the values' skews going their own ways: the
    bitmap's aligned 16-byte stores and its single bytes at the two ends"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(63)
    plan = ref.level_plan(rnd, 1, 1, 2 * C + 300, 0.3, runs=(1, 50), packed=(8, 64))
    data, n, present = rle_ref.encode(plan, 1), ref.rows_of(plan), ref.present_of(plan, 1)
    gaps, at = [], 16
    for i in range(16):   # 16 copies, copy i at i past a 16-byte boundary
        gaps.append((i - at) % 16)
        at += gaps[-1] + len(data)
    src, offs = _pack([data] * 16, start=16, gap=lambda i: gaps[i])
    assert {o % 16 for o in offs} == set(range(16))
    values = b"\x11" * 3 + ref.random_values(rnd, present + 16, 8)
    segs, d_at, b_at = [], 0, 0
    for bs in range(16):
        for ds in range(16):
            w = 1 << ((bs + ds) & 3)
            d_at, b_at = H.next_at(d_at, ds), H.next_at(b_at, bs)
            m = n - (bs * 16 + ds) % 23
            segs.append((offs[(bs + ds) % 16], len(data), d_at, m, 1, w, 0, 1, 3 + (bs * 5 + ds) % 16, present, b_at))
            d_at += m * w
            b_at += (m + 7) // 8
    _unnull(batch, dev, sentinel, src, values, segs, d_at + 64, b_at + 64)


def test_headers_and_payloads_across_the_walk_chunks(pkg, batch, dev, sentinel):
    """packed payloads that skip more than two of the walk's chunks between short runs, headers of every length on the chunks' edges, at several
    skews of the source; behind a length prefix too, with the values behind the levels"""
    chunk = pkg.unrle_walk_chunk()
    rnd = random.Random(64)
    cases = []
    for skew in (0, 5, 15):
        plan = [("rle", 5, 3), ("packed", [rnd.randrange(4) for _ in range(8 * 200)], 2), ("rle", 3, 0xFF, 3),
                ("packed", [rnd.randrange(4) for _ in range(8 * (3 * chunk // 2))]), ("packed", [1, 2, 3, 3, 3, 0, 3, 3], 5), ("rle", 2, 3)]
        plan += [("rle", 1 + i % 5, 3 * (i & 1), 1 + (i + skew) % 5) for i in range(chunk // 2)]   # headers of 1 .. 5 bytes over several chunks
        data, present = rle_ref.encode(plan, 2), ref.present_of(plan, 3)
        values = ref.random_values(rnd, present, 2)
        cases.append((data, 2, 3, 2, 0, values, present, None, True))
        cases.append((ref.v1_body(data, values) + b"\x77", 2, 3, 2, PF, b"", 0, None, True))
    src, vals, segs, size, bsize = _layout(cases)
    got = _unnull(batch, dev, sentinel, src, vals, segs, size, bsize)
    assert all(r[3] == ref.OK and r[6] == 0 and r[5] == r[7] for r in got)


def test_one_long_segment_and_a_second_behind_it(pkg, batch, dev, sentinel):
    """a segment of about three hundred items, which several blocks share, and a second one of another shape right behind it in the source, the
    destination and the bitmaps; then both at destinations that are no multiple of the width"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(65)
    p1 = ref.level_plan(rnd, 1, 1, 300 * C + 77, 0.3, runs=(1, 900), packed=(8, 504))
    p2 = ref.level_plan(rnd, 3, 5, 9 * C + 5, 0.9, runs=(1, 70), packed=(8, 64))
    first, second = rle_ref.encode(p1, 1), rle_ref.encode(p2, 3)
    n1, n2, v1, v2 = ref.rows_of(p1), ref.rows_of(p2), ref.present_of(p1, 1), ref.present_of(p2, 5)
    src, offs = _pack([first, second], start=5, gap=lambda i: 0)
    values = ref.random_values(rnd, v1, 4) + ref.random_values(rnd, v2, 2)
    d_src, d_values = _upload(src), _upload(values)
    for skew in (0, 1):
        d1, b1 = 12 + skew + 4 * n1, 3 + (n1 + 7) // 8
        segs = [(offs[0], len(first), 12 + skew, n1, 1, 4, 0, 1, 0, v1, 3), (offs[1], len(second), d1, n2, 3, 2, 0, 5, 4 * v1, v2, b1)]
        got = _unnull(batch, dev, sentinel, src, values, segs, d1 + 2 * n2 + 64, b1 + (n2 + 7) // 8 + 64, d_src, d_values)
        assert [r[5:] for r in got] == [(v1, 0, v1), (v2, 0, v2)] and n1 > 300 * C


def test_more_items_than_two_carry_passes(pkg, batch, dev, sentinel):
    """a segment of so many items that the carry launch takes more than two passes; slots of one byte, so that the buffers stay a few MiB"""
    C, span = pkg.unrle_item_elems(), pkg.undelta_carry_span()
    rnd = random.Random(66)
    plan = ref.level_plan(rnd, 1, 1, (2 * span + 3) * C + 77, 0.5, runs=(200, 5000), packed=(8, 504))
    data, n, present = rle_ref.encode(plan, 1), ref.rows_of(plan), ref.present_of(plan, 1)
    assert (n + C - 1) // C > 2 * span and n < 11 << 20
    values = np.random.default_rng(67).integers(1, 256, size=present, dtype=np.uint8).tobytes()
    src, offs = _pack([data], start=7)
    got = _unnull(batch, dev, sentinel, src, values, [(offs[0], len(data), 13, n, 1, 1, 0, 1, 0, present, 5)], 13 + n + 64, 5 + (n + 7) // 8 + 64)
    assert got[0][5:] == (present, 0, present)


def test_counting_alone_and_small_capacities(pkg, batch, dev, sentinel):
    """a call whose capacities are all 0 needs no destination, no values and no bitmap, is the walk alone, and gives unrle's five fields with
    present 0 and missing 0; with LENGTH_PREFIX its `consumed` says where the values begin; cap < count writes cap slots and ceil(cap / 8)
    validity bytes and nothing behind them"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(68)
    shapes = [(1, 1, 0), (2, 2, 50), (3, 7, 5 * C + 3), (0, 0, 3 * C), (9, 300, C)]
    plans = [ref.level_plan(rnd, k, level, n, 0.3, runs=(1, 300), packed=(8, 200)) if n else [] for k, level, n in shapes]
    datas = [rle_ref.encode(p, k) for p, (k, _, _) in zip(plans, shapes)]
    present = [ref.present_of(p, level) for p, (_, level, _) in zip(plans, shapes)]
    bodies = [ref.v1_body(d, b"\x55" * (3 * v)) for d, v in zip(datas, present)]
    src, offs = _pack(bodies)
    d_src = _upload(src)
    sp = d_src.data_ptr()
    bits, levels = [k for k, _, _ in shapes], [level for _, level, _ in shapes]
    full = [rle_ref.decode(d, k, 8)[1] for d, k in zip(datas, bits)]
    want = [(c, 4 + used, runs, st, k, 0, 0, 3 * v) for (c, used, runs, st, k), v in zip(full, present)]
    assert batch.unnull_segments([sp + o for o in offs], [len(b) for b in bodies], None, None, None, None, [0] * 5, bits, levels, [1] * 5, [PF] * 5) == want
    assert batch.last_unnull_ms(1) > 0.0 and all(batch.last_unnull_ms(p) == 0.0 for p in (2, 3, 4))   # (counting is the walk alone)
    want = [(c, used, runs, st, k, 0, 0, 9) for c, used, runs, st, k in full]
    assert batch.unnull_segments([sp + o + 4 for o in offs], [len(d) for d in datas], [None] * 5, [9] * 5, [None] * 5, None, [0] * 5, bits, levels, [4] * 5, None) == want
    cases = [(d, k, level, w, 0, ref.random_values(rnd, v, w), v, cap, True)
             for d, (k, level, _), v, w, cap in zip(datas, shapes, present, [1, 4, 8, 2, 2], [4, 17, 0, 10 ** 9, C - 1])]
    _unnull(batch, dev, sentinel, *_layout(cases))


def test_bad_arguments_launch_nothing(pkg, batch, dev, sentinel):
    _fresh(dev, 4096, 512)
    sp, dp, bp = dev["src"].data_ptr(), dev["dst"].data_ptr(), dev["valid"].data_ptr()
    lv = ([sp, sp + 100, sp + 200], [100] * 3)
    rest = ([sp + 300] * 3, [8] * 3, [dp, dp + 1000, dp + 2000], [bp, bp + 100, None], [10] * 3)
    for bad in (3, 0, 16, 255):
        with pytest.raises(RuntimeError, match="unnull segment 1: width is not 1, 2, 4 or 8"):
            batch.unnull_segments(*lv, *rest, [1] * 3, [1] * 3, [4, bad, 2])
    with pytest.raises(RuntimeError, match="unnull segment 2: unknown flag bits"):
        batch.unnull_segments(*lv, *rest, [1] * 3, [1] * 3, [4, 8, 2], [0, 1, 4])
    with pytest.raises(RuntimeError, match="unnull segment 1: values that follow the levels without a length prefix"):
        batch.unnull_segments(*lv, *rest, [1] * 3, [1] * 3, [4, 8, 2], [0, 2, 3])
    with pytest.raises(RuntimeError, match="unnull segment 1: field of more than 32 bits"):
        batch.unnull_segments(*lv, *rest, [1, 33, 1], [1] * 3, [4, 8, 2])
    with pytest.raises(RuntimeError, match=r"unnull segment 0: a capacity above 2\^56"):
        batch.unnull_segments([sp], [100], [sp], [8], [dp], None, [(1 << 56) + 1], [1], [1], [1])
    with pytest.raises(RuntimeError, match=r"unnull segment 0: more than 2\^56 values"):
        batch.unnull_segments([sp], [100], [sp], [(1 << 56) + 1], [dp], None, [10], [1], [1], [1])
    with pytest.raises(RuntimeError, match="unnull segment 1: no destination"):
        batch.unnull_segments(lv[0][:2], [100] * 2, [sp, sp], [8, 8], [dp, None], None, [10, 10], [1, 1], [1, 1], [4, 4])
    with pytest.raises(RuntimeError, match="unnull segment 1: no values for a count and a capacity that are not 0"):
        batch.unnull_segments(lv[0][:2], [100] * 2, [sp, None], [8, 8], [dp, dp + 1000], None, [10, 10], [1, 1], [1, 1], [4, 4])
    with pytest.raises(RuntimeError, match="invalid unnull arguments"):   # capacities that are not 0, and no values at all
        batch.unnull_segments(*lv, None, None, *rest[2:], [1] * 3, [1] * 3, [4, 8, 2])
    _compare(dev, sentinel[:4096], dev["vsentinel_host"][:512])
    assert batch.last_unnull_ms() == 0.0   # (nothing was launched)
    assert batch.unnull_segments([], [], [], [], [], [], [], [], [], []) == []
    assert batch.unnull_segments([sp + 7, sp + 7], [0, 0], [None, None], [0, 0], [dp, dp], [bp, bp], [5, 5], [17, 1], [0, 0], [1, 8], [0, 1]) == [
        (0, 0, 0, ref.OK, 17, 0, 0, 0), (0, 0, 0, ref.BAD_LENGTH, 1, 0, 0, 0)]
    _compare(dev, sentinel[:4096], dev["vsentinel_host"][:512])


# ------------------------------------------------------------------ the outputs of a decode call
class _Pages:
    """streams of one decode call: v1 bodies (prefix, levels, values), v2 value streams whose levels lie outside, and streams that are neither
    -> raws, streams, and per stream (k, level, w, levels outside or None: a v1 body) -- None for a stream that is not a page"""

    def __init__(self):
        rnd = random.Random(69)
        C = 1024

        def page(k, level, w, n, share, v2, extra=0):
            plan = ref.level_plan(rnd, k, level, n, share, runs=(1, 400), packed=(8, 504)) if n else []
            levels = rle_ref.encode(plan, k)
            values = ref.random_values(rnd, ref.present_of(plan, level) + extra, w)
            return (values, (k, level, w, levels)) if v2 else (ref.v1_body(levels, values), (k, level, w, None))

        made = [page(1, 1, 4, 5000, 0.3, False), page(1, 1, 8, 1, 1.0, False), (b"not a page at all" * 9, None), page(2, 3, 2, 3 * C + 9, 0.9, True), page(1, 1, 4, 4096, 0.0, True),
                page(3, 5, 1, 0, 0.5, False), page(1, 1, 2, 20003, 0.5, False, extra=4), page(9, 300, 8, 700, 0.4, True)]
        self.raws, self.of = [m[0] for m in made], [m[1] for m in made]
        self.streams = [_stream(r) for r in self.raws]
        self.levels = [None if of is None or of[3] is None else _upload(of[3]) for of in self.of]


@pytest.fixture(scope="module")
def pages():
    return _Pages()


def _check_outputs(pkg, b, dev, sentinel, pages, skip, delivered=None):
    """unnull_outputs of the pages' streams in both forms into fresh buffers: the slots, the bitmaps, their results, and sentinel where a stream was
    skipped, whose result is zeros; delivered: what the streams delivered, where that is not all of their bytes"""
    n = len(pages.raws)
    raws = delivered or pages.raws
    want_res, slots, bitmaps = [], [], []
    for i, (raw, of) in enumerate(zip(raws, pages.of)):
        if of is None or i in skip:
            want_res.append(ZERO); slots.append(b""); bitmaps.append(b"")
            continue
        k, level, w, levels = of
        rows = ref.decode(raw, k, level, w, PF, cap=0)[2][0] if levels is None else rle_ref.decode(levels, k, 8)[1][0]
        s, v, res = ref.outputs(raw, k, level, w, PF, cap=rows) if levels is None else ref.outputs(levels, k, level, w, 0, raw, len(raw) // w, rows)
        want_res.append(res); slots.append(s); bitmaps.append(v)
    skipped = {i for i, of in enumerate(pages.of) if of is None or i in skip}
    offs, size = H.slots([len(s) for s in slots], skipped)
    boffs, bsize = H.slots([len(v) + 1 for v in bitmaps], skipped, start=3)
    want, want_bits = sentinel[:size].copy(), dev["vsentinel_host"][:bsize].copy()
    for s, v, o, bo in zip(slots, bitmaps, offs, boffs):
        if o is not None:
            want[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
            want_bits[bo:bo + len(v)] = np.frombuffer(v, dtype=np.uint8)
    _fresh(dev, size, bsize)
    dp, bp = dev["dst"].data_ptr(), dev["valid"].data_ptr()
    bits, levels, widths = ([0 if of is None else of[j] for of in pages.of] for j in range(3))
    widths = [w or 1 for w in widths]
    lp = [None if t is None else t.data_ptr() for t in pages.levels]
    ll = [0 if of is None or of[3] is None else len(of[3]) for of in pages.of]
    got = b.unnull_outputs([None if o is None else dp + o for o in offs], [None if o is None else bp + o for o in boffs], [r[0] for r in want_res], bits, levels, widths, lp, ll)
    assert got == want_res, [(i, a, c) for i, (a, c) in enumerate(zip(got, want_res)) if a != c][:3]
    _compare(dev, want, want_bits)
    counted = b.count_levels_outputs(bits, lp, ll)
    assert [r[:5] for i, r in enumerate(counted) if pages.of[i] is not None and i not in skip] == [r[:5] for i, r in enumerate(want_res) if pages.of[i] is not None and i not in skip]
    assert all(r[5:7] == (0, 0) for r in counted)
    _compare(dev, want, want_bits)   # (counting writes nothing)
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
            b.count_levels_outputs([1] * n)
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.count_levels_outputs([1] * n)
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, c) for c in caps]
        ms, digests = b.last_kernel_ms(), b.digest_outputs()
        got = _check_outputs(pkg, b, dev, sentinel, pages, skip={1})
        assert got[0][5] > 0 and got[0][6] == 0 and got[6][7] == got[6][5] + 4   # (values left over are the caller's to judge)
        assert b.last_kernel_ms() == ms and b.digest_outputs() == digests   # (not a decode call: the accessors say what they said)
        dp = dev["dst"].data_ptr()
        with pytest.raises(RuntimeError, match="unnull stream 3: width"):
            b.unnull_outputs([dp if s == 3 else None for s in range(n)], None, [1] * n, [1] * n, [1] * n, [3] * n)
    finally:
        b.close()


def test_outputs_of_decode_host_and_packed(pkg, dev, sentinel, pages):
    n = len(pages.raws)
    b = pkg.Batch(n)
    try:
        results, outs = b.decode_host(pages.streams, [len(r) for r in pages.raws], FLAGS)
        assert [r.result for r in results] == [1] * n and outs == pages.raws
        _check_outputs(pkg, b, dev, sentinel, pages, skip={0, 5})
        results, outs = b.decode_packed(pages.streams, flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(r)) for r in pages.raws]
        view, launches = b._packed_view(n), b.last_packed_launches()
        _check_outputs(pkg, b, dev, sentinel, pages, skip={4})
        assert b._packed_view(n) == view and view[0] != 0 and b.last_packed_launches() == launches   # BrotliAmdBatchPackedOutput still returns the buffer
    finally:
        b.close()


def test_a_stream_delivered_truncated(pkg, dev, sentinel, pages):
    """a v1 body and a v2 value stream given less room than they need (with the eager limit): exactly their decoded_size bytes are taken, so
    the body's values end early and the last rows that are there are missing"""
    import torch
    datas, caps = pages.streams, [len(r) for r in pages.raws]
    caps[0] -= 1001
    caps[3] = 10
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    offs = [sum(caps[:i]) + 1 for i in range(len(caps))]
    arena = torch.from_numpy(sentinel[:sum(caps) + 4096].copy()).cuda()
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS | EAGER)
        results = b.wait()
        assert [r.result for r in results] == [3, 1, 1, 3, 1, 1, 1, 1] and results[0].decoded_size == caps[0] and results[3].decoded_size == 10
        delivered = [r[:c] for r, c in zip(pages.raws, caps)]
        got = _check_outputs(pkg, b, dev, sentinel, pages, skip=set(), delivered=delivered)
        assert got[0][6] == 251 and got[3][7] == 5 and got[3][6] == got[3][5] - 5
    finally:
        b.close()


def test_outputs_as_tensors(pkg, dev):
    import torch
    tensors = H.tensors_module()
    rnd = random.Random(70)

    def levels_of(mask):
        """the levels of a column: an RLE run for every stretch of rows of one kind, so that they hold exactly the rows"""
        plan, i, lv = [], 0, [int(m) for m in mask]
        while i < len(lv):
            j = i
            while j < len(lv) and lv[j] == lv[i]:
                j += 1
            plan.append(("rle", j - i, lv[i])); i = j
        return rle_ref.encode(plan, 1)

    g = torch.Generator().manual_seed(71)
    f32 = torch.randn(33 * 7, generator=g)
    m32 = torch.rand(33 * 7, generator=g) < 0.7
    i64 = torch.randint(-1 << 40, 1 << 40, (4096,), generator=g)
    m64 = torch.repeat_interleave(torch.rand(128, generator=g) < 0.5, 32)
    plain = torch.randn((3, 5), generator=g)
    import shuffle_ref
    lv64 = levels_of(m64.tolist())
    raws = [ref.v1_body(levels_of(m32.tolist()), f32[m32].numpy().tobytes()), i64[m64].numpy().tobytes(), shuffle_ref.shuffle(plain.numpy().tobytes(), 4)]
    d_lv = _upload(lv64)[:len(lv64)]
    b = pkg.Batch(len(raws))
    try:
        results, _ = b.decode_packed([_stream(r) for r in raws], flags=FLAGS)
        assert [r.result for r in results] == [1] * len(raws)
        specs = [(torch.float32, (33, 7), (("nulls", 1),)), (torch.int64, (4096,), (("nulls", 1, d_lv),)), (torch.float32, (3, 5))]
        got = tensors.outputs_as_tensors(b, specs)
        for (t, valid), o, m in zip(got[:2], [torch.where(m32, f32, torch.zeros(())).reshape(33, 7), torch.where(m64, i64, torch.zeros((), dtype=torch.int64))], [m32, m64]):
            assert t.is_cuda and t.dtype == o.dtype and tuple(t.shape) == tuple(o.shape) and t.data_ptr() % 64 == 0
            assert torch.equal(t.cpu().view(torch.uint8), o.contiguous().view(torch.uint8))
            assert valid.is_cuda and valid.dtype == torch.uint8 and valid.numel() == (m.numel() + 7) // 8 and valid.data_ptr() % 64 == 0
            assert valid.cpu().numpy().tobytes() == np.packbits(m.numpy(), bitorder="little").tobytes()
        assert torch.equal(got[2].cpu(), plain)

        def wrong(i, spec):
            return [spec if k == i else s for k, s in enumerate(specs)]

        with pytest.raises(ValueError, match=r"stream 0: 231 levels, but shape \(300,\) is 300 elements"):
            tensors.outputs_as_tensors(b, wrong(0, (torch.float32, (300,), (("nulls", 1),))))
        with pytest.raises(ValueError, match=r"stream 0: 231 levels, but shape \(225,\) is 225 elements"):
            tensors.outputs_as_tensors(b, wrong(0, (torch.float32, (225,), (("nulls", 1),))))
        for other in ("shuffle", "delta", ("rle", 8), "dbp"):
            with pytest.raises(ValueError, match="stream 0: \"nulls\" stands alone"):
                tensors.outputs_as_tensors(b, wrong(0, (torch.float32, (33, 7), (("nulls", 1), other))))
        with pytest.raises(ValueError, match="stream 0: \"nulls\" without its level"):
            tensors.outputs_as_tensors(b, wrong(0, (torch.float32, (33, 7), ("nulls",))))
        for bad in (("nulls", 1, 2), ("nulls", -1), ("nulls", 1 << 32), ("nulls", True), ("nulls", 1, d_lv, 0)):
            with pytest.raises(ValueError, match=r"stream 0: \(\"nulls\", level\) names the definition level"):
                tensors.outputs_as_tensors(b, wrong(0, (torch.float32, (33, 7), (bad,))))
        with pytest.raises(ValueError, match="stream 1: its levels are a torch.int32 tensor"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.int64, (4096,), (("nulls", 1, d_lv.to(torch.int32)),))))
        with pytest.raises(ValueError, match="stream 1: its levels are .* on the host"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.int64, (4096,), (("nulls", 1, d_lv.cpu()),))))
        # a row that is there without a value: float64 elements of the stream's float32 values; values left over: int32 elements of int64 values
        with pytest.raises(ValueError, match=r"stream 0: \d+ of its \d+ rows that are there have no value: the stream holds \d+ values"):
            tensors.outputs_as_tensors(b, wrong(0, (torch.float64, (33, 7), (("nulls", 1),))))
        with pytest.raises(ValueError, match=r"stream 1: \d+ values for the \d+ rows that are there: values are left over"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.int32, (4096,), (("nulls", 1, d_lv),))))
        # levels that do not end well, and a prefix that says more than there is
        results, _ = b.decode_packed([_stream(raws[0]), _stream(raws[1]), _stream(b"\xff\xff\x00\x00" + raws[0][4:])], flags=FLAGS)
        with pytest.raises(ValueError, match=r"stream 1: runs that the stream's end cuts \(status 3\)"):
            tensors.outputs_as_tensors(b, [None, (torch.int64, (4096,), (("nulls", 1, _upload(lv64 + b"\x82")[:len(lv64) + 1]),)), None])
        with pytest.raises(ValueError, match=r"stream 2: a length in front of the levels that is cut or says more than there is \(status 5\)"):
            tensors.outputs_as_tensors(b, [None, None, (torch.float32, (33, 7), (("nulls", 1),))])
    finally:
        b.close()


def test_pyarrow_pages_from_decode_call_to_tensor(pkg, dev):
    """the data page that pyarrow wrote for every nullable column (tests/golden/null_pages/), each body Brotli-compressed here, in ONE decode
    call; outputs_as_tensors with both ("nulls", ...) forms gives the columns and their bitmaps"""
    import torch
    import null_pages
    tensors = H.tensors_module()
    pages = null_pages.load()
    assert len(pages) == 40
    dtypes = {"int32": torch.int32, "int64": torch.int64, "float32": torch.float32, "float64": torch.float64}
    keep = [_upload(levels) for _, _, levels, _, _ in pages]
    specs = [(dtypes[e["type"]], (e["rows"],), (("nulls", 1) if e["version"] == 1 else ("nulls", 1, t[:len(levels)]),)) for (e, _, levels, _, _), t in zip(pages, keep)]
    streams = [_stream(body) for _, body, _, _, _ in pages]
    b = pkg.Batch(len(streams))
    try:
        results, _ = b.decode_packed(streams, flags=FLAGS)
        assert [r.result for r in results] == [1] * len(streams)
        got = tensors.outputs_as_tensors(b, specs)
        for (e, _, _, column, mask), (t, valid) in zip(pages, got):
            assert t.is_cuda and t.numel() == e["rows"] and t.cpu().numpy().tobytes() == column, e["label"]
            assert valid.cpu().numpy().tobytes() == mask, e["label"]
    finally:
        b.close()
