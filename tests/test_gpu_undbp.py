"""Undbp on the device (needs a real MI355X): the kernels (csrc/brotli_undbp_kernels.hip) through BrotliAmdBatchUndbpSegments,
BrotliAmdBatchUndbpOutputs after the three kinds of decode call, and tensors.outputs_as_tensors, against the reference (dbp_ref.py) and against
the host hook.  Destinations come from one buffer prefilled with a sentinel pattern, and the WHOLE destination buffer is compared with the
expectation: a byte written outside a segment's elements fails the test.  All comparisons are exact."""
import os
import random

import numpy as np
import pytest

import dbp_ref as ref
import seg_filter_harness as H
from conftest import ROOT
from seg_filter_harness import fresh_dst as _fresh_dst, pack as _pack, stream as _stream, slots as _slots, upload as _upload

pytestmark = pytest.mark.gpu
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT
ZEROS = (0, 0, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def table():
    """the table of the tests without a device -> (source, segments, destination size)"""
    return ref.short_table()


@pytest.fixture(scope="module")
def sentinel():
    return H.sentinel(20 << 20)


@pytest.fixture(scope="module")
def dev(table, sentinel):
    return H.device_buffers(np.frombuffer(table[0], dtype=np.uint8), sentinel)


@pytest.fixture(scope="module")
def batch(pkg):
    b = pkg.Batch(1)   # (the number of segments is not bound by max_streams)
    yield b
    b.close()


def _undbp(batch, dev, src, sentinel, segs, size, d_src=None):
    """segs: [(source offset, source length, destination offset, cap, width)] -> one call into a fresh destination of `size` bytes, the whole
    destination and all results compared; d_src: the device's copy of src where it is not the module's source"""
    src = bytes(src)
    return H.counted_call(batch.undbp_segments, ref.elements_bytes, ("src", "len", "dst", "cap", "w"), dev, src,
                          _upload(src) if d_src is None else d_src, sentinel, segs, size)


def _lay(datas, offs, widths, start=2, caps=None):
    """-> (segments with room for all their values (or caps), the destination's size)"""
    segs, d_at = [], start
    for i, (d, o, w) in enumerate(zip(datas, offs, widths)):
        count = ref.decode(d, w, 0)[1][0]
        cap = count if caps is None else caps[i]
        segs.append((o, len(d), d_at, cap, w))
        d_at += min(cap, count) * w + i % 5
    return segs, d_at + 16


def test_three_thousand_short_segments_and_the_host_hook(pkg, batch, dev, table, sentinel):
    """more than two chunks of a thousand segments, every ending, every alignment of source and destination; the kernels' results and bytes
    are the host hook's"""
    src, segs, size = table
    assert {s[0] % 16 for s in segs} == set(range(16)) and {s[2] % 16 for s in segs} == set(range(16))
    got = _undbp(batch, dev, src, sentinel, segs, size, d_src=dev["src"])
    assert batch.last_undbp_ms() > 0.0
    assert all(batch.last_undbp_ms(p) > 0.0 for p in (1, 2, 3, 4)) and batch.last_undbp_ms(5) == 0.0
    hook_dst, hook_res = pkg.undbp_host(src, segs, size, fill=sentinel[:size].tobytes())
    assert hook_res == got
    assert hook_dst == dev["dst"][:size].cpu().numpy().tobytes()


def test_one_long_segment_and_a_second_behind_it(pkg, batch, dev, sentinel):
    """a segment of so many items that the carry launch takes more than two passes, which every block shares, and a second one of another
    shape right behind it in the source and in the destination; fields of one bit, so that the source stays a few MiB"""
    C, span = pkg.undbp_item_deltas(), pkg.undelta_carry_span()
    n = (2 * span + 3) * C + 77
    bits = np.random.default_rng(41).integers(0, 2, size=n, dtype=np.uint8)
    first = ref.encode_bits(bits, first=-5)
    second = ref.encode(ref.random_values(random.Random(42), 9 * C + 5, 21), 256, 4)
    src, offs = _pack([first, second], start=5, gap=lambda i: 0)
    counts = [n + 1, 9 * C + 5]
    assert (counts[0] - 1 + C - 1) // C > 2 * span and len(src) < 5 << 20
    d1 = 12 + counts[0]
    segs = [(offs[0], len(first), 12, counts[0], 1), (offs[1], len(second), d1, counts[1], 8)]
    got = _undbp(batch, dev, src, sentinel, segs, d1 + 8 * counts[1] + 64)
    assert got[0][4] == got[1][4] == ref.OK and got[0][0] == n + 1


def test_more_items_than_a_carry_pass_at_width_four(pkg, batch, dev, sentinel):
    """the long segment's first items once more with elements of four bytes at a destination that is no multiple of four"""
    C = pkg.undbp_item_deltas()
    bits = np.random.default_rng(43).integers(0, 2, size=300 * C + 5, dtype=np.uint8)
    data = ref.encode_bits(bits, first=1 << 40, B=1024, M=8)
    src, offs = _pack([data], start=7)
    _undbp(batch, dev, src, sentinel, [(offs[0], len(data), 13, len(bits) + 1, 4)], 13 + 4 * (len(bits) + 1) + 64)


def test_block_headers_across_the_walk_chunks(pkg, batch, dev, sentinel):
    """a block whose ten-byte min_delta and width bytes straddle a chunk's edge at each of their bytes, at several skews of the source and at the
    first and a later edge"""
    chunk = pkg.undbp_walk_chunk()
    rnd = random.Random(44)
    datas, skews = [], []
    for edge in (1, 2):
        for back in range(0, 15):   # the block begins `back` bytes in front of the edge
            skew = (3 * len(datas) + 1) % 16
            target = edge * chunk - skew - back
            values = ref.random_values(rnd, 1 + 128 * (edge + 2) + 40, 3)
            for pad in range(2, 6):   # the header's length makes the rest a multiple of four
                hdr = 2 + 1 + pad + len(ref.varint(ref.zigzag(values[0])))
                if (target - hdr - 5 * edge) % 4 == 0:
                    break
            total = (target - hdr - 5 * edge) // 4   # the widths of the blocks in front, together
            table = [total // (4 * edge) + (1 if i < total % (4 * edge) else 0) for i in range(4 * edge)]
            assert max(table) <= 64 and min(table) >= 4
            data = ref.encode(values, 128, 4, widen=lambda b, j, k: table[4 * b + j] if b < edge else k,
                              vlen=lambda p: pad if p == "N" else 10 if p == ("min", edge) else 1 if isinstance(p, tuple) and p[1] < edge else 0)
            assert ref.block_offsets(data)[edge] == target
            datas.append(data)
            skews.append(skew)
    src, offs = bytearray(), []
    for d, skew in zip(datas, skews):
        src += b"\x80" * ((skew - len(src)) % 16)   # (continuation bytes between the segments: nothing may be read as a varint there)
        offs.append(len(src))
        src += d
    segs, size = _lay(datas, offs, [[2, 4, 8][i % 3] for i in range(len(datas))], start=1)
    got = _undbp(batch, dev, bytes(src), sentinel, segs, size)
    assert all(r[4] == ref.OK for r in got)


def test_shapes_and_item_edges(pkg, batch, dev, sentinel):
    """N around a group, a miniblock, a block and an item for every (B, M); the block of mixed widths; sums that wrap at 64 bits"""
    C = pkg.undbp_item_deltas()
    rnd = random.Random(45)
    datas, widths = [], []
    for B, M in [(128, 1), (128, 4), (256, 4), (1024, 8), (1024, 32), (65536, 4)]:
        V = B // M
        for n in sorted({0, 1, 2, 33, 34, V + 1, V + 2, B + 1, B + 2, C, C + 1, C + 2, 2 * C + 1}):
            if B == 65536 and n > 2 * C + 1:
                continue
            datas.append(ref.encode(ref.random_values(rnd, n, rnd.choice([0, 1, 7, 12, 30])), B, M)); widths.append(rnd.choice(ref.WIDTHS))
    datas.append(ref.encode(ref.random_values(rnd, 65536 + 2, 5), 65536, 4)); widths.append(2)
    mixed, B, M, _ = ref.mixed_width_block(rnd)
    for w in ref.WIDTHS:
        datas.append(ref.encode(mixed, B, M, mins=lambda b, lo: 0)); widths.append(w)
        datas.append(ref.encode([0, -(1 << 63), 5, 5 - (1 << 63), (1 << 64) - 1, 0, 1 << 63] * 700, 128, 4)); widths.append(w)
    datas.append(ref.encode(ref.random_values(rnd, 3 * C + 9, 9), 256, 8, widen=lambda b, j, k: [k, 64, k + 1, 33][(b + j) % 4])); widths.append(8)
    for data, _, _ in ref.PINNED:
        datas.append(data); widths.append(8)
    src, offs = _pack(datas)
    segs, size = _lay(datas, offs, widths)
    got = _undbp(batch, dev, src, sentinel, segs, size)
    assert all(r[4] == ref.OK for r in got)
    assert got[-4:] == [(len(v), c, len(v), 1 if len(v) > 1 else 0, ref.OK, 128, 4) for _, v, c in ref.PINNED]


def test_counting_alone_and_small_capacities(pkg, batch, dev, sentinel):
    """a call whose capacities are all 0 needs no destination and gives the results of the call that writes; cap < count writes cap elements
    and nothing behind them"""
    C = pkg.undbp_item_deltas()
    rnd = random.Random(46)
    widths = [1, 4, 8, 2, 2]
    datas = [ref.encode(ref.random_values(rnd, n, 14), 128, 4) for n in [0, 50, 5 * C + 3, 3 * C, C]]
    src, offs = _pack(datas)
    d_src = _upload(src)
    sp = d_src.data_ptr()
    want = [ref.decode(d, w, 0)[1] for d, w in zip(datas, widths)]
    args = ([sp + o for o in offs], [len(d) for d in datas])
    assert batch.undbp_segments(*args, None, [0] * 5, widths) == want
    assert batch.last_undbp_ms(1) > 0.0 and all(batch.last_undbp_ms(p) == 0.0 for p in (2, 3, 4))   # (counting is the walk alone)
    assert batch.undbp_segments(*args, [None] * 5, [0] * 5, widths, [0] * 5) == want
    segs, size = _lay(datas, offs, widths, start=3, caps=[4, 17, 2 * C + 1, 10 ** 9, C - 1])
    assert _undbp(batch, dev, src, sentinel, segs, size + 64, d_src=d_src) == want
    segs, size = _lay(datas, offs, widths, start=3, caps=[1, 1, C + 1, C, 2])
    assert _undbp(batch, dev, src, sentinel, segs, size + 64, d_src=d_src) == want


def test_every_status(pkg, batch, dev, sentinel):
    """every stop at the first, a middle and the last block, and in the header: the status, and the bytes in front of the stop"""
    rnd = random.Random(47)
    datas, widths = [], []
    for B, M in [(128, 4), (1024, 8)]:
        values = ref.random_values(rnd, 1 + 30 * B, 9)
        for _, tail, _, _, _ in ref.stops(B, M):
            for front in (0, 7, 30):
                datas.append(ref.encode(values[:1 + front * B], B, M, declared=1 + (front + 1) * B) + tail); widths.append(rnd.choice(ref.WIDTHS))
    datas += [ref.varint(64) + ref.varint(2) + ref.varint(5) + ref.varint(0) + bytes(50), b"\x80" * 10 + b"\x00" + bytes(50), b"", b"\x80\x01\x04"]
    widths += [4, 4, 4, 4]
    src, offs = _pack(datas)
    segs, d_at = [], 6
    for d, o, w in zip(datas, offs, widths):
        count = ref.decode(d, w, 0)[1][0]
        segs.append((o, len(d), d_at, count + 3, w))
        d_at += count * w + 3
    got = _undbp(batch, dev, src, sentinel, segs, d_at + 16)
    assert {r[4] for r in got} == {ref.BAD_HEADER, ref.BAD_WIDTH, ref.TRUNCATED} and sum(1 for r in got if r[0] > 30 * 128) >= 6


def test_bad_arguments_launch_nothing(pkg, batch, dev, sentinel):
    _fresh_dst(dev, 4096)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    three = ([sp, sp + 100, sp + 200], [100] * 3, [dp, dp + 1000, dp + 2000], [10] * 3)
    for bad in (3, 0, 16, 255):
        with pytest.raises(RuntimeError, match="undbp segment 1: width is not 1, 2, 4 or 8"):
            batch.undbp_segments(*three, [4, bad, 2])
    for flag in (1, 2, 128):
        with pytest.raises(RuntimeError, match="undbp segment 2: unknown flag bits"):
            batch.undbp_segments(*three, [4, 8, 2], [0, 0, flag])
    with pytest.raises(RuntimeError, match=r"undbp segment 0: a capacity above 2\^56"):
        batch.undbp_segments([sp], [100], [dp], [(1 << 56) + 1], [1])
    with pytest.raises(RuntimeError, match="undbp segment 1: no destination"):
        batch.undbp_segments([sp, sp + 100], [100] * 2, [dp, None], [10, 10], [4, 4])
    H.compare(dev, sentinel[:4096])
    assert batch.last_undbp_ms() == 0.0   # (nothing was launched)
    assert batch.undbp_segments([], [], [], [], []) == []
    assert batch.undbp_segments([sp + 7, sp + 7], [0, 0], [dp, dp], [5, 5], [4, 8]) == [(0, 0, 0, 0, ref.TRUNCATED, 0, 0)] * 2
    H.compare(dev, sentinel[:4096])


def test_golden_pages(pkg, batch, dev, sentinel):
    """the page bodies that pyarrow wrote (tests/golden/dbp/) decode to their columns, and end exactly at the page's end"""
    import dbp_pages
    pages = dbp_pages.load()
    assert len(pages) == 30
    datas = [body for _, body, _ in pages]
    src, offs = _pack(datas)
    segs, d_at = [], 4
    for (e, body, column), o in zip(pages, offs):
        segs.append((o, len(body), d_at, e["values"], e["bits"] // 8))
        d_at += len(column) + 1
    got = _undbp(batch, dev, src, sentinel, segs, d_at + 16)
    host = dev["dst"][:d_at].cpu().numpy().tobytes()
    for (e, body, column), s, r in zip(pages, segs, got):
        assert r[:3] == (e["values"], len(body), e["values"]) and r[4] == ref.OK, e["label"]
        assert host[s[2]:s[2] + len(column)] == column, e["label"]


# ------------------------------------------------------------------ the outputs of a decode call
@pytest.fixture(scope="module")
def arrays():
    """seeded columns -> [(the values as a numpy array, width, their stream's bytes with bytes behind the last block for some, the brotli stream)]"""
    rnd = random.Random(48)
    out = []
    for m, w, B, M, trail in [(0, 2, 128, 4, 0), (1, 4, 128, 4, 3), (7, 2, 128, 4, 0), (7, 8, 256, 4, 0), (4096, 2, 128, 4, 0), (4096, 4, 256, 4, 40),
                              (4096, 1, 1024, 8, 0), (100003, 4, 128, 4, 0), (33, 8, 128, 1, 0)]:
        values = ref.random_values(rnd, m, 8 * w if m < 1000 else 11)
        raw = ref.encode(values, B, M) + bytes(rnd.randrange(256) for _ in range(trail))
        out.append((np.array([v & ((1 << (8 * w)) - 1) for v in values], dtype="<u%d" % w), w, raw, _stream(raw)))
    return out


def _check_outputs(b, dev, sentinel, arrays, skip):
    """undbp_outputs of the arrays' streams into a fresh destination: the original values, their results, and sentinel in the slot that was
    skipped, whose result is zeros"""
    offs, size = _slots([x.nbytes for x, *_ in arrays], skip)
    want = sentinel[:size].copy()
    for (x, *_), o in zip(arrays, offs):
        if o is not None:
            want[o:o + x.nbytes] = np.frombuffer(x.tobytes(), dtype=np.uint8)
    _fresh_dst(dev, size)
    dp = dev["dst"].data_ptr()
    full = [ref.decode(raw, w, 0)[1] for _, w, raw, _ in arrays]
    got = b.undbp_outputs([None if o is None else dp + o for o in offs], [len(a[0]) for a in arrays], [a[1] for a in arrays])
    assert got == [ZEROS if o is None else r for r, o in zip(full, offs)]
    assert all(r[4] == ref.OK and r[0] == len(a[0]) for r, a in zip(full, arrays)) and full[5][1] == len(arrays[5][2]) - 40
    H.compare(dev, want)
    assert b.count_dbp_outputs() == full
    H.compare(dev, want)   # (counting writes nothing)


def test_outputs_of_decode_device(pkg, dev, sentinel, arrays):
    import torch
    datas, caps = [a[3] for a in arrays], [len(a[2]) for a in arrays]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(sum(caps) + 64, dtype=torch.uint8, device="cuda")   # the outputs back to back, at whatever alignment that gives
    offs = [sum(caps[:i]) + 3 for i in range(len(caps))]
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        with pytest.raises(RuntimeError, match="no decode call"):
            b.out_n = len(datas)
            b.count_dbp_outputs()
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.count_dbp_outputs()
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, n) for n in caps]
        ms, digests = b.last_kernel_ms(), b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={5})
        assert b.last_kernel_ms() == ms and b.digest_outputs() == digests   # (not a decode call: the accessors say what they said)
        with pytest.raises(RuntimeError, match="undbp stream 0: width"):
            b.undbp_outputs([dev["dst"].data_ptr() + 4096 * i for i in range(len(datas))], [1] * len(datas), [3] * len(datas))
    finally:
        b.close()


def test_outputs_of_decode_host_and_packed(pkg, dev, sentinel, arrays):
    b = pkg.Batch(len(arrays))
    try:
        results, outs = b.decode_host([a[3] for a in arrays], [len(a[2]) for a in arrays], FLAGS)
        assert [r.result for r in results] == [1] * len(arrays) and outs == [a[2] for a in arrays]
        _check_outputs(b, dev, sentinel, arrays, skip={0, 7})
        results, outs = b.decode_packed([a[3] for a in arrays], flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(a[2])) for a in arrays]
        view, launches = b._packed_view(len(arrays)), b.last_packed_launches()
        _check_outputs(b, dev, sentinel, arrays, skip={8})
        assert b._packed_view(len(arrays)) == view and view[0] != 0 and b.last_packed_launches() == launches   # BrotliAmdBatchPackedOutput still returns the buffer
    finally:
        b.close()


def test_truncated_delivery(pkg, dev, sentinel, arrays):
    """a stream given less room than it needs (with the eager limit) and a corrupt one: exactly decoded_size bytes are taken, and the blocks that
    their end cuts are reported as the reference reports them"""
    import torch
    x, w, raw, stream = arrays[4]   # 4096 values
    borked = open(os.path.join(ROOT, "tests", "golden", "testdata", "borked.compressed"), "rb").read()
    datas, caps, widths = [stream, borked, stream], [1003, 4096, len(raw)], [2, 1, 2]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(2 * 4096 + 2 * len(raw) + 64, dtype=torch.uint8, device="cuda")
    offs = [1, len(raw) + 2, len(raw) + 4096 + 3]
    torch.cuda.synchronize()
    b = pkg.Batch(3)
    try:
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS | EAGER)
        results = b.wait()
        assert [r.result for r in results] == [3, 0, 1], [r.result for r in results]
        sizes = [r.decoded_size for r in results]
        assert sizes[0] == 1003 and sizes[2] == len(raw)
        host = arena.cpu().numpy()
        delivered = [host[o:o + n].tobytes() for o, n in zip(offs, sizes)]
        assert delivered[0] == raw[:1003]
        segs, d_at = [], 5
        for d, ww in zip(delivered, widths):
            count = ref.decode(d, ww, 0)[1][0]
            segs.append((0, len(d), d_at, min(count, 100000), ww))
            d_at += min(count, 100000) * ww
        want = sentinel[:d_at + 64].copy()
        want_res = []
        for d, (_, _, o, cap, ww) in zip(delivered, segs):
            elems, res = ref.elements_bytes(d, ww, cap)
            want[o:o + len(elems)] = np.frombuffer(elems, dtype=np.uint8)
            want_res.append(res)
        _fresh_dst(dev, d_at + 64)
        got = b.undbp_outputs([dev["dst"].data_ptr() + s[2] for s in segs], [s[3] for s in segs], widths)
        assert got == want_res and got[0][4] == ref.TRUNCATED and got[0][1] == 1003 and got[2][:2] == (len(x), len(raw))
        H.compare(dev, want)
    finally:
        b.close()


def test_outputs_as_tensors(pkg, dev):
    import torch
    import delta_ref
    tensors = H.tensors_module()
    g = torch.Generator().manual_seed(49)
    ids = torch.cumsum(torch.randint(0, 5, (1000,), generator=g, dtype=torch.int64), 0)
    originals = [(torch.randint(-(1 << 20), 1 << 20, (33, 7), generator=g, dtype=torch.int32), ("dbp",), 0),
                 (torch.randint(0, 256, (257,), generator=g, dtype=torch.uint8), ("dbp",), 9),   # bytes behind the last block
                 (ids, ("dbp", "delta"), 0),
                 (torch.randint(-(1 << 62), 1 << 62, (4096,), generator=g, dtype=torch.int64), ("dbp",), 0),
                 (torch.randn((3, 5), generator=g), None, 0),                                  # a plain 2-tuple: shuffled
                 (torch.randint(0, 200, (11,), generator=g, dtype=torch.uint8), None, 0),    # the stream that is skipped
                 (ids[:77].to(torch.int16), ("dbp", "delta"), 0)]

    def encode(t, flt, trail):
        import shuffle_ref
        raw, w = t.contiguous().view(torch.uint8).numpy().tobytes(), t.element_size()
        if flt is None:
            return _stream(shuffle_ref.shuffle(raw, w))
        if "delta" in flt:
            raw = delta_ref.delta(raw, w)
        return _stream(ref.encode(np.frombuffer(raw, dtype="<u%d" % w).tolist(), 128, 4) + b"\x5a" * trail)

    streams = [encode(t, f, trail) for t, f, trail in originals]
    b = pkg.Batch(len(streams))
    try:
        results, _ = b.decode_packed(streams, flags=FLAGS)
        assert [r.result for r in results] == [1] * len(streams)
        specs = [(t.dtype, tuple(t.shape)) if f is None else (t.dtype, tuple(t.shape), f) for t, f, _ in originals]
        specs[5] = None
        got = tensors.outputs_as_tensors(b, specs)
        assert got[5] is None
        for i, (t, (o, _, _)) in enumerate(zip(got, originals)):
            if t is None:
                continue
            assert t.is_cuda and t.dtype == o.dtype and tuple(t.shape) == tuple(o.shape) and t.data_ptr() % 64 == 0, i
            assert torch.equal(t.cpu().view(torch.uint8), o.contiguous().view(torch.uint8)), i
        assert len({t.untyped_storage().data_ptr() for t in got if t is not None}) == 1   # views of one buffer

        def wrong(i, spec):
            return [spec if k == i else s for k, s in enumerate(specs)]

        for shape in ((300,), (250,)):   # another number of values than numel, more or fewer
            with pytest.raises(ValueError, match=r"stream 1: 257 values in its blocks, but shape"):
                tensors.outputs_as_tensors(b, wrong(1, (torch.uint8, shape, ("dbp",))))
        for other in ("shuffle", "bitshuffle", ("bitpack", 3), "varint", "rle"):
            with pytest.raises(ValueError, match="stream 0: \"dbp\" stands alone"):
                tensors.outputs_as_tensors(b, wrong(0, (torch.int32, (33, 7), ("dbp", other))))
        with pytest.raises(ValueError, match="stream 0: \"dbp\" stands alone"):
            tensors.outputs_as_tensors(b, wrong(0, (torch.int32, (33, 7), ("delta", "dbp"))))
        # streams that do not end well are refused
        body = ref.encode([1, 2, 3], 128, 4)
        results, _ = b.decode_packed([_stream(body[:-1]), _stream(ref.varint(64) + body[2:]), _stream(body[:6] + b"\x41" + body[7:])], flags=FLAGS)
        with pytest.raises(ValueError, match=r"stream 0: blocks that the stream's end cuts \(status 3\) after 1 of 3 declared values"):
            tensors.outputs_as_tensors(b, [(torch.uint8, (3,), ("dbp",)), None, None])
        with pytest.raises(ValueError, match=r"stream 1: a header that is none \(status 1\)"):
            tensors.outputs_as_tensors(b, [None, (torch.uint8, (3,), ("dbp",)), None])
        with pytest.raises(ValueError, match=r"stream 2: a miniblock of more than 64 bits \(status 2\)"):
            tensors.outputs_as_tensors(b, [None, None, (torch.uint8, (3,), ("dbp",))])
    finally:
        b.close()
