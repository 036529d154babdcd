"""Unrle on the device (needs a real MI355X): the kernels (csrc/brotli_unrle_kernels.hip) through BrotliAmdBatchUnrleSegments,
BrotliAmdBatchUnrleOutputs after the three kinds of decode call, and tensors.outputs_as_tensors, against the reference (rle_ref.py) and against
the host hook.  Destinations come from one buffer prefilled with a sentinel pattern, and the WHOLE destination buffer is compared with the
expectation: a byte written outside a segment's elements fails the test.  All comparisons are exact."""
import os
import random

import numpy as np
import pytest

import rle_ref as ref
import seg_filter_harness as H
from conftest import ROOT
from seg_filter_harness import fresh_dst as _fresh_dst, pack as _pack, stream as _stream, slots as _slots, upload as _upload

pytestmark = pytest.mark.gpu
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT


@pytest.fixture(scope="module")
def table():
    """the table of the tests without a device -> (source, segments, destination size)"""
    return ref.short_table()


@pytest.fixture(scope="module")
def sentinel():
    return H.sentinel(3 << 20)


@pytest.fixture(scope="module")
def dev(table, sentinel):
    return H.device_buffers(np.frombuffer(table[0], dtype=np.uint8), sentinel)


@pytest.fixture(scope="module")
def batch(pkg):
    b = pkg.Batch(1)   # (the number of segments is not bound by max_streams)
    yield b
    b.close()


def _unrle(batch, dev, src, sentinel, segs, size, d_src=None):
    """segs: [(source offset, source length, destination offset, cap, bits, width, flags)] -> one call into a fresh destination of `size` bytes,
    the whole destination and all results compared; d_src: the device's copy of src where it is not the module's source"""
    src = bytes(src)
    return H.counted_call(batch.unrle_segments, ref.elements_bytes, ("src", "len", "dst", "cap", "bits", "w", "flags"), dev, src,
                          _upload(src) if d_src is None else d_src, sentinel, segs, size)


def test_three_thousand_short_segments_and_the_host_hook(pkg, batch, dev, table, sentinel):
    """more than two chunks of a thousand segments, every shape, every ending, every alignment of source and destination; the kernels' results
    and bytes are the host hook's"""
    src, segs, size = table
    assert {s[0] % 16 for s in segs} == set(range(16)) and {s[2] % 16 for s in segs} == set(range(16))
    got = _unrle(batch, dev, src, sentinel, segs, size, d_src=dev["src"])
    assert batch.last_unrle_ms() > 0.0
    assert all(batch.last_unrle_ms(p) > 0.0 for p in (1, 2)) and batch.last_unrle_ms(3) == 0.0
    hook_dst, hook_res = pkg.unrle_host(src, segs, size, fill=sentinel[:size].tobytes())
    assert hook_res == got
    assert hook_dst == dev["dst"][:size].cpu().numpy().tobytes()


def test_one_long_segment_and_a_second_behind_it(pkg, batch, dev, sentinel):
    """a segment of a few hundred items, which several blocks share, and a second one of another shape right behind it in the source and in
    the destination"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(31)
    first = ref.encode(ref.random_plan(rnd, 12, 300 * C + 77, hlen=True), 12)
    second = ref.encode(ref.random_plan(rnd, 7, 9 * C + 5, packed=(8, 64), repeated=(1, 70)), 7, True)
    src, offs = _pack([first, second], start=5, gap=lambda i: 0)
    counts = [ref.decode(first, 12, 4, 0, 0)[1][0], ref.decode(second, 0, 1, 1, 0)[1][0]]
    assert counts[0] > 300 * C
    d1 = 12 + 4 * counts[0]
    segs = [(offs[0], len(first), 12, counts[0], 12, 4, 0), (offs[1], len(second), d1, counts[1], 0, 1, ref.WIDTH_BYTE)]
    got = _unrle(batch, dev, src, sentinel, segs, d1 + counts[1] + 64)
    assert got[0][3] == got[1][3] == ref.OK and got[1][4] == 7
    # the same at a destination that is no multiple of the width: element by element
    segs = [(offs[0], len(first), 13, counts[0], 12, 4, 0), (offs[1], len(second), d1 + 1, counts[1], 0, 1, ref.WIDTH_BYTE)]
    _unrle(batch, dev, src, sentinel, segs, d1 + counts[1] + 64)


def _filler(rnd, upto):
    """runs of 16-bit fields -- 3 bytes a repeated one, 17 a packed one -- that take exactly `upto` bytes"""
    assert upto >= 34
    plan, b = [], 2 * upto % 3   # (17 b is 2 b mod 3)
    for _ in range(b):
        plan.append(("packed", [rnd.randrange(1 << 16) for _ in range(8)]))
    for _ in range((upto - 17 * b) // 3):
        plan.append(("rle", rnd.randrange(1, 9), rnd.randrange(1 << 16)))
    rnd.shuffle(plan)
    assert len(ref.encode(plan, 16)) == upto
    return plan


def test_headers_and_values_across_the_walk_chunks(pkg, batch, dev, sentinel):
    """headers of 1 .. 5 bytes whose bytes straddle a chunk's edge at each of their bytes, repeated values that straddle it, and a packed payload
    that skips more than two chunks, at several skews of the source and at the first and a later edge"""
    chunk = pkg.unrle_walk_chunk()
    rnd = random.Random(32)
    datas, skews = [], []
    for edge in (1, 2):
        for hl in range(1, 6):
            for back in range(0, hl + 2):   # the header begins `back` bytes in front of the edge: back == hl + 1 leaves one byte of the value in front
                skew = (3 * len(datas) + 1) % 16
                plan = _filler(rnd, edge * chunk - skew - back)
                plan.append(("rle", 5, 0xABCD, hl))
                plan.append(("packed", [rnd.randrange(1 << 16) for _ in range(8 * 200)], 2))   # 3200 bytes: the stage jumps
                plan += [("rle", 3, 7, hl), ("packed", [1, 2, 3, 4, 5, 6, 7, 8], hl), ("rle", 2, 0xFFFF)]
                datas.append(ref.encode(plan, 16))
                skews.append(skew)
    src, offs = bytearray(), []
    for d, skew in zip(datas, skews):
        src += b"\x80" * ((skew - len(src)) % 16)   # (continuation bytes between the segments: nothing may be read as a header there)
        offs.append(len(src))
        src += d
    segs, d_at = [], 1
    for i, (d, o) in enumerate(zip(datas, offs)):
        count = ref.decode(d, 16, 2, 0, 0)[1][0]
        segs.append((o, len(d), d_at, count, 16, [2, 4, 8][i % 3], 0))
        d_at += count * segs[-1][5] + i % 3
    got = _unrle(batch, dev, bytes(src), sentinel, segs, d_at + 16)
    assert all(r[3] == ref.OK for r in got)


def test_runs_across_item_edges(pkg, batch, dev, sentinel):
    """a repeated run and a packed run that each span three items, packed groups that are not aligned to the items, and more than 64 runs in one
    item"""
    C = pkg.unrle_item_elems()
    datas, shapes = [], []
    for k, w in [(3, 1), (12, 2), (12, 4), (17, 4), (32, 8), (0, 1), (1, 8)]:
        for lead in (1, 3, 5):
            datas.append(ref.encode(ref.straddling_plans(k, C, lead), k)); shapes.append((k, w))
        datas.append(ref.encode(ref.many_runs_plan(k, C + C // 2, k), k)); shapes.append((k, w))
    src, offs = _pack(datas)
    segs, d_at = [], 2
    for i, (d, o, (k, w)) in enumerate(zip(datas, offs, shapes)):
        count = ref.decode(d, k, w, 0, 0)[1][0]
        segs.append((o, len(d), d_at, count, k, w, 0))
        d_at += count * w + i % 5
    got = _unrle(batch, dev, src, sentinel, segs, d_at + 16)
    assert all(r[3] == ref.OK for r in got) and max(r[2] for r in got) > C


def test_counting_alone_and_small_capacities(pkg, batch, dev, sentinel):
    """a call whose capacities are all 0 needs no destination and gives the results of the call that writes; cap < count writes cap elements
    and nothing behind them"""
    C = pkg.unrle_item_elems()
    rnd = random.Random(33)
    shapes = [(5, 1), (12, 4), (20, 8), (0, 2), (9, 2)]
    datas = [ref.encode(ref.random_plan(rnd, k, n, packed=(8, 200), repeated=(1, 300)), k) for (k, _), n in zip(shapes, [0, 50, 5 * C + 3, 3 * C, C])]
    src, offs = _pack(datas)
    d_src = _upload(src)
    sp = d_src.data_ptr()
    want = [ref.decode(d, k, w, 0, 0)[1] for d, (k, w) in zip(datas, shapes)]
    args = ([sp + o for o in offs], [len(d) for d in datas])
    assert batch.unrle_segments(*args, None, [0] * 5, [k for k, _ in shapes], [w for _, w in shapes]) == want
    assert batch.last_unrle_ms(1) > 0.0 and batch.last_unrle_ms(2) == 0.0   # (counting is the walk alone)
    assert batch.unrle_segments(*args, [None] * 5, [0] * 5, [k for k, _ in shapes], [w for _, w in shapes], [0] * 5) == want
    segs, d_at = [], 3
    for d, o, (k, w), res, cap in zip(datas, offs, shapes, want, [4, 17, 2 * C + 1, 10 ** 9, C - 1]):
        segs.append((o, len(d), d_at, cap, k, w, 0))
        d_at += min(cap, res[0]) * w + 1   # (the next one begins one byte behind: a store beyond cap would hit it, or the sentinel between)
    assert _unrle(batch, dev, src, sentinel, segs, d_at + 64, d_src=d_src) == want


def test_every_status(pkg, batch, dev, sentinel):
    """every stop behind a few runs: the status, and the bytes in front of the stop"""
    rnd = random.Random(34)
    datas, shapes = [], []
    for k, w in [(3, 1), (12, 4), (32, 8)]:
        plan = ref.random_plan(rnd, k, 2500, packed=(8, 24), repeated=(1, 300))
        for _, tail, _ in ref.stops(k):
            datas.append(ref.encode(plan, k) + tail); shapes.append((k, w, 0))
        datas.append(b"\x21" + ref.encode(plan, k)); shapes.append((0, w, ref.WIDTH_BYTE))
    datas.append(b""); shapes.append((0, 4, ref.WIDTH_BYTE))
    src, offs = _pack(datas)
    segs, d_at = [], 6
    for d, o, (k, w, f) in zip(datas, offs, shapes):
        count = ref.decode(d, k, w, f, 0)[1][0]
        segs.append((o, len(d), d_at, count + 3, k, w, f))
        d_at += count * w + 3
    got = _unrle(batch, dev, src, sentinel, segs, d_at + 16)
    assert {r[3] for r in got} == {ref.BAD_HEADER, ref.ZERO_RUN, ref.TRUNCATED, ref.BAD_WIDTH} and sum(1 for r in got if r[0] > 2500) >= 15


def test_bad_arguments_launch_nothing(pkg, batch, dev, sentinel):
    _fresh_dst(dev, 4096)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    three = ([sp, sp + 100, sp + 200], [100] * 3, [dp, dp + 1000, dp + 2000], [10] * 3)
    for bad in (3, 0, 16, 255):
        with pytest.raises(RuntimeError, match="unrle segment 1: width is not 1, 2, 4 or 8"):
            batch.unrle_segments(*three, [3] * 3, [4, bad, 2])
    with pytest.raises(RuntimeError, match="unrle segment 2: unknown flag bits"):
        batch.unrle_segments(*three, [3] * 3, [4, 8, 2], [0, 1, 2])
    with pytest.raises(RuntimeError, match="unrle segment 1: field of more than 32 bits"):
        batch.unrle_segments(*three, [3, 33, 3], [4, 8, 2])
    with pytest.raises(RuntimeError, match="unrle segment 0: field is wider than the element"):
        batch.unrle_segments(*three, [17, 3, 3], [2, 8, 2])
    with pytest.raises(RuntimeError, match=r"unrle segment 0: a capacity above 2\^56"):
        batch.unrle_segments([sp], [100], [dp], [(1 << 56) + 1], [3], [1])
    with pytest.raises(RuntimeError, match="unrle segment 1: no destination"):
        batch.unrle_segments([sp, sp + 100], [100] * 2, [dp, None], [10, 10], [3, 3], [4, 4])
    H.compare(dev, sentinel[:4096])
    assert batch.last_unrle_ms() == 0.0   # (nothing was launched)
    assert batch.unrle_segments([], [], [], [], [], []) == []
    assert batch.unrle_segments([sp + 7, sp + 7], [0, 0], [dp, dp], [5, 5], [3, 9], [4, 8], [0, 1]) == [(0, 0, 0, ref.OK, 3), (0, 0, 0, ref.BAD_WIDTH, 0)]
    H.compare(dev, sentinel[:4096])


# ------------------------------------------------------------------ the outputs of a decode call
@pytest.fixture(scope="module")
def arrays():
    """seeded values as runs, of at least 0, 1, 7, 4096 and 100 003 values (a plan ends with its last run) -> [(the values as a numpy array, k, width, flags, their runs' bytes, the stream)]"""
    rnd = random.Random(35)
    out = []
    for m, k, w, f in [(0, 3, 2, 0), (1, 4, 4, 0), (7, 9, 2, 1), (7, 32, 8, 0), (4096, 12, 2, 0), (4096, 12, 4, 1), (4096, 1, 1, 1), (100003, 20, 4, 0), (33, 0, 4, 0)]:
        plan = ref.random_plan(rnd, k, m, packed=(8, 504), repeated=(1, 2000)) if m else []
        raw = ref.encode(plan, k, bool(f))
        vals = np.array(ref.plan_values(plan), dtype="<u%d" % w)   # (the last packed group's padding included)
        out.append((vals, k, w, f, raw, _stream(raw)))
    return out


def _check_outputs(b, dev, sentinel, arrays, skip):
    """unrle_outputs of the arrays' streams into a fresh destination: the original values, their results, and sentinel in the slot that was
    skipped, whose result is zeros"""
    offs, size = _slots([x.nbytes for x, *_ in arrays], skip)
    want = sentinel[:size].copy()
    for (x, *_), o in zip(arrays, offs):
        if o is not None:
            want[o:o + x.nbytes] = np.frombuffer(x.tobytes(), dtype=np.uint8)
    _fresh_dst(dev, size)
    dp = dev["dst"].data_ptr()
    full = [ref.decode(raw, k, w, f, 0)[1] for _, k, w, f, raw, _ in arrays]
    got = b.unrle_outputs([None if o is None else dp + o for o in offs], [len(a[0]) for a in arrays], [9 if a[3] else a[1] for a in arrays], [a[2] for a in arrays],
                          [a[3] for a in arrays])
    assert got == [(0, 0, 0, 0, 0) if o is None else r for r, o in zip(full, offs)]
    assert all(r[3] == ref.OK and r[0] == len(a[0]) for r, a in zip(full, arrays))
    H.compare(dev, want)
    assert [r[:4] for r in b.count_rle_outputs([a[1] for a in arrays])] == [ref.decode(a[4], a[1], 4, 0, 0)[1][:4] for a in arrays]
    assert b.count_rle_outputs()[2] == full[2]   # (its first byte is its k)
    H.compare(dev, want)   # (counting writes nothing)


def test_outputs_of_decode_device(pkg, dev, sentinel, arrays):
    import torch
    datas, caps = [a[5] for a in arrays], [len(a[4]) for a in arrays]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(sum(caps) + 64, dtype=torch.uint8, device="cuda")   # the outputs back to back, at whatever alignment that gives
    offs = [sum(caps[:i]) + 3 for i in range(len(caps))]
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        with pytest.raises(RuntimeError, match="no decode call"):
            b.out_n = len(datas)
            b.count_rle_outputs()
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.count_rle_outputs()
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, n) for n in caps]
        ms, digests = b.last_kernel_ms(), b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={5})
        assert b.last_kernel_ms() == ms and b.digest_outputs() == digests   # (not a decode call: the accessors say what they said)
        with pytest.raises(RuntimeError, match="unrle stream 0: width"):
            b.unrle_outputs([dev["dst"].data_ptr() + 4096 * i for i in range(len(datas))], [1] * len(datas), [1] * len(datas), [3] * len(datas))
    finally:
        b.close()


def test_outputs_of_decode_host_and_packed(pkg, dev, sentinel, arrays):
    b = pkg.Batch(len(arrays))
    try:
        results, outs = b.decode_host([a[5] for a in arrays], [len(a[4]) for a in arrays], FLAGS)
        assert [r.result for r in results] == [1] * len(arrays) and outs == [a[4] for a in arrays]
        _check_outputs(b, dev, sentinel, arrays, skip={0, 7})
        results, outs = b.decode_packed([a[5] for a in arrays], flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(a[4])) for a in arrays]
        view, launches = b._packed_view(len(arrays)), b.last_packed_launches()
        _check_outputs(b, dev, sentinel, arrays, skip={8})
        assert b._packed_view(len(arrays)) == view and view[0] != 0 and b.last_packed_launches() == launches   # BrotliAmdBatchPackedOutput still returns the buffer
    finally:
        b.close()


def test_truncated_delivery(pkg, dev, sentinel, arrays):
    """a stream given less room than it needs (with the eager limit) and a corrupt one: exactly decoded_size bytes are taken, and the runs that
    their end cuts are reported as the reference reports them"""
    import torch
    x, k, w, f, raw, stream = arrays[4]   # 4096 values of 12 bits
    borked = open(os.path.join(ROOT, "tests", "golden", "testdata", "borked.compressed"), "rb").read()
    datas, caps, bits, widths = [stream, borked, stream], [1003, 4096, len(raw)], [12, 5, 12], [2, 1, 2]
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
        for d, kk, ww in zip(delivered, bits, widths):
            count = ref.decode(d, kk, ww, 0, 0)[1][0]
            segs.append((0, len(d), d_at, min(count, 100000), kk, ww, 0))
            d_at += min(count, 100000) * ww
        want = sentinel[:d_at + 64].copy()
        want_res = []
        for d, (_, _, o, cap, kk, ww, _) in zip(delivered, segs):
            elems, res = ref.elements_bytes(d, kk, ww, 0, cap)
            want[o:o + len(elems)] = np.frombuffer(elems, dtype=np.uint8)
            want_res.append(res)
        _fresh_dst(dev, d_at + 64)
        got = b.unrle_outputs([dev["dst"].data_ptr() + s[2] for s in segs], [s[3] for s in segs], bits, widths)
        assert got == want_res and got[0][1] <= 1003 and got[2] == (len(x), len(raw), got[2][2], ref.OK, 12)
        H.compare(dev, want)
    finally:
        b.close()


def test_outputs_as_tensors(pkg, dev):
    import torch
    import delta_ref
    tensors = H.tensors_module()
    g = torch.Generator().manual_seed(36)
    rnd = random.Random(37)
    ids = torch.cumsum(torch.randint(0, 5, (1000,), generator=g, dtype=torch.int64), 0)
    originals = [(torch.randint(0, 1 << 12, (33, 7), generator=g, dtype=torch.int32), 12, (("rle", 12),)),
                 (torch.randint(0, 1 << 5, (257,), generator=g, dtype=torch.uint8), 5, ("rle",)),
                 (ids, 3, (("rle", 3), "delta")),
                 (torch.randint(0, 2, (4096,), generator=g, dtype=torch.uint8), 1, ("rle",)),
                 (torch.randn((3, 5), generator=g), None, None),                                  # a plain 2-tuple: shuffled
                 (torch.randint(0, 200, (11,), generator=g, dtype=torch.uint8), None, None),    # the stream that is skipped
                 (ids[:77].to(torch.int16), 3, ("rle", "delta"))]

    def runs_of(values, k, width_byte):
        """seeded runs over the values: repeats as RLE runs where there are some, the rest in packed groups, the last one padded"""
        plan, i = [], 0
        while i < len(values):
            j = i
            while j < len(values) and values[j] == values[i]:
                j += 1
            if j - i >= 4 or rnd.random() < 0.1:
                plan.append(("rle", j - i, values[i])); i = j
            else:
                take = values[i:i + 8 * rnd.randrange(1, 5)]
                plan.append(("packed", take + [0] * (-len(take) % 8))); i += len(take)
        return ref.encode(plan, k, width_byte)

    def encode(t, k, flt):
        import shuffle_ref
        raw, w = t.contiguous().view(torch.uint8).numpy().tobytes(), t.element_size()
        if flt is None:
            return _stream(shuffle_ref.shuffle(raw, w))
        if "delta" in flt:
            raw = delta_ref.delta(raw, w)
        return _stream(runs_of(np.frombuffer(raw, dtype="<u%d" % w).tolist(), k, "rle" in flt))

    streams = [encode(t, k, f) for t, k, f in originals]
    b = pkg.Batch(len(streams))
    try:
        results, _ = b.decode_packed(streams, flags=FLAGS)
        assert [r.result for r in results] == [1] * len(streams)
        specs = [(t.dtype, tuple(t.shape)) if f is None else (t.dtype, tuple(t.shape), f) for t, _, f in originals]
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

        with pytest.raises(ValueError, match=r"stream 1: 2\d\d values in its runs, but shape"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.uint8, (300,), ("rle",))))
        tensors.outputs_as_tensors(b, wrong(1, (torch.uint8, (250,), ("rle",))))   # more values than numel: padding, not judged
        for other in ("shuffle", "bitshuffle", ("bitpack", 3), "varint"):
            with pytest.raises(ValueError, match="stream 0: \"rle\" with"):
                tensors.outputs_as_tensors(b, wrong(0, (torch.int32, (33, 7), (("rle", 12), other))))
        with pytest.raises(ValueError, match="stream 0: rle fields of 33 bits"):
            tensors.outputs_as_tensors(b, wrong(0, (torch.int64, (33, 7), (("rle", 33),))))
        with pytest.raises(ValueError, match="stream 1: rle fields of 9 bits"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.uint8, (257,), (("rle", 9),))))
        with pytest.raises(ValueError, match=r"stream 0: \(\"rle\", k\) names the field width"):
            tensors.outputs_as_tensors(b, wrong(0, (torch.int32, (33, 7), (("rle", 12, "big"),))))
        # runs that do not end well: the same number of values, refused all the same
        body = ref.encode([("rle", 3, 1)], 4)
        results, _ = b.decode_packed([_stream(body + b"\x82"), _stream(b"\x09" + body), _stream(body + b"\x00\x00")], flags=FLAGS)
        with pytest.raises(ValueError, match=r"stream 0: runs that the stream's end cuts \(status 3\) after 3 values in 2 of its 3 delivered bytes"):
            tensors.outputs_as_tensors(b, [(torch.uint8, (3,), (("rle", 4),)), None, None])
        with pytest.raises(ValueError, match=r"stream 1: a width byte that is none \(status 4\)"):
            tensors.outputs_as_tensors(b, [None, (torch.uint8, (3,), ("rle",)), None])
        with pytest.raises(ValueError, match=r"stream 2: a run of no values \(status 2\)"):
            tensors.outputs_as_tensors(b, [None, None, (torch.uint8, (3,), (("rle", 4),))])
    finally:
        b.close()
