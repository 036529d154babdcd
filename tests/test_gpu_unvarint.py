"""Unvarint on the device (needs a real MI355X): the kernels (csrc/brotli_unvarint_kernels.hip) through BrotliAmdBatchUnvarintSegments,
BrotliAmdBatchUnvarintOutputs after the three kinds of decode call, and tensors.outputs_as_tensors, against numpy (varint_ref.py) and against
the host hook.  Sources come from one seeded read-only buffer, destinations from one buffer prefilled with a sentinel pattern, and the WHOLE
destination buffer is compared with the expectation: a byte written outside a segment's elements fails the test.  The source bytes are random --
half of them end a varint, some five hundred varints a MiB are overlong --, so an index that is off by one shows in every element behind it.
All comparisons are exact."""
import os

import numpy as np
import pytest

import seg_filter_harness as H
import varint_ref as ref
from conftest import ROOT
from seg_filter_harness import fresh_dst as _fresh_dst, stream as _stream, slots as _slots

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 4, 8]
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT


@pytest.fixture(scope="module")
def sizes(pkg):
    """from the hooks: a long segment that spans more than two passes of the carry launch's loop, a second one behind it, and the buffers"""
    tile, span = pkg.unvarint_tile(), pkg.undelta_carry_span()
    long_len = 2 * span * tile + 3 * tile + 4099
    second_len = 5 * tile + 77
    return {"tile": tile, "span": span, "long": long_len, "second": second_len, "bytes": long_len + second_len + (3 << 20) + 64}


@pytest.fixture(scope="module")
def source(sizes):
    """seeded bytes: computed once, never changed"""
    return H.source(20273, sizes["bytes"])


@pytest.fixture(scope="module")
def sentinel(sizes):
    return H.sentinel(sizes["bytes"])


@pytest.fixture(scope="module")
def dev(source, sentinel):
    return H.device_buffers(source, sentinel)


@pytest.fixture(scope="module")
def batch(pkg):
    b = pkg.Batch(1)   # (the number of segments is not bound by max_streams)
    yield b
    b.close()


def _unvarint(batch, dev, src, sentinel, segs, size, d_src=None):
    """segs: [(source offset, source length, destination offset, cap, width, flags)] -> one call into a fresh destination of `size` bytes, the
    whole destination and all results compared; d_src: the device's copy of src where it is not the module's source"""
    return H.counted_call(batch.unvarint_segments, ref.elements_bytes, ("src", "len", "dst", "cap", "w", "flags"), dev, src,
                          dev["src"] if d_src is None else d_src, sentinel, segs, size)


def test_three_thousand_short_segments_and_the_host_hook(pkg, batch, dev, source, sentinel):
    """the table of the tests without a device: more than two chunks of the walk's prefix sum, mixed widths, flags and capacities; the
    kernels' results and bytes are the host hook's"""
    data = source[:1 << 19]
    segs, size = ref.short_table(len(data))
    got = _unvarint(batch, dev, data, sentinel, segs, size)
    assert batch.last_unvarint_ms() > 0.0
    assert all(batch.last_unvarint_ms(p) > 0.0 for p in (1, 2, 3)) and batch.last_unvarint_ms(4) == 0.0
    hook_dst, hook_res = pkg.unvarint_host(data.tobytes(), segs, size, fill=sentinel[:size].tobytes())
    assert hook_res == got
    assert hook_dst == dev["dst"][:size].cpu().numpy().tobytes()


def test_one_long_segment_and_a_second_behind_it(pkg, batch, dev, source, sentinel, sizes):
    """more than two passes of the carry launch's loop over the long one's tiles; a second long one of another width lies right behind it in
    memory, so a carry must stop at the boundary, and no varint reaches back across it"""
    assert sizes["long"] > 2 * sizes["span"] * sizes["tile"]
    s0 = 5
    d1 = 9 + sizes["long"] + 3   # (the long one's elements are one byte each: at most as many as its bytes)
    segs = [(s0, sizes["long"], 9, sizes["long"], 1, 0), (s0 + sizes["long"], sizes["second"], d1, sizes["second"], 8, 1)]
    assert d1 % 8 != 0
    got = _unvarint(batch, dev, source, sentinel, segs, d1 + 8 * sizes["second"] + 64)
    assert got[0][2] > 1000 and got[1][0] > sizes["second"] // 3


@pytest.mark.parametrize("boundary", [4096, "tile"])
def test_varints_across_wave_and_tile_edges(pkg, batch, dev, sentinel, boundary):
    """varints of every length 1 .. 12 ending at every offset -12 .. +12 around a wave's edge and a tile's: one that ends in a tile's first bytes
    begins in the tile before"""
    import torch
    b = pkg.unvarint_tile() if boundary == "tile" else boundary
    src, places, overlong = ref.boundary_segments(b, 2 * b, 20272 + b)
    src = np.frombuffer(src, dtype=np.uint8)
    d_src = torch.from_numpy(src.copy()).cuda()
    assert d_src.data_ptr() % 16 == 0   # (every segment is then a whole number of tiles, and the edges lie where the test puts them)
    segs, d_at = [], 1
    for i, (s, l) in enumerate(places):
        segs.append((s, l, d_at, l, WIDTHS[i % 4], (i // 4) & 1))
        d_at += l * WIDTHS[i % 4] + i % 3
    assert d_at + 16 <= len(sentinel)
    got = _unvarint(batch, dev, src, sentinel, segs, d_at + 16, d_src=d_src)
    assert sum(r[2] for r in got) == overlong > 20


def test_counting_alone_and_small_capacities(pkg, batch, dev, source, sentinel, sizes):
    """a call whose capacities are all 0 needs no destination and gives the counts of the call that writes; cap < m on a long segment writes cap
    elements and nothing behind them"""
    tile = sizes["tile"]
    lens = [0, 1, 100, tile - 1, 3 * tile + 5, 40 * tile + 1234, 7]
    at, places = 11, []
    for l in lens:
        places.append((at, l))
        at += l + 3
    sp = dev["src"].data_ptr()
    counted = batch.unvarint_segments([sp + s for s, _ in places], [l for _, l in places], None, [0] * len(places), [1] * len(places))
    assert counted == [ref.unvarint(source[s:s + l])[1] for s, l in places]
    assert batch.unvarint_segments([sp + s for s, _ in places], [l for _, l in places], [None] * len(places), [0] * len(places), [8] * len(places), [1] * len(places)) == counted
    segs, d_at = [], 3
    for (s, l), (m, _, _), w in zip(places, counted, [4, 8, 2, 1, 8, 4, 2]):
        cap = m // 2 if l > 1000 else m + 5
        segs.append((s, l, d_at, cap, w, 1))
        d_at += min(m, cap) * w + 1   # (the next one begins one byte behind: a store beyond cap would hit it, or the sentinel between)
    assert segs[5][3] < counted[5][0] and segs[5][3] * 4 > 30 * tile // 2
    assert _unvarint(batch, dev, source, sentinel, segs, d_at + 64) == counted


def test_bad_arguments_launch_nothing(pkg, batch, dev, source, sentinel):
    _fresh_dst(dev, 4096)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    for bad in (3, 0, 16, 255):
        with pytest.raises(RuntimeError, match="unvarint segment 1: width is not 1, 2, 4 or 8"):
            batch.unvarint_segments([sp, sp + 100, sp + 200], [100] * 3, [dp, dp + 1000, dp + 2000], [10] * 3, [4, bad, 2])
    with pytest.raises(RuntimeError, match="unvarint segment 2: unknown flag bits"):
        batch.unvarint_segments([sp, sp + 100, sp + 200], [100] * 3, [dp, dp + 1000, dp + 2000], [10] * 3, [4, 8, 2], [0, 1, 2])
    with pytest.raises(RuntimeError, match=r"unvarint segment 0: a capacity above 2\^56"):
        batch.unvarint_segments([sp], [100], [dp], [(1 << 56) + 1], [1])
    with pytest.raises(RuntimeError, match="unvarint segment 1: no destination"):
        batch.unvarint_segments([sp, sp + 100], [100] * 2, [dp, None], [10, 10], [4, 4])
    H.compare(dev, sentinel[:4096])
    assert batch.unvarint_segments([], [], [], [], []) == []
    assert batch.unvarint_segments([sp + 7, sp + 7], [0, 0], [dp, dp], [5, 5], [4, 8]) == [(0, 0, 0)] * 2
    assert batch.last_unvarint_ms() == 0.0   # (nothing was launched)
    for w in WIDTHS:   # nothing is read behind the aligned span around a source: the source buffer's last bytes
        tail = len(source) - 37
        _unvarint(batch, dev, source, sentinel, [(tail, 37, 33, 37, w, 0), (len(source) - 1, 1, 400, 1, w, 1)], 512)


# ------------------------------------------------------------------ the outputs of a decode call
@pytest.fixture(scope="module")
def arrays():
    """seeded integers as varints, of 0, 1, 7, 4096 and 100 003 values -> [(the values as a numpy array, width, flags, the stream of their varints)]"""
    rng = np.random.default_rng(20274)
    out = []
    for m, w, f in [(0, 2, 0), (1, 4, 0), (7, 2, 1), (7, 8, 0), (4096, 2, 0), (4096, 4, 1), (4096, 8, 1), (4096, 1, 0), (100003, 4, 0), (100003, 8, 1), (33, 4, 0)]:
        if f:
            x = rng.integers(-(1 << (8 * w - 1)), 1 << (8 * w - 1), size=m, dtype=np.int64) >> rng.integers(0, 8 * w - 6, size=m)
        else:
            x = (rng.integers(0, 1 << 63, size=m, dtype=np.uint64) >> rng.integers(64 - 8 * w, 60, size=m).astype(np.uint64)).astype(np.uint64)
        raw = ref.varint(x.tolist(), bool(f))
        out.append((x.astype(np.int64 if f else np.uint64).astype("<i%d" % w if f else "<u%d" % w), w, f, raw, _stream(raw)))
    return out


def _check_outputs(b, dev, sentinel, arrays, skip):
    """unvarint_outputs of the arrays' streams into a fresh destination: the original arrays, their results, and sentinel in the slot that was
    skipped, whose result is zeros"""
    offs, size = _slots([x.nbytes for x, _, _, _, _ in arrays], skip)
    want = sentinel[:size].copy()
    for (x, _, _, _, _), o in zip(arrays, offs):
        if o is not None:
            want[o:o + x.nbytes] = np.frombuffer(x.tobytes(), dtype=np.uint8)
    _fresh_dst(dev, size)
    dp = dev["dst"].data_ptr()
    got = b.unvarint_outputs([None if o is None else dp + o for o in offs], [len(x) for x, _, _, _, _ in arrays], [w for _, w, _, _, _ in arrays],
                             [f for _, _, f, _, _ in arrays])
    assert got == [(0, 0, 0) if o is None else (len(x), len(raw), 0) for (x, _, _, raw, _), o in zip(arrays, offs)]
    H.compare(dev, want)
    assert b.count_varints_outputs() == [(len(x), len(raw), 0) for x, _, _, raw, _ in arrays]
    H.compare(dev, want)   # (counting writes nothing)


def test_outputs_of_decode_device(pkg, dev, sentinel, arrays):
    import torch
    datas, caps = [a[4] for a in arrays], [len(a[3]) for a in arrays]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(sum(caps) + 64, dtype=torch.uint8, device="cuda")   # the outputs back to back, at whatever alignment that gives
    offs = [sum(caps[:i]) + 3 for i in range(len(caps))]
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        with pytest.raises(RuntimeError, match="no decode call"):
            b.out_n = len(datas)
            b.count_varints_outputs()
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.count_varints_outputs()
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, n) for n in caps]
        ms, digests = b.last_kernel_ms(), b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={5})
        assert b.last_kernel_ms() == ms and b.digest_outputs() == digests   # (not a decode call: the accessors say what they said)
        with pytest.raises(RuntimeError, match="unvarint stream 0: width"):
            b.unvarint_outputs([dev["dst"].data_ptr() + 4096 * i for i in range(len(datas))], [1] * len(datas), [3] * len(datas))
    finally:
        b.close()


def test_outputs_of_decode_host_and_packed(pkg, dev, sentinel, arrays):
    b = pkg.Batch(len(arrays))
    try:
        results, outs = b.decode_host([a[4] for a in arrays], [len(a[3]) for a in arrays], FLAGS)
        assert [r.result for r in results] == [1] * len(arrays) and outs == [a[3] for a in arrays]
        _check_outputs(b, dev, sentinel, arrays, skip={0, 8})
        results, outs = b.decode_packed([a[4] for a in arrays], flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(a[3])) for a in arrays]
        view, launches = b._packed_view(len(arrays)), b.last_packed_launches()
        _check_outputs(b, dev, sentinel, arrays, skip={10})
        assert b._packed_view(len(arrays)) == view and view[0] != 0 and b.last_packed_launches() == launches   # BrotliAmdBatchPackedOutput still returns the buffer
    finally:
        b.close()


def test_truncated_delivery(pkg, dev, sentinel, arrays):
    """a stream given less room than it needs (with the eager limit) and a corrupt one: exactly decoded_size bytes are taken, and what trails the
    last end in them is left over"""
    import torch
    x, w, f, raw, stream = arrays[5]   # 4096 zigzag int32
    borked = open(os.path.join(ROOT, "tests", "golden", "testdata", "borked.compressed"), "rb").read()
    datas, caps, widths, flags = [stream, borked, stream], [1003, 4096, len(raw)], [4, 2, 4], [1, 0, 1]
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
        for d, ww, ff in zip(delivered, widths, flags):
            segs.append((0, len(d), d_at, len(d), ww, ff))
            d_at += len(d) * ww
        want = sentinel[:d_at + 64].copy()
        want_res = []
        for d, (_, _, o, cap, ww, ff) in zip(delivered, segs):
            elems, res = ref.elements_bytes(d, ww, ff, cap)
            want[o:o + len(elems)] = np.frombuffer(elems, dtype=np.uint8)
            want_res.append(res)
        _fresh_dst(dev, d_at + 64)
        got = b.unvarint_outputs([dev["dst"].data_ptr() + s[2] for s in segs], [s[3] for s in segs], widths, flags)
        assert got == want_res and got[0][1] <= 1003 and got[2] == (4096, len(raw), 0)
        H.compare(dev, want)
    finally:
        b.close()


def test_outputs_as_tensors(pkg, dev):
    import torch
    import delta_ref
    tensors = H.tensors_module()
    g = torch.Generator().manual_seed(20275)
    ids = torch.cumsum(torch.randint(0, 5000, (1000,), generator=g, dtype=torch.int64), 0)
    originals = [(torch.randint(0, 1 << 40, (33, 7), generator=g, dtype=torch.int64), ("varint",)),
                 (torch.randint(-(1 << 30), 1 << 30, (257,), generator=g, dtype=torch.int32), (("varint", "zigzag"),)),
                 (ids, ("varint", "delta")),
                 (torch.randint(-3000, 3000, (5, 3), generator=g, dtype=torch.int16), ("varint", "zigzag")),
                 (torch.randn((3, 5), generator=g), None),                                   # a plain 2-tuple: shuffled
                 (torch.randint(0, 200, (11,), generator=g, dtype=torch.uint8), None),     # the stream that is skipped
                 (ids[:77].to(torch.int32), (("varint", "zigzag"), "delta"))]

    def encode(t, flt):
        import shuffle_ref
        raw, w = t.contiguous().view(torch.uint8).numpy().tobytes(), t.element_size()
        if flt is None:
            return _stream(shuffle_ref.shuffle(raw, w))
        if "delta" in flt:
            raw = delta_ref.delta(raw, w)
        zig = "zigzag" in flt or ("varint", "zigzag") in flt
        values = np.frombuffer(raw, dtype=("<i%d" if zig else "<u%d") % w)
        return _stream(ref.varint(values.tolist(), zig))

    streams = [encode(t, f) for t, f in originals]
    b = pkg.Batch(len(streams))
    try:
        results, _ = b.decode_packed(streams, flags=FLAGS)
        assert [r.result for r in results] == [1] * len(streams)
        specs = [(t.dtype, tuple(t.shape)) if f is None else (t.dtype, tuple(t.shape), f) for t, f in originals]
        specs[5] = None
        got = tensors.outputs_as_tensors(b, specs)
        assert got[5] is None
        for i, (t, (o, _)) in enumerate(zip(got, originals)):
            if t is None:
                continue
            assert t.is_cuda and t.dtype == o.dtype and tuple(t.shape) == tuple(o.shape) and t.data_ptr() % 64 == 0, i
            assert torch.equal(t.cpu().view(torch.uint8), o.contiguous().view(torch.uint8)), i
        assert len({t.untyped_storage().data_ptr() for t in got if t is not None}) == 1   # views of one buffer

        def wrong(i, spec):
            return [spec if k == i else s for k, s in enumerate(specs)]

        with pytest.raises(ValueError, match="stream 1: 257 varints, but shape"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.int32, (256,), (("varint", "zigzag"),))))
        with pytest.raises(ValueError, match="stream 1: 257 varints, but shape"):
            tensors.outputs_as_tensors(b, wrong(1, (torch.int32, (258,), ("varint",))))
        for other in ("shuffle", "bitshuffle", ("bitpack", 3)):
            with pytest.raises(ValueError, match="stream 0: \"varint\" with"):
                tensors.outputs_as_tensors(b, wrong(0, (torch.int64, (33, 7), ("varint", other))))
        with pytest.raises(ValueError, match="stream 0: unknown varint option 'big'"):
            tensors.outputs_as_tensors(b, wrong(0, (torch.int64, (33, 7), (("varint", "big"),))))
        # an unfinished varint at the end, and an overlong one: the same number of varints, refused all the same
        tail = _stream(ref.varint([1, 2, 3]) + b"\x80")
        over = _stream(b"\x01" + b"\x80" * 10 + b"\x01" + b"\x02")
        results, _ = b.decode_packed([tail, over], flags=FLAGS)
        with pytest.raises(ValueError, match="stream 0: 4 delivered bytes, but its varints end after 3"):
            tensors.outputs_as_tensors(b, [(torch.int32, (3,), ("varint",)), None])
        with pytest.raises(ValueError, match="stream 1: 1 varints of more than ten bytes"):
            tensors.outputs_as_tensors(b, [None, (torch.int32, (3,), ("varint",))])
    finally:
        b.close()
