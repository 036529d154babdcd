"""Undelta on the device (needs a real MI355X): the kernels (csrc/brotli_undelta_kernels.hip) through BrotliAmdBatchUndeltaSegments,
BrotliAmdBatchUndeltaOutputs after the three kinds of decode call, and tensors.outputs_as_tensors, against numpy (delta_ref.py).  Sources come
from one seeded read-only buffer, destinations from one buffer prefilled with a sentinel pattern, and the WHOLE destination buffer is compared
with the expectation: a byte written outside a segment fails the test.  The source bytes are random, so the sums wrap at every width, and a
missing or doubled carry shows in every byte behind it.  All comparisons are exact."""
import ctypes
import os
import random

import numpy as np
import pytest

import delta_ref as ref
import seg_filter_harness as H
from conftest import ROOT
from seg_filter_harness import fresh_dst as _fresh_dst, next_at as _next_at, stream as _stream, slots as _slots

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 4, 8]
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT


@pytest.fixture(scope="module")
def sizes(pkg):
    """from the hooks: a long segment that spans more than two passes of the carry launch's loop, a second one behind it, and the buffers"""
    tile, span = pkg.undelta_tile(), pkg.undelta_carry_span()
    long_len = 2 * span * tile + 3 * tile + 4099
    second_len = 5 * tile + 77
    return {"tile": tile, "span": span, "long": long_len, "second": second_len, "bytes": long_len + second_len + (3 << 20) + 64}


@pytest.fixture(scope="module")
def source(sizes):
    """seeded bytes: computed once, never changed"""
    return H.source(20268, sizes["bytes"])


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


def _compare(dev, want, segs=None):
    H.compare(dev, want, segs, names="(src, dst, len, w)")


def _undelta(batch, dev, source, sentinel, segs, size, in_place=()):
    """segs: [(source offset, destination offset, length, width)] -> one call into a fresh destination of `size` bytes, everything compared.
    The segments whose index is in `in_place` have their deltas copied to their destination first and are then transformed there."""
    import torch
    want = sentinel[:size].copy()
    for s, d, l, w in segs:
        assert s + l <= len(source) and d + l <= size
        want[d:d + l] = np.frombuffer(ref.undelta(source[s:s + l].tobytes(), w), dtype=np.uint8)
    _fresh_dst(dev, size)
    for i in in_place:
        s, d, l, _ = segs[i]
        dev["dst"][d:d + l].copy_(dev["src"][s:s + l])
    torch.cuda.synchronize()
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    batch.undelta_segments([dp + d if i in in_place else sp + s for i, (s, d, _, _) in enumerate(segs)], [dp + d for _, d, _, _ in segs],
                           [l for _, _, l, _ in segs], [w for _, _, _, w in segs])
    _compare(dev, want, segs)


def test_every_alignment_and_short_length(pkg, batch, dev, source, sentinel):
    """w x source alignment 0..15 x 16 lengths, the destination alignment running against the source's so that every (src % 16, dst % 16, w) and
    every (dst % 16, w, length) occurs; neighbours back to back wherever the walk through the alignments allows it; the table shuffled; one call"""
    segs, s_at, d_at = [], 0, 0
    for w in WIDTHS:
        lens = [0, 1, w - 1, w, w + 1, 15, 16, 17, 16 * w - 1, 16 * w, 16 * w + 1, 255, 256, 257, 1023, 1025]
        for k, l in enumerate(lens):
            for sa in range(16):
                s_at, d_at = _next_at(s_at, sa), _next_at(d_at, (sa + k) % 16)
                segs.append((s_at, d_at, l, w))
                s_at += l; d_at += l
    assert len(segs) == 4 * 16 * 16
    assert {(s % 16, d % 16, w) for s, d, _, w in segs} == {(a, b, w) for a in range(16) for b in range(16) for w in WIDTHS}
    for w in WIDTHS:
        for l in {l for _, _, l, ww in segs if ww == w}:
            assert {d % 16 for _, d, ll, ww in segs if (ll, ww) == (l, w)} == set(range(16)), (w, l)
    random.Random(1).shuffle(segs)   # (the table's order is not the buffers')
    _undelta(batch, dev, source, sentinel, segs, d_at + 64)
    assert batch.last_undelta_ms() > 0.0
    assert all(batch.last_undelta_ms(p) > 0.0 for p in (1, 2, 3)) and batch.last_undelta_ms(4) == 0.0


def test_tile_wave_and_block_edges(pkg, batch, dev, source, sentinel, sizes):
    """tile - 1, tile, tile + 1, 2 tile + w + 1, 64 x 16 +- 1 and 256 x 16 +- 1 bytes for every width at odd alignments, back to back; m = 1, 15,
    17 and 4097 elements, with and without left-over bytes"""
    tile = sizes["tile"]
    segs, s_at, d_at, turn = [], 1, 3, 0
    for w in WIDTHS:
        lens = [tile - 1, tile, tile + 1, 2 * tile + w + 1] + [k * 16 + d for k in (64, 256) for d in (-1, 1)]
        lens += [w * m + r for m in (1, 15, 17, 4097) for r in sorted({0, w - 1})]
        for l in lens:
            s_at, d_at = _next_at(s_at, (2 * turn + 1) % 16), _next_at(d_at, (6 * turn + 3) % 16)
            turn += 1
            segs.append((s_at, d_at, l, w))
            s_at += l; d_at += l
    assert all(s % 2 == 1 and d % 2 == 1 for s, d, _, _ in segs)
    _undelta(batch, dev, source, sentinel, segs, d_at + 64)


def test_one_long_segment_among_five_thousand_short_ones(pkg, batch, dev, source, sentinel, sizes):
    """more segments than one chunk of the prefix sum in LDS holds; the long one is spread over every block and its carries take more than two
    passes of the carry launch's loop; a second long one of another width lies right behind it, so a carry must stop at the boundary"""
    assert sizes["long"] > 2 * sizes["span"] * sizes["tile"]
    rnd = random.Random(3)
    items = [(rnd.randrange(0, 301), rnd.choice(WIDTHS)) for _ in range(5000)]
    items.insert(2500, (sizes["long"], 2))
    items.insert(2501, (sizes["second"], 8))
    segs, s_at, d_at = [], 5, 9
    for i, (l, w) in enumerate(items):
        if i != 2501 and rnd.random() < 0.1:
            s_at += rnd.randrange(1, 40); d_at += rnd.randrange(1, 40)
        if i == 2500:   # (so that the second long one, of width 8, begins at an odd address)
            d_at = _next_at(d_at, (3 - l) % 8, 8)
        segs.append((s_at, d_at, l, w))
        s_at += l; d_at += l
    assert segs[2501][1] == segs[2500][1] + segs[2500][2] and segs[2501][1] % 8 != 0
    _undelta(batch, dev, source, sentinel, segs, d_at + 64)


def test_a_tile_that_spans_a_stretch_of_empty_segments(pkg, batch, dev, source, sentinel, sizes):
    """the tile kernels take the segment table a chunk at a time (csrc/brotli_seg_walk.h: a prefix sum of 1024 segments): two segments that
    share a tile with 2500 empty ones between them -- the tile begins in one chunk, finds nothing in the next and ends in the one after, where
    its summary is made and a segment's first unit restarts the sum; mixed widths, odd alignments, gaps of sentinel bytes between some neighbours"""
    rnd = random.Random(5)
    tile = sizes["tile"]
    lens = [tile // 2 + 7] + [0] * 2500 + [tile + 9, 5, 0, 1] + [0] * 1100 + [3 * tile]
    widths = iter([2, 8, 4, 1, 8])   # of the five segments that have bytes
    segs, s_at, d_at = [], 3, 9
    for l in lens:
        if rnd.random() < 0.1:
            s_at += rnd.randrange(1, 3); d_at += rnd.randrange(1, 3)
        segs.append((s_at, d_at, l, next(widths) if l else rnd.choice(WIDTHS)))
        s_at += l; d_at += l
    units0 = (segs[0][1] + segs[0][2] + 15) // 16 - segs[0][1] // 16
    assert 0 < units0 < tile // 16 and all(l == 0 for _, _, l, _ in segs[1:2501]) and segs[2501][2] > tile   # the first tile goes on 2501 segments later
    _undelta(batch, dev, source, sentinel, segs, d_at + 64)


def test_in_place_among_out_of_place(pkg, batch, dev, source, sentinel, sizes):
    """element-aligned segments with source and destination the same memory, among out-of-place ones, in one call; in place at an address that is
    no multiple of the width is refused and writes nothing"""
    rnd = random.Random(4)
    tile = sizes["tile"]
    segs, inp, s_at, d_at = [], set(), 3, 1
    for i in range(400):
        w = rnd.choice(WIDTHS)
        l = rnd.choice([0, 1, w, 7 * w + 3, 100, 1000, 4097]) if i != 200 else 3 * tile + 5 * w + 1
        if i % 3 != 1:
            d_at = _next_at(d_at + rnd.randrange(0, 3), 0, w)
            inp.add(i)
        else:
            d_at += rnd.randrange(0, 3)
        segs.append((s_at, d_at, l, w))
        s_at += l; d_at += l
    assert 200 in inp and {w for i, (_, _, _, w) in enumerate(segs) if i in inp} == set(WIDTHS)
    _undelta(batch, dev, source, sentinel, segs, d_at + 64, in_place=inp)
    # refused: nothing is launched, the destination keeps its sentinel
    _fresh_dst(dev, 4096)
    dp, sp = dev["dst"].data_ptr(), dev["src"].data_ptr()
    for w in (2, 4, 8):
        with pytest.raises(RuntimeError, match="in place"):
            batch.undelta_segments([sp, dp + 1024 + w - 1, sp + 64], [dp, dp + 1024 + w - 1, dp + 512], [64, 100, 64], [4, w, 4])
    _compare(dev, sentinel[:4096])


def test_no_segment_empty_segments_and_the_last_byte(pkg, batch, dev, source, sentinel):
    """nothing is read behind the aligned span around a source: the source buffer's last bytes"""
    _undelta(batch, dev, source, sentinel, [], 256)
    assert pkg.load_library().BrotliAmdBatchUndeltaSegments(batch._h, 0, None, None, None, None, None) == 0
    _undelta(batch, dev, source, sentinel, [(7, 21, 0, 4), (7, 21, 0, 8)], 256)
    assert batch.last_undelta_ms() == 0.0   # (nothing was launched)
    for w in WIDTHS:
        _undelta(batch, dev, source, sentinel, [(len(source) - 1, 33, 1, w)], 256)
        _undelta(batch, dev, source, sentinel, [(len(source) - 5 * w, 35, 5 * w, w)], 256)
    _undelta(batch, dev, source, sentinel, [(len(source) - 1, 33, 1, 2), (0, 34, 1, 8), (len(source) - 41, 35, 41, 4)], 256)


def test_bad_arguments_launch_nothing(pkg, batch, dev, source, sentinel):
    L = pkg.load_library()
    _fresh_dst(dev, 4096)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    for bad in (3, 0, 16, 255):
        with pytest.raises(RuntimeError, match="width"):
            batch.undelta_segments([sp, sp + 100, sp + 200], [dp, dp + 100, dp + 200], [100, 100, 100], [4, bad, 2])
    _compare(dev, sentinel[:4096])
    one_p, one_l, one_w = (ctypes.c_void_p * 1)(sp), (ctypes.c_size_t * 1)(4), (ctypes.c_uint8 * 1)(4)
    one_d = (ctypes.c_void_p * 1)(dp)
    for args in ((None, one_d, one_l, one_w), (one_p, None, one_l, one_w), (one_p, one_d, None, one_w), (one_p, one_d, one_l, None)):
        assert L.BrotliAmdBatchUndeltaSegments(batch._h, 1, args[0], args[1], args[2], args[3], None) < 0 and pkg.last_error()
    _compare(dev, sentinel[:4096])


# ------------------------------------------------------------------ the outputs of a decode call
@pytest.fixture(scope="module")
def arrays():
    """seeded sorted int64 timestamps, int32 offsets, int16 and uint8 samples, of 0, 1, 7, 4096 and 100 003 bytes (left-over bytes behind the
    last whole element where the size is no multiple of the width) -> [(the array's bytes, width, the stream of its deltas)]"""
    rng = np.random.default_rng(20269)
    out = []
    for nbytes, w in [(0, 2), (1, 4), (7, 2), (7, 8), (4096, 2), (4096, 4), (4096, 8), (4096, 1), (100003, 4), (100003, 8), (100003, 2), (7, 4)]:
        m = nbytes // w
        if w == 1:
            x = rng.integers(0, 256, size=m, dtype=np.uint8).tobytes()
        elif w == 2:
            x = rng.integers(-300, 300, size=m, dtype=np.int16).tobytes()
        elif w == 4:
            x = np.cumsum(rng.integers(0, 5000, size=m), dtype=np.int64).astype(np.int32).tobytes()
        else:
            x = (1700000000000000000 + np.cumsum(rng.integers(0, 10 ** 9, size=m), dtype=np.int64)).astype(np.int64).tobytes()
        x += rng.integers(0, 256, size=nbytes - len(x), dtype=np.uint8).tobytes()
        assert len(x) == nbytes
        out.append((x, w, _stream(ref.delta(x, w))))
    return out


def _check_outputs(b, dev, sentinel, arrays, skip):
    """undelta_outputs of the arrays' streams into a fresh destination: the original arrays, and sentinel in the slot that was skipped"""
    offs, size = _slots([len(x) for x, _, _ in arrays], skip)
    want = sentinel[:size].copy()
    for (x, _, _), o in zip(arrays, offs):
        if o is not None:
            want[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    _fresh_dst(dev, size)
    dp = dev["dst"].data_ptr()
    b.undelta_outputs([None if o is None else dp + o for o in offs], [w for _, w, _ in arrays])
    _compare(dev, want)


def test_outputs_of_decode_device(pkg, dev, sentinel, arrays):
    import torch
    datas, caps = [c for _, _, c in arrays], [len(x) for x, _, _ in arrays]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(sum(caps) + 64, dtype=torch.uint8, device="cuda")   # the outputs back to back, at whatever alignment that gives
    offs = [sum(caps[:i]) + 3 for i in range(len(caps))]
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        with pytest.raises(RuntimeError, match="no decode call"):
            b.out_n = len(datas)
            b.undelta_outputs([dev["dst"].data_ptr()] * len(datas), [w for _, w, _ in arrays])
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.undelta_outputs([dev["dst"].data_ptr()] * len(datas), [w for _, w, _ in arrays])
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, n) for n in caps]
        ms, digests = b.last_kernel_ms(), b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={5})
        assert b.last_kernel_ms() == ms and b.digest_outputs() == digests   # (not a decode call: the accessors say what they said)
        with pytest.raises(RuntimeError, match="width"):
            b.undelta_outputs([dev["dst"].data_ptr() + 4096 * i for i in range(len(datas))], [3] * len(datas))
        b.relaunch()
        b.wait()
        _check_outputs(b, dev, sentinel, arrays, skip=set())
    finally:
        b.close()


def test_outputs_of_decode_host(pkg, dev, sentinel, arrays):
    b = pkg.Batch(len(arrays))
    try:
        results, outs = b.decode_host([c for _, _, c in arrays], [len(x) for x, _, _ in arrays], FLAGS)
        assert [r.result for r in results] == [1] * len(arrays)
        assert outs == [ref.delta(x, w) for x, w, _ in arrays]
        digests = b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={0, 8})
        assert b.digest_outputs() == digests
    finally:
        b.close()


def test_outputs_of_decode_packed(pkg, dev, sentinel, arrays):
    b = pkg.Batch(len(arrays))
    try:
        results, outs = b.decode_packed([c for _, _, c in arrays], flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(x)) for x, _, _ in arrays]
        view, launches, digests = b._packed_view(len(arrays)), b.last_packed_launches(), b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={11})
        assert b._packed_view(len(arrays)) == view and view[0] != 0   # BrotliAmdBatchPackedOutput still returns the buffer
        assert b.last_packed_launches() == launches and b.digest_outputs() == digests
        blob = b.packed_fetch(view[1][-1])
        assert [blob[view[1][i]:view[1][i + 1]] for i in range(len(arrays))] == outs
    finally:
        b.close()


def test_truncated_delivery(pkg, dev, sentinel, arrays):
    """a stream given less room than it needs (with the eager limit) and a corrupt one: exactly decoded_size bytes are transformed, by the rule for
    that many bytes, and the byte behind them keeps its sentinel"""
    import torch
    x, w, stream = arrays[5]   # 4096 bytes of int32
    assert (len(x), w) == (4096, 4)
    borked = open(os.path.join(ROOT, "tests", "golden", "testdata", "borked.compressed"), "rb").read()
    datas, caps, widths = [stream, borked, stream], [1003, 4096, 4096], [4, 2, 4]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(3 * 4096 + 64, dtype=torch.uint8, device="cuda")
    offs = [1, 4096 + 2, 2 * 4096 + 3]
    torch.cuda.synchronize()
    b = pkg.Batch(3)
    try:
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS | EAGER)
        results = b.wait()
        assert [r.result for r in results] == [3, 0, 1], [r.result for r in results]
        sizes = [r.decoded_size for r in results]
        assert sizes[0] == 1003 and sizes[0] % 4 != 0 and sizes[2] == 4096
        host = arena.cpu().numpy()
        delivered = [host[o:o + n].tobytes() for o, n in zip(offs, sizes)]
        assert delivered[0] == ref.delta(x, w)[:1003]
        d_offs, size = _slots(sizes)
        want = sentinel[:size].copy()
        for o, d, ww in zip(d_offs, delivered, widths):
            want[o:o + len(d)] = np.frombuffer(ref.undelta(d, ww), dtype=np.uint8)
        _fresh_dst(dev, size)
        b.undelta_outputs([dev["dst"].data_ptr() + o for o in d_offs], widths)
        _compare(dev, want)
    finally:
        b.close()


def test_outputs_as_tensors(pkg, dev):
    import torch
    import shuffle_ref
    tensors = H.tensors_module()
    g = torch.Generator().manual_seed(20270)
    stamps = 1700000000000000000 + torch.cumsum(torch.randint(0, 10 ** 9, (1000,), generator=g, dtype=torch.int64), 0)
    originals = [(stamps, ("shuffle", "delta")),
                 (torch.cumsum(torch.randint(0, 70000, (33, 7), generator=g, dtype=torch.int32).flatten(), 0, dtype=torch.int32).reshape(33, 7), ("delta",)),
                 (torch.randint(-30000, 30000, (257,), generator=g, dtype=torch.int16), ("shuffle", "delta")),
                 (torch.randint(0, 256, (5, 3), generator=g, dtype=torch.uint8), ("delta",)),
                 (torch.randn((3, 5, 7), generator=g).to(torch.bfloat16), ("shuffle", "delta")),   # a bf16 tensor's bit patterns
                 (torch.randn((1, 1), generator=g), None),                                           # the stream that is skipped
                 (torch.randn((11, 13), generator=g), ()),
                 (torch.randn((9,), generator=g, dtype=torch.float64), None),                        # a plain 2-tuple: shuffled
                 (stamps[:77].to(torch.int64), ("delta",))]

    def encode(t, flt):
        raw, w = t.contiguous().view(torch.uint8).numpy().tobytes(), t.element_size()
        flt = ("shuffle",) if flt is None else flt
        if "delta" in flt:
            raw = ref.delta(raw, w)
        if "shuffle" in flt:
            raw = shuffle_ref.shuffle(raw, w)
        return _stream(raw)

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
            assert t.is_cuda and t.dtype == o.dtype and tuple(t.shape) == tuple(o.shape), i
            assert t.data_ptr() % 64 == 0, i
            assert torch.equal(t.cpu().view(torch.uint8), o.contiguous().view(torch.uint8)), i
        assert len({t.untyped_storage().data_ptr() for t in got if t is not None}) == 1   # views of one buffer
        wrong = list(specs)
        wrong[2] = (torch.int16, (257,), ("shuffle", "xor"))
        with pytest.raises(ValueError, match="stream 2.*xor"):
            tensors.outputs_as_tensors(b, wrong)
    finally:
        b.close()
