"""Unshuffle on the device (needs a real MI355X): the kernel (csrc/brotli_unshuffle_kernels.hip) through BrotliAmdBatchUnshuffleSegments,
BrotliAmdBatchUnshuffleOutputs after the three kinds of decode call, and tensors.outputs_as_tensors, against numpy (shuffle_ref.py).  Sources come
from one seeded read-only buffer, destinations from one buffer prefilled with a sentinel pattern, and the WHOLE destination buffer is compared
with the expectation: a byte written outside a segment fails the test."""
import ctypes
import os
import random

import numpy as np
import pytest

import shuffle_ref as ref
import seg_filter_harness as H
from conftest import ROOT
from seg_filter_harness import fresh_dst as _fresh_dst, next_at as _next_at, stream as _stream, slots as _slots

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 4, 8]
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT
SRC_BYTES = (16 << 20) + 64
DST_BYTES = (9 << 20) + 64


@pytest.fixture(scope="module")
def source():
    """16 MiB + 64 of seeded bytes: computed once, never changed"""
    return H.source(20264, SRC_BYTES)


@pytest.fixture(scope="module")
def sentinel():
    return H.sentinel(DST_BYTES)


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


def _unshuffle(batch, dev, source, sentinel, segs, size):
    """segs: [(source offset, destination offset, length, width)] -> one launch into a fresh destination of `size` bytes, everything compared"""
    want = sentinel[:size].copy()
    for s, d, l, w in segs:
        assert s + l <= len(source) and d + l <= size
        want[d:d + l] = np.frombuffer(ref.unshuffle(source[s:s + l].tobytes(), w), dtype=np.uint8)
    _fresh_dst(dev, size)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    batch.unshuffle_segments([sp + s for s, _, _, _ in segs], [dp + d for _, d, _, _ in segs], [l for _, _, l, _ in segs], [w for _, _, _, w in segs])
    _compare(dev, want, segs)


def test_every_alignment_and_short_length(pkg, batch, dev, source, sentinel):
    """w x source alignment 0..15 x 16 lengths, the destination alignment running against the source's so that every (src % 16, dst % 16, w) and
    every (dst % 16, w, length) occurs; neighbours back to back wherever the walk through the alignments allows it; the table shuffled; one launch"""
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
    _unshuffle(batch, dev, source, sentinel, segs, d_at + 64)
    assert batch.last_unshuffle_ms() > 0.0


def test_tile_and_wave_edges(pkg, batch, dev, source, sentinel):
    """tile - 1, tile, tile + 1, 2 tile + w + 1 and 1024 k +- 1 bytes for every width at odd alignments, back to back; m = 1, 15, 17 and 4097
    elements, with and without left-over bytes: a plane's start k m then takes every residue mod 16"""
    tile = pkg.unshuffle_tile()
    segs, s_at, d_at, turn = [], 1, 3, 0
    for w in WIDTHS:
        lens = [tile - 1, tile, tile + 1, 2 * tile + w + 1] + [1024 * k + d for k in (1, 2, 3, 16) for d in (-1, 1)]
        lens += [w * m + r for m in (1, 15, 17, 4097) for r in sorted({0, w - 1})]
        for l in lens:
            s_at, d_at = _next_at(s_at, (2 * turn + 1) % 16), _next_at(d_at, (6 * turn + 3) % 16)
            turn += 1
            segs.append((s_at, d_at, l, w))
            s_at += l; d_at += l
    assert all(s % 2 == 1 and d % 2 == 1 for s, d, _, _ in segs)
    _unshuffle(batch, dev, source, sentinel, segs, d_at + 64)


def test_one_long_segment_among_five_thousand_short_ones(pkg, batch, dev, source, sentinel):
    """more segments than one chunk of the prefix sum in LDS holds; the long one is spread over every block"""
    rnd = random.Random(3)
    items = [(rnd.randrange(0, 301), rnd.choice(WIDTHS)) for _ in range(5000)]
    items.insert(2500, ((8 << 20) + 3, 4))
    segs, s_at, d_at = [], 5, 9
    for l, w in items:
        if rnd.random() < 0.1:
            s_at += rnd.randrange(1, 40); d_at += rnd.randrange(1, 40)
        segs.append((s_at, d_at, l, w))
        s_at += l; d_at += l
    _unshuffle(batch, dev, source, sentinel, segs, d_at + 64)


def test_a_tile_that_spans_a_stretch_of_empty_segments(pkg, batch, dev, source, sentinel):
    """the kernel takes the segment table a chunk at a time (csrc/brotli_seg_walk.h: a prefix sum of 1024 segments): two segments that share a
    tile with 2500 empty ones between them -- the tile begins in one chunk, finds nothing in the next and ends in the one after; mixed widths,
    odd alignments, gaps of sentinel bytes between some neighbours"""
    rnd = random.Random(5)
    tile = pkg.unshuffle_tile()
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
    _unshuffle(batch, dev, source, sentinel, segs, d_at + 64)


def test_no_segment_empty_segments_and_the_last_byte(pkg, batch, dev, source, sentinel):
    _unshuffle(batch, dev, source, sentinel, [], 256)
    assert pkg.load_library().BrotliAmdBatchUnshuffleSegments(batch._h, 0, None, None, None, None, None) == 0
    _unshuffle(batch, dev, source, sentinel, [(7, 21, 0, 4), (7, 21, 0, 8)], 256)
    for w in WIDTHS:
        _unshuffle(batch, dev, source, sentinel, [(len(source) - 1, 33, 1, w)], 256)
    _unshuffle(batch, dev, source, sentinel, [(len(source) - 1, 33, 1, 2), (0, 34, 1, 8), (len(source) - 41, 35, 41, 4)], 256)


def test_bad_arguments_launch_nothing(pkg, batch, dev, source, sentinel):
    L = pkg.load_library()
    _fresh_dst(dev, 4096)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    for bad in (3, 0, 16, 255):
        with pytest.raises(RuntimeError, match="width"):
            batch.unshuffle_segments([sp, sp + 100, sp + 200], [dp, dp + 100, dp + 200], [100, 100, 100], [4, bad, 2])
    _compare(dev, sentinel[:4096])
    one_p, one_l, one_w = (ctypes.c_void_p * 1)(sp), (ctypes.c_size_t * 1)(4), (ctypes.c_uint8 * 1)(4)
    one_d = (ctypes.c_void_p * 1)(dp)
    for args in ((None, one_d, one_l, one_w), (one_p, None, one_l, one_w), (one_p, one_d, None, one_w), (one_p, one_d, one_l, None)):
        assert L.BrotliAmdBatchUnshuffleSegments(batch._h, 1, args[0], args[1], args[2], args[3], None) < 0 and pkg.last_error()
    _compare(dev, sentinel[:4096])


# ------------------------------------------------------------------ the outputs of a decode call
@pytest.fixture(scope="module")
def arrays():
    """seeded int16, float32 and float64 arrays and one of int8, of 0, 1, 7, 4096 and 100 003 bytes (left-over bytes behind the last whole
    element where the size is no multiple of the width) -> [(the array's bytes, width, the stream of its byte planes)]"""
    rng = np.random.default_rng(20265)
    out = []
    for nbytes, w in [(0, 2), (1, 4), (7, 2), (7, 8), (4096, 2), (4096, 4), (4096, 8), (4096, 1), (100003, 4), (100003, 8), (100003, 2), (7, 4)]:
        m = nbytes // w
        if w == 1:
            x = rng.integers(-128, 128, size=m, dtype=np.int8).tobytes()
        elif w == 2:
            x = rng.integers(-300, 300, size=m, dtype=np.int16).tobytes()
        elif w == 4:
            x = rng.normal(size=m).astype(np.float32).tobytes()
        else:
            x = rng.normal(size=m).astype(np.float64).tobytes()
        x += rng.integers(0, 256, size=nbytes - len(x), dtype=np.uint8).tobytes()
        assert len(x) == nbytes
        out.append((x, w, _stream(ref.shuffle(x, w))))
    return out


def _check_outputs(b, dev, sentinel, arrays, skip):
    """unshuffle_outputs of the arrays' streams into a fresh destination: the original arrays, and sentinel in the slot that was skipped"""
    offs, size = _slots([len(x) for x, _, _ in arrays], skip)
    want = sentinel[:size].copy()
    for (x, _, _), o in zip(arrays, offs):
        if o is not None:
            want[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    _fresh_dst(dev, size)
    dp = dev["dst"].data_ptr()
    b.unshuffle_outputs([None if o is None else dp + o for o in offs], [w for _, w, _ in arrays])
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
            b.unshuffle_outputs([dev["dst"].data_ptr()] * len(datas), [w for _, w, _ in arrays])
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.unshuffle_outputs([dev["dst"].data_ptr()] * len(datas), [w for _, w, _ in arrays])
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, n) for n in caps]
        ms, digests = b.last_kernel_ms(), b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={5})
        assert b.last_kernel_ms() == ms and b.digest_outputs() == digests   # (not a decode call: the accessors say what they said)
        with pytest.raises(RuntimeError, match="width"):
            b.unshuffle_outputs([dev["dst"].data_ptr() + 4096 * i for i in range(len(datas))], [3] * len(datas))
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
        assert outs == [ref.shuffle(x, w) for x, w, _ in arrays]
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
    x, w, stream = arrays[5]   # 4096 bytes of float32
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
        assert delivered[0] == ref.shuffle(x, w)[:1003]
        d_offs, size = _slots(sizes)
        want = sentinel[:size].copy()
        for o, d, ww in zip(d_offs, delivered, widths):
            want[o:o + len(d)] = np.frombuffer(ref.unshuffle(d, ww), dtype=np.uint8)
        _fresh_dst(dev, size)
        b.unshuffle_outputs([dev["dst"].data_ptr() + o for o in d_offs], widths)
        _compare(dev, want)
    finally:
        b.close()


def test_outputs_as_tensors(pkg, dev):
    import torch
    tensors = H.tensors_module()
    g = torch.Generator().manual_seed(20266)
    originals = [torch.randn((3, 5, 7), generator=g).to(torch.bfloat16), torch.randn((11, 13), generator=g), torch.randn((9,), generator=g, dtype=torch.float64),
                 torch.randint(-128, 128, (5, 3), generator=g, dtype=torch.int8), torch.randn((1, 1), generator=g), torch.randn((257, 3), generator=g).to(torch.bfloat16)]
    streams = [_stream(ref.shuffle(t.contiguous().view(torch.uint8).numpy().tobytes(), t.element_size())) for t in originals]
    b = pkg.Batch(len(streams))
    try:
        with pytest.raises(RuntimeError, match="no outputs"):
            tensors.outputs_as_tensors(b, [None] * len(streams))
        results, _ = b.decode_packed(streams, flags=FLAGS)
        assert [r.result for r in results] == [1] * len(streams)
        specs = [(t.dtype, tuple(t.shape)) for t in originals]
        specs[4] = None
        got = tensors.outputs_as_tensors(b, specs)
        assert got[4] is None
        for i, (t, o) in enumerate(zip(got, originals)):
            if t is None:
                continue
            assert t.is_cuda and t.dtype == o.dtype and tuple(t.shape) == tuple(o.shape), i
            assert t.data_ptr() % 64 == 0, i
            assert torch.equal(t.cpu(), o), i
        assert len({t.untyped_storage().data_ptr() for t in got if t is not None}) == 1   # views of one buffer
        wrong = list(specs)
        wrong[1] = (torch.float32, (11, 12))
        with pytest.raises(ValueError, match="stream 1"):
            tensors.outputs_as_tensors(b, wrong)
        wrong[1] = (torch.float64, (11, 13))
        with pytest.raises(ValueError, match="stream 1"):
            tensors.outputs_as_tensors(b, wrong)
    finally:
        b.close()
