"""Bit-unshuffle on the device (needs a real MI355X): the kernel (csrc/brotli_bitunshuffle_kernels.hip) through BrotliAmdBatchBitUnshuffleSegments,
BrotliAmdBatchBitUnshuffleOutputs after the three kinds of decode call, and tensors.outputs_as_tensors, against numpy (bitshuffle_ref.py).  Sources
come from one seeded read-only buffer, destinations from one buffer prefilled with a sentinel pattern, and the WHOLE destination buffer is
compared with the expectation: a byte written outside a segment fails the test."""
import ctypes
import os
import random

import numpy as np
import pytest

import bitshuffle_ref as ref
import shuffle_ref
import seg_filter_harness as H
from conftest import ROOT
from seg_filter_harness import fresh_dst as _fresh_dst, next_at as _next_at, stream as _stream

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 4, 8]
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT
SRC_BYTES = (16 << 20) + 64
DST_BYTES = (12 << 20) + 64


@pytest.fixture(scope="module")
def source():
    """16 MiB + 64 of seeded bytes: computed once, never changed"""
    return H.source(20271, SRC_BYTES)


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
    H.compare(dev, want, segs, names="(src, dst, len, w, block)")


def _bitunshuffle(batch, dev, source, sentinel, segs, size, blocks_none=False):
    """segs: [(source offset, destination offset, length, width, block)] -> one launch into a fresh destination of `size` bytes, everything compared"""
    want = sentinel[:size].copy()
    for s, d, l, w, blk in segs:
        assert s + l <= len(source) and d + l <= size
        want[d:d + l] = np.frombuffer(ref.bitunshuffle(source[s:s + l].tobytes(), w, blk), dtype=np.uint8)
    _fresh_dst(dev, size)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    batch.bitunshuffle_segments([sp + s[0] for s in segs], [dp + s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs],
                                None if blocks_none else [s[4] for s in segs])
    _compare(dev, want, segs)


def test_every_alignment_and_short_length(pkg, batch, dev, source, sentinel):
    """w x source alignment 0..15 x 16 lengths, the destination alignment running against the source's so that every (src % 16, dst % 16, w) and
    every (dst % 16, w, length) occurs; neighbours back to back wherever the walk through the alignments allows it; the block size cycling
    through 0, 8, 24, 2048; the table shuffled; one launch"""
    segs, s_at, d_at = [], 0, 0
    for w in WIDTHS:
        lens = [0, 1, 8 * w - 1, 8 * w, 8 * w + 1, 15, 17, 32 * w, 32 * w + 8 * w, 64 * w + 3, 255, 256, 257, 1023, 1025, 24 * w + 2]
        assert len(lens) == 16
        for k, l in enumerate(lens):
            for sa in range(16):
                s_at, d_at = _next_at(s_at, sa), _next_at(d_at, (sa + k) % 16)
                segs.append((s_at, d_at, l, w, (0, 8, 24, 2048)[(len(segs) + len(segs) // 16) % 4]))
                s_at += l; d_at += l
    assert len(segs) == 4 * 16 * 16
    assert {(s % 16, d % 16, w) for s, d, _, w, _ in segs} == {(a, b, w) for a in range(16) for b in range(16) for w in WIDTHS}
    for w in WIDTHS:
        for l in {s[2] for s in segs if s[3] == w}:
            assert {s[1] % 16 for s in segs if (s[2], s[3]) == (l, w)} == set(range(16)), (w, l)
            assert {s[4] for s in segs if (s[2], s[3]) == (l, w)} == {0, 8, 24, 2048}, (w, l)
    random.Random(1).shuffle(segs)   # (the table's order is not the buffers')
    _bitunshuffle(batch, dev, source, sentinel, segs, d_at + 64)
    assert batch.last_bitunshuffle_ms() > 0.0


def test_tile_and_wave_edges(pkg, batch, dev, source, sentinel):
    """tile - 1, tile, tile + 1 and 2 tile + 8 w + 1 bytes for every width at destination alignments 0 and odd, under the block sizes 0, 32,
    8192 / w and 1000 (whose B w does not divide the tile): block edges inside tiles, on tile edges and inside a wave's run of fast items;
    m = 8, 24, 40 and 4104 elements, with and without left-over bytes.  Sources may be shared: they are only read."""
    tile = pkg.bitunshuffle_tile()
    segs, d_at, turn = [], 0, 0
    for w in WIDTHS:
        lens = [tile - 1, tile, tile + 1, 2 * tile + 8 * w + 1] + [w * m + r for m in (8, 24, 40, 4104) for r in sorted({0, w - 1})]
        for l in lens:
            for blk in (0, 32, 8192 // w, 1000):
                for aligned in (True, False):
                    d_at = _next_at(d_at, 0 if aligned else (turn | 1) % 16)   # (turn is odd here: 1, 3, .., 15 in turns)
                    segs.append(((5 * turn + 1) % 64, d_at, l, w, blk))
                    turn += 1
                    d_at += l
    assert {s[1] % 16 for s in segs} >= {0, 1, 3, 5, 7, 9, 11, 13, 15}
    _bitunshuffle(batch, dev, source, sentinel, segs, d_at + 64)


@pytest.mark.parametrize("w,blk", [(4, 2048), (8, 0)])
def test_one_long_segment_among_five_thousand_short_ones(pkg, batch, dev, source, sentinel, w, blk):
    """more segments than one chunk of the prefix sum in LDS holds; the long one (8 MiB + 3, its destination at a multiple of 16: the fast way)
    is spread over every block; empty segments among the short ones, and one that ends on the source allocation's last byte"""
    rnd = random.Random(3)
    items = [(rnd.choice([0, 0, rnd.randrange(0, 301)]) if rnd.random() < 0.1 else rnd.randrange(0, 301), rnd.choice(WIDTHS),
              rnd.choice([0, 8, 24, 32, 40, 2048])) for _ in range(5000)]
    items.insert(2500, ((8 << 20) + 3, w, blk))
    segs, s_at, d_at = [], 5, 9
    for l, ww, b in items:
        if rnd.random() < 0.1:
            s_at += rnd.randrange(1, 40); d_at += rnd.randrange(1, 40)
        if l > 1 << 20:
            d_at = _next_at(d_at, 0)
        segs.append((s_at, d_at, l, ww, b))
        s_at += l; d_at += l
    segs.append((len(source) - 77, d_at + 3, 77, 2, 8))
    d_at += 80
    assert sum(1 for s in segs if s[2] == 0) > 20
    _bitunshuffle(batch, dev, source, sentinel, segs, d_at + 64)


def test_no_segment_empty_segments_null_blocks_and_the_last_byte(pkg, batch, dev, source, sentinel):
    _bitunshuffle(batch, dev, source, sentinel, [], 256)
    assert pkg.load_library().BrotliAmdBatchBitUnshuffleSegments(batch._h, 0, None, None, None, None, None, None) == 0
    _bitunshuffle(batch, dev, source, sentinel, [(7, 21, 0, 4, 0), (7, 21, 0, 8, 8)], 256)
    for w in WIDTHS:
        _bitunshuffle(batch, dev, source, sentinel, [(len(source) - 1, 33, 1, w, 0)], 256)
    _bitunshuffle(batch, dev, source, sentinel, [(len(source) - 1, 33, 1, 2, 0), (0, 34, 1, 8, 8), (len(source) - 41, 35, 41, 4, 8)], 256)
    # block_elems == NULL: all 0
    _bitunshuffle(batch, dev, source, sentinel, [(3, 16, 1000, 2, 0), (2000, 1100, 4099, 4, 0), (9000, 5300, 640, 1, 0)], 8192, blocks_none=True)


def test_bad_arguments_launch_nothing(pkg, batch, dev, source, sentinel):
    L = pkg.load_library()
    _fresh_dst(dev, 4096)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    three = ([sp, sp + 100, sp + 200], [dp, dp + 100, dp + 200], [100, 100, 100])
    for bad in (3, 0, 16, 255):
        with pytest.raises(RuntimeError, match="width"):
            batch.bitunshuffle_segments(*three, [4, bad, 2], [0, 0, 0])
    for bad in (1, 4, 12, 2049, (1 << 32) - 1):
        with pytest.raises(RuntimeError, match="block"):
            batch.bitunshuffle_segments(*three, [4, 4, 2], [0, 8, bad])
    _compare(dev, sentinel[:4096])
    one_p, one_l, one_w, one_b = (ctypes.c_void_p * 1)(sp), (ctypes.c_size_t * 1)(4), (ctypes.c_uint8 * 1)(4), (ctypes.c_uint32 * 1)(0)
    one_d = (ctypes.c_void_p * 1)(dp)
    for args in ((None, one_d, one_l, one_w), (one_p, None, one_l, one_w), (one_p, one_d, None, one_w), (one_p, one_d, one_l, None)):
        assert L.BrotliAmdBatchBitUnshuffleSegments(batch._h, 1, args[0], args[1], args[2], args[3], one_b, None) < 0 and "argument" in pkg.last_error()
    _compare(dev, sentinel[:4096])


# ------------------------------------------------------------------ the outputs of a decode call
@pytest.fixture(scope="module")
def arrays():
    """seeded int8, int16, float32 and float64 arrays of 0, 1, 7, 4096, 4100 and 100 003 bytes -- left-over bytes behind the last whole element
    where the size is no multiple of the width, left-over elements where their number is no multiple of 8 -- bit-shuffled in blocks
    -> [(the array's bytes, width, block, the stream of its bit planes)]"""
    rng = np.random.default_rng(20272)
    out = []
    for nbytes, w, blk in [(0, 2, 0), (1, 4, 0), (7, 2, 8), (7, 8, 0), (4096, 2, 0), (4096, 4, 2048), (4096, 8, 1024), (4096, 1, 8192), (100003, 4, 2048),
                           (100003, 8, 0), (100003, 2, 4096), (4100, 4, 0), (100003, 1, 1000)]:
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
        out.append((x, w, blk, _stream(ref.bitshuffle(x, w, blk))))
    assert any(len(x) % w for x, w, _, _ in out) and any((len(x) // w) % 8 for x, w, _, _ in out)
    return out


def _slots(sizes, skip=()):
    return H.slots(sizes, skip, start=16)


def _check_outputs(b, dev, sentinel, arrays, skip):
    """bitunshuffle_outputs of the arrays' streams into a fresh destination: the original arrays, and sentinel in the slots that were skipped"""
    offs, size = _slots([len(a[0]) for a in arrays], skip)
    want = sentinel[:size].copy()
    for a, o in zip(arrays, offs):
        if o is not None:
            want[o:o + len(a[0])] = np.frombuffer(a[0], dtype=np.uint8)
    _fresh_dst(dev, size)
    dp = dev["dst"].data_ptr()
    b.bitunshuffle_outputs([None if o is None else dp + o for o in offs], [a[1] for a in arrays], [a[2] for a in arrays])
    _compare(dev, want)
    assert b.last_bitunshuffle_ms() > 0.0


def test_outputs_of_decode_device(pkg, dev, sentinel, arrays):
    import torch
    datas, caps = [a[3] for a in arrays], [len(a[0]) for a in arrays]
    widths, blocks = [a[1] for a in arrays], [a[2] for a in arrays]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(sum(caps) + 64, dtype=torch.uint8, device="cuda")   # the outputs back to back, at whatever alignment that gives
    offs = [sum(caps[:i]) + 3 for i in range(len(caps))]
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        with pytest.raises(RuntimeError, match="no decode call"):
            b.out_n = len(datas)
            b.bitunshuffle_outputs([dev["dst"].data_ptr()] * len(datas), widths, blocks)
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.bitunshuffle_outputs([dev["dst"].data_ptr()] * len(datas), widths, blocks)
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, n) for n in caps]
        ms, digests = b.last_kernel_ms(), b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={5})
        assert b.last_kernel_ms() == ms and b.digest_outputs() == digests   # (not a decode call: the accessors say what they said)
        with pytest.raises(RuntimeError, match="width"):
            b.bitunshuffle_outputs([dev["dst"].data_ptr() + 4096 * i for i in range(len(datas))], [3] * len(datas), blocks)
        with pytest.raises(RuntimeError, match="block"):
            b.bitunshuffle_outputs([dev["dst"].data_ptr() + 4096 * i for i in range(len(datas))], widths, [4] * len(datas))
        b.relaunch()
        b.wait()
        _check_outputs(b, dev, sentinel, arrays, skip=set())
    finally:
        b.close()


def test_outputs_of_decode_host(pkg, dev, sentinel, arrays):
    b = pkg.Batch(len(arrays))
    try:
        results, outs = b.decode_host([a[3] for a in arrays], [len(a[0]) for a in arrays], FLAGS)
        assert [r.result for r in results] == [1] * len(arrays)
        assert outs == [ref.bitshuffle(x, w, blk) for x, w, blk, _ in arrays]
        digests = b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={0, 8})
        assert b.digest_outputs() == digests
    finally:
        b.close()


def test_outputs_of_decode_packed(pkg, dev, sentinel, arrays):
    b = pkg.Batch(len(arrays))
    try:
        results, outs = b.decode_packed([a[3] for a in arrays], flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(a[0])) for a in arrays]
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
    x, w, blk, stream = arrays[5]   # 4096 bytes of float32
    assert (len(x), w) == (4096, 4)
    borked = open(os.path.join(ROOT, "tests", "golden", "testdata", "borked.compressed"), "rb").read()
    datas, caps, widths, blocks = [stream, borked, stream], [1003, 4096, 4096], [4, 2, 4], [64, 8, blk]
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
        d_offs, size = _slots(sizes)
        want = sentinel[:size].copy()
        for o, d, ww, bb in zip(d_offs, delivered, widths, blocks):
            want[o:o + len(d)] = np.frombuffer(ref.bitunshuffle(d, ww, bb), dtype=np.uint8)
        _fresh_dst(dev, size)
        b.bitunshuffle_outputs([dev["dst"].data_ptr() + o for o in d_offs], widths, blocks)
        _compare(dev, want)
    finally:
        b.close()


def test_outputs_as_tensors(pkg, dev):
    import torch
    tensors = H.tensors_module()
    assert "bitshuffle" in tensors.FILTERS
    g = torch.Generator().manual_seed(20273)
    originals = [torch.randint(-500, 500, (33, 7), generator=g, dtype=torch.int16), torch.randn((1031, 5), generator=g),
                 torch.randint(0, 1 << 40, (1000,), generator=g, dtype=torch.int64), torch.randn((11, 13), generator=g).to(torch.bfloat16),
                 torch.randint(-128, 128, (4099,), generator=g, dtype=torch.int8), torch.randint(0, 1000, (777,), generator=g, dtype=torch.int32)]
    filters = [("bitshuffle",), (("bitshuffle", 2048),), ("bitshuffle", "delta"), ("shuffle",), (("bitshuffle", 64), "delta"), ("shuffle", "delta")]

    def raw(t):
        return t.contiguous().view(torch.uint8).numpy().tobytes()

    def delta(t):
        """the wrapping differences of the flattened array's bit patterns"""
        a = np.frombuffer(raw(t), dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[t.element_size()])
        return np.diff(a, prepend=a.dtype.type(0)).astype(a.dtype).tobytes()

    stored = []
    for t, f in zip(originals, filters):
        x = delta(t) if "delta" in f else raw(t)
        head = f[0]
        if head == "shuffle":
            x = shuffle_ref.shuffle(x, t.element_size())
        else:
            x = ref.bitshuffle(x, t.element_size(), head[1] if isinstance(head, tuple) else 0)
        stored.append(_stream(x))
    b = pkg.Batch(len(stored))
    try:
        results, _ = b.decode_packed(stored, flags=FLAGS)
        assert [r.result for r in results] == [1] * len(stored)
        specs = [(t.dtype, tuple(t.shape), f) for t, f in zip(originals, filters)]
        got = tensors.outputs_as_tensors(b, specs)
        for i, (t, o) in enumerate(zip(got, originals)):
            assert t.is_cuda and t.dtype == o.dtype and tuple(t.shape) == tuple(o.shape), i
            assert t.data_ptr() % 64 == 0, i
            assert torch.equal(t.cpu(), o), i
        assert len({t.untyped_storage().data_ptr() for t in got}) == 1   # views of one buffer
        assert b.last_bitunshuffle_ms() > 0.0
        wrong = list(specs)
        wrong[3] = (originals[3].dtype, tuple(originals[3].shape), ("shuffle", "bitshuffle"))
        with pytest.raises(ValueError, match="stream 3"):
            tensors.outputs_as_tensors(b, wrong)
        wrong[3] = (originals[3].dtype, tuple(originals[3].shape), (("bitshuffle", 12),))
        with pytest.raises(ValueError, match="stream 3"):
            tensors.outputs_as_tensors(b, wrong)
        wrong[3] = (originals[3].dtype, tuple(originals[3].shape), ("xor",))
        with pytest.raises(ValueError, match="stream 3"):
            tensors.outputs_as_tensors(b, wrong)
    finally:
        b.close()
