"""Bit-unpack on the device (needs a real MI355X): the kernel (csrc/brotli_bitunpack_kernels.hip) through BrotliAmdBatchBitUnpackSegments,
BrotliAmdBatchBitUnpackOutputs after the three kinds of decode call, and tensors.outputs_as_tensors, against numpy (bitpack_ref.py).  Sources
come from one seeded read-only buffer, destinations from one buffer prefilled with a sentinel pattern, and the WHOLE destination buffer is
compared with the expectation: a byte written outside a segment fails the test.  The results are integers: every comparison is exact."""
import ctypes
import os
import random

import numpy as np
import pytest

import bitpack_ref as ref
import bitshuffle_ref
import shuffle_ref
import seg_filter_harness as H
from conftest import ROOT
from seg_filter_harness import fresh_dst as _fresh_dst, next_at as _next_at, stream as _stream

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 4, 8]
MSB, SIGNED = ref.MSB_FIRST, ref.SIGNED
FLAGS = 1        # BROTLI_AMD_BATCH_LARGE_WINDOW
EAGER = 64       # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT
SRC_BYTES = (16 << 20) + 64
DST_BYTES = (14 << 20) + 64
# (w, k, flags): k = 1, k = 8 w at every width, fields of more than 32 bits, both orders and both extensions
SHAPES = [(1, 1, 0), (1, 8, MSB), (1, 3, SIGNED), (1, 4, MSB | SIGNED), (2, 16, 0), (2, 5, MSB | SIGNED), (2, 12, MSB), (2, 1, SIGNED),
          (4, 32, MSB), (4, 20, SIGNED), (4, 7, 0), (4, 31, MSB | SIGNED), (8, 64, MSB), (8, 40, 0), (8, 33, MSB | SIGNED), (8, 13, SIGNED)]


@pytest.fixture(scope="module")
def source():
    """16 MiB + 64 of seeded bytes: computed once, never changed"""
    return H.source(20274, SRC_BYTES)


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
    H.compare(dev, want, segs, names="(src, dst, count, w, k, flags)", dst_len=lambda s: s[2] * s[3])


def _bitunpack(batch, dev, source, sentinel, segs, size, flags_none=False, spare=0):
    """segs: [(source offset, destination offset, count, width, bits, flags)] -> one launch into a fresh destination of `size` bytes, everything
    compared.  A segment's source is given as its ceil(count bits / 8) bytes and `spare` more."""
    want = sentinel[:size].copy()
    for s, d, m, w, k, f in segs:
        assert s + ref.src_bytes(m, k) + spare <= len(source) and d + m * w <= size
        want[d:d + m * w] = np.frombuffer(ref.unpack(source[s:s + ref.src_bytes(m, k)].tobytes(), m, k, w, f), dtype=np.uint8)
    _fresh_dst(dev, size)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    batch.bitunpack_segments([sp + s[0] for s in segs], [ref.src_bytes(s[2], s[4]) + spare for s in segs], [dp + s[1] for s in segs], [s[2] for s in segs],
                             [s[4] for s in segs], [s[3] for s in segs], None if flags_none else [s[5] for s in segs])
    _compare(dev, want, segs)


def _alignment_segments():
    """the counts 0 .. 100 x source alignment 0..15, the destination alignment and the shape running against them"""
    segs, s_at, d_at = [], 0, 0
    for m in range(101):
        for sa in range(16):
            w, k, f = SHAPES[(m + 3 * sa + m // 16) % 16]
            s_at, d_at = _next_at(s_at, sa), _next_at(d_at, (sa + m) % 16)
            segs.append((s_at, d_at, m, w, k, f))
            s_at += ref.src_bytes(m, k); d_at += m * w
    return segs, d_at


def test_every_alignment_and_short_count(pkg, batch, dev, source, sentinel):
    """one launch of short segments: every (src % 16, dst % 16), every dst % 16 and src % 16 under every shape of SHAPES, every count 0 .. 100;
    the table shuffled"""
    segs, d_at = _alignment_segments()
    full = [s for s in segs if s[2] > 0]
    assert {(s[0] % 16, s[1] % 16) for s in full} == {(a, b) for a in range(16) for b in range(16)}
    for shape in SHAPES:
        mine = [s for s in full if s[3:] == shape]
        assert {s[1] % 16 for s in mine} == set(range(16)) and {s[0] % 16 for s in mine} == set(range(16)), shape
        assert {s[2] for s in mine} == set(range(1, 101)), shape   # every count under every shape
        assert shape[0] == 1 or any(s[1] % shape[0] for s in mine), shape   # a destination that is no multiple of the width
    assert {s[2] for s in segs} == set(range(101))
    assert {1, 8, 16, 32, 64} <= {s[4] for s in segs} and any(s[4] > 32 for s in segs)
    random.Random(1).shuffle(segs)   # (the table's order is not the buffers')
    _bitunpack(batch, dev, source, sentinel, segs, d_at + 64)
    assert batch.last_bitunpack_ms() > 0.0


def test_tile_and_wave_edges(pkg, batch, dev, source, sentinel):
    """destinations that end one element short of, on and one element past a tile's edge, past 64 slots and past 256 slots, for every other
    shape of SHAPES at destination alignments 0 and odd.  Sources may be shared: they are only read."""
    tile = pkg.bitunpack_tile()
    segs, d_at, turn = [], 0, 0
    for w, k, f in SHAPES[::2] + [(8, 64, 0), (8, 63, MSB)]:
        per = tile // w
        for m in (per - 1, per, per + 1, 64 * 32 + 1, 64 * 32 + 33, 256 * 32 + 1, 256 * 32 + 33):
            for aligned in (True, False):
                d_at = _next_at(d_at, 0 if aligned else (turn | 1) % 16)
                segs.append(((5 * turn + 1) % 64, d_at, m, w, k, f))
                turn += 1
                d_at += m * w
    assert {s[1] % 16 for s in segs} >= {0, 1, 3, 5, 7, 9, 11, 13, 15}
    _bitunpack(batch, dev, source, sentinel, segs, d_at + 64)


@pytest.mark.parametrize("w,k,f", [(4, 12, 0), (8, 40, MSB | SIGNED)])
def test_one_long_segment_among_five_thousand_short_ones(pkg, batch, dev, source, sentinel, w, k, f):
    """more segments than one chunk of the prefix sum in LDS holds; the long one (8 MiB of destination and three elements, its destination at a
    multiple of 16: the fast way) is spread over every block; empty segments among the short ones, and one whose source ends on the source
    allocation's last byte"""
    rnd = random.Random(3)
    items = [(0 if rnd.random() < 0.05 else rnd.randrange(0, 301),) + rnd.choice(SHAPES) for _ in range(5000)]
    items.insert(2500, ((8 << 20) // w + 3, w, k, f))
    segs, s_at, d_at = [], 5, 9
    for m, ww, kk, ff in items:
        if rnd.random() < 0.1:
            s_at += rnd.randrange(1, 40); d_at += rnd.randrange(1, 40)
        if m > 1 << 16:
            d_at = _next_at(d_at, 0)
        segs.append((s_at, d_at, m, ww, kk, ff))
        s_at += ref.src_bytes(m, kk); d_at += m * ww
    segs.append((len(source) - ref.src_bytes(77, 11), d_at + 3, 77, 2, 11, MSB))
    d_at += 3 + 77 * 2
    assert sum(1 for s in segs if s[2] == 0) > 20
    _bitunpack(batch, dev, source, sentinel, segs, d_at + 64)


def test_no_segment_empty_segments_null_flags_and_spare_source(pkg, batch, dev, source, sentinel):
    _bitunpack(batch, dev, source, sentinel, [], 256)
    assert pkg.load_library().BrotliAmdBatchBitUnpackSegments(batch._h, 0, None, None, None, None, None, None, None, None) == 0
    _bitunpack(batch, dev, source, sentinel, [(7, 21, 0, 4, 9, 0), (7, 21, 0, 8, 64, MSB)], 256)
    assert batch.last_bitunpack_ms() == 0.0   # (segments of no elements: nothing was launched)
    for w, k, f in SHAPES:   # one element whose field ends on the source allocation's last byte
        _bitunpack(batch, dev, source, sentinel, [(len(source) - ref.src_bytes(1, k), 33, 1, w, k, f)], 256)
    # flags == NULL: all 0
    _bitunpack(batch, dev, source, sentinel, [(3, 16, 1000, 2, 9, 0), (2000, 2100, 1025, 4, 17, 0), (9000, 6300, 640, 1, 5, 0)], 8192, flags_none=True)
    # source bytes behind the fields are ignored
    _bitunpack(batch, dev, source, sentinel, [(3, 16, 1000, 2, 9, MSB), (2000, 2100, 33, 8, 47, SIGNED)], 8192, spare=11)


def test_bad_arguments_launch_nothing(pkg, batch, dev, source, sentinel):
    L = pkg.load_library()
    _fresh_dst(dev, 4096)
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    three = ([sp, sp + 100, sp + 200], [100, 100, 100], [dp, dp + 1000, dp + 2000], [10, 10, 10])
    for bits, widths, flags, text in (([3, 0, 3], [1, 1, 1], None, "segment 1.*field"), ([3, 3, 9], [1, 1, 1], None, "segment 2.*field"),
                                      ([3, 17, 3], [1, 2, 1], None, "field"), ([3, 33, 3], [1, 4, 1], None, "field"), ([3, 65, 3], [1, 8, 1], None, "field"),
                                      ([3, 3, 3], [1, 3, 1], None, "segment 1.*width"), ([3, 3, 3], [0, 1, 1], None, "width"), ([3, 3, 3], [1, 1, 16], None, "width"),
                                      ([3, 3, 3], [1, 1, 1], [0, 4, 0], "segment 1.*flag"), ([3, 3, 3], [1, 1, 1], [0, 0, 255], "flag")):
        with pytest.raises(RuntimeError, match=text):
            batch.bitunpack_segments(*three, bits, widths, flags)
    with pytest.raises(RuntimeError, match="segment 2.*source bytes"):   # 100 bytes hold 266 fields of 3 bits
        batch.bitunpack_segments(three[0], three[1], three[2], [266, 266, 267], [3, 3, 3], [1, 1, 1])
    with pytest.raises(RuntimeError, match="2\\^56"):
        batch.bitunpack_segments(three[0], three[1], three[2], [10, (1 << 56) + 1, 10], [3, 1, 3], [1, 1, 1])
    _compare(dev, sentinel[:4096])
    one_p, one_l, one_c, one_b = (ctypes.c_void_p * 1)(sp), (ctypes.c_size_t * 1)(4), (ctypes.c_uint64 * 1)(4), (ctypes.c_uint8 * 1)(4)
    one_d, one_w = (ctypes.c_void_p * 1)(dp), (ctypes.c_uint8 * 1)(1)
    good = (one_p, one_l, one_d, one_c, one_b, one_w)
    for hole in range(6):
        args = [None if i == hole else a for i, a in enumerate(good)]
        assert L.BrotliAmdBatchBitUnpackSegments(batch._h, 1, *args, None, None) < 0 and "argument" in pkg.last_error()
    _compare(dev, sentinel[:4096])


# ------------------------------------------------------------------ the outputs of a decode call
@pytest.fixture(scope="module")
def arrays():
    """seeded arrays of 0, 1, 7, 4096, 4101 and 100 003 elements, packed
    -> [(the elements' bytes, count, width, bits, flags, the packed bytes, their stream)]"""
    rng = np.random.default_rng(20275)
    out = []
    for m, (w, k, f) in [(0, (2, 9, 0)), (1, (4, 17, MSB)), (7, (1, 3, SIGNED)), (7, (8, 64, 0)), (4096, (1, 4, SIGNED)), (4096, (2, 12, MSB)),
                         (4096, (4, 20, 0)), (4096, (8, 40, MSB | SIGNED)), (100003, (1, 1, MSB)), (100003, (4, 7, SIGNED)), (100003, (2, 16, MSB)),
                         (4101, (8, 33, 0)), (100003, (1, 5, 0))]:
        packed = rng.integers(0, 256, size=ref.src_bytes(m, k), dtype=np.uint8)
        if m and (m * k) % 8:   # the pad bits are zero, as a packer leaves them
            pad = 8 - (m * k) % 8
            packed[-1] &= (0xFF << pad) & 0xFF if f & MSB else 0xFF >> pad
        packed = packed.tobytes()
        out.append((ref.unpack(packed, m, k, w, f), m, w, k, f, packed, _stream(packed)))
    return out


def _slots(sizes, skip=()):
    return H.slots(sizes, skip, start=16)


def _check_outputs(b, dev, sentinel, arrays, skip, counts=True):
    """bitunpack_outputs of the arrays' streams into a fresh destination: the original arrays, and sentinel in the slots that were skipped.
    counts=False: counts == NULL, every stream's count is floor(8 delivered bytes / k) -- up to 7 // k elements more than the array's"""
    ms = [a[1] if counts else len(a[5]) * 8 // a[3] for a in arrays]
    offs, size = _slots([m * a[2] for m, a in zip(ms, arrays)], skip)
    want = sentinel[:size].copy()
    for a, m, o in zip(arrays, ms, offs):
        if o is not None:
            want[o:o + m * a[2]] = np.frombuffer(ref.unpack(a[5], m, a[3], a[2], a[4]), dtype=np.uint8)
            assert want[o:o + a[1] * a[2]].tobytes() == a[0]
    _fresh_dst(dev, size)
    dp = dev["dst"].data_ptr()
    # (a skipped stream's parameters are not looked at: they are given as ones that would be refused)
    b.bitunpack_outputs([None if o is None else dp + o for o in offs], [0 if o is None else a[3] for a, o in zip(arrays, offs)],
                        [3 if o is None else a[2] for a, o in zip(arrays, offs)], ms if counts else None,
                        [255 if o is None else a[4] for a, o in zip(arrays, offs)])
    _compare(dev, want)
    assert b.last_bitunpack_ms() > 0.0


def test_outputs_of_decode_device(pkg, dev, sentinel, arrays):
    import torch
    datas, caps = [a[6] for a in arrays], [len(a[5]) for a in arrays]
    bits, widths = [a[3] for a in arrays], [a[2] for a in arrays]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(sum(caps) + 64, dtype=torch.uint8, device="cuda")   # the outputs back to back, at whatever alignment that gives
    offs = [sum(caps[:i]) + 3 for i in range(len(caps))]
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        with pytest.raises(RuntimeError, match="no decode call"):
            b.out_n = len(datas)
            b.bitunpack_outputs([dev["dst"].data_ptr()] * len(datas), bits, widths)
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.bitunpack_outputs([dev["dst"].data_ptr()] * len(datas), bits, widths)
        results = b.wait()
        assert [(r.result, r.decoded_size) for r in results] == [(1, n) for n in caps]
        ms, digests = b.last_kernel_ms(), b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={5})
        assert b.last_kernel_ms() == ms and b.digest_outputs() == digests   # (not a decode call: the accessors say what they said)
        _fresh_dst(dev, 4096)
        with pytest.raises(RuntimeError, match="stream 0.*width"):
            b.bitunpack_outputs([dev["dst"].data_ptr() + 16 * i for i in range(len(datas))], [1] * len(datas), [3] * len(datas), [0] * len(datas))
        with pytest.raises(RuntimeError, match="stream 0.*field"):
            b.bitunpack_outputs([dev["dst"].data_ptr() + 16 * i for i in range(len(datas))], [9] * len(datas), [1] * len(datas), [0] * len(datas))
        _compare(dev, sentinel[:4096])
        b.relaunch()
        b.wait()
        _check_outputs(b, dev, sentinel, arrays, skip=set(), counts=False)
    finally:
        b.close()


def test_outputs_of_decode_host(pkg, dev, sentinel, arrays):
    b = pkg.Batch(len(arrays))
    try:
        results, outs = b.decode_host([a[6] for a in arrays], [len(a[5]) for a in arrays], FLAGS)
        assert [r.result for r in results] == [1] * len(arrays)
        assert outs == [a[5] for a in arrays]
        digests = b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={0, 8})
        assert b.digest_outputs() == digests
    finally:
        b.close()


def test_outputs_of_decode_packed(pkg, dev, sentinel, arrays):
    b = pkg.Batch(len(arrays))
    try:
        results, outs = b.decode_packed([a[6] for a in arrays], flags=FLAGS)
        assert [(r.result, r.decoded_size) for r in results] == [(1, len(a[5])) for a in arrays]
        view, launches, digests = b._packed_view(len(arrays)), b.last_packed_launches(), b.digest_outputs()
        _check_outputs(b, dev, sentinel, arrays, skip={11})
        assert b._packed_view(len(arrays)) == view and view[0] != 0   # BrotliAmdBatchPackedOutput still returns the buffer
        assert b.last_packed_launches() == launches and b.digest_outputs() == digests
        blob = b.packed_fetch(view[1][-1])
        assert [blob[view[1][i]:view[1][i + 1]] for i in range(len(arrays))] == outs
    finally:
        b.close()


def test_truncated_delivery(pkg, dev, sentinel, arrays):
    """a stream given less room than it needs (with the eager limit) and a corrupt one: with counts=None exactly floor(8 decoded_size / k) elements
    are written, and the byte behind them keeps its sentinel; with the arrays' own counts the call fails, names the stream and writes nothing"""
    import torch
    _, m, w, k, f, packed, stream = arrays[6]   # 4096 fields of 20 bits into four bytes
    assert (m, w, k, len(packed)) == (4096, 4, 20, 10240)
    borked = open(os.path.join(ROOT, "tests", "golden", "testdata", "borked.compressed"), "rb").read()
    datas, caps = [stream, borked, stream], [1003, 4096, 10240]
    bits, widths, flags = [20, 11, 20], [4, 2, 4], [f, MSB | SIGNED, f]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(2 * 4096 + 10240 + 64, dtype=torch.uint8, device="cuda")
    offs = [1, 4096 + 2, 2 * 4096 + 3]
    torch.cuda.synchronize()
    b = pkg.Batch(3)
    try:
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS | EAGER)
        results = b.wait()
        assert [r.result for r in results] == [3, 0, 1], [r.result for r in results]
        sizes = [r.decoded_size for r in results]
        assert sizes[0] == 1003 and (sizes[0] * 8) % 20 != 0 and sizes[2] == 10240
        host = arena.cpu().numpy()
        delivered = [host[o:o + n].tobytes() for o, n in zip(offs, sizes)]
        counts = [len(d) * 8 // kk for d, kk in zip(delivered, bits)]
        assert counts[0] == 401 and counts[2] == 4096
        d_offs, size = _slots([c * ww for c, ww in zip(counts, widths)])
        want = sentinel[:size].copy()
        for o, d, c, kk, ww, ff in zip(d_offs, delivered, counts, bits, widths, flags):
            want[o:o + c * ww] = np.frombuffer(ref.unpack(d, c, kk, ww, ff), dtype=np.uint8)
        _fresh_dst(dev, size)
        dst = [dev["dst"].data_ptr() + o for o in d_offs]
        b.bitunpack_outputs(dst, bits, widths, None, flags)
        _compare(dev, want)
        b.bitunpack_outputs(dst, bits, widths, counts, flags)   # the same counts, given
        _compare(dev, want)
        # stream 0 delivered 1003 bytes, which hold 401 fields and not the 4096 its array has
        _fresh_dst(dev, size)
        with pytest.raises(RuntimeError, match="stream 0.*source bytes"):
            b.bitunpack_outputs(dst, bits, widths, [4096, counts[1], 4096], flags)
        with pytest.raises(RuntimeError, match="stream 0.*source bytes"):
            b.bitunpack_outputs(dst, bits, widths, [402, 0, 0], flags)
        _compare(dev, sentinel[:size])
        b.bitunpack_outputs([None, None, dst[2]], bits, widths, [4096, 1 << 60, 4096], flags)   # (a skipped stream's count is not looked at)
        want = sentinel[:size].copy()
        want[d_offs[2]:d_offs[2] + 4096 * 4] = np.frombuffer(arrays[6][0], dtype=np.uint8)
        _compare(dev, want)
    finally:
        b.close()


def test_outputs_as_tensors(pkg, dev):
    import torch
    tensors = H.tensors_module()
    assert "bitpack" in tensors.FILTERS
    g = torch.Generator().manual_seed(20276)
    originals = [torch.randint(-8, 8, (33, 7), generator=g, dtype=torch.int8),            # ("bitpack", 4, "signed")
                 torch.randint(0, 2, (1031,), generator=g, dtype=torch.uint8),           # ("bitpack", 1)
                 torch.randint(0, 2, (77, 3), generator=g, dtype=torch.uint8).bool(),    # ("bitpack", 1, "big"): numpy.packbits
                 torch.randint(-2048, 2048, (4099,), generator=g, dtype=torch.int16),    # ("bitpack", 12, "signed", "big")
                 torch.randint(0, 4096, (513,), generator=g, dtype=torch.int16),         # ("bitpack", 12)
                 torch.cumsum(torch.randint(0, 1 << 20, (1000,), generator=g, dtype=torch.int64), 0),   # (("bitpack", 20), "delta")
                 torch.randn((11, 13), generator=g),                                      # plain
                 torch.randn((129, 5), generator=g).to(torch.bfloat16),                   # shuffled
                 torch.randint(0, 1000, (777,), generator=g, dtype=torch.int32)]          # bit-shuffled
    filters = [(("bitpack", 4, "signed"),), (("bitpack", 1),), (("bitpack", 1, "big"),), (("bitpack", 12, "signed", "big"),), (("bitpack", 12),),
               (("bitpack", 20), "delta"), (), ("shuffle",), ("bitshuffle",)]

    def raw(t):
        return t.contiguous().view(torch.uint8).numpy().tobytes()

    def delta(t):
        """the wrapping differences of the flattened array's bit patterns"""
        a = np.frombuffer(raw(t), dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[t.element_size()])
        return np.diff(a, prepend=a.dtype.type(0)).astype(a.dtype).tobytes()

    stored = []
    for t, f in zip(originals, filters):
        x = delta(t) if "delta" in f else raw(t)
        head = f[0] if f else None
        if isinstance(head, tuple):
            values = np.frombuffer(x, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[t.element_size()])
            x = ref.pack(values, head[1], MSB if "big" in head else 0)
        elif head == "shuffle":
            x = shuffle_ref.shuffle(x, t.element_size())
        elif head == "bitshuffle":
            x = bitshuffle_ref.bitshuffle(x, t.element_size(), 0)
        stored.append(_stream(x))
    assert stored[2] is not None and len(ref.pack(originals[2].view(torch.uint8).numpy().reshape(-1), 1, MSB)) == 29   # 231 bits
    assert ref.pack(originals[2].view(torch.uint8).numpy().reshape(-1), 1, MSB) == np.packbits(originals[2].numpy().reshape(-1)).tobytes()
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
        assert b.last_bitunpack_ms() > 0.0
        wrong = list(specs)
        wrong[4] = (torch.int16, (513,), (("bitpack", 12), "shuffle"))
        with pytest.raises(ValueError, match="stream 4"):
            tensors.outputs_as_tensors(b, wrong)
        wrong[4] = (torch.int16, (513,), (("bitpack", 17),))
        with pytest.raises(ValueError, match="stream 4"):
            tensors.outputs_as_tensors(b, wrong)
        wrong[4] = (torch.int16, (513,), (("bitpack", 12, "middle"),))
        with pytest.raises(ValueError, match="stream 4"):
            tensors.outputs_as_tensors(b, wrong)
        wrong[4] = (torch.int16, (514,), (("bitpack", 12),))   # 771 bytes, not the 770 delivered
        with pytest.raises(ValueError, match="stream 4"):
            tensors.outputs_as_tensors(b, wrong)
    finally:
        b.close()


def test_the_segment_table_goes_with_its_owner(pkg, dev):
    """brotli_amd_debug_live_bytes is back at its baseline after a batch object that made the new call is closed"""
    L = pkg.load_library()
    L.brotli_amd_debug_live_bytes.restype = None
    L.brotli_amd_debug_live_bytes.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]

    def live():
        d, pin = ctypes.c_size_t(0), ctypes.c_size_t(0)
        L.brotli_amd_debug_live_bytes(ctypes.byref(d), ctypes.byref(pin))
        return d.value, pin.value

    base = live()
    b = pkg.Batch(1)
    fresh = live()
    sp, dp = dev["src"].data_ptr(), dev["dst"].data_ptr()
    b.bitunpack_segments([sp + 1] * 100, [64] * 100, [dp + 128 * i for i in range(100)], [40] * 100, [12] * 100, [2] * 100)
    held = live()
    assert held[0] > fresh[0]
    b.bitunpack_segments([sp] * 10, [64] * 10, [dp + 128 * i for i in range(10)], [7] * 10, [3] * 10, [1] * 10, [SIGNED] * 10)
    assert live() == held   # (a smaller table: the same buffer again)
    b.close()
    assert live() == base
