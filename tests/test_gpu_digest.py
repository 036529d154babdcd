"""Digests on the device (needs a real MI355X): the CRC kernel (csrc/brotli_crc_kernels.hip) through BrotliAmdBatchDigestSegments, and
BrotliAmdBatchDigestOutputs after the three kinds of decode call, against zlib and a table-driven CRC-32C over the same bytes.  Segments lie
back to back in one seeded source wherever a case allows it, so a byte taken from a neighbour changes the answer."""
import ctypes
import random

import numpy as np
import pytest

import copy_vectors as cv
import digest_ref as ref

pytestmark = pytest.mark.gpu
KINDS = [ref.CRC32, ref.CRC32C]
FLAGS = 1   # BROTLI_AMD_BATCH_LARGE_WINDOW


@pytest.fixture(scope="module")
def source():
    """16 MiB + 64 of seeded bytes: computed once, never changed"""
    a = np.random.default_rng(20262).integers(0, 256, size=(16 << 20) + 64, dtype=np.uint8)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def dev_source(source):
    import torch
    t = torch.from_numpy(source.copy()).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


@pytest.fixture(scope="module")
def batch(pkg):
    b = pkg.Batch(1)   # (the number of segments is not bound by max_streams)
    yield b
    b.close()


def _digest(batch, dev_source, source, segs, kind):
    """segs: [(source offset, length)] -> asserts every digest"""
    got = batch.digest_segments([dev_source.data_ptr() + s for s, _ in segs], [l for _, l in segs], kind)
    assert len(got) == len(segs)
    bad = []
    for k, (s, l) in enumerate(segs):
        assert s + l <= len(source)
        want = ref.crc(kind, source[s:s + l].tobytes())
        if got[k] != want:
            bad.append((k, s, l, hex(got[k]), hex(want)))
    assert not bad, (len(bad), bad[:8])
    return got


def _packed(lens, at=0, gaps=None):
    """segments back to back from `at` on (gaps: rnd -> now and then a few bytes between)"""
    segs = []
    for l in lens:
        if gaps is not None and gaps.random() < 0.1:
            at += gaps.randrange(1, 70)
        segs.append((at, l))
        at += l
    return segs


@pytest.mark.parametrize("kind", KINDS)
def test_every_alignment_and_short_length(pkg, batch, dev_source, source, kind):
    """source alignment 0..15 x lengths {0 .. 257}: one launch; neighbours back to back wherever the walk through the alignments allows it"""
    segs, at = [], 0
    for l in (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 255, 256, 257):
        left = set(range(16))
        while left:
            while at % 16 not in left:
                at += 1
            left.discard(at % 16)
            segs.append((at, l))
            at += l
    assert len(segs) == 16 * 17 and {(s % 16, l) for s, l in segs} == {(a, l) for a in range(16) for l in (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 255, 256, 257)}
    random.Random(1).shuffle(segs)   # (the table's order is not the source's)
    _digest(batch, dev_source, source, segs, kind)


def test_one_segment_and_none(pkg, batch, dev_source, source):
    for kind in KINDS:
        for segs in ([], [(0, 1)], [(len(source) - 1, 1)], [(0, 1), (len(source) - 1, 1)], [(5, 0), (5, 0)], [(3, 0)]):
            _digest(batch, dev_source, source, segs, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_tile_edges(pkg, batch, dev_source, source, kind):
    """tile - 1, tile, tile + 1 and 3 tile + 5 bytes at alignments 3, 11 and 0, back to back; one segment that ends where the allocation ends"""
    tile = pkg.load_library().BrotliAmdDebugDigestTile()
    lens = [tile - 1, tile, tile + 1, 3 * tile + 5]
    segs, at = [], 3
    for l in lens:
        segs.append((at, l)); at += l
    at = (at + 15) // 16 * 16 + 11
    for l in reversed(lens):
        segs.append((at, l)); at += l
    for l in lens:
        at = (at + 15) // 16 * 16
        segs.append((at, l)); at += l
    segs.append((len(source) - (tile + 1), tile + 1))
    segs.append((len(source) - 2 * tile - 16, 2 * tile + 16))   # ... and one that ends there with a whole word
    _digest(batch, dev_source, source, segs, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_one_long_segment_among_a_thousand_short_ones(pkg, batch, dev_source, source, kind):
    rnd = random.Random(3)
    lens = [rnd.randrange(1, 301) for _ in range(1000)]
    lens.insert(500, ((8 << 20) if kind == ref.CRC32 else (4 << 20)) + 3)
    _digest(batch, dev_source, source, _packed(lens, at=5), kind)


@pytest.mark.parametrize("n", [65, 257, 5000])
def test_more_segments_than_a_wave_or_a_block_covers(pkg, batch, dev_source, source, n):
    rnd = random.Random(n)
    lens = [rnd.choice([0, 0, 1, 3, 16, rnd.randrange(0, 41), rnd.randrange(0, 41), rnd.randrange(0, 700)]) for _ in range(n)]
    segs = _packed(lens, at=n % 16, gaps=rnd)
    for kind in KINDS:
        _digest(batch, dev_source, source, segs, kind)


def test_a_tile_that_spans_a_stretch_of_empty_segments(pkg, batch, dev_source, source):
    """the kernel takes the segment table a chunk at a time (a prefix sum of a thousand-odd segments): two segments that share a tile with
    2500 empty ones between them -- the tile begins in one chunk, finds nothing in the next and ends in the one after"""
    tile = pkg.load_library().BrotliAmdDebugDigestTile()
    lens = [tile // 2 + 7] + [0] * 2500 + [tile + 9, 5, 0, 1] + [0] * 1100 + [3 * tile]
    for kind in KINDS:
        _digest(batch, dev_source, source, _packed(lens, at=9), kind)


def test_the_same_table_twice_gives_the_same_words(pkg, batch, dev_source, source):
    rnd = random.Random(6)
    lens = [rnd.randrange(0, 2000) for _ in range(3000)] + [(2 << 20) + 1] + [rnd.randrange(0, 100) for _ in range(500)]
    segs = _packed(lens, at=1)
    first = _digest(batch, dev_source, source, segs, ref.CRC32)
    assert _digest(batch, dev_source, source, segs, ref.CRC32) == first
    assert isinstance(batch.last_digest_ms(), float)


def _digest_repeated(batch, dev_source, source, segs, kind):
    """as _digest for tables in which the same few long segments come again and again: a reference once per distinct segment"""
    got = batch.digest_segments([dev_source.data_ptr() + s for s, _ in segs], [l for _, l in segs], kind)
    want = {}
    for s, l in set(segs):
        want[(s, l)] = ref.crc(kind, source[s:s + l].tobytes())
    bad = [(k, s, l, hex(got[k]), hex(want[(s, l)])) for k, (s, l) in enumerate(segs) if got[k] != want[(s, l)]]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("kind", KINDS)
def test_more_than_sixty_four_tiles_a_block(pkg, batch, dev_source, source, kind):
    """What a block carries from tile to tile.  A launch has at most four blocks a CU, so a table of more than 64 x 1024 tiles gives every block
    more than 64: a wave's waiting sums fill all its lanes and are settled in the middle of the walk, then gather again.  Segments may repeat
    and overlap (batch.h): the same long segment many times -- the whole source for CRC-32, 4 MiB of it for CRC-32C, whose reference is a
    Python loop -- at two alignments, overlapping ones, and 1100 short ones between them, so that the long ones lie on both sides of the
    boundaries between chunks of the segment table, where sums that wait are settled too."""
    tile = pkg.load_library().BrotliAmdDebugDigestTile()
    rnd = random.Random(40 + kind)
    long_len = (16 << 20) if kind == ref.CRC32 else (4 << 20)
    longs = [(0, long_len), (5, long_len + 7), (tile + 3, long_len // 2), (tile // 2, long_len // 2 + tile)]   # (the last two overlap each other and the first)
    count = (80 * 1024 * tile) // long_len
    segs = [longs[0] if k % 8 else longs[1 + (k // 8) % 3] for k in range(count)]
    assert sum(l for _, l in segs) > 70 * 1024 * tile
    for _ in range(1100):
        segs.insert(rnd.randrange(0, len(segs) + 1), (rnd.randrange(0, 1 << 20), rnd.randrange(0, 301)))
    big = [k for k, (_, l) in enumerate(segs) if l >= long_len // 2]
    assert len(segs) > 1024 and big[0] < 1024 < big[-1]
    _digest_repeated(batch, dev_source, source, segs, kind)


@pytest.mark.parametrize("repeats", [3, 5])
def test_a_few_tiles_a_block(pkg, batch, dev_source, source, repeats):
    """more tiles than blocks, fewer than 64 a block: 3 and 5 times the 16 MiB source are 1536 and 2560 tiles, so a block takes one to three, and a
    wave's sums wait beside one another without ever filling its lanes"""
    segs = [(3, (16 << 20) - 1)] * repeats + [(100, 50)]
    _digest_repeated(batch, dev_source, source, segs, ref.CRC32)


def test_argument_failures(pkg, batch, dev_source):
    L = pkg.load_library()
    one_ptr, one_len, out = (ctypes.c_void_p * 1)(dev_source.data_ptr()), (ctypes.c_size_t * 1)(4), (ctypes.c_uint32 * 1)()
    for args in ((None, one_len, out), (one_ptr, None, out), (one_ptr, one_len, None)):
        assert L.BrotliAmdBatchDigestSegments(batch._h, 1, 1, args[0], args[1], args[2], None) < 0 and pkg.last_error()
    for kind in (0, 3):
        assert L.BrotliAmdBatchDigestSegments(batch._h, kind, 1, one_ptr, one_len, out, None) < 0 and "kind" in pkg.last_error()
    assert L.BrotliAmdBatchDigestSegments(batch._h, 1, 0, None, None, None, None) == 0


# ------------------------------------------------------------------ the outputs of a decode call
OUTPUT_LABELS = ["T-text-cf", "W-edge-w10-ctx", "W-edge-w16-cf", "L-n64-d64-cf", "D-p0-d15-cf",
                 "T-text-ctx/99360/None",       # too small a capacity
                 "M-rows-w22-ctx/1308809/flip", # a damaged stream: an error
                 "T-text-cf4/198785/flip",      # another: its input ends early
                 "W-edge-w16-cf/68445/cut"]


@pytest.fixture(scope="module")
def streams():
    by = {label: (c, cap) for label, c, cap, _, _ in cv.leg_set()}
    return [by[label] for label in OUTPUT_LABELS]


def _want(kind, results, outs):
    assert [len(o) for o in outs] == [r.decoded_size for r in results]
    return [ref.crc(kind, o) for o in outs]


def test_outputs_of_decode_device(pkg, streams):
    import torch
    datas, caps = [c for c, _ in streams], [cap for _, cap in streams]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    arena = torch.zeros(sum(caps) + 64, dtype=torch.uint8, device="cuda")   # the outputs back to back, at whatever alignment that gives
    offs = [sum(caps[:i]) + 3 for i in range(len(caps))]
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        b.decode_device([t.data_ptr() for t in d_in], [len(d) for d in datas], [arena.data_ptr() + o for o in offs], caps, FLAGS)
        with pytest.raises(RuntimeError, match="wait"):   # a launch nobody has waited for
            b.digest_outputs(ref.CRC32)
        results = b.wait()
        assert {r.result for r in results} >= {0, 1, 3}, [r.result for r in results]   # an error, successes, NEEDS_MORE_OUTPUT
        host = arena.cpu().numpy()
        outs = [host[o:o + r.decoded_size].tobytes() for o, r in zip(offs, results)]
        ms = b.last_kernel_ms()
        first = {}
        for kind in KINDS:
            first[kind] = b.digest_outputs(kind)
            assert first[kind] == _want(kind, results, outs), kind
        assert b.last_kernel_ms() == ms   # (not a decode call: the accessors say what they said)
        b.relaunch()
        again = b.wait()
        assert [(r.result, r.decoded_size) for r in again] == [(r.result, r.decoded_size) for r in results]
        for kind in KINDS:
            assert b.digest_outputs(kind) == first[kind]
    finally:
        b.close()


def test_outputs_of_decode_host(pkg, streams):
    b = pkg.Batch(len(streams))
    try:
        results, outs = b.decode_host([c for c, _ in streams], [cap for _, cap in streams], FLAGS)
        for kind in KINDS:
            assert b.digest_outputs(kind) == _want(kind, results, outs), kind
    finally:
        b.close()


def test_outputs_of_decode_device_packed(pkg, streams):
    import torch
    datas = [c for c, _ in streams]
    d_in = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    torch.cuda.synchronize()
    b = pkg.Batch(len(datas))
    try:
        results, ptr, offsets = b.decode_device_packed([t.data_ptr() for t in d_in], [len(d) for d in datas], flags=FLAGS)
        blob = b.packed_fetch(offsets[-1])
        outs = [blob[offsets[i]:offsets[i + 1]] for i in range(len(datas))]
        for kind in KINDS:
            assert b.digest_outputs(kind) == _want(kind, results, outs), kind
        ptr2, offsets2 = b._packed_view(len(datas))   # BrotliAmdBatchPackedOutput still returns the buffer
        assert (ptr2, offsets2) == (ptr, offsets) and ptr != 0
        assert b.packed_fetch(offsets[-1]) == blob
    finally:
        b.close()


def test_outputs_of_a_fresh_batch(pkg):
    b = pkg.Batch(4)
    try:
        out = (ctypes.c_uint32 * 4)()
        assert pkg.load_library().BrotliAmdBatchDigestOutputs(b._h, 1, out) < 0 and "no decode call" in pkg.last_error()
        assert pkg.load_library().BrotliAmdBatchDigestOutputs(b._h, 1, None) < 0
    finally:
        b.close()


def test_the_digest_buffer_goes_with_its_owner(pkg, dev_source):
    """the segment table and the digests are one owned buffer of the batch object (csrc/brotli_host.h: Buffer), reused from call to call"""
    L = pkg.load_library()
    L.brotli_amd_debug_live_bytes.restype = None
    L.brotli_amd_debug_live_bytes.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]

    def live():
        dev, pin = ctypes.c_size_t(0), ctypes.c_size_t(0)
        L.brotli_amd_debug_live_bytes(ctypes.byref(dev), ctypes.byref(pin))
        return dev.value, pin.value

    base = live()
    b = pkg.Batch(1)
    fresh = live()
    b.digest_segments([dev_source.data_ptr() + 1] * 100, [50] * 100)
    held = live()
    assert held[0] > fresh[0]
    b.digest_segments([dev_source.data_ptr()] * 10, [7] * 10, ref.CRC32C)
    assert live() == held   # (a smaller table: the same buffer again)
    b.close()
    assert live() == base
