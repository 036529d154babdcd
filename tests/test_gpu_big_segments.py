"""Every segment kernel past 2^32 bits, bytes and elements (needs a real MI355X): the ragged copy, the digests, unshuffle, undelta, bit-unshuffle,
bit-unpack, unvarint, unrle, undict and undlba on single segments of L = 2^32 + 2^20 + 5 bytes and more, where a 64-bit position narrowed by
mistake -- a unit index times 16, a tile index times its units, j m of a byte plane, an element index times k bits, a run's payload bit, an
item number times 1024, a count, an offset sum -- corrupts silently and every suite of 16 MiB stays green.

The source is big_segments.py's: a seeded period of P = 262147 bytes repeated on the device, so that the bytes at p and p - 2^k never agree by
construction (asserted on the sampled windows).  Every case checks (a) every result field, exactly; (b) host windows of 4 KiB at the segment's
first and last bytes, around every threshold it crosses (bit 2^32 = byte 2^29, byte and element 2^31 and 2^32, j m of each plane, in source and
destination terms) and at 32 seeded places, against big_segments.py's closed forms, which test_big_segments_cpu.py proves against the
whole-array references; (c) the WHOLE destination on the device against a torch restatement, in pieces of at most 2 GiB; (d) 64 sentinel bytes
in front of and behind each destination, and the short segments beside the long one.  All comparisons are exact; no time is asserted.

One source buffer and one destination buffer for the module; the peak of device memory stays under 24 GiB (asserted when the module ends, and
printed with every case's device and wall time: run with -s to see the table).  The one skip: less free device memory than BUDGET.

Three shapes differ from the round ones first thought of, each because the round one does not cross the threshold it is there for: unshuffle
w = 8 takes the smallest length whose plane 7 begins past 2^32 + 2^20; bit-unpack (31, 4) takes the smallest count whose SOURCE passes
2^32 + 2^20 bytes (31 / 32 of L destination bytes stay below 2^32); unvarint takes the smallest source that holds 2^32 + 2^20 varints (7 / 8
of L bytes are fewer than 2^32).

Out of scope here: undbp alone (its walk is one wave per block header, and undlba's run covers the shared item code); undict-bytes and undba
(their byte-a-lane phases take seconds per GiB: profiles/undba.txt, profiles/undict_bytes.txt); unnull; the outputs of a decode call at this
size (digest_outputs and the *_outputs calls: no decode call here); Brotli streams of more than 4 GiB of output."""
import ctypes
import random
import time

import numpy as np
import pytest

import big_segments as B
import digest_ref

pytestmark = pytest.mark.gpu

P = B.P
L = (1 << 32) + (1 << 20) + 5
PAST = (1 << 32) + (1 << 20)                # what a position has to pass to be past the last threshold
T29, T31, T32 = 1 << 29, 1 << 31, 1 << 32
ROOM = 4 * P                                # bytes in front of the source that a test may overwrite: a header directly in front of a payload
LEN8 = 8 * ((PAST + 6) // 7) + 3            # unshuffle w = 8: the smallest length, with a tail, for which 7 (len // 8) >= 2^32 + 2^20
SRC_BYTES = LEN8 + 4096                     # the longest source of any case, and room for the skews
DST_BYTES = 5 * (1 << 30) + (1 << 20)       # the longest destination: the RLE run of 5 2^30 + 3 bytes
BUDGET = 20 << 30                           # free device memory the module asks for: source, destination, unvarint's own source, the torch pieces
PEAK = 24 << 30

TIMES = []                                  # (case, device ms, the call's wall ms)


# ---------------------------------------------------------------- the buffers
class Big:
    def __init__(self):
        import torch
        self.per = B.period(20263)
        self.d_per = torch.from_numpy(self.per.copy()).cuda()
        self.buf = self.d_per.repeat((ROOM + SRC_BYTES + P - 1) // P + 1)   # built on the device: byte ROOM + p is per[p % P]
        self.dst = torch.empty(DST_BYTES, dtype=torch.uint8, device="cuda")
        self.guard = (torch.arange(B.GUARD, device="cuda") * 3 + 7).to(torch.uint8)
        torch.cuda.synchronize()
        assert self.buf.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0 and len(self.buf) >= ROOM + SRC_BYTES + 64

    def s0(self, align, least=0):
        """the first source position >= least whose device address is `align` past a multiple of 16"""
        return least + (align - (ROOM + least)) % 16

    def src(self, s0, n):
        assert 0 <= s0 and s0 + n <= SRC_BYTES
        return self.buf[ROOM + s0:ROOM + s0 + n]

    def src_ptr(self, s0):
        return self.buf.data_ptr() + ROOM + s0

    def fresh(self, spans, fill=0xA5):
        """the destination in front of a call: `fill` from its first byte to behind the last span, and the guard pattern in front of and behind
        each span [d, d + n)"""
        end = max(d + n for d, n in spans) + B.GUARD
        assert end <= DST_BYTES
        self.dst[:end].fill_(fill)
        for d, n in spans:
            assert d >= B.GUARD
            self.dst[d - B.GUARD:d] = self.guard
            self.dst[d + n:d + n + B.GUARD] = self.guard

    def guards_intact(self, spans, what):
        import torch
        for d, n in spans:
            assert torch.equal(self.dst[d - B.GUARD:d], self.guard), (what, "the guard in front of", d)
            assert torch.equal(self.dst[d + n:d + n + B.GUARD], self.guard), (what, "the guard behind", d + n)


@pytest.fixture(scope="module")
def big():
    import torch
    torch.cuda.init()
    free, _ = torch.cuda.mem_get_info()
    if free < BUDGET:
        pytest.skip("%d bytes of device memory are free, this module needs %d" % (free, BUDGET))
    torch.cuda.reset_peak_memory_stats()
    b = Big()
    yield b
    peak = torch.cuda.max_memory_allocated()
    print("\nbig segments: peak device memory %d bytes (%.2f GiB)" % (peak, peak / 2.0 ** 30))
    for name, dev_ms, wall_ms in TIMES:
        print("big segments: %-58s device %9.3f ms   call %9.3f ms" % (name, dev_ms, wall_ms))
    del b
    torch.cuda.empty_cache()
    assert peak < PEAK, peak


@pytest.fixture(scope="module")
def batch(pkg):
    b = pkg.Batch(1)   # (the number of segments is not bound by max_streams)
    yield b
    b.close()


def _timed(name, call, last_ms=None):
    """the call, its wall time, and its device time: the library's own where it has one, events around the call where not"""
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    e1.record()
    torch.cuda.synchronize()
    TIMES.append((name, last_ms() if last_ms is not None else e0.elapsed_time(e1), wall))
    return out


def _upload(data, front=0):
    """bytes on the device, `front` bytes past a multiple of 16, with 16 bytes of room behind them -> (the tensor that owns them, their address)"""
    import torch
    t = torch.frombuffer(bytearray(front) + bytearray(data) + bytearray(16), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + front


# ---------------------------------------------------------------- the checks that every case shares
def _first_difference(got, want):
    at = int(np.flatnonzero(got != want)[0])
    return at, int(got[at]), int(want[at])


def _host_windows(name, t, base, wins, window):
    """(b): the bytes [base + a, base + b) of the device tensor t against window(a, b), for every window; one copy to the host"""
    import torch
    if not wins:
        return
    got = torch.cat([t[base + a:base + b] for a, b in wins]).cpu().numpy()
    at = 0
    for a, b in wins:
        want = window(a, b)
        assert len(want) == b - a
        piece = got[at:at + b - a]
        if not np.array_equal(piece, want):
            i, g, w = _first_difference(piece, want)
            raise AssertionError("%s: window [%d, %d): byte %d (2^32 %+d) is %#x, not %#x; %d of its bytes differ"
                                 % (name, a, b, a + i, a + i - T32, g, w, int((piece != want).sum())))
        at += b - a


def _equal(name, a, b):
    """(c) for a copy: two device tensors, in pieces of 1 GiB"""
    import torch
    assert len(a) == len(b), (name, len(a), len(b))
    for i in range(0, len(a), 1 << 30):
        assert torch.equal(a[i:i + (1 << 30)], b[i:i + (1 << 30)]), (name, "the piece from byte", i)


def _thresholds(n, more=()):
    """the bytes of a destination of n bytes at which a narrowed position would first go wrong"""
    return [t for t in [T29, T31, T32] + list(more) if 0 < t < n]


def _source_windows(n, seed):
    """the windows on which the condition on the INPUTS is asserted: those of a source of n bytes"""
    return B.windows(n, [T29, T31, T32], seed)


# ---------------------------------------------------------------- torch restatements (c)
_INT = {}


def _ints(t, w):
    """a piece of device bytes as little-endian elements of w bytes -> int64, unsigned for w < 8 (a copy: any address)"""
    import torch
    if not _INT:
        _INT.update({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64})
    x = t.clone().view(_INT[w]).to(torch.int64)
    return x & ((1 << (8 * w)) - 1) if w in (2, 4) else x


def _t_unshuffle(name, src, dst, n, w):
    import torch
    m = n // w
    planes = src[:w * m].view(w, m)
    step = (1 << 30) // w
    for e0 in range(0, m, step):
        e1 = min(m, e0 + step)
        assert torch.equal(dst[e0 * w:e1 * w].view(e1 - e0, w), planes[:, e0:e1].t()), (name, "elements from", e0)
    assert torch.equal(dst[w * m:n], src[w * m:n]), (name, "the tail")


def _t_undelta(name, src, dst, n, w):
    """torch.cumsum in int64 with a carried sum and a mask"""
    import torch
    m, mask, carry = n // w, (1 << (8 * w)) - 1, 0
    step = 1 << 26
    for e0 in range(0, m, step):
        e1 = min(m, e0 + step)
        c = torch.cumsum(_ints(src[e0 * w:e1 * w], w), 0)
        c += carry
        if w < 8:
            c &= mask
        assert torch.equal(c, _ints(dst[e0 * w:e1 * w], w)), (name, "elements from", e0)
        carry = int(c[-1])
    assert torch.equal(dst[w * m:n], src[w * m:n]), (name, "the tail")


def _t_rows(name, s4, d3):
    """bit rows back into elements.  s4: (blocks, w, 8, R) -- row 8 j + k of a block is s4[:, j, k] --; d3: (blocks, 8 R, w)"""
    import torch
    nb, w, _, R = s4.shape
    out = torch.zeros((nb, R, 8, w), dtype=torch.uint8, device=s4.device)
    for t in range(8):
        for k in range(8):
            out[:, :, t, :] |= (((s4[:, :, k, :] >> t) & 1) << k).permute(0, 2, 1)
    assert torch.equal(out.view(nb, 8 * R, w), d3), name


def _t_bitunshuffle(name, src, dst, n, w, block):
    import torch
    m = n // w
    piece = 1 << 28   # bytes of destination at a time
    if block == 0 or block >= m:
        o, c = 0, m // 8 * 8
        s4 = src[:c * w].view(1, w, 8, c // 8)
        step = piece // (8 * w)
        for r0 in range(0, c // 8, step):
            r1 = min(c // 8, r0 + step)
            _t_rows((name, "rows' bytes from", r0), s4[..., r0:r1], dst[8 * r0 * w:8 * r1 * w].view(1, 8 * (r1 - r0), w))
    else:
        full = m // block
        s4 = src[:full * block * w].view(full, w, 8, block // 8)
        d3 = dst[:full * block * w].view(full, block, w)
        step = max(1, piece // (block * w))
        for b0 in range(0, full, step):
            _t_rows((name, "blocks from", b0), s4[b0:b0 + step], d3[b0:b0 + step])
        o, c = full * block * w, (m - full * block) // 8 * 8
        if c:
            _t_rows((name, "the last block"), src[o:o + c * w].view(1, w, 8, c // 8), dst[o:o + c * w].view(1, c, w))
    assert torch.equal(dst[o + c * w:n], src[o + c * w:n]), (name, "the tail")


def _t_fields(src, g0, g1, k, flags):
    """the fields of the groups g0 .. g1 - 1 of 8 fields (k bytes each) by shifts and masks -> int64 (groups, 8), sign-extended with SIGNED"""
    import torch
    b = src[g0 * k:g1 * k].view(-1, k).to(torch.int64)
    cols = []
    for t in range(8):
        if flags & B.MSB_FIRST:
            assert k == 1
            v = (b[:, 0] >> (7 - t)) & 1
        else:
            o, sh = divmod(t * k, 8)
            v = b[:, o].clone()
            for j in range(1, (sh + k + 7) // 8):
                v |= b[:, o + j] << (8 * j)
            v = (v >> sh) & ((1 << k) - 1)
        if flags & B.SIGNED:
            v = (v ^ (1 << (k - 1))) - (1 << (k - 1))
        cols.append(v)
    return torch.stack(cols, 1)


def _t_bitunpack(name, src, dst, count, k, w, flags, lookup=None):
    """every whole group of 8 elements (the count % 8 behind them are in the last host window); lookup: undict's table, int64"""
    import torch
    assert k <= 32
    step = 1 << 22
    mask = (1 << (8 * w)) - 1
    for g0 in range(0, count // 8, step):
        g1 = min(count // 8, g0 + step)
        v = _t_fields(src, g0, g1, k, flags).view(-1)
        v = lookup[v] if lookup is not None else v
        if w < 8:
            v &= mask
        assert torch.equal(v, _ints(dst[8 * g0 * w:8 * g1 * w], w)), (name, "groups from", g0)


def _t_unvarint(name, src, dst, n, flags, kept):
    """w = 1: the low 8 bits of every varint from its first two bytes, 0 for an overlong one, in pieces of 256 periods (a period ends with a
    terminator, so a piece begins with a varint: its j-th start and its j-th terminator are one varint's); the first `kept` elements are
    compared -> (count, consumed, overlong)"""
    import torch
    count = overlong = consumed = 0
    step = 256 * P
    pos = torch.arange(step, device=src.device)
    for p0 in range(0, n, step):
        s = src[p0:min(n, p0 + step)]
        term = s < 0x80
        begins = torch.ones_like(term)
        begins[1:] = term[:-1]
        e = pos[:len(s)][term]
        if not len(e):
            continue
        st = pos[:len(s)][begins][:len(e)]
        ln = e - st + 1
        v = (s[st] & 0x7F).to(torch.int32) | torch.where(ln >= 2, (s[torch.clamp(st + 1, max=len(s) - 1)] & 0x7F).to(torch.int32) << 7, 0)
        if flags & B.ZIGZAG:
            v = (v >> 1) ^ -(v & 1)
        over = ln > 10
        v = torch.where(over, 0, v & 0xFF).to(torch.uint8)
        take = max(0, min(len(e), kept - count))
        if take:
            assert torch.equal(v[:take], dst[count:count + take]), (name, "elements from", count)
        consumed = p0 + int(e[-1]) + 1
        count, overlong = count + len(e), overlong + int(over.sum())
    return count, consumed, overlong


# ---------------------------------------------------------------- the ragged copy
def _ragged_copy(pkg, segs):
    """segs: [(source address, destination address, length)]"""
    lib = pkg.load_library()
    n = len(segs)
    a_src = (ctypes.c_void_p * n)(*[s for s, _, _ in segs])
    a_dst = (ctypes.c_void_p * n)(*[d for _, d, _ in segs])
    a_len = (ctypes.c_size_t * n)(*[l for _, _, l in segs])
    assert lib.BrotliAmdDebugRaggedCopy(n, a_src, a_dst, a_len) == 0, pkg.last_error()


def _copy_case(pkg, big, name, table, seed):
    """table: [(s0, length)], the destinations back to back behind a guard, the first long one 11 past a multiple of 16; everything compared"""
    first_long = next(i for i, (_, l) in enumerate(table) if l > (1 << 20))
    d_at = B.GUARD + (11 - B.GUARD - sum(l for _, l in table[:first_long])) % 16
    segs = []
    for s0, l in table:
        segs.append((s0, d_at, l))
        d_at += l
    span = (segs[0][1], d_at - segs[0][1])
    big.fresh([span])
    assert (big.dst.data_ptr() + segs[first_long][1]) % 16 == 11
    _timed(name, lambda: _ragged_copy(pkg, [(big.src_ptr(s), big.dst.data_ptr() + d, l) for s, d, l in segs]))
    big.guards_intact([span], name)
    at = 0   # the segment's first unit's byte in the table
    for s0, d, l in segs:
        if l <= (1 << 20):
            _host_windows(name, big.dst, d, [(0, l)] if l else [], lambda a, b: B.copy_window(big.per, s0, a, b))
        else:
            wins = B.windows(l, _thresholds(l, [T32 - at, T32 + T29 - at]), seed)
            B.assert_distinct(big.per, s0, wins)
            _host_windows(name, big.dst, d, wins, lambda a, b: B.copy_window(big.per, s0, a, b))
            _equal(name, big.dst[d:d + l], big.src(s0, l))
        at += l


def _shorts(rnd, count):
    return [(rnd.randrange(0, 1 << 20), rnd.randrange(0, 301)) for _ in range(count)]


def test_ragged_copy_one_long_segment_among_short_ones(pkg, big):
    """[100 short segments, one of L, 100 short segments], the long one's source 5 and its destination 11 past a multiple of 16"""
    rnd = random.Random(1)
    s0 = big.s0(5, 1000)
    assert big.src_ptr(s0) % 16 == 5
    _copy_case(pkg, big, "ragged copy: 100 short, L, 100 short", _shorts(rnd, 100) + [(s0, L)] + _shorts(rnd, 100), 1)


def test_ragged_copy_a_long_segment_behind_2_to_the_28_units(pkg, big):
    """a segment of 4 GiB in front of one of 2^29 + 3 bytes: the second one's first unit is beyond unit 2^28, its base beyond byte 2^32"""
    rnd = random.Random(2)
    _copy_case(pkg, big, "ragged copy: 3 short, 4 GiB, 2^29 + 3, 3 short", _shorts(rnd, 3) + [(big.s0(5, 3), T32), (big.s0(9, 7777), T29 + 3)] + _shorts(rnd, 3), 2)


# ---------------------------------------------------------------- the digests
@pytest.mark.parametrize("kind", [digest_ref.CRC32, digest_ref.CRC32C])
def test_digests(big, batch, kind):
    """one segment of L; one of 2^29 + 7 bytes, whose bit count passes 2^32; the L segment between short ones"""
    rnd = random.Random(kind)
    long_s0, bits_s0 = big.s0(5, 100), big.s0(13, 3)
    want_long = B.crc_periodic(kind, big.per, long_s0, L)
    for name, table in (("L", [(long_s0, L)]), ("2^29 + 7", [(bits_s0, T29 + 7)]), ("50 short, L, 50 short", _shorts(rnd, 50) + [(long_s0, L)] + _shorts(rnd, 50))):
        name = "digest kind %d: %s" % (kind, name)
        for s0, l in table:
            if l > (1 << 20):
                B.assert_distinct(big.per, s0, _source_windows(l, kind))
        got = _timed(name, lambda: batch.digest_segments([big.src_ptr(s) for s, _ in table], [l for _, l in table], kind), batch.last_digest_ms)
        want = [want_long if (s, l) == (long_s0, L) else B.crc_periodic(kind, big.per, s, l) for s, l in table]
        assert got == want, (name, [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3])


# ---------------------------------------------------------------- the filters with a width per segment
def _width_case(big, name, call, last_ms, n, w, window, torch_check, marks, s_align=5, d_align=0, in_place=False, seed=0):
    """One launch over [a short segment, the long one of n bytes, a short segment], back to back behind a guard, the long one's source and
    destination at the given residues mod 16.  call(src addresses, dst addresses, lengths); window(s0, n) -> the window reference of a segment;
    torch_check(name, src, dst, n); marks: the destination bytes, beside 2^29, 2^31 and 2^32, around which windows are placed"""
    lens = [37 * w + 3, n, 53 * w + 1]
    s0s = [big.s0(3, 200), big.s0(s_align, 1000), big.s0(9, 70000)]
    d0 = B.GUARD + (d_align - B.GUARD - lens[0]) % 16
    ds = [d0, d0 + lens[0], d0 + lens[0] + n]
    span = (d0, sum(lens))
    big.fresh([span])
    assert (big.dst.data_ptr() + ds[1]) % 16 == d_align and (big.src_ptr(s0s[1]) % 16 == s_align or in_place)
    dp = big.dst.data_ptr()
    if in_place:   # the long segment alone: its address is a multiple of the width, the short ones' are not
        big.dst[ds[1]:ds[1] + n].copy_(big.src(s0s[1], n))
        _timed(name, lambda: call([big.src_ptr(s0s[0]), dp + ds[1], big.src_ptr(s0s[2])], [dp + d for d in ds], lens), last_ms)
    else:
        _timed(name, lambda: call([big.src_ptr(s) for s in s0s], [dp + d for d in ds], lens), last_ms)
    big.guards_intact([span], name)
    for i in (0, 2):
        _host_windows(name + ": short segment %d" % i, big.dst, ds[i], [(0, lens[i])], window(s0s[i], lens[i]))
    wins = B.windows(n, _thresholds(n, marks), seed)
    B.assert_distinct(big.per, s0s[1], _source_windows(n, seed))
    _host_windows(name, big.dst, ds[1], wins, window(s0s[1], n))
    torch_check(name, big.src(s0s[1], n), big.dst[ds[1]:ds[1] + n], n)


def _plane_marks(n, w):
    """the destination bytes whose SOURCE byte is byte 2^29, 2^31, 2^32 or 2^32 + 2^20 of the segment (the planes' starts j m and their last
    bytes are the source of the destination's first w and last w bytes: the windows at the segment's two ends hold them)"""
    m, out = n // w, []
    for t in (T29, T31, T32, PAST):
        j = t // m
        if j < w:
            out.append((t - j * m) * w + j)
    return out


@pytest.mark.parametrize("w,n", [(2, L), (4, L), (8, LEN8)])
def test_unshuffle(big, batch, w, n):
    """w = 2 and 4 at L: m and 3 m pass 2^31; w = 8 at the smallest length for which plane 7's 7 m passes 2^32 + 2^20; every one with a tail"""
    m = n // w
    assert n % w and (w - 1) * m >= (PAST if w == 8 else T31)
    _width_case(big, "unshuffle w = %d, %d bytes" % (w, n), lambda s, d, l: batch.unshuffle_segments(s, d, l, [w] * 3), batch.last_unshuffle_ms, n, w,
                lambda s0, nn: (lambda a, b: B.unshuffle_window(big.per, s0, nn, w, a, b)), lambda name, s, d, nn: _t_unshuffle(name, s, d, nn, w),
                _plane_marks(n, w), d_align=11, seed=w)


@pytest.mark.parametrize("w,in_place", [(1, False), (8, False), (4, True)])
def test_undelta(pkg, big, batch, w, in_place):
    """w = 1 at L: the elements pass 2^32; w = 8 at L: more than 260 000 tiles and their carries; w = 4 in place"""
    assert L // pkg.undelta_tile() > 260000
    _width_case(big, "undelta w = %d at L%s" % (w, ", in place" if in_place else ""), lambda s, d, l: batch.undelta_segments(s, d, l, [w] * 3),
                batch.last_undelta_ms, L, w, lambda s0, nn: (lambda a, b: B.undelta_window(big.per, s0, nn, w, a, b)),
                lambda name, s, d, nn: _t_undelta(name, s, d, nn, w), [P * w, T32 // w * w], d_align=0 if in_place else 3, in_place=in_place, seed=10 + w)


@pytest.mark.parametrize("w,block,n,d_align", [(1, 0, L, 0), (4, 2048, L, 0), (1, 8192, L, 11)])
def test_bitunshuffle(big, batch, w, block, n, d_align):
    """w = 1 with one block at L: eight rows of m / 8 bytes, a little more than 2^29 each, so that rows 0, 3 and 7 hold the source's bytes 2^29,
    2^31 and 2^32; w = 4 with the default block of 8192 / w at L; both at a destination that is a multiple of 16, the fast way.  The bit-by-bit
    way -- a destination 11 past a multiple of 16 -- at L as well (19 ms), with w = 1 in blocks of 8192, whose element numbers pass 2^32"""
    R = n // w // 8   # one block: the bytes of a row; the elements whose row bytes are the source's bytes 2^29, 2^31 and 2^32
    rows = [] if block else [8 * (t - t // R * R) * w for t in (T29, T31, T32) if t // R < 8 * w]
    _width_case(big, "bit-unshuffle w = %d, block %d, %d bytes, dst %% 16 = %d" % (w, block, n, d_align),
                lambda s, d, l: batch.bitunshuffle_segments(s, d, l, [w] * 3, [block] * 3), batch.last_bitunshuffle_ms, n, w,
                lambda s0, nn: (lambda a, b: B.bitunshuffle_window(big.per, s0, nn, w, block, a, b)),
                lambda name, s, d, nn: _t_bitunshuffle(name, s, d, nn, w, block), rows + [n // w // 8 * 8 * w], d_align=d_align, seed=20 + w)


# ---------------------------------------------------------------- bit-unpack
def _count_for_source(k, nbytes):
    """the smallest count of fields of k bits that take at least nbytes of source"""
    return (8 * nbytes + k - 1) // k


@pytest.mark.parametrize("k,w,flags,count,d_align", [
    (3, 1, 0, L, 0), (31, 4, 0, _count_for_source(31, PAST), 0), (1, 1, B.MSB_FIRST | B.SIGNED, T32 + 64 + 3, 0),
    (3, 1, 0, L, 11)])
def test_bitunpack(big, batch, k, w, flags, count, d_align):
    """(3, 1) into L bytes: the source bit passes 2^32 at its byte 2^29 and the element count passes 2^32; (31, 4) from a source of more than 2^32
    bytes; (1, 1) MSB-first and signed at 2^32 + 64 + 3 elements; and (3, 1) the byte-by-byte way, at a destination 11 past a multiple of 16"""
    name = "bit-unpack (%d, %d) flags %d, %d elements, dst %% 16 = %d" % (k, w, flags, count, d_align)
    src_len = (count * k + 7) // 8
    s0 = big.s0(5, 1000)
    d = B.GUARD + (d_align - B.GUARD) % 16
    big.fresh([(d, count * w)])
    # around the elements whose fields hold source bit 2^32, source bytes 2^31 and 2^32, and around element and byte 2^31 and 2^32
    marks = [t * 8 // k * w for t in (T29, T31, T32)] + [T31 * w, T32 * w]
    _timed(name, lambda: batch.bitunpack_segments([big.src_ptr(s0)], [src_len], [big.dst.data_ptr() + d], [count], [k], [w], [flags]), batch.last_bitunpack_ms)
    big.guards_intact([(d, count * w)], name)
    B.assert_distinct(big.per, s0, _source_windows(src_len, k))
    _host_windows(name, big.dst, d, B.windows(count * w, _thresholds(count * w, marks), k), lambda a, b: B.bitunpack_window(big.per, s0, count, k, w, flags, a, b))
    _t_bitunpack(name, big.src(s0, src_len), big.dst[d:d + count * w], count, k, w, flags)


# ---------------------------------------------------------------- unvarint
@pytest.fixture(scope="module")
def varints(big):
    """unvarint's own source: a period in which 7 of 8 bytes are terminators and the last byte is one, three overlong varints in it, repeated
    on the device until it holds 2^32 + 2^20 varints and two bytes of a varint that does not end"""
    import torch
    per = B.varint_period(20264)
    n = B.unvarint_length(per, PAST)
    while per[n % P] < 0x80:   # (go on to the next continuation byte and end behind it, inside a varint: consumed < the length)
        n += 1
    n += 1
    buf = torch.from_numpy(per.copy()).cuda().repeat((n + 64 + P - 1) // P + 1)
    yield per, buf, n
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("flags,cap", [(0, 1 << 56), (B.ZIGZAG, 1 << 56), (0, T32 + 10)])
def test_unvarint(big, batch, varints, flags, cap):
    """w = 1, plain and zigzag, and once with a capacity of 2^32 + 10 below the count; count, consumed and overlong exact"""
    per, buf, n = varints
    name = "unvarint w = 1 flags %d, %d source bytes, cap %s" % (flags, n, "none" if cap == 1 << 56 else "2^32 + 10")
    want = B.unvarint_result(per, n)
    assert want[0] >= PAST and want[0] > T32 + 10 and want[1] < n and n > T32 and want[2] >= 3 * (n // P)
    kept = min(cap, want[0])
    d = B.GUARD + 16
    big.fresh([(d, kept)])
    got = _timed(name, lambda: batch.unvarint_segments([buf.data_ptr()], [n], [big.dst.data_ptr() + d], [cap], [1], [flags]), batch.last_unvarint_ms)
    assert got == [want], (name, got, want)
    big.guards_intact([(d, kept)], name)
    B.assert_distinct(per, 0, _source_windows(n, 5))
    marks = [int(t * want[0] / n) for t in (T31, T32)]   # about where the source's byte 2^31 and 2^32 end up
    _host_windows(name, big.dst, d, B.windows(kept, _thresholds(kept, marks), 30 + flags), lambda a, b: B.unvarint_window(per, n, 1, flags, cap, a, b))
    assert _t_unvarint(name, buf, big.dst[d:d + kept], n, flags, kept) == want


# ---------------------------------------------------------------- unrle and undict
def _rle_source(big, plan, k):
    """the segment's bytes on the device.  A plan whose one packed run's payload is the module's source at s0 gets its front written into the
    room directly in front of that payload; every other plan is materialised on the host -> (what owns the bytes, the address, the length)"""
    import torch
    n = sum(B.run_bytes(r, k) for r in plan)
    if len(plan) == 1 and plan[0][0] == "packed" and plan[0][1] * k // 8 > (1 << 24):
        front = B.run_front(plan[0], k)
        s0 = plan[0][3]
        assert plan[0][2] is big.per and s0 == 0 and len(front) <= ROOM   # (the room: no test's source)
        big.buf[ROOM + s0 - len(front):ROOM + s0] = torch.frombuffer(bytearray(front), dtype=torch.uint8).cuda()
        return None, big.src_ptr(s0) - len(front), n
    data = B.rle_materialise(plan, k)
    assert len(data) == n
    t, ptr = _upload(data, 3)
    return t, ptr, n


def _t_runs(name, big, plan, k, w, kept, d, lookup=None):
    """(c) run by run: an RLE run's elements are all its value (or the entry it names), a packed run's are bit-unpack's restatement of its payload"""
    import torch
    start = 0
    for run in plan:
        lo, hi = start, min(kept, start + run[1])
        if lo < hi and run[0] == "rle":
            v = run[2] if lookup is None else int(lookup[run[2]]) if run[2] < len(lookup) else 0
            want = np.array([v], dtype="<i8").view(np.uint8)[:w]
            want_t = torch.from_numpy(want.copy()).cuda()
            for a in range(lo, hi, (1 << 30) // w):
                b = min(hi, a + (1 << 30) // w)
                assert bool((big.dst[d + a * w:d + b * w].view(-1, w) == want_t).all()), (name, "the RLE run from element", start, "elements from", a)
        elif lo < hi:
            payload = torch.from_numpy(B.materialise(run[2], run[3], run[1] * k // 8)).cuda() if run[2] is not big.per else big.src(run[3], run[1] * k // 8)
            _t_bitunpack((name, "the packed run from element", start), payload, big.dst[d + lo * w:d + hi * w], (hi - lo) // 8 * 8, k, w, 0, lookup)
        start += run[1]


GIANT_RLE = [("rle", 5 * (1 << 30) + 3, 0x55)]                       # k = 7: one run of 5 2^30 + 3 values from six source bytes, five of them the header
THREE_RUNS = [("rle", T32 + 5, 0x2A), ("packed", 4096, None, 3), ("rle", 77, 0x7F)]   # k = 7: the second and third run begin beyond element 2^32


def _plan(big, name):
    if name == "rle":
        return 7, GIANT_RLE
    if name == "packed":
        return 1, [("packed", T32 + (1 << 13), big.per, 0)]   # k = 1: the payload's bit offset passes 2^32
    return 7, [r if r[0] == "rle" else ("packed", r[1], big.per, r[3]) for r in THREE_RUNS]


@pytest.mark.parametrize("cap", ["all", "in front of 2^32", "behind 2^32"])
@pytest.mark.parametrize("which", ["rle", "packed", "three runs"])
def test_unrle(big, batch, which, cap):
    """one RLE run of 5 2^30 + 3 values of k = 7 (its header's five bytes allow 2^34); one bit-packed run at k = 1 of 2^32 + 2^13 values; three runs
    (RLE, packed, RLE) whose second and third begin beyond element 2^32; each with all its elements, with a capacity of 2^32 - 5 and with one of
    2^32 + 7, into w = 1.  count, consumed, runs and status are what the segment holds, whatever the capacity"""
    k, plan = _plan(big, which)
    name = "unrle %s, k = %d, cap %s" % (which, k, cap)
    want = B.rle_result(plan, k)
    assert len(B.rle_header(GIANT_RLE[0][1] << 1)) == 5 and want[0] > T32 + 7
    cap = {"all": want[0], "in front of 2^32": T32 - 5, "behind 2^32": T32 + 7}[cap]
    kept = min(cap, want[0])
    own, ptr, n = _rle_source(big, plan, k)
    d = B.GUARD + 16 + 5
    big.fresh([(d, kept)])
    got = _timed(name, lambda: batch.unrle_segments([ptr], [n], [big.dst.data_ptr() + d], [cap], [k], [1]), batch.last_unrle_ms)
    assert got == [want] and want[1] == n, (name, got, want)
    big.guards_intact([(d, kept)], name)
    marks = [T32 + 5, T32 + 5 + 4096] if which == "three runs" else []
    _host_windows(name, big.dst, d, B.windows(kept, _thresholds(kept, marks), 40), lambda a, b: B.rle_window(plan, k, 1, cap, a, b))
    _t_runs(name, big, plan, k, 1, kept, d)


@pytest.mark.parametrize("which", ["rle", "packed"])
def test_undict_wide_entries(big, batch, which):
    """the RLE giant and the k = 1 packed giant as indices into a dictionary of 2 entries of w = 8: 2^29 + 5 elements, 4 GiB and 40 bytes of
    destination (the packed run holds 2^29 + 8 fields, the capacity keeps 2^29 + 5)"""
    import torch
    table = np.array([0x0123456789ABCDEF, 0xFEDCBA9876543210], dtype=np.uint64)
    count = T29 + 5
    plan = [("rle", count, 1)] if which == "rle" else [("packed", T29 + 8, big.per, 0)]
    name = "undict %s giant, k = 1, w = 8, %d elements" % (which, count)
    want = B.undict_result(plan, 1, 2, count)
    assert want[5:] == (0, B.NONE) and count * 8 > T32
    own, ptr, n = _rle_source(big, plan, 1)
    d_table, table_ptr = _upload(table.astype("<u8").tobytes(), 8)
    d = B.GUARD + 16
    big.fresh([(d, count * 8)])
    got = _timed(name, lambda: batch.undict_segments([ptr], [n], [big.dst.data_ptr() + d], [count], [1], [8], [0], [table_ptr], [2]), batch.last_undict_ms)
    assert got == [want], (name, got, want)
    big.guards_intact([(d, count * 8)], name)
    _host_windows(name, big.dst, d, B.windows(count * 8, _thresholds(count * 8), 50), lambda a, b: B.undict_window(plan, 1, 8, table, 2, count, a, b))
    _t_runs(name, big, plan, 1, 8, count, d, torch.from_numpy(table.view(np.int64).copy()).cuda())


def test_undict_one_bad_index_beyond_element_2_to_the_32(big, batch):
    """k = 2, w = 1, three entries: an RLE run of 2^32 + 3 good indices, a packed run whose field 1 is 3, an RLE run -- bad is 1 and first_bad is
    element 2^32 + 4"""
    import torch
    table = np.array([7, 9, 11], dtype=np.uint64)
    plan = [("rle", T32 + 3, 1), ("packed", 8, np.array([0x0C, 0x00], dtype=np.uint8), 0), ("rle", 5, 2)]
    name = "undict one bad index at element 2^32 + 4, k = 2, w = 1"
    count = T32 + 3 + 8 + 5
    want = B.undict_result(plan, 2, 3, count)
    assert want == (count, 6 + 3 + 2, 3, 0, 2, 1, T32 + 4), want
    own, ptr, n = _rle_source(big, plan, 2)
    d_table, table_ptr = _upload(table.astype(np.uint8).tobytes(), 1)
    d = B.GUARD + 16 + 7
    big.fresh([(d, count)])
    got = _timed(name, lambda: batch.undict_segments([ptr], [n], [big.dst.data_ptr() + d], [count], [2], [1], [0], [table_ptr], [3]), batch.last_undict_ms)
    assert got == [want], (name, got, want)
    big.guards_intact([(d, count)], name)
    _host_windows(name, big.dst, d, B.windows(count, _thresholds(count), 51), lambda a, b: B.undict_window(plan, 2, 1, table, 3, count, a, b))
    assert bool((big.dst[d:d + T32 + 3] == 9).all())
    assert big.dst[d + T32 + 3:d + count].cpu().tolist() == [7, 0, 7, 7, 7, 7, 7, 7] + [11] * 5


# ---------------------------------------------------------------- undlba
DLBA_COUNT, DLBA_LENGTH = (1 << 20) + 3, 4099


@pytest.mark.parametrize("flags,base,data_cap", [(B.OFFSETS64, 0, None), (0, 0, None), (B.OFFSETS64, 0, T32 + 1), (B.OFFSETS64 | B.ENDS_ONLY, (1 << 33) + 1, None)])
def test_undlba(big, batch, flags, base, data_cap):
    """a page of 2^20 + 3 strings of 4099 bytes -- lengths of width-0 miniblocks, about 4.003 GiB of data from the periodic source --: int64
    offsets exact past 2^32 and bytes == data_avail; int32 offsets, the int64 ones truncated; a data capacity of 2^32 + 1, cut to the byte;
    ends only, on an offset base of 2^33 + 1"""
    import torch
    name = "undlba 2^20 + 3 strings of 4099 bytes, flags %d, base %d, data cap %s" % (flags, base, data_cap)
    head = B.dlba_lengths(DLBA_COUNT, DLBA_LENGTH)
    avail = DLBA_COUNT * DLBA_LENGTH
    s0 = 0   # (the lengths lie in the room in front of the source, which is no test's source)
    assert avail > PAST and len(head) <= ROOM and avail + s0 <= SRC_BYTES
    big.buf[ROOM + s0 - len(head):ROOM + s0] = torch.frombuffer(bytearray(head), dtype=torch.uint8).cuda()
    want = B.dlba_result(DLBA_COUNT, DLBA_LENGTH, avail, DLBA_COUNT)
    assert want[10] == want[11] == avail and want[7] == 0
    kept = avail if data_cap is None else data_cap
    ow = 8 if flags & B.OFFSETS64 else 4
    o_len = (DLBA_COUNT + (0 if flags & B.ENDS_ONLY else 1)) * ow
    offsets = torch.full((o_len + 2 * B.GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets[:B.GUARD] = big.guard
    offsets[B.GUARD + o_len:] = big.guard
    d = B.GUARD + 16 + 9
    big.fresh([(d, kept)])
    got = _timed(name, lambda: batch.undlba_segments([big.src_ptr(s0) - len(head)], [len(head) + avail], [offsets.data_ptr() + B.GUARD], [big.dst.data_ptr() + d],
                                                     [kept], [DLBA_COUNT], [flags], [base]), batch.last_undlba_ms)
    assert got == [want], (name, got, want)
    big.guards_intact([(d, kept)], name)
    assert torch.equal(offsets[:B.GUARD], big.guard) and torch.equal(offsets[B.GUARD + o_len:], big.guard), name
    # the offsets: every one on the host against the closed form, and on the device against base + i length
    _host_windows(name + ": offsets", offsets, B.GUARD, [(0, o_len)], lambda a, b: B.dlba_offsets_window(DLBA_COUNT, DLBA_LENGTH, DLBA_COUNT, base, flags, a, b))
    first = 1 if flags & B.ENDS_ONLY else 0
    ends = torch.arange(first, DLBA_COUNT + 1, device="cuda", dtype=torch.int64) * DLBA_LENGTH + base
    assert int(ends[-1]) == base + avail and int(ends[-1]) > T32
    assert torch.equal(ends & ((1 << 32) - 1) if ow == 4 else ends, _ints(offsets[B.GUARD:B.GUARD + o_len], ow)), name
    if ow == 4:
        assert base + avail >= T32 and int(_ints(offsets[B.GUARD + o_len - 4:B.GUARD + o_len], 4)[0]) == (base + avail) % T32   # truncated, not saturated
    # the data
    B.assert_distinct(big.per, s0, _source_windows(kept, 60))
    _host_windows(name, big.dst, d, B.windows(kept, _thresholds(kept, [T32 // DLBA_LENGTH * DLBA_LENGTH]), 60), lambda a, b: B.copy_window(big.per, s0, a, b))
    _equal(name, big.dst[d:d + kept], big.src(s0, kept))
