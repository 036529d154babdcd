"""What the tests of segments beyond 2^32 bits, bytes and elements share (test_big_segments_cpu.py, test_gpu_big_segments.py): a source that is
cheap at any length -- a seeded period of P bytes repeated, byte p being period[p % P] --, and for every segment kernel a closed form that gives
the destination bytes of any window [a, b) of ONE segment from the period and the segment's parameters alone, in O(P + b - a) numpy work.  A
segment's source begins at byte s0 of the periodic stream.  Nothing here imports the package or reads csrc; test_big_segments_cpu.py proves
every closed form against the whole-array references (shuffle_ref, delta_ref, bitshuffle_ref, bitpack_ref, varint_ref, rle_ref, dict_ref,
dlba_ref, digest_ref, zlib) on materialised bytes before test_gpu_big_segments.py trusts them."""
import random
import zlib

import numpy as np

import digest_ref

P = 262147        # the period: an odd prime near 2^18, so that p and p - 2^k never fall on the same byte of the period
GUARD = 64        # sentinel bytes in front of and behind a destination
WINDOW = 4096     # bytes of a host window
MSB_FIRST, SIGNED = 1, 2          # bit-unpack's flags
ZIGZAG = 1                        # unvarint's flag
OFFSETS64, ENDS_ONLY = 2, 4       # undlba's flags
NONE = (1 << 64) - 1              # first_bad where nothing was bad
M64 = (1 << 64) - 1


def is_prime(n):
    if n < 2:
        return False
    i = 2
    while i * i <= n:
        if n % i == 0:
            return False
        i += 1
    return True


assert P % 2 == 1 and is_prime(P) and all((1 << k) % P for k in (29, 31, 32))


def period(seed, size=P):
    """`size` seeded bytes, never changed"""
    a = np.random.default_rng(seed).integers(0, 256, size=size, dtype=np.uint8)
    a.setflags(write=False)
    return a


def at(per, s0, idx):
    """the source bytes at the segment's positions idx (an int64 array, or anything numpy makes one of)"""
    return per[(np.asarray(idx, dtype=np.int64) + s0) % len(per)]


def materialise(per, s0, n):
    """the n bytes of a segment: for small totals only"""
    return at(per, s0, np.arange(n, dtype=np.int64))


def equal_share(per, s0, a, b, k):
    """the share of the source bytes p in [a, b), p >= 2^k, that equal the byte at p - 2^k (0.0 where there is no such p)"""
    a = max(a, 1 << k)
    if a >= b:
        return 0.0
    p = np.arange(a, b, dtype=np.int64)
    return float((at(per, s0, p) == at(per, s0, p - (1 << k))).mean())


def assert_distinct(per, s0, wins):
    """a condition on the INPUTS: inside the sampled windows fewer than 1 % of the bytes equal the byte 2^29, 2^31 or 2^32 in front of them, so
    that a position narrowed by one of these cannot give the right bytes by chance (random bytes: 1 / 256)"""
    for k in (29, 31, 32):
        for a, b in wins:
            share = equal_share(per, s0, a, b, k)
            assert share < 0.01, (k, a, b, share)


def windows(n, thresholds=(), seed=0, count=32, size=WINDOW):
    """the windows of a destination (or a source) of n bytes: its first and last `size` bytes, `size` bytes around every threshold inside it, and
    `count` seeded random ones -> [(a, b)], each inside [0, n), none empty"""
    out = [(0, min(n, size)), (max(0, n - size), n)]
    for t in thresholds:
        if 0 < t < n:
            out.append((max(0, t - size // 2), min(n, t + size // 2)))
    rnd = random.Random(seed)
    for _ in range(count):
        a = rnd.randrange(0, max(1, n - size))
        out.append((a, min(n, a + size)))
    return [w for w in dict.fromkeys(out) if w[0] < w[1]]


# ---- the ragged copy ----
def copy_window(per, s0, a, b):
    return at(per, s0, np.arange(a, b, dtype=np.int64))


# ---- unshuffle: out[p] = src[(p % w) m + p // w] for p < w m, out[p] = src[p] behind ----
def unshuffle_window(per, s0, n, w, a, b):
    m = n // w
    p = np.arange(a, b, dtype=np.int64)
    return at(per, s0, np.where(p < w * m, (p % w) * m + p // w, p))


# ---- undelta: element e is the sum of the elements 0 .. e, mod 2^(8 w) ----
def _element_period(per, s0, w):
    """the elements of w bytes are periodic too, with a period of len(per) ELEMENTS (w periods of bytes; w and an odd prime share no factor)
    -> (the running sums over one period of elements, its total), uint64, wrapping"""
    i = np.arange(len(per), dtype=np.int64) * w
    x = np.zeros(len(per), dtype=np.uint64)
    for t in range(w):
        x |= at(per, s0, i + t).astype(np.uint64) << np.uint64(8 * t)
    c = np.cumsum(x, dtype=np.uint64)
    return c, c[-1]


def undelta_window(per, s0, n, w, a, b):
    """the sum of e // P whole periods of elements and of a partial one, wrapped at the element's width; the len % w bytes behind stay"""
    assert len(per) % 2 == 1 and w in (1, 2, 4, 8)
    m = n // w
    out = at(per, s0, np.arange(a, b, dtype=np.int64)).copy()
    e0, e1 = a // w, min(m, (b + w - 1) // w)
    if e0 >= e1:
        return out
    c, total = _element_period(per, s0, w)
    e = np.arange(e0, e1, dtype=np.int64)
    with np.errstate(over="ignore"):
        v = (e // len(per)).astype(np.uint64) * total + c[e % len(per)]
    by = v.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :w].reshape(-1)   # bytes e0 w .. e1 w of the destination
    lo, hi = max(a, e0 * w), min(b, e1 * w)
    out[lo - a:hi - a] = by[lo - e0 * w:hi - e0 * w]
    return out


# ---- bit-unshuffle: blocks of `block` elements, a block's shuffled form being 8 w rows of c / 8 bytes ----
def bitunshuffle_window(per, s0, n, w, block, a, b):
    m = n // w
    p = np.arange(a, b, dtype=np.int64)
    if block == 0 or block >= m:
        o = np.zeros_like(p)
        c = np.full_like(p, m // 8 * 8)
    else:
        assert block % 8 == 0
        b0 = np.minimum(p // w // block, (m - 1) // block) * block   # the first element of the byte's block
        o = b0 * w
        c = np.where(m - b0 >= block, block, (m - b0) // 8 * 8)
    inside = p < o + c * w           # (behind a block's transposed elements, and behind the last whole element: copied)
    q = np.where(inside, p - o, 0)
    i, j = q // w, q % w
    r = np.maximum(c // 8, 1)
    v = np.zeros(len(p), dtype=np.uint8)
    for k in range(8):
        bit = (at(per, s0, np.where(inside, o + (8 * j + k) * r + i // 8, 0)) >> (i % 8).astype(np.uint8)) & 1
        v |= (bit << k).astype(np.uint8)
    return np.where(inside, v, at(per, s0, p))


# ---- bit-unpack: field i is the k bits from bit i k on ----
def fields(per, s0, k, e0, e1, flags=0):
    """the fields e0 .. e1 - 1 of k bits of the source as uint64, sign-extended to 64 bits with SIGNED; the positions in Python integers"""
    assert 1 <= k <= 64 and e0 <= e1
    if e0 == e1:
        return np.zeros(0, dtype=np.uint64)
    bit0, bit1 = e0 * k, e1 * k
    raw = at(per, s0, np.arange(bit0 // 8, (bit1 + 7) // 8, dtype=np.int64))
    bits = np.unpackbits(raw, bitorder="big" if flags & MSB_FIRST else "little")[bit0 % 8:bit0 % 8 + (e1 - e0) * k].reshape(e1 - e0, k).astype(np.uint64)
    place = np.arange(k, dtype=np.uint64)
    if flags & MSB_FIRST:
        place = np.uint64(k - 1) - place
    v = (bits << place).sum(axis=1, dtype=np.uint64)
    if flags & SIGNED and k < 64:
        s = np.uint64(1 << (k - 1))
        with np.errstate(over="ignore"):
            v = (v ^ s) - s
    return v


def _elements_window(v, e0, w, a, b):
    """the bytes [a, b) of a destination whose elements e0 .. are v"""
    by = v.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :w].reshape(-1)
    return by[a - e0 * w:b - e0 * w]


def bitunpack_window(per, s0, count, k, w, flags, a, b):
    assert 0 <= a <= b <= count * w
    e0, e1 = a // w, (b + w - 1) // w
    return _elements_window(fields(per, s0, k, e0, e1, flags), e0, w, a, b)


# ---- unvarint: a period whose last byte is a terminator, so that the elements are periodic as well ----
def varint_period(seed, size=P, overlong=(11, 12, 30)):
    """a period in which 7 of 8 bytes end a varint and the last byte does, with one varint of each of the lengths `overlong` in it"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 0x80, size=size, dtype=np.uint8)
    a[rng.random(size) < 1 / 8] |= 0x80
    for j, n in enumerate(overlong):
        lo = size // 7 * (j + 1)
        a[lo - 1] &= 0x7F
        a[lo:lo + n - 1] |= 0x80
        a[lo + n - 1] &= 0x7F
    a[-1] &= 0x7F
    a.setflags(write=False)
    return a


def _varint_elements(per, flags):
    """one period's elements as uint64, the offset behind each of them, and which are overlong"""
    assert per[-1] < 0x80
    ends = np.flatnonzero(per < 0x80)
    starts = np.concatenate(([0], ends[:-1] + 1))
    lens = ends - starts + 1
    v = np.zeros(len(ends), dtype=np.uint64)
    for j in range(10):
        has = lens > j
        g = (per[np.minimum(starts + j, len(per) - 1)] & 0x7F).astype(np.uint64)
        v |= np.where(has, g << np.uint64(7 * j), np.uint64(0))   # (the shift by 63 drops the tenth byte's bits above bit 0)
    if flags & ZIGZAG:
        v = (v >> np.uint64(1)) ^ (np.uint64(0) - (v & np.uint64(1)))
    over = lens > 10
    v[over] = 0
    return v, ends + 1, over


def unvarint_result(per, n):
    """(count, consumed, overlong) of the first n bytes of the periodic stream from byte 0 on"""
    _, behind, over = _varint_elements(per, 0)
    q, r = divmod(n, len(per))
    part = int(np.searchsorted(behind, r, side="right"))   # the varints that end inside the partial period
    return (q * len(behind) + part, q * len(per) + (int(behind[part - 1]) if part else 0), q * int(over.sum()) + int(over[:part].sum()))


def unvarint_length(per, count):
    """the smallest number of source bytes that hold `count` varints"""
    _, behind, _ = _varint_elements(per, 0)
    q, r = divmod(count, len(behind))
    return q * len(per) + (int(behind[r - 1]) if r else 0)


def unvarint_window(per, n, w, flags, cap, a, b):
    """bytes [a, b) of the destination of the first min(count, cap) elements of the segment of the stream's first n bytes"""
    count = unvarint_result(per, n)[0]
    assert 0 <= a <= b <= min(count, cap) * w
    v, _, _ = _varint_elements(per, flags)
    e0, e1 = a // w, (b + w - 1) // w
    return _elements_window(v[np.arange(e0, e1, dtype=np.int64) % len(v)], e0, w, a, b)


# ---- unrle and undict: a plan of runs ----
# a run: ("rle", count, value) or ("packed", count, per, s0) -- count a multiple of 8, the payload the count k / 8 bytes of that periodic stream
def rle_header(h):
    """a run's header: LEB128, the shortest form (at most 5 bytes)"""
    out = bytearray()
    while True:
        out.append((h & 0x7F) | (0x80 if h >> 7 else 0))
        h >>= 7
        if not h:
            assert len(out) <= 5
            return bytes(out)


def run_front(run, k):
    """what stands in front of a run's payload: the header, and an RLE run's value"""
    if run[0] == "rle":
        return rle_header(run[1] << 1) + int(run[2]).to_bytes((k + 7) // 8, "little")
    assert run[1] % 8 == 0 and run[1]
    return rle_header(run[1] // 8 << 1 | 1)


def run_bytes(run, k):
    return len(run_front(run, k)) + (run[1] * k // 8 if run[0] == "packed" else 0)


def rle_materialise(plan, k):
    """the segment's bytes: for plans whose packed runs are small"""
    out = bytearray()
    for run in plan:
        out += run_front(run, k)
        if run[0] == "packed":
            out += materialise(run[2], run[3], run[1] * k // 8).tobytes()
    return bytes(out)


def rle_result(plan, k):
    """(count, consumed, runs, status, bits) of a well-formed segment, whatever its capacity"""
    return (sum(r[1] for r in plan), sum(run_bytes(r, k) for r in plan), len(plan), 0, k)


def rle_elements(plan, k, e0, e1):
    """the elements e0 .. e1 - 1 as uint64, not truncated"""
    out = np.zeros(e1 - e0, dtype=np.uint64)
    start = 0
    for run in plan:
        lo, hi = max(e0, start), min(e1, start + run[1])
        if lo < hi:
            out[lo - e0:hi - e0] = np.uint64(run[2]) if run[0] == "rle" else fields(run[2], run[3], k, lo - start, hi - start) if k else 0
        start += run[1]
    assert e1 <= start
    return out


def rle_window(plan, k, w, cap, a, b):
    assert 0 <= a <= b <= min(rle_result(plan, k)[0], cap) * w
    e0, e1 = a // w, (b + w - 1) // w
    return _elements_window(rle_elements(plan, k, e0, e1), e0, w, a, b)


def _lookup(idx, table, entries):
    ok = idx < np.uint64(entries)
    v = np.zeros(len(idx), dtype=np.uint64)
    v[ok] = table[idx[ok].astype(np.int64)]
    return v, ok


def undict_window(plan, k, w, table, entries, cap, a, b):
    """table: the dictionary's entries as unsigned integers; an index at or above `entries` gives 0"""
    assert 0 <= a <= b <= min(rle_result(plan, k)[0], cap) * w
    e0, e1 = a // w, (b + w - 1) // w
    v, _ = _lookup(rle_elements(plan, k, e0, e1), np.asarray(table, dtype=np.uint64), entries)
    return _elements_window(v, e0, w, a, b)


def undict_result(plan, k, entries, cap):
    """unrle's five fields, and (bad, first_bad) of the first min(count, cap) elements.  An RLE run is bad as a whole or not at all; a packed
    run is looked at field by field only where k bits can name an entry that is not there"""
    bad, first, start = 0, NONE, 0
    for run in plan:
        take = max(0, min(run[1], cap - start))
        if take and run[0] == "rle" and run[2] >= entries:
            bad, first = bad + take, min(first, start)
        elif take and run[0] == "packed" and (1 << k) > entries:
            for lo in range(0, take, 1 << 20):
                miss = np.flatnonzero(fields(run[2], run[3], k, lo, min(take, lo + (1 << 20))) >= np.uint64(entries))
                if len(miss):
                    bad, first = bad + len(miss), min(first, start + lo + int(miss[0]))
        start += run[1]
    return rle_result(plan, k) + (bad, first)


# ---- undlba: a page of N strings of one length ----
def _leb(v):
    out = bytearray()
    while True:
        out.append((v & 0x7F) | (0x80 if v >> 7 else 0))
        v >>= 7
        if not v:
            return bytes(out)


def dlba_lengths(count, length, B=128, M=4):
    """the DELTA_BINARY_PACKED stream of `count` lengths that are all `length`: the header, and a block of min_delta 0 and M widths of 0 for
    every B deltas -- no payload"""
    assert count >= 1 and length >= 0
    blocks = (count - 1 + B - 1) // B
    return _leb(B) + _leb(M) + _leb(count) + _leb(length << 1) + (b"\x00" + b"\x00" * M) * blocks


def dlba_result(count, length, data_avail, cap, B=128, M=4):
    """(count, consumed, declared, blocks, status, block_values, miniblocks, data_status, bad, first_bad, bytes, data_avail)"""
    total = min(count, cap) * length
    return (count, len(dlba_lengths(count, length, B, M)), count, (count - 1 + B - 1) // B, 0, B, M, 0 if total <= data_avail else 1, 0, NONE,
            total, data_avail)


def dlba_offsets_window(count, length, cap, base, flags, a, b):
    """bytes [a, b) of the offsets: base + i length, truncated to the offsets' width; without offsets[0] with ENDS_ONLY"""
    w = 8 if flags & OFFSETS64 else 4
    first = 1 if flags & ENDS_ONLY else 0
    assert 0 <= a <= b <= (min(count, cap) + 1 - first) * w
    e0, e1 = a // w, (b + w - 1) // w
    v = [(base + (i + first) * length) & M64 for i in range(e0, e1)]
    return _elements_window(np.array(v, dtype=np.uint64), e0, w, a, b)


# ---- the digests: CRC(A + B) = CRC(A) x^(8 |B|) + CRC(B), by square and multiply on (crc, length) ----
def crc_join(kind, x, y):
    return (digest_ref.mulmod(kind, x[0], digest_ref.xpow(kind, 8 * y[1])) ^ y[0], x[1] + y[1])


def crc_repeat(kind, x, q):
    """(crc, length) of q copies of what x is the (crc, length) of"""
    out = (0, 0)
    while q:
        if q & 1:
            out = crc_join(kind, out, x)
        x = crc_join(kind, x, x)
        q >>= 1
    return out


def crc_one(kind, data):
    data = bytes(data)
    return zlib.crc32(data) & 0xFFFFFFFF if kind == digest_ref.CRC32 else digest_ref.crc32c(data)


def crc_periodic(kind, per, s0, n):
    """the digest of the n bytes of a segment: the CRC of one period, folded over n // P repeats, and of the remainder"""
    if n < len(per):
        return crc_one(kind, materialise(per, s0, n).tobytes())
    turned = np.roll(per, -(s0 % len(per)))
    q, r = divmod(n, len(per))
    whole = crc_repeat(kind, (crc_one(kind, turned), len(per)), q) if q else (0, 0)
    return crc_join(kind, whole, (crc_one(kind, turned[:r]), r))[0]
