"""The numpy reference of the unvarint calls (include/brotli/batch.h): LEB128 varints back into elements, vectorised over the ends, and a plain
serial decoder to check it against.  A byte with bit 7 clear ends a varint; a varint of more than ten bytes is overlong and its element is 0; bits
at and above bit 64 are dropped; zigzag is (v >> 1) ^ -(v & 1) in front of the truncation to the element's width."""
import random

import numpy as np

ZIGZAG = 1
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}

# the examples of batch.h: (source bytes, width, flags, elements as unsigned integers of the width, (count, consumed, overlong))
EXAMPLES = [
    (bytes.fromhex("9601ac02e58e26"), 4, 0, [150, 300, 624485], (3, 7, 0)),
    (b"\xff" * 9 + b"\x01", 8, 0, [(1 << 64) - 1], (1, 10, 0)),
    (b"\xff" * 9 + b"\x7f", 8, 0, [(1 << 64) - 1], (1, 10, 0)),
    (bytes.fromhex("01020304feffffff0f"), 4, ZIGZAG, [0xFFFFFFFF, 1, 0xFFFFFFFE, 2, 2147483647], (5, 9, 0)),
    (b"\x80" * 10 + bytes.fromhex("01058080"), 4, 0, [0, 5], (2, 12, 1)),
]


def unvarint(data, width=8, flags=0):
    """-> (the elements as a numpy array of the width's unsigned dtype, (count, consumed, overlong)); every varint that ends in `data`"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    ends = np.flatnonzero(a < 0x80)
    m = len(ends)
    if m == 0:
        return np.zeros(0, dtype=DTYPES[width]), (0, 0, 0)
    out = np.empty(m, dtype=DTYPES[width])
    overlong = 0
    groups = min(10, 8 * width // 7 + 1)   # the bytes of a varint that reach the element's 8 w bits (and, with zigzag, the bit above them)
    for lo in range(0, m, 1 << 22):        # (a few million ends at a time: a segment of a hundred megabytes stays in memory)
        e = ends[lo:lo + (1 << 22)]
        starts = np.concatenate(([0 if lo == 0 else ends[lo - 1] + 1], e[:-1] + 1))
        lens = e - starts + 1
        vals = np.zeros(len(e), dtype=np.uint64)
        for j in range(groups):   # byte j of every varint that has one
            has = lens > j
            if not has.any():
                break
            group = (a[np.minimum(starts + j, len(a) - 1)] & 0x7F).astype(np.uint64)
            vals |= np.where(has, group << np.uint64(7 * j), np.uint64(0))   # (a shift of 63 drops the tenth byte's bits above bit 0)
        if flags & ZIGZAG:
            vals = (vals >> np.uint64(1)) ^ (np.uint64(0) - (vals & np.uint64(1)))
        over = lens > 10
        vals[over] = 0
        overlong += int(over.sum())
        out[lo:lo + len(e)] = vals.astype(DTYPES[width])
    return out, (m, int(ends[-1]) + 1, overlong)


def unvarint_serial(data, width=8, flags=0):
    """the same, one byte after the other in plain Python -> ([elements as ints], (count, consumed, overlong))"""
    out, count, consumed, overlong = [], 0, 0, 0
    v, n = 0, 0
    for p, b in enumerate(bytes(data)):
        if n < 10:
            v |= (b & 0x7F) << (7 * n)
        n += 1
        if b < 0x80:
            v &= (1 << 64) - 1
            if flags & ZIGZAG:
                v = (v >> 1) ^ (((1 << 64) - (v & 1)) & ((1 << 64) - 1))
            if n > 10:
                v, overlong = 0, overlong + 1
            out.append(v & ((1 << (8 * width)) - 1))
            count, consumed = count + 1, p + 1
            v, n = 0, 0
    return out, (count, consumed, overlong)


def varint(values, zigzag=False):
    """the encoder, for tests that need a stream of given values: 64-bit values (signed ones with zigzag) -> bytes, the shortest form"""
    out = bytearray()
    for x in values:
        x = int(x)
        x = ((x << 1) ^ (x >> 63)) & ((1 << 64) - 1) if zigzag else x & ((1 << 64) - 1)
        while x >= 0x80:
            out.append(0x80 | (x & 0x7F))
            x >>= 7
        out.append(x)
    return bytes(out)


def elements_bytes(data, width, flags, cap):
    """what a segment's destination holds behind the call: the first min(count, cap) elements, little-endian -> (bytes, result)"""
    vals, res = unvarint(data, width, flags)
    return vals[:cap].astype("<u%d" % width).tobytes(), res


# ---- the cases that the tests without a device and the tests on the device share ----
def boundary_segments(boundary, seg_len, seed):
    """varints of every length 1 .. 12 whose last byte lies at every offset -12 .. +12 from `boundary`, each in a segment of seg_len bytes of
    one-byte varints that begins at a multiple of seg_len of the source (so `boundary` is an address boundary where seg_len and the source's
    address are multiples of it; what would begin in front of its segment is left out) -> (source, [(source offset, length)], overlong ones)"""
    rng = np.random.default_rng(seed)
    cases = [(L, off) for L in range(1, 13) for off in range(-12, 13) if boundary + off - L + 1 >= 0]
    src = rng.integers(0, 0x80, size=seg_len * len(cases), dtype=np.uint8)
    for i, (L, off) in enumerate(cases):
        end = i * seg_len + boundary + off
        assert end - L + 1 >= i * seg_len and end < (i + 1) * seg_len
        src[end - L + 1:end] = rng.integers(0x80, 0x100, size=L - 1, dtype=np.uint8)
        src[end] = rng.integers(0, 0x80)
        if L == 10:
            src[end] |= 0x7E * (i & 1)   # a tenth byte with high bits set: dropped
    return src.tobytes(), [(i * seg_len, seg_len) for i in range(len(cases))], sum(1 for L, _ in cases if L > 10)


def short_table(data_len, count=3000, seed=7):
    """`count` short segments of 0 .. 300 bytes, mixed widths, flags and capacities, empty ones among them, over a source of data_len bytes (the
    sources may overlap each other: they are only read) -> ([(source offset, source length, destination offset, cap, width, flags)], the
    destination's size)"""
    rnd = random.Random(seed)
    lens = [rnd.randrange(0, 301) if rnd.random() < 0.9 else 0 for _ in range(count)]
    segs, s_at, d_at = [], 1, 7
    for l in lens:
        s_at = (s_at + rnd.randrange(0, 40)) % (data_len - 400)
        w = rnd.choice([1, 2, 4, 8])
        cap = rnd.choice([l, l, l, 0, 3])
        segs.append((s_at, l, d_at, cap, w, rnd.randrange(2)))
        d_at += min(cap, l) * w + rnd.choice([0, 0, 1, 5])
    return segs, d_at + 64
