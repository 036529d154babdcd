"""The reference of the undlba calls (include/brotli/batch.h): Parquet's DELTA_LENGTH_BYTE_ARRAY -- a DELTA_BINARY_PACKED stream of lengths and,
directly behind it, the values' bytes -- back into an Arrow string column.  An encoder from a list of byte strings over dbp_ref.encode with its
knobs, a serial decoder of the whole contract, a numpy one that is checked against it, the five examples of batch.h pinned by hand, and what
the tests without a device and the tests on the device share: the expected buffers of a table of segments, and the tables themselves.
A result is (count, consumed, declared, blocks, status, block_values, miniblocks, data_status, bad, first_bad, bytes, data_avail)."""
import random

import numpy as np

import dbp_ref

OFFSETS64, ENDS_ONLY, SKIP = 2, 4, 8
DATA_OK, DATA_SHORT = 0, 1
NONE = (1 << 64) - 1          # first_bad where no length was negative; a segment's offset where it has no such destination
OK, BAD_HEADER, BAD_WIDTH, TRUNCATED = dbp_ref.OK, dbp_ref.BAD_HEADER, dbp_ref.BAD_WIDTH, dbp_ref.TRUNCATED
M64 = (1 << 64) - 1

# pinned by hand: (bytes, offsets on a base of 0, the data delivered to a capacity that holds it, the result)
PINNED = [
    (bytes.fromhex("80 01 04 04 00 02 00 00 00 00 61 62 62 63 63 63"), [0, 0, 1, 3, 6], b"abbccc", (4, 10, 4, 1, OK, 128, 4, DATA_OK, 0, NONE, 6, 6)),
    (bytes.fromhex("80 01 04 01 06 78 79 7a"), [0, 3], b"xyz", (1, 5, 1, 0, OK, 128, 4, DATA_OK, 0, NONE, 3, 3)),
    (bytes.fromhex("80 01 04 01 01 61 62"), [0, 0], b"", (1, 5, 1, 0, OK, 128, 4, DATA_OK, 1, 0, 0, 2)),
    (bytes.fromhex("80 01 04 01 0a 61 62"), [0, 5], b"ab", (1, 5, 1, 0, OK, 128, 4, DATA_SHORT, 0, NONE, 5, 2)),
    (bytes.fromhex("80 01 04 00 00"), [0], b"", (0, 5, 0, 0, OK, 128, 4, DATA_OK, 0, NONE, 0, 0)),
]


# ---- the encoder ----
def encode(values, lengths=None, **knobs):
    """byte strings -> the page body; lengths: what is written in place of their lengths (any integers: negative and oversized ones are how a
    test makes a bad page); knobs: dbp_ref.encode's (B, M, widen, vlen, junk, cut, declared, mins)"""
    values = [bytes(v) for v in values]
    return dbp_ref.encode([len(v) for v in values] if lengths is None else list(lengths), **knobs) + b"".join(values)


# ---- one segment ----
def length_of(v):
    """a 64-bit value -> (its length, whether it is bad): the low 32 bits as a signed int32, a negative one empty"""
    low = v & 0xFFFFFFFF
    return (0, 1) if low >> 31 else (low, 0)


def column_serial(seg, cap=None, offset_base=0, data_cap=None):
    """-> ([offsets[0 .. m]] as unbounded ints, the bytes delivered, the result), element after element; cap None: all elements; cap 0:
    nothing but the walk; data_cap None: as much as there is"""
    seg = bytes(seg)
    vals, res = dbp_ref.decode_serial(seg, 8, cap)
    consumed = res[1]
    avail = len(seg) - consumed
    if cap == 0:
        return [], b"", res + (DATA_OK, 0, NONE, 0, avail)
    offsets, bad, first_bad = [offset_base], 0, NONE
    for e, v in enumerate(vals):
        n, b = length_of(v)
        if b:
            bad += 1
            first_bad = min(first_bad, e)
        offsets.append(offsets[-1] + n)
    total = offsets[-1] - offset_base
    keep = min(total, avail) if data_cap is None else min(total, avail, data_cap)
    return offsets, seg[consumed:consumed + keep], res + (DATA_OK if total <= avail else DATA_SHORT, bad, first_bad, total, avail)


def column(seg, cap=None, offset_base=0, data_cap=None):
    """the same with numpy where the lengths are summed up; offsets as a numpy array of Python ints is avoided: -> (offsets as a list, data,
    result)"""
    seg = bytes(seg)
    vals, res = dbp_ref.decode(seg, 8, cap)
    consumed = res[1]
    avail = len(seg) - consumed
    if cap == 0:
        return [], b"", res + (DATA_OK, 0, NONE, 0, avail)
    low = (vals & np.uint64(0xFFFFFFFF)).astype(np.int64)
    neg = low >= (1 << 31)
    lens = np.where(neg, 0, low)
    ends = np.cumsum(lens, dtype=np.int64)   # (2^56 elements of 2^31 bytes do not fit a test)
    total = int(ends[-1]) if len(ends) else 0
    bad = int(neg.sum())
    first_bad = int(np.argmax(neg)) if bad else NONE
    keep = min(total, avail) if data_cap is None else min(total, avail, data_cap)
    return [offset_base] + [offset_base + int(x) for x in ends], seg[consumed:consumed + keep], res + (DATA_OK if total <= avail else DATA_SHORT, bad, first_bad, total, avail)


def offsets_bytes(offsets, flags):
    """the offsets as the call stores them: truncated to 4 bytes, or 8 with OFFSETS64; without offsets[0] with ENDS_ONLY"""
    w = 8 if flags & OFFSETS64 else 4
    return b"".join((o & ((1 << 8 * w) - 1)).to_bytes(w, "little") for o in (offsets[1:] if flags & ENDS_ONLY else offsets))


def offsets_array(offsets, flags):
    """... and as numpy: faster for a long column"""
    a = np.array(offsets[1:] if flags & ENDS_ONLY else offsets, dtype=np.uint64)
    return (a if flags & OFFSETS64 else a.astype(np.uint32)).astype("<u8" if flags & OFFSETS64 else "<u4").tobytes()


# ---- a table of segments, as the host hook takes it ----
# a segment: (source offset, source length, offsets offset or NONE, data offset or NONE, data capacity, capacity, offset base, flags)
def sentinel(size, salt=0):
    return ((np.arange(size, dtype=np.uint64) % 251 + 3 + salt) % 256).astype(np.uint8).tobytes()


def expected(src, segs, offsets_size, data_size):
    """-> (the offsets buffer, the data buffer, [the results]) behind a call over sentinel() buffers"""
    want_o, want_d, results = bytearray(sentinel(offsets_size)), bytearray(sentinel(data_size, 7)), []
    for s, l, o_at, d_at, data_cap, cap, base, flags in segs:
        offsets, data, res = column(src[s:s + l], cap, base, data_cap if d_at != NONE else 0)
        results.append(res)
        if cap and o_at != NONE:
            ob = offsets_array(offsets, flags)
            assert o_at + len(ob) <= offsets_size, (o_at, len(ob), offsets_size)
            want_o[o_at:o_at + len(ob)] = ob
        if cap and d_at != NONE:
            assert d_at + len(data) <= data_size, (d_at, len(data), data_size)
            want_d[d_at:d_at + len(data)] = data
    return bytes(want_o), bytes(want_d), results


def first_difference(got, want):
    return next((i, got[i], want[i]) for i in range(min(len(got), len(want))) if got[i] != want[i]) if got != want else None


def random_strings(rnd, count, lengths):
    """`count` byte strings whose lengths are drawn from `lengths`, of seeded bytes"""
    return [rnd.randbytes(rnd.choice(lengths)) for _ in range(count)]


def layout(rnd, bodies, flags=0, caps=None, data_caps=None, base=0, gap=(0, 1, 5), o_at=3, d_at=5):
    """segments one behind the other, each with room for all it delivers -> (src, segs, offsets_size, data_size)"""
    src, segs = bytearray(b"\x5a"), []
    for j, body in enumerate(bodies):
        cap = caps[j] if caps is not None else dbp_ref.decode(body, 8, 0)[1][0]
        offsets, data, _ = column(body, cap, base) if cap else ([], b"", None)
        data_cap = data_caps[j] if data_caps is not None else len(data) + 3
        s_at = len(src) + rnd.choice(gap)
        src += b"\xc3" * (s_at - len(src)) + body
        segs.append((s_at, len(body), o_at, d_at, data_cap, cap, base, flags))
        o_at += len(offsets_array(offsets, flags)) + rnd.choice(gap)
        d_at += min(len(data), data_cap) + rnd.choice(gap)
    return bytes(src) + b"\x3c" * 16, segs, o_at + 40, d_at + 40


def short_table(count=3000, seed=23):
    """`count` short segments, empty ones among them, of mixed flags, capacities, data capacities, block shapes and endings -- cut streams,
    every undbp stop with bytes behind it, negative and oversized lengths, left-over bytes -> (src, segs, offsets_size, data_size)"""
    rnd = random.Random(seed)
    stops = dbp_ref.stops()
    src, segs, o_at, d_at = bytearray(b"\x5a"), [], 1, 2
    for i in range(count):
        flags = (OFFSETS64 if rnd.random() < 0.3 else 0) | (ENDS_ONLY if rnd.random() < 0.3 else 0)
        kind = i % 12
        if kind == 0:
            body = b""
        else:
            B, M = rnd.choice([(128, 4), (128, 1), (256, 4), (256, 8)])
            strings = random_strings(rnd, rnd.randrange(0, 200), rnd.choice([[0], [1], [0, 1, 2, 3], [5, 16, 17], [0, 40]]))
            lengths = [len(s) for s in strings]
            if kind == 1 and lengths:
                lengths[rnd.randrange(len(lengths))] = -rnd.randrange(1, 1000)
            elif kind == 2 and lengths:
                lengths[rnd.randrange(len(lengths))] += rnd.randrange(1, 50)   # (the data is short)
            elif kind == 3 and lengths:
                lengths[rnd.randrange(len(lengths))] += 1 << 32   # (a length's upper bits are not looked at)
            body = encode(strings, lengths, B=B, M=M)
            if kind == 4:
                body = body[:rnd.randrange(len(body))]
            elif kind == 5:
                body += rnd.randbytes(rnd.randrange(1, 9))   # (left-over bytes)
            elif kind == 6:   # a stop behind whole blocks, and bytes behind it
                full = random_strings(rnd, B + 1, [0, 1, 2])
                more = rnd.choice(stops)
                body = dbp_ref.encode([len(s) for s in full], B, M, declared=B + 1 + 40) + more[1] + b"".join(full)
            elif kind == 7:   # a header that is none
                body = dbp_ref.varint(rnd.choice([0, 64, 192, 65664])) + body[2:]
        count_ = dbp_ref.decode(body, 8, 0)[1][0]
        cap = rnd.choice([count_, count_, count_ + 5, count_ // 2, 0, 3])
        offsets, data, _ = column(body, cap) if cap else ([], b"", None)
        data_cap = rnd.choice([len(data), len(data) + 9, len(data) // 2, 0])
        has_o, has_d = rnd.random() < 0.9, rnd.random() < 0.9
        s_at = len(src) + rnd.randrange(0, 4)
        src += b"\xc3" * (s_at - len(src)) + body
        segs.append((s_at, len(body), o_at if has_o else NONE, d_at if has_d else NONE, data_cap if has_d else 0, cap, rnd.choice([0, 0, 1000, (1 << 32) - 5]), flags))
        o_at += (len(offsets_array(offsets, flags)) if has_o else 0) + rnd.choice([0, 0, 1, 5])
        d_at += (min(len(data), data_cap) if has_d else 0) + rnd.choice([0, 0, 1, 5])
    return bytes(src) + b"\x3c" * 16, segs, o_at + 64, d_at + 64
