"""The reference of the undba calls (include/brotli/batch.h): Parquet's DELTA_BYTE_ARRAY -- a DELTA_BINARY_PACKED stream of prefix lengths, one
of suffix lengths and the suffix bytes, directly behind one another -- back into an Arrow string column.  A plain serial decoder of the whole
contract on dbp_ref, an encoder from a list of byte strings (the longest common prefix, or any prefixes and suffix lengths a test wants), the
examples of batch.h pinned by hand, and what the tests without a device and the tests on the device share: the expected buffers of a table of
segments, and the tables themselves.
A result is (count_p, consumed_p, declared_p, blocks_p, status_p, block_values_p, miniblocks_p, data_status, count_s, consumed_s, declared_s,
blocks_s, status_s, block_values_s, miniblocks_s, bad_kind, first_bad, bytes, suffix_bytes, data_avail)."""
import random

import numpy as np

import dbp_ref
import dlba_ref

OFFSETS64, ENDS_ONLY, SKIP = 2, 4, 8
DATA_OK, DATA_SHORT, DATA_BAD, DATA_COUNTS_DIFFER = 0, 1, 2, 4
BAD_NONE, BAD_PREFIX_NEGATIVE, BAD_SUFFIX_NEGATIVE, BAD_PREFIX_LONG = 0, 1, 2, 3
NONE = (1 << 64) - 1          # first_bad where no element broke a rule; a segment's offset where it has no such destination
OK, BAD_HEADER, BAD_WIDTH, TRUNCATED = dbp_ref.OK, dbp_ref.BAD_HEADER, dbp_ref.BAD_WIDTH, dbp_ref.TRUNCATED
R_STATUS, R_COUNT_P, R_COUNT_S, R_KIND, R_FIRST_BAD, R_BYTES, R_SUFFIX, R_AVAIL = 7, 0, 8, 15, 16, 17, 18, 19   # places in a result

sentinel, offsets_bytes, offsets_array, first_difference = dlba_ref.sentinel, dlba_ref.offsets_bytes, dlba_ref.offsets_array, dlba_ref.first_difference

_H = bytes.fromhex
_ONE = (1, 5, 1, 0, OK, 128, 4)
_TWO = (2, 10, 2, 1, OK, 128, 4)
# pinned by hand: (bytes, offsets on a base of 0, the data delivered to a capacity that holds it, the result)
PINNED = [
    (_H("80 01 04 01 00  80 01 04 01 06  78 79 7a"), [0, 3], b"xyz", _ONE + (DATA_OK,) + _ONE + (BAD_NONE, NONE, 3, 3, 3)),
    (_H("80 01 04 02 00 04 00 00 00 00  80 01 04 02 06 03 00 00 00 00  61 62 63 64"), [0, 3, 6], b"abcabd", _TWO + (DATA_OK,) + _TWO + (BAD_NONE, NONE, 6, 4, 4)),
    (_H("80 01 04 02 00 08 00 00 00 00  80 01 04 02 06 03 00 00 00 00  61 62 63 64"), [0, 3, 3], b"abc",
     _TWO + (DATA_BAD,) + _TWO + (BAD_PREFIX_LONG, 1, 3, 3, 4)),
    (_H("80 01 04 02 00 04 00 00 00 00  80 01 04 02 06 03 00 00 00 00  61 62 63"), [0, 3, 6], b"abcab\0", _TWO + (DATA_SHORT,) + _TWO + (BAD_NONE, NONE, 6, 4, 3)),
    (_H("80 01 04 02 00 01 00 00 00 00  80 01 04 02 02 01 00 00 00 00  61"), [0, 1, 1], b"a", _TWO + (DATA_BAD,) + _TWO + (BAD_PREFIX_NEGATIVE, 1, 1, 1, 1)),
    (_H("80 01 04 01 02  80 01 04 01 02  61"), [0, 0], b"", _ONE + (DATA_BAD,) + _ONE + (BAD_PREFIX_LONG, 0, 0, 0, 1)),
    (_H("80 01 04 00 00  80 01 04 00 00"), [0], b"", (0, 5, 0, 0, OK, 128, 4, DATA_OK, 0, 5, 0, 0, OK, 128, 4, BAD_NONE, NONE, 0, 0, 0)),
]


# ---- the encoder ----
def common_prefix(a, b):
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def encode(strings, prefixes=None, suffix_lengths=None, p_knobs=None, s_knobs=None, **knobs):
    """byte strings -> the page body.  prefixes None: the longest common prefix with the string in front; a list: any legal shorter prefix
    (the suffix is the rest of the string), or anything at all (an integer that is no legal prefix makes a bad page: the suffix is then the
    string from min(max(p, 0), len) on).  suffix_lengths: what is written in place of the suffixes' lengths.  knobs: dbp_ref.encode's for
    both streams (B, M, ..); p_knobs and s_knobs: for one of them on top."""
    strings = [bytes(v) for v in strings]
    if prefixes is None:
        prefixes = [0] * min(len(strings), 1) + [common_prefix(strings[i - 1], strings[i]) for i in range(1, len(strings))]
    prefixes = list(prefixes)
    suffixes = [v[min(max(p & 0xFFFFFFFF if p >= 1 << 32 else p, 0), len(v)):] for v, p in zip(strings, prefixes)]
    lens = [len(x) for x in suffixes] if suffix_lengths is None else list(suffix_lengths)
    return dbp_ref.encode(prefixes, **dict(knobs, **(p_knobs or {}))) + dbp_ref.encode(lens, **dict(knobs, **(s_knobs or {}))) + b"".join(suffixes)


# ---- one segment ----
def int32(v):
    low = int(v) & 0xFFFFFFFF
    return low - (1 << 32) if low >> 31 else low


def column(seg, cap=None, offset_base=0, data_cap=None):
    """-> ([offsets[0 .. m]] as unbounded ints, the bytes delivered, the result), element after element; cap None: all elements; cap 0:
    nothing but the walks; data_cap None: everything.  With a data_cap no more than data_cap bytes of any element are ever made: a page may
    declare elements of 2^31 bytes over a few bytes of source"""
    seg = bytes(seg)
    pv, rp = dbp_ref.decode(seg, 8, cap)
    sv, rs = dbp_ref.decode(seg[rp[1]:], 8, cap)
    at = rp[1] + rs[1]
    avail = len(seg) - at
    differ = DATA_COUNTS_DIFFER if rp[0] != rs[0] and rp[4] == OK and rs[4] == OK else 0
    if cap == 0:
        return [], b"", rp + (DATA_OK | differ,) + rs + (BAD_NONE, NONE, 0, 0, avail)
    m = min(len(pv), len(sv))
    offsets, data, first_bad, kind, q, d_prev, prev, total = [offset_base], bytearray(), NONE, BAD_NONE, 0, 0, b"", 0
    for i in range(m):
        p, s = int32(pv[i]), int32(sv[i])
        if first_bad == NONE:
            k = BAD_PREFIX_NEGATIVE if p < 0 else BAD_SUFFIX_NEGATIVE if s < 0 else BAD_PREFIX_LONG if p > d_prev else BAD_NONE
            if k != BAD_NONE:
                first_bad, kind = i, k
        if first_bad == NONE:
            prev = prev[:p]   # (prev holds min(its length, data_cap) bytes: all that a byte below data_cap can come from)
            need = s if data_cap is None else max(0, min(s, data_cap - len(prev)))
            suffix = seg[at + q:at + q + need] if at + q < len(seg) else b""
            prev = prev + suffix + bytes(need - len(suffix))   # (a suffix byte behind the segment's end reads as 0)
            data += prev if data_cap is None else prev[:max(0, data_cap - len(data))]
            q += s
            d_prev = p + s
            total += d_prev
        offsets.append(offset_base + total)
    status = (DATA_SHORT if q > avail else 0) | (DATA_BAD if first_bad != NONE else 0) | differ
    return offsets, bytes(data), rp + (status,) + rs + (kind, first_bad, total, q, avail)


def expected(src, segs, offsets_size, data_size):
    """-> (the offsets buffer, the data buffer, [the results]) behind a call over sentinel() buffers"""
    want_o, want_d, results = bytearray(sentinel(offsets_size)), bytearray(sentinel(data_size, 7)), []
    cache = {}
    for s, l, o_at, d_at, data_cap, cap, base, flags in segs:
        key = (s, l, cap, base, data_cap if d_at != NONE else 0)
        if key not in cache:
            cache[key] = column(src[s:s + l], cap, base, key[4])
        offsets, data, res = cache[key]
        results.append(res)
        if cap and o_at != NONE:
            ob = offsets_array(offsets, flags)
            assert o_at + len(ob) <= offsets_size, (o_at, len(ob), offsets_size)
            want_o[o_at:o_at + len(ob)] = ob
        if cap and d_at != NONE:
            assert d_at + len(data) <= data_size, (d_at, len(data), data_size)
            want_d[d_at:d_at + len(data)] = data
    return bytes(want_o), bytes(want_d), results


def counts(body):
    """the values of the two streams, whatever their status is"""
    rp = dbp_ref.decode(body, 8, 0)[1]
    return rp[0], dbp_ref.decode(body[rp[1]:], 8, 0)[1][0]


def layout(rnd, bodies, flags=0, caps=None, data_caps=None, base=0, gap=(0, 1, 5), o_at=3, d_at=5):
    """segments one behind the other, each with room for all it delivers -> (src, segs, offsets_size, data_size)"""
    src, segs = bytearray(b"\x5a"), []
    for j, body in enumerate(bodies):
        cap = caps[j] if caps is not None else max(counts(body))
        offsets, data, _ = column(body, cap, base, None if data_caps is None else data_caps[j]) if cap else ([], b"", None)
        data_cap = data_caps[j] if data_caps is not None else len(data) + 3
        s_at = len(src) + rnd.choice(gap)
        src += b"\xc3" * (s_at - len(src)) + body
        segs.append((s_at, len(body), o_at, d_at, data_cap, cap, base, flags))
        o_at += len(offsets_array(offsets, flags)) + rnd.choice(gap)
        d_at += min(len(data), data_cap) + rnd.choice(gap)
    return bytes(src) + b"\x3c" * 16, segs, o_at + 40, d_at + 40


def huge_page(repeats):
    """a legal page whose elements DECLARE 2^31 - 1 bytes and more over ten bytes of source -> (the body, its elements): the suffix bytes behind
    the source's end read as 0, the data is SHORT, and what a call does must follow what it stores, never what is declared"""
    big = (1 << 31) - 1
    prefixes = [0, big, big, 5] + [big] * repeats + [7]
    suffixes = [big, big, 3, big] + [0] * repeats + [2]
    return dbp_ref.encode(prefixes) + dbp_ref.encode(suffixes) + b"0123456789", len(prefixes)


def sorted_strings(rnd, count, stem=b"", tail=(0, 1, 2, 5, 12), alphabet=b"abc"):
    """`count` sorted byte strings behind a common stem: neighbours share long prefixes, and repeats are among them"""
    return sorted(stem + bytes(rnd.choice(alphabet) for _ in range(rnd.choice(tail))) for _ in range(count))


def short_table(count=3000, seed=29):
    """`count` short segments, empty ones among them, of mixed flags, capacities, data capacities, block shapes and endings -- cut streams,
    every undbp stop in either stream with bytes behind it, each of the three bad rules with upper bits set, short and left-over data,
    differing counts -> (src, segs, offsets_size, data_size)"""
    rnd = random.Random(seed)
    stops = dbp_ref.stops()
    src, segs, o_at, d_at = bytearray(b"\x5a"), [], 1, 2
    for i in range(count):
        flags = (OFFSETS64 if rnd.random() < 0.3 else 0) | (ENDS_ONLY if rnd.random() < 0.3 else 0)
        kind = i % 16
        if kind == 0:
            body = b""
        else:
            B, M = rnd.choice([(128, 4), (128, 1), (256, 4), (256, 8)])
            strings = sorted_strings(rnd, rnd.randrange(0, 200), rnd.choice([b"", b"k/", b"prefix-of-some-length/"])) if rnd.random() < 0.8 else \
                dlba_ref.random_strings(rnd, rnd.randrange(0, 200), [0, 1, 2, 3])
            prefixes = [0] + [common_prefix(strings[x - 1], strings[x]) for x in range(1, len(strings))]
            if rnd.random() < 0.3:
                prefixes = [rnd.randrange(0, p + 1) for p in prefixes]   # (any shorter prefix is legal)
            lens = [len(v) - p for v, p in zip(strings, prefixes)]
            up = rnd.choice([0, 1 << 32, 5 << 40])   # (upper bits are not looked at)
            if kind == 1 and strings:
                prefixes[rnd.randrange(len(strings))] = -rnd.randrange(1, 1000)
            elif kind == 2 and strings:
                lens[rnd.randrange(len(strings))] = -rnd.randrange(1, 1000) + up
            elif kind == 3 and strings:
                x = rnd.randrange(len(strings))
                prefixes[x] = (len(strings[x - 1]) if x else 0) + rnd.randrange(1, 4) + up
            elif kind == 4 and strings:
                lens[rnd.randrange(len(strings))] += rnd.randrange(1, 50)   # (the data is short)
            elif kind == 5 and strings:
                x = rnd.randrange(len(strings))
                prefixes[x] += up
                lens[x] += up
            body = encode(strings, prefixes, lens, B=B, M=M)
            if kind == 6:
                body = body[:rnd.randrange(len(body))]
            elif kind == 7:
                body += rnd.randbytes(rnd.randrange(1, 9))   # (left-over bytes)
            elif kind in (8, 9):   # a stop behind whole blocks in P or in S, and bytes behind it
                full = sorted_strings(rnd, B + 1)
                more = rnd.choice(stops)
                pre = [0] + [common_prefix(full[x - 1], full[x]) for x in range(1, len(full))]
                suf = [len(v) - p for v, p in zip(full, pre)]
                tail = b"".join(v[p:] for v, p in zip(full, pre))
                if kind == 8:
                    body = dbp_ref.encode(pre, B, M, declared=B + 1 + 40) + more[1] + dbp_ref.encode(suf, B, M) + tail
                else:
                    body = dbp_ref.encode(pre, B, M) + dbp_ref.encode(suf, B, M, declared=B + 1 + 40) + more[1] + tail
            elif kind == 10:   # a header that is none, in P
                body = dbp_ref.varint(rnd.choice([0, 64, 192, 65664])) + body[2:]
            elif kind == 11 and strings:   # ... and in S
                at = dbp_ref.decode(body, 8, 0)[1][1]
                body = body[:at] + dbp_ref.varint(rnd.choice([0, 64, 192, 65664])) + body[at + 2:]
            elif kind == 12 and strings:   # the streams' counts differ
                extra = rnd.randrange(1, 40)
                body = dbp_ref.encode(prefixes + [0] * (extra if i & 16 else 0), B, M) + dbp_ref.encode(lens + [1] * (0 if i & 16 else extra), B, M) + \
                    b"".join(v[p:] for v, p in zip(strings, prefixes)) + b"z" * extra
        count_ = max(counts(body))
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
