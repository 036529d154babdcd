"""The reference of the undict-bytes calls (include/brotli/batch.h): dictionary-index runs and a dictionary of PLAIN byte arrays back into an Arrow
string column.  The indices are rle_ref's; the dictionary is parsed serially here, with every cut rule of the contract, and the take is plain
Python / numpy.  Also what the tests without a device and the tests on the device share: the pinned vectors, the expected buffers of a table of
segments, and the tables themselves."""
import random

import numpy as np

import rle_ref

WIDTH_BYTE, OFFSETS64, ENDS_ONLY, SKIP = 1, 2, 4, 8
ALL = (1 << 64) - 1
NONE = (1 << 64) - 1          # first_bad where no element was bad; a segment's offset where it has no such destination
DICT_OK, DICT_CUT = 0, 1
OK, BAD_HEADER, ZERO_RUN, TRUNCATED, BAD_WIDTH = rle_ref.OK, rle_ref.BAD_HEADER, rle_ref.ZERO_RUN, rle_ref.TRUNCATED, rle_ref.BAD_WIDTH


# ---- the dictionary ----
def dictionary_bytes(entries):
    """PLAIN byte arrays: per entry a 4-byte little-endian length, then the bytes"""
    return b"".join(len(e).to_bytes(4, "little") + bytes(e) for e in entries)


def parse_dictionary(d, bound=ALL):
    """-> ([the entries], the bytes they take, DICT_OK or DICT_CUT): the dictionary ends at `bound` entries, at its last byte exactly, or at the
    first entry whose 4 length bytes or value bytes the end cuts"""
    d = bytes(d)
    entries, pos = [], 0
    while len(entries) < bound and pos < len(d):
        if len(d) - pos < 4:
            return entries, pos, DICT_CUT
        n = int.from_bytes(d[pos:pos + 4], "little")
        if n > len(d) - pos - 4:
            return entries, pos, DICT_CUT
        entries.append(d[pos + 4:pos + 4 + n])
        pos += 4 + n
    return entries, pos, DICT_OK


# ---- one segment ----
def column(data, k, flags, dictionary, bound=ALL, cap=None, offset_base=0):
    """-> ([offsets[0 .. m]] as unbounded ints, the elements' bytes together, the result's tuple (count, consumed, runs, status, bits, bad,
    first_bad, bytes, dict_entries, dict_consumed, dict_status)); cap None: all elements; cap 0: nothing of the dictionary is looked at"""
    idx, res = rle_ref.decode(data, k, 8, flags & WIDTH_BYTE, cap)
    if cap == 0:
        return [], b"", res + (0, NONE, 0, 0, 0, 0)
    entries, consumed, status = parse_dictionary(dictionary, bound)
    D = len(entries)
    idx = [int(v) for v in idx]
    bad = [e for e, v in enumerate(idx) if v >= D]
    parts = [entries[v] if v < D else b"" for v in idx]
    offsets = [offset_base]
    for p in parts:
        offsets.append(offsets[-1] + len(p))
    return offsets, b"".join(parts), res + (len(bad), bad[0] if bad else NONE, offsets[-1] - offset_base, D, consumed, status)


def offsets_bytes(offsets, flags):
    """the offsets as the call stores them: truncated to 4 bytes, or 8 with OFFSETS64; without offsets[0] with ENDS_ONLY"""
    w = 8 if flags & OFFSETS64 else 4
    return b"".join((o & ((1 << 8 * w) - 1)).to_bytes(w, "little") for o in (offsets[1:] if flags & ENDS_ONLY else offsets))


# pinned by hand from the format text: (k, flags, runs, dictionary, bound, (the elements, bad, first_bad, bytes, D, dict_status))
EIGHT = [b"", b"a", b"bc", b"def", b"ghij", b"klmno", b"pqrstu", b"vwxyz01"]
PINNED = [
    (3, 0, bytes.fromhex("0388C6FA"), dictionary_bytes(EIGHT), ALL, (EIGHT, 0, NONE, 28, 8, DICT_OK)),
    (3, 0, bytes.fromhex("1005"), dictionary_bytes(EIGHT), 5, ([b""] * 8, 8, 0, 0, 5, DICT_OK)),
    (3, 0, bytes.fromhex("1005"), dictionary_bytes(EIGHT), 6, ([b"klmno"] * 8, 0, NONE, 40, 6, DICT_OK)),
    (0, 0, bytes.fromhex("07"), dictionary_bytes([b"xy", b"z"]), ALL, ([b"xy"] * 24, 0, NONE, 48, 2, DICT_OK)),
    # the third entry is cut inside its length bytes: 01 00 00 00 'a', 02 00 00 00 'b' 'c', 03 00
    (3, 0, bytes.fromhex("0388C6FA"), bytes.fromhex("0100000061" "020000006263" "0300"), ALL, ([b"a", b"bc"] + [b""] * 6, 6, 2, 3, 2, DICT_CUT)),
]


# ---- a table of segments, as the host hook takes it ----
# a segment: (source offset, source length, offsets offset or NONE, data offset or NONE, data capacity, capacity, offset base, dictionary
# offset, dictionary length, dictionary entries or ALL, bits, flags)
def sentinel(size, salt=0):
    return ((np.arange(size, dtype=np.uint64) % 251 + 3 + salt) % 256).astype(np.uint8).tobytes()


def expected(src, dictionary, segs, offsets_size, data_size):
    """-> (the offsets buffer, the data buffer, [the results]) behind a call over sentinel() buffers"""
    want_o, want_d, results = bytearray(sentinel(offsets_size)), bytearray(sentinel(data_size, 7)), []
    for s, l, o_at, d_at, data_cap, cap, base, t, tl, bound, k, flags in segs:
        offsets, data, res = column(src[s:s + l], k, flags, dictionary[t:t + tl], bound, cap, base)
        results.append(res)
        if cap and o_at != NONE:
            ob = offsets_bytes(offsets, flags)
            assert o_at + len(ob) <= offsets_size, (o_at, len(ob), offsets_size)
            want_o[o_at:o_at + len(ob)] = ob
        if cap and d_at != NONE:
            kept = data[:data_cap]
            assert d_at + len(kept) <= data_size, (d_at, len(kept), data_size)
            want_d[d_at:d_at + len(kept)] = kept
    return bytes(want_o), bytes(want_d), results


def first_difference(got, want):
    return next((i, got[i], want[i]) for i in range(min(len(got), len(want))) if got[i] != want[i]) if got != want else None


def random_entries(rnd, count, lengths):
    """`count` entries whose lengths are drawn from `lengths`, of seeded bytes"""
    return [bytes(rnd.getrandbits(8) for _ in range(rnd.choice(lengths))) for _ in range(count)]


def layout(rnd, datas, dictionary_at, dictionary_len, k, flags=0, caps=None, data_caps=None, bound=ALL, base=0, gap=(0, 1, 5), dictionary=None):
    """segments one behind the other, each with room for all it delivers -> (src, segs, offsets_size, data_size); dictionary: its bytes, for the
    sizes"""
    src, segs, o_at, d_at = bytearray(b"\x5a"), [], 3, 5
    for j, data in enumerate(datas):
        cap = caps[j] if caps is not None else rle_ref.decode(data, k, 8, flags & WIDTH_BYTE, 0)[1][0]
        offsets, body, _ = column(data, k, flags, dictionary[dictionary_at:dictionary_at + dictionary_len], bound, cap, base) if cap else ([], b"", None)
        data_cap = data_caps[j] if data_caps is not None else len(body) + 3
        s_at = len(src) + rnd.choice(gap)
        src += b"\xc3" * (s_at - len(src)) + data
        segs.append((s_at, len(data), o_at, d_at, data_cap, cap, base, dictionary_at, dictionary_len, bound, 77 if flags & WIDTH_BYTE else k, flags))
        o_at += len(offsets_bytes(offsets, flags)) + rnd.choice(gap)
        d_at += min(len(body), data_cap) + rnd.choice(gap)
    return bytes(src) + b"\x3c" * 16, segs, o_at + 40, d_at + 40


def short_table(count=3000, dictionaries=40, seed=19):
    """`count` short segments, empty ones among them, of mixed field widths, flags, capacities, data capacities and endings, over `dictionaries`
    dictionaries in one buffer, cut ones and an empty one among them -> (src, dictionary, segs, offsets_size, data_size)"""
    rnd = random.Random(seed)
    blob, where = bytearray(b"\x11\x22\x33"), []
    for j in range(dictionaries):
        d = dictionary_bytes(random_entries(rnd, rnd.choice([0, 1, 5, 16, 33]) if j else 0, [0, 1, 2, 3, 7, 15, 16, 17, 40]))
        if j % 7 == 3 and d:
            d = d[:rnd.randrange(1, len(d))]
        where.append((len(blob), len(d)))
        blob += d + b"\x77" * rnd.randrange(0, 3)
    src, segs, o_at, d_at = bytearray(b"\x5a"), [], 1, 2
    for _ in range(count):
        k = rnd.choice([0, 1, 3, 5, 6, 9])
        flags = (WIDTH_BYTE if rnd.random() < 0.3 else 0) | (OFFSETS64 if rnd.random() < 0.3 else 0) | (ENDS_ONLY if rnd.random() < 0.3 else 0)
        if rnd.random() < 0.1:
            data = b""
        else:
            data = rle_ref.encode(rle_ref.random_plan(rnd, k, rnd.randrange(1, 60), packed=(8, 24), repeated=(1, 30), hlen=rnd.random() < 0.2), k, bool(flags & WIDTH_BYTE))
            pick = rnd.random()
            if pick < 0.1:
                data = data[:rnd.randrange(len(data))]
            elif pick < 0.2:
                data += rnd.choice(rle_ref.stops(k))[1]
        t, tl = rnd.choice(where)
        bound = rnd.choice([ALL, ALL, 3, 100])
        count_ = rle_ref.decode(data, k, 8, flags & WIDTH_BYTE, 0)[1][0]
        cap = rnd.choice([count_, count_, count_ + 5, count_ // 2, 0, 3])
        offsets, body, _ = column(data, k, flags, bytes(blob[t:t + tl]), bound, cap) if cap else ([], b"", None)
        data_cap = rnd.choice([len(body), len(body) + 9, len(body) // 2, 0])
        has_o, has_d = rnd.random() < 0.9, rnd.random() < 0.9
        s_at = len(src) + rnd.randrange(0, 4)
        src += b"\xc3" * (s_at - len(src)) + data
        segs.append((s_at, len(data), o_at if has_o else NONE, d_at if has_d else NONE, data_cap if has_d else 0, cap, rnd.choice([0, 0, 1000, (1 << 32) - 5]), t, tl, bound,
                     77 if flags & WIDTH_BYTE else k, flags))
        o_at += (len(offsets_bytes(offsets, flags)) if has_o else 0) + rnd.choice([0, 0, 1, 5])
        d_at += (min(len(body), data_cap) if has_d else 0) + rnd.choice([0, 0, 1, 5])
    return bytes(src) + b"\x3c" * 16, bytes(blob), segs, o_at + 64, d_at + 64
