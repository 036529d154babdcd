"""The reference of the undict calls (include/brotli/batch.h): dictionary-index runs back into values.  The runs are unrle's -- rle_ref.decode,
called with an element width of 8 so that only k <= 32 binds -- and the values a numpy take of the dictionary with the bound check: an index at or
above the dictionary's entries gives 0 and is counted.  -> elements and the seven-field result (unrle's five, bad, first_bad)."""
import random

import numpy as np

import rle_ref

WIDTH_BYTE = rle_ref.WIDTH_BYTE
NO_STREAM = 0xFFFFFFFF
NONE = (1 << 64) - 1   # first_bad where no element was bad
OK, BAD_HEADER, ZERO_RUN, TRUNCATED, BAD_WIDTH = rle_ref.OK, rle_ref.BAD_HEADER, rle_ref.ZERO_RUN, rle_ref.TRUNCATED, rle_ref.BAD_WIDTH
WIDTHS = rle_ref.WIDTHS
DTYPES = rle_ref.DTYPES

ENTRIES16 = [0x1110, 0x2221, 0x3332, 0x4443, 0x5554, 0x6665, 0x7776, 0x8887]   # eight uint16 entries

# pinned by hand from the contract: (k, flags, the segment's bytes, width, the dictionary's entries, the elements, (bad, first_bad))
PINNED = [
    (3, 0, bytes.fromhex("0388C6FA"), 2, ENTRIES16, ENTRIES16, (0, NONE)),               # indices 0 .. 7: the eight entries in order
    (3, 0, bytes.fromhex("1005"), 2, ENTRIES16[:5], [0] * 8, (8, 0)),                    # 8 x index 5 with D = 5: all bad
    (3, 0, bytes.fromhex("1005"), 2, ENTRIES16[:6], [0x6665] * 8, (0, NONE)),            # ... with D = 6: 8 x entry 5
    (0, 0, bytes.fromhex("07"), 2, ENTRIES16, [0x1110] * 24, (0, NONE)),                 # k = 0: 24 x entry 0
    (77, WIDTH_BYTE, bytes.fromhex("030388C6FA"), 1, [9, 8, 7, 6, 5, 4], [9, 8, 7, 6, 5, 4, 0, 0], (2, 6)),   # the width byte says 3; D = 6
]


def dictionary_bytes(entries, w):
    return np.array(entries, dtype="<u%d" % w).tobytes()


def decode(data, k, w, flags, dictionary, entries, cap=None):
    """dictionary: the bytes that hold `entries` entries of w bytes (more may follow: they are not the dictionary's)
    -> (the first min(count, cap) values as a numpy array of the width's unsigned dtype, (count, consumed, runs, status, bits, bad, first_bad))"""
    idx, res = rle_ref.decode(data, k, 8, flags, cap)
    idx = idx.astype(np.uint64)
    table = np.frombuffer(bytes(dictionary[:entries * w]), dtype="<u%d" % w)
    ok = idx < np.uint64(entries)
    vals = np.zeros(len(idx), dtype=DTYPES[w])
    if ok.any():
        vals[ok] = table[idx[ok].astype(np.int64)]
    bad = np.flatnonzero(~ok)
    return vals, res + (len(bad), int(bad[0]) if len(bad) else NONE)


def elements_bytes(data, k, w, flags, dictionary, entries, cap):
    """what a segment's destination holds behind the call -> (bytes, result)"""
    vals, res = decode(data, k, w, flags, dictionary, entries, cap)
    return vals.astype("<u%d" % w).tobytes(), res


def random_dictionary(rnd, entries, w):
    return bytes(rnd.getrandbits(8) for _ in range(entries * w))


def many_runs_plan(seed, runs=900, k=9):
    """short runs of k-bit indices, so that an item of 1024 elements holds several batches of 64 runs: every fifth is a packed run of 8 values,
    the others are repeated runs of 1 + i % 3.  With 900 runs: 2880 elements in three items of 321, 320 and 260 runs, and every batch's first
    element lies inside a lane's 16 elements, none at a lane's edge"""
    rnd = random.Random(seed)
    top = (1 << k) - 1
    return [("packed", [rnd.randint(0, top) for _ in range(8)]) if i % 5 == 4 else ("rle", 1 + i % 3, rnd.randint(0, top)) for i in range(runs)]


def runs_per_item(plan, item):
    """the runs of a plan that hold an element of each item of `item` elements"""
    at, out = 0, []
    for run in plan:
        m = run[1] if run[0] == "rle" else len(run[1])
        for j in range(at // item, (at + m - 1) // item + 1):
            out += [0] * (j + 1 - len(out))
            out[j] += 1
        at += m
    return out


def short_table(count=3000, seed=12, max_k=32):
    """`count` short segments of mixed shapes, flags, capacities and endings (rle_ref.short_table's), each with a dictionary of its own size at
    any alignment in one dictionary buffer: larger than its indices, smaller, of one entry, of none.  Fields of up to max_k bits; with max_k <= 10
    every index, in range or not, stays inside the dictionary buffer
    -> (the source, the dictionary buffer, [(source offset, source length, destination offset, cap, bits, width, flags, dictionary offset,
    entries)], the destination's size)"""
    rnd = random.Random(seed)
    src, segs, d_at = bytearray(b"\x5a"), [], 7
    dictionary = bytes(random.Random(seed + 1).getrandbits(8) for _ in range(1 << 14))
    for _ in range(count):
        k, w = rnd.randrange(max_k + 1), rnd.choice(WIDTHS)
        flags = WIDTH_BYTE if rnd.random() < 0.3 else 0
        if rnd.random() < 0.1:
            data = b""
        else:
            plan = rle_ref.random_plan(rnd, k, rnd.randrange(1, 120), packed=(8, 40), repeated=(1, 60), hlen=rnd.random() < 0.2)
            data = rle_ref.encode(plan, k, bool(flags))
            pick = rnd.random()
            if pick < 0.1:
                data = data[:rnd.randrange(len(data))]          # cut anywhere
            elif pick < 0.2:
                data += rnd.choice(rle_ref.stops(k))[1]
            elif pick < 0.25 and flags:
                data = bytes([rnd.choice([33, 255])]) + data[1:]
        count_ = rle_ref.decode(data, k, 8, flags, 0)[1][0]
        cap = rnd.choice([count_, count_, count_ + 5, count_ // 2, 0, 3])
        top = 1 << min(k, 10)
        entries = rnd.choice([top, top, top, max(1, top // 2), top - 1, 1, 0, 5])
        t_at = rnd.randrange(0, len(dictionary) - max(entries, top) * w + 1)
        s_at = len(src) + rnd.randrange(0, 4)
        src += b"\xc3" * (s_at - len(src)) + data
        segs.append((s_at, len(data), d_at, cap, 77 if flags else k, w, flags, t_at, entries))   # (with WIDTH_BYTE the argument is not looked at)
        d_at += min(cap, count_) * w + rnd.choice([0, 0, 1, 5])
    return bytes(src) + b"\x3c" * 16, dictionary, segs, d_at + 64
