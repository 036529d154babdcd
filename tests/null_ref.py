"""The reference of the unnull calls (include/brotli/batch.h): dense values spread over nulls by definition levels.  The levels are unrle's runs
-- rle_ref.decode, called with an element width of 8 so that only k <= 32 binds --, and the rest is numpy: the mask level_i == level, the ranks
by cumsum, the take with the bound check (a present slot of rank >= V is missing: 0, and counted), and the bitmap by
np.packbits(..., bitorder="little").  The prefix and follow rules are spelt out here.
-> the slots, the validity bytes and the eight-field result (unrle's five, present, missing, values)."""
import random

import numpy as np

import rle_ref

LENGTH_PREFIX, VALUES_FOLLOW = 1, 2
OK, BAD_HEADER, ZERO_RUN, TRUNCATED, BAD_LENGTH = rle_ref.OK, rle_ref.BAD_HEADER, rle_ref.ZERO_RUN, rle_ref.TRUNCATED, 5
WIDTHS = rle_ref.WIDTHS
DTYPES = rle_ref.DTYPES
NO_BITMAP = (1 << 64) - 1

V1_EXAMPLE = bytes.fromhex("0200000003A50A0014001E002800")

# pinned by hand from the contract: (k, level, flags, the segment's bytes, width, the dense values (None: they follow), cap (None: all),
# the slots, the validity bytes, (count, consumed, present, missing, values))
PINNED = [
    (1, 1, 0, bytes.fromhex("03A5"), 2, [10, 20, 30, 40], None, [10, 0, 20, 0, 0, 30, 0, 40], bytes.fromhex("A5"), (8, 2, 4, 0, 4)),
    (3, 5, 0, bytes.fromhex("1005"), 1, list(range(1, 9)), None, list(range(1, 9)), bytes.fromhex("FF"), (8, 2, 8, 0, 8)),
    (3, 5, 0, bytes.fromhex("1005"), 1, list(range(1, 7)), None, [1, 2, 3, 4, 5, 6, 0, 0], bytes.fromhex("FF"), (8, 2, 8, 2, 6)),   # a missing value
    (3, 2, 0, bytes.fromhex("0388C6FA"), 4, [9], None, [0, 0, 9, 0, 0, 0, 0, 0], bytes.fromhex("04"), (8, 4, 1, 0, 1)),
    (9, 300, 0, bytes.fromhex("062C01"), 1, [7, 8, 9], None, [7, 8, 9], bytes.fromhex("07"), (3, 3, 3, 0, 3)),                      # an RLE value is not masked
    (9, 44, 0, bytes.fromhex("062C01"), 1, [7, 8, 9], None, [0, 0, 0], bytes.fromhex("00"), (3, 3, 0, 0, 3)),
    (0, 0, 0, bytes.fromhex("07"), 1, list(range(1, 11)), 10, list(range(1, 11)), bytes.fromhex("FF03"), (24, 1, 10, 0, 10)),
    (1, 1, LENGTH_PREFIX | VALUES_FOLLOW, V1_EXAMPLE, 2, None, None, [10, 0, 20, 0, 0, 30, 0, 40], bytes.fromhex("A5"), (8, 6, 4, 0, 4)),
]


def values_bytes(values, w):
    return np.array(values, dtype="<u%d" % w).tobytes()


def v1_body(levels, values):
    """a v1 data page's body: the levels behind their length, then the values"""
    return len(levels).to_bytes(4, "little") + bytes(levels) + bytes(values)


def runs_of(data, flags):
    """the prefix rule -> (the runs' offset, the runs) or None: BAD_LENGTH"""
    data = bytes(data)
    if not flags & LENGTH_PREFIX:
        return 0, data
    if len(data) < 4:
        return None
    L = int.from_bytes(data[:4], "little")
    if L > len(data) - 4:
        return None
    return 4, data[4:4 + L]


def decode(data, k, level, w, flags, values=b"", V=0, cap=None):
    """data: the segment; values: the bytes that hold V dense values of w bytes (more may follow: they are not the values'), not looked at
    with VALUES_FOLLOW -> (the first m = min(count, cap) slots as a numpy array of the width's unsigned dtype, the ceil(m / 8) validity bytes,
    (count, consumed, runs, status, bits, present, missing, values))"""
    data = bytes(data)
    follow = bool(flags & VALUES_FOLLOW)
    where = runs_of(data, flags)
    if where is None:
        return np.zeros(0, dtype=DTYPES[w]), b"", (0, 0, 0, BAD_LENGTH, k, 0, 0, 0 if follow else V)
    off, runs = where
    lv, (count, consumed, nruns, status, bits) = rle_ref.decode(runs, k, 8, 0, cap)
    consumed += off
    if follow:
        V = (len(data) - consumed) // w if status == OK else 0
        values = data[consumed:]
    table = np.frombuffer(bytes(values[:V * w]), dtype="<u%d" % w)
    mask = lv.astype(np.uint64) == np.uint64(level)
    ranks = np.cumsum(mask, dtype=np.int64) - mask.astype(np.int64)   # the present slots in front of each
    have = mask & (ranks < V)
    slots = np.zeros(len(lv), dtype=DTYPES[w])
    if have.any():
        slots[have] = table[ranks[have]]
    valid = np.packbits(mask, bitorder="little").tobytes()
    return slots, valid, (count, consumed, nruns, status, bits, int(mask.sum()), int((mask & ~have).sum()), V)


def outputs(data, k, level, w, flags, values=b"", V=0, cap=None):
    """what a segment's destination and bitmap hold behind the call -> (slot bytes, validity bytes, result)"""
    slots, valid, res = decode(data, k, level, w, flags, values, V, cap)
    return slots.astype("<u%d" % w).tobytes(), valid, res


# ---- the cases that the tests without a device and the tests on the device share ----
def level_plan(rnd, k, level, total, null_share, runs=(1, 40), packed=(8, 40), other=None):
    """seeded runs of levels with about null_share nulls that hold at least `total` levels: RLE runs of one level and packed runs of mixed ones;
    other: the levels a null may have (None: everything k bits hold but `level`)"""
    top = (1 << k) - 1
    nulls = other if other is not None else [v for v in range(min(top, 7) + 1) if v != level] or [level]
    pick = lambda: rnd.choice(nulls) if rnd.random() < null_share else level
    plan, have = [], 0
    while have < total:
        if rnd.random() < 0.5:
            m = rnd.randrange(max(packed[0], 8) // 8, packed[1] // 8 + 1) * 8
            plan.append(("packed", [min(pick(), top) for _ in range(m)]))
        else:
            m = rnd.randint(*runs)
            plan.append(("rle", m, pick() if k else 0))
        have += m
    return plan


def present_of(plan, level):
    """the levels of a plan that equal `level`, run by run"""
    return sum((run[1] if run[2] == level else 0) if run[0] == "rle" else sum(1 for v in run[1] if v == level) for run in plan)


def rows_of(plan):
    return sum(run[1] if run[0] == "rle" else len(run[1]) for run in plan)


def random_values(rnd, count, w):
    return bytes(rnd.getrandbits(8) for _ in range(count * w))


def short_table(count=3000, seed=21):
    """`count` short segments of mixed shapes, flags, capacities, endings and value counts -- exactly the present slots, one fewer, none, more --,
    with and without a bitmap, each with bytes of its own
    -> (the source, the values buffer, [(source offset, source length, destination offset, cap, bits, width, flags, level, values offset,
    values count, validity offset)], the destination's size, the bitmaps' size)"""
    rnd = random.Random(seed)
    src, segs, d_at, b_at = bytearray(b"\x5a"), [], 7, 3
    values = bytes(random.Random(seed + 1).getrandbits(8) for _ in range(1 << 12))
    for _ in range(count):
        k, w = rnd.choice([0, 1, 1, 1, 2, 3, 8, 9, 32]), rnd.choice(WIDTHS)
        level = rnd.choice([0, (1 << k) - 1, ((1 << k) - 1) // 2])
        if rnd.random() < 0.1:
            data = b""
        else:
            plan = level_plan(rnd, k, level, rnd.randrange(1, 120), rnd.choice([0.0, 0.3, 0.9, 1.0]), hlen_off(rnd))
            data = rle_ref.encode(plan, k)
            pick = rnd.random()
            if pick < 0.1:
                data = data[:rnd.randrange(len(data))]          # cut anywhere
            elif pick < 0.2:
                data += rnd.choice(rle_ref.stops(k))[1]
        flags = rnd.choice([0, 0, LENGTH_PREFIX, LENGTH_PREFIX | VALUES_FOLLOW])
        present = int((rle_ref.decode(data, k, 8, 0)[0].astype(np.uint64) == np.uint64(level)).sum())
        V = rnd.choice([present, present, present + 3, max(0, present - 1), 0])
        v_at = rnd.randrange(0, len(values) - V * w + 1)
        if flags & LENGTH_PREFIX:
            body = len(data).to_bytes(4, "little") + data
            if flags & VALUES_FOLLOW:
                body += values[v_at:v_at + V * w] + bytes(rnd.randrange(0, w))   # left-over bytes behind the last whole value
            pick = rnd.random()
            if pick < 0.05:
                body = body[:rnd.randrange(0, 5)]                                  # a prefix that is cut, or an empty body behind one
            elif pick < 0.1:
                body = (len(body) - 3).to_bytes(4, "little") + body[4:]            # L one above the room
            data = body
        count_ = decode(data, k, level, w, flags, values[v_at:], V, 0)[2][0]
        cap = rnd.choice([count_, count_, count_ + 5, count_ // 2, 0, 3])
        m = min(cap, count_)
        s_at = len(src) + rnd.randrange(0, 4)
        src += b"\xc3" * (s_at - len(src)) + data
        bitmap = rnd.random() < 0.8
        segs.append((s_at, len(data), d_at, cap, k, w, flags, level, v_at, V, b_at if bitmap else NO_BITMAP))
        d_at += m * w + rnd.choice([0, 0, 1, 5])
        if bitmap:
            b_at += (m + 7) // 8 + rnd.choice([0, 0, 1])
    return bytes(src) + b"\x3c" * 16, values, segs, d_at + 64, b_at + 32


def hlen_off(rnd):
    """run lengths of a plan of the table: short ones, so that many runs fall into a lane's 16 slots"""
    return rnd.choice([(1, 40), (1, 5), (10, 90)])
