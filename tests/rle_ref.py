"""The reference of the unrle calls (include/brotli/batch.h): Parquet's RLE / bit-packed hybrid.  An encoder from a plan of runs, a plain serial
decoder of the whole contract -- statuses and results included --, and a numpy decoder for large inputs.  A header is a LEB128 varint h of 1 .. 5
bytes; an odd h is a bit-packed run of h >> 1 groups of 8 fields of k bits, LSB-first; an even h is h >> 1 times the little-endian value in the
ceil(k / 8) bytes behind it, not masked."""
import random

import numpy as np

WIDTH_BYTE = 1
OK, BAD_HEADER, ZERO_RUN, TRUNCATED, BAD_WIDTH = 0, 1, 2, 3, 4
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
WIDTHS = [1, 2, 4, 8]

# pinned by hand from the format's grammar: (k, bytes, values)
PINNED = [
    (3, bytes.fromhex("0388C6FA"), list(range(8))),   # the format text's packing example inside a run
    (3, bytes.fromhex("1005"), [5] * 8),
    (9, bytes.fromhex("062C01"), [300] * 3),
    (3, bytes.fromhex("900307"), [7] * 200),
    (0, bytes.fromhex("07"), [0] * 24),
]


# ---- the encoder ----
def header(h, nbytes=None):
    """the varint of h in nbytes bytes (None: the shortest form), padded with continuation bytes"""
    out = bytearray()
    while True:
        out.append(h & 0x7F)
        h >>= 7
        if not h:
            break
    if nbytes is not None:
        assert len(out) <= nbytes <= 5, (len(out), nbytes)
        out.extend(b"\x00" * (nbytes - len(out)))
    for i in range(len(out) - 1):
        out[i] |= 0x80
    return bytes(out)


def pack_fields(values, k):
    """fields of k bits, LSB-first -> ceil(len k / 8) bytes"""
    bits = 0
    for j, v in enumerate(values):
        assert 0 <= v < (1 << k) or (k == 0 and v == 0), (v, k)
        bits |= v << (j * k)
    return bits.to_bytes((len(values) * k + 7) // 8, "little")


def encode(plan, k, width_byte=False):
    """plan: [("rle", count, value) or ("packed", values) -- 8 g of them --, each with an optional header length behind it] -> the segment's bytes;
    an RLE value may be wider than k bits (it is not masked) but not than ceil(k / 8) bytes"""
    out = bytearray([k] if width_byte else [])
    for run in plan:
        if run[0] == "rle":
            _, count, value = run[:3]
            out += header(count << 1, run[3] if len(run) > 3 else None) + int(value).to_bytes((k + 7) // 8, "little")
        else:
            values = list(run[1])
            assert len(values) % 8 == 0 and values
            out += header((len(values) // 8) << 1 | 1, run[2] if len(run) > 2 else None) + pack_fields(values, k)
    return bytes(out)


def plan_values(plan):
    out = []
    for run in plan:
        out += [run[2]] * run[1] if run[0] == "rle" else list(run[1])
    return out


def random_plan(rnd, k, total, packed=(8, 504), repeated=(8, 2000), hlen=False):
    """seeded runs, packed ones of packed[0] .. packed[1] values (multiples of 8) and repeated ones of repeated[0] .. repeated[1], that hold at
    least `total` values; hlen: every header has a random length"""
    plan, have = [], 0
    top = (1 << k) - 1
    extra = lambda h: (rnd.randint(len(header(h)), 5),) if hlen else ()
    while have < total:
        if rnd.random() < 0.5 and packed[1] >= 8:
            m = rnd.randrange(max(packed[0], 8) // 8, packed[1] // 8 + 1) * 8
            plan.append(("packed", [rnd.randint(0, top) for _ in range(m)]) + extra(m // 8 << 1 | 1))
        else:
            m = rnd.randint(*repeated)
            plan.append(("rle", m, rnd.randint(0, top)) + extra(m << 1))
        have += m
    return plan


# ---- the serial decoder: the contract, one byte after the other ----
def _start(data, k, w, flags):
    """-> (k, the first header's offset, None) or (k, 0, BAD_WIDTH)"""
    if not flags & WIDTH_BYTE:
        return k, 0, None
    if len(data) == 0:
        return 0, 0, BAD_WIDTH
    k = data[0]
    return (k, 0, BAD_WIDTH) if k > 32 or k > 8 * w else (k, 1, None)


def _header(data, off):
    """the header at off -> (h, its length, None) or (0, 0, the stop)"""
    h = i = 0
    while True:
        if off + i >= len(data):
            return 0, 0, TRUNCATED
        b = data[off + i]
        h |= (b & 0x7F) << (7 * i)
        i += 1
        if b < 0x80:
            break
        if i == 5:
            return 0, 0, BAD_HEADER
    return (0, 0, ZERO_RUN) if h >> 1 == 0 else (h, i, None)


def decode_serial(data, k, w, flags=0, cap=None):
    """-> ([the first min(count, cap) values as ints of w bytes], (count, consumed, runs, status, bits))"""
    data = bytes(data)
    k, off, stop = _start(data, k, w, flags)
    if stop is not None:
        return [], (0, 0, 0, stop, k)
    out, count, runs, status, n, mask = [], 0, 0, OK, len(data), (1 << (8 * w)) - 1
    room = lambda: (1 << 62) if cap is None else max(0, cap - len(out))
    while off < n:
        h, i, stop = _header(data, off)
        if stop is not None:
            status = stop
            break
        at, c = off + i, h >> 1
        if h & 1:
            need, have = c * k, n - at
            m = 8 * c if need <= have else have * 8 // k
            bits = int.from_bytes(data[at:at + min(need, have)], "little")
            out += [(bits >> (j * k)) & ((1 << k) - 1) & mask for j in range(min(m, room()))]
            count, runs = count + m, runs + (1 if m else 0)
            if need > have:
                status, off = TRUNCATED, n
                break
            off = at + need
        else:
            nb = (k + 7) // 8
            if at + nb > n:
                status = TRUNCATED
                break
            out += [int.from_bytes(data[at:at + nb], "little") & mask] * min(c, room())
            count, runs, off = count + c, runs + 1, at + nb
    return out, (count, off, runs, status, k)


# ---- the numpy decoder: the headers one after the other, every run's values at once ----
def decode(data, k, w, flags=0, cap=None):
    """-> (the first min(count, cap) values as a numpy array of the width's unsigned dtype, (count, consumed, runs, status, bits))"""
    data = bytes(data)
    a = np.frombuffer(data, dtype=np.uint8)
    k, off, stop = _start(data, k, w, flags)
    if stop is not None:
        return np.zeros(0, dtype=DTYPES[w]), (0, 0, 0, stop, k)
    parts, kept, count, runs, status, n = [], 0, 0, 0, OK, len(data)
    weights = (np.uint64(1) << np.arange(k, dtype=np.uint64)) if k else None
    while off < n:
        h, i, stop = _header(data, off)
        if stop is not None:
            status = stop
            break
        at, c = off + i, h >> 1
        room = (1 << 62) if cap is None else max(0, cap - kept)
        if h & 1:
            need, have = c * k, n - at
            m = 8 * c if need <= have else have * 8 // k
            take = min(m, room)
            if take:
                if k == 0:
                    vals = np.zeros(take, dtype=np.uint64)
                else:
                    bits = np.unpackbits(a[at:at + (take * k + 7) // 8], bitorder="little")[:take * k].reshape(take, k)
                    vals = (bits.astype(np.uint64) * weights).sum(axis=1, dtype=np.uint64)
                parts.append(vals.astype(DTYPES[w]))
                kept += take
            count, runs = count + m, runs + (1 if m else 0)
            if need > have:
                status, off = TRUNCATED, n
                break
            off = at + need
        else:
            nb = (k + 7) // 8
            if at + nb > n:
                status = TRUNCATED
                break
            take = min(c, room)
            if take:
                parts.append(np.full(take, int.from_bytes(data[at:at + nb], "little") & ((1 << (8 * w)) - 1), dtype=DTYPES[w]))
                kept += take
            count, runs, off = count + c, runs + 1, at + nb
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=DTYPES[w])), (count, off, runs, status, k)


def elements_bytes(data, k, w, flags, cap):
    """what a segment's destination holds behind the call: the first min(count, cap) elements, little-endian -> (bytes, result)"""
    vals, res = decode(data, k, w, flags, cap)
    return vals.astype("<u%d" % w).tobytes(), res


# ---- the cases that the tests without a device and the tests on the device share ----
def shapes():
    """every field width with every element width that takes it"""
    return [(k, w) for k in range(33) for w in WIDTHS if k <= 8 * w]


def straddling_plans(k, item, lead):
    """runs around the edges of items of `item` elements: an RLE run of `lead` values in front, so that the packed groups behind it are not
    aligned to the items, then a repeated run and a packed run that each span three items, and a tail"""
    rnd = random.Random(1000 * k + lead)
    top = (1 << k) - 1
    span = ((2 * item + item // 2) + 7) // 8 * 8
    return [("rle", lead, rnd.randint(0, top)), ("packed", [rnd.randint(0, top) for _ in range(span)]), ("rle", span + 3, rnd.randint(0, top)),
            ("packed", [rnd.randint(0, top) for _ in range(16)]), ("rle", 1, rnd.randint(0, top))]


def many_runs_plan(k, runs, seed):
    """runs of one value: more than 64 of them fall into one item"""
    rnd = random.Random(seed)
    return [("rle", 1, rnd.randint(0, (1 << k) - 1)) for _ in range(runs)]


def stops(k):
    """every stop: (name, what to put where a run would begin, the status).  Each is a prefix of bytes that ends the decode where it stands;
    the truncated forms must be the segment's last bytes"""
    nb = (k + 7) // 8
    out = [("bad header", b"\x80\x80\x80\x80\x80\x01", BAD_HEADER), ("zero rle run", b"\x00" + b"\x00" * nb, ZERO_RUN), ("zero packed run", b"\x01", ZERO_RUN),
           ("header cut", b"\x82\x80", TRUNCATED), ("all 35 bits", b"\xff\xff\xff\xff\x7f", TRUNCATED if k else None)]
    if nb:
        out.append(("value cut", header(6) + b"\x01" * (nb - 1), TRUNCATED))
    if k:
        out.append(("payload cut", header(5) + b"\xa5" * (2 * k - 1), TRUNCATED))   # two groups announced, one byte short
    return [s for s in out if s[2] is not None]


def short_table(count=3000, seed=11):
    """`count` short segments, empty ones among them, of mixed shapes, flags, capacities and endings, each with bytes of its own
    -> (the source, [(source offset, source length, destination offset, cap, bits, width, flags)], the destination's size)"""
    rnd = random.Random(seed)
    src, segs, d_at = bytearray(b"\x5a"), [], 7
    all_shapes = shapes()
    for _ in range(count):
        k, w = rnd.choice(all_shapes)
        flags = WIDTH_BYTE if rnd.random() < 0.3 else 0
        if rnd.random() < 0.1:
            data = b""
        else:
            plan = random_plan(rnd, k, rnd.randrange(1, 120), packed=(8, 40), repeated=(1, 60), hlen=rnd.random() < 0.2)
            data = encode(plan, k, bool(flags))
            pick = rnd.random()
            if pick < 0.1:
                data = data[:rnd.randrange(len(data))]          # cut anywhere
            elif pick < 0.2:
                name, tail, _ = rnd.choice(stops(k))
                data += tail
            elif pick < 0.25 and flags:
                data = bytes([rnd.choice([33, 8 * w + 1, 255])]) + data[1:]
        count_, _, _, _, _ = decode(data, k, w, flags, 0)[1]
        cap = rnd.choice([count_, count_, count_ + 5, count_ // 2, 0, 3])
        s_at = len(src) + rnd.randrange(0, 4)
        src += b"\xc3" * (s_at - len(src)) + data
        segs.append((s_at, len(data), d_at, cap, 77 if flags else k, w, flags))   # (with WIDTH_BYTE the argument is not looked at)
        d_at += min(cap, count_) * w + rnd.choice([0, 0, 1, 5])
    return bytes(src) + b"\x3c" * 16, segs, d_at + 64
