"""The reference for undbp: Parquet's DELTA_BINARY_PACKED as include/brotli/batch.h states it.  An encoder from a PLAN (so that a test chooses B
and M, widths above the needed ones, the varints' lengths, the junk in unneeded width bytes and a cut last padding), a serial decoder of the
whole contract, stops included, a numpy decoder that is checked against the serial one, and the four examples of batch.h pinned by hand.
A result is (count, consumed, declared, blocks, status, block_values, miniblocks)."""
import random

import numpy as np

OK, BAD_HEADER, BAD_WIDTH, TRUNCATED = 0, 1, 2, 3
WIDTHS = (1, 2, 4, 8)
M64 = (1 << 64) - 1
U32 = (1 << 32) - 1

# (bytes, values, consumed)
PINNED = [
    (bytes.fromhex("80 01 04 05 0e 02 00 00 00 00"), [7, 8, 9, 10, 11], 10),
    (bytes.fromhex("80 01 04 08 0e 03 02 00 00 00 c0 3f 00 00 00 00 00 00"), [7, 5, 3, 1, 2, 3, 4, 5], 18),
    (bytes.fromhex("80 01 04 01 01"), [-1], 5),
    (bytes.fromhex("80 01 04 02 00 ff ff ff ff ff ff ff ff ff 01 00 ee ee ee"), [0, -(1 << 63)], 19),
]


def zigzag(v):
    """a signed or unsigned 64-bit value -> its zigzag form"""
    v &= M64
    return ((v << 1) & M64) ^ (M64 if v >> 63 else 0)


def unzigzag(u):
    return (u >> 1) ^ (M64 if u & 1 else 0)


def varint(v, length=0):
    """v < 2^64 as a LEB128 varint, padded with 80 .. 00 to `length` bytes where that is longer"""
    out = bytearray()
    while True:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
        if v == 0 and len(out) >= length:
            break
    out[-1] &= 0x7F
    return bytes(out)


def pack(fields, k):
    """fields of k bits, LSB-first -> bytes (their number times k is a multiple of 8)"""
    acc = 0
    for i, f in enumerate(fields):
        acc |= f << (i * k)
    return acc.to_bytes(len(fields) * k // 8, "little")


def encode(values, B=128, M=4, widen=None, vlen=0, junk=0xEE, cut=0, declared=None, mins=None):
    """values (any integers, taken mod 2^64) -> the stream.  widen(block, miniblock, needed width) -> the width to write (at or above the needed
    one); vlen: the length every varint is padded to (or a function of its place: "B", "M", "N", "first", ("min", block)); junk: the byte in
    the unneeded width bytes (or a function of (block, miniblock)); cut: payload bytes dropped from the stream's end; declared: N where it is
    not len(values); mins(block, the least delta) -> the min_delta to write (the fields are the deltas minus it, mod 2^64)"""
    V = B // M
    ln = vlen if callable(vlen) else (lambda place: vlen)
    n = len(values)
    out = bytearray(varint(B, ln("B")) + varint(M, ln("M")) + varint(n if declared is None else declared, ln("N")) + varint(zigzag(values[0]) if n else 0, ln("first")))
    deltas = [(values[i + 1] - values[i]) & M64 for i in range(n - 1)]
    for b, at in enumerate(range(0, len(deltas), B)):
        blk = deltas[at:at + B]
        signed = [d - (1 << 64) if d >> 63 else d for d in blk]
        lo = min(signed) if mins is None else mins(b, min(signed))
        out += varint(zigzag(lo), ln(("min", b)))
        need = (len(blk) + V - 1) // V
        widths, payloads = [], []
        for j in range(M):
            if j >= need:
                widths.append(junk(b, j) if callable(junk) else junk)
                continue
            fields = [(d - lo) & M64 for d in blk[j * V:(j + 1) * V]]
            k = max(f.bit_length() for f in fields)
            if widen is not None:
                k = max(k, widen(b, j, k))
            widths.append(k)
            payloads.append(pack(fields + [0] * (V - len(fields)), k))
        out += bytes(widths) + b"".join(payloads)
    return bytes(out[:len(out) - cut]) if cut else bytes(out)


def read_varint(data, off):
    """-> (value, bytes, status)"""
    v = 0
    for i in range(10):
        if off + i >= len(data):
            return 0, 0, TRUNCATED
        b = data[off + i]
        v |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return v & M64, i + 1, OK
    return 0, 0, BAD_HEADER


def decode_serial(data, w=8, cap=None):
    """-> (the first min(count, cap) values mod 2^(8 w), result), value after value"""
    mask = (1 << (8 * w)) - 1
    hdr, off = [], 0
    for _ in range(4):
        v, nb, st = read_varint(data, off)
        if st != OK:
            return [], (0, 0, 0, 0, st, 0, 0)
        hdr.append(v)
        off += nb
    B, M, N, first = hdr
    rep = (min(B, U32), min(M, U32))
    if B == 0 or B % 128 or B > 65536 or M == 0 or B % M or (B // M) % 32:
        return [], (0, 0, N, 0, BAD_HEADER) + rep
    V = B // M
    if N == 0:
        return [], (0, off, 0, 0, OK) + rep
    vals, v, blocks, status = [unzigzag(first)], unzigzag(first), 0, OK
    total = N - 1
    done = 0
    while done < total:
        md, nb, st = read_varint(data, off)
        if st != OK:
            status = st
            break
        wat = off + nb
        if wat + M > len(data):
            status = TRUNCATED
            break
        remaining = total - done
        need = min(M, (remaining + V - 1) // V)
        if any(k > 64 for k in data[wat:wat + need]):
            status = BAD_WIDTH
            break
        pos, got, md = wat + M, 0, unzigzag(md)
        for j in range(need):
            k = data[wat + j]
            nbytes = V * k // 8
            want = min(V, remaining - got)
            if pos + nbytes > len(data):
                want = min(want, (len(data) - pos) * 8 // k)
                status = TRUNCATED
            acc = int.from_bytes(data[pos:pos + nbytes], "little")
            for t in range(want):
                v = (v + md + ((acc >> (t * k)) & ((1 << k) - 1))) & M64
                vals.append(v)
            got += want
            if status != OK:
                pos = len(data)
                break
            pos += nbytes
        blocks += 1 if got else 0
        done += got
        off = pos
        if status != OK:
            break
    keep = len(vals) if cap is None else min(cap, len(vals))
    return [x & mask for x in vals[:keep]], (len(vals), off, N, blocks, status) + rep


def decode(data, w=8, cap=None):
    """the same with numpy where a miniblock's fields are unpacked and summed: -> (a numpy array of uint64, result)"""
    hdr, off = [], 0
    none = np.zeros(0, dtype=np.uint64)
    for _ in range(4):
        v, nb, st = read_varint(data, off)
        if st != OK:
            return none, (0, 0, 0, 0, st, 0, 0)
        hdr.append(v)
        off += nb
    B, M, N, first = hdr
    rep = (min(B, U32), min(M, U32))
    if B == 0 or B % 128 or B > 65536 or M == 0 or B % M or (B // M) % 32:
        return none, (0, 0, N, 0, BAD_HEADER) + rep
    V = B // M
    if N == 0:
        return none, (0, off, 0, 0, OK) + rep
    raw = np.frombuffer(data, dtype=np.uint8)
    parts, blocks, status, done, total = [], 0, OK, 0, N - 1
    while done < total and status == OK:
        md, nb, st = read_varint(data, off)
        wat = off + nb
        if st != OK or wat + M > len(data):
            status = st if st != OK else TRUNCATED
            break
        remaining = total - done
        need = min(M, (remaining + V - 1) // V)
        if need and int(raw[wat:wat + need].max()) > 64:
            status = BAD_WIDTH
            break
        pos, got = wat + M, 0
        for j in range(need):
            k = int(raw[wat + j])
            nbytes = V * k // 8
            want = min(V, remaining - got)
            if pos + nbytes > len(data):
                want, status = min(want, (len(data) - pos) * 8 // k), TRUNCATED
            if k == 0:
                fields = np.zeros(want, dtype=np.uint64)
            else:
                bits = np.unpackbits(raw[pos:pos + (want * k + 7) // 8], bitorder="little")[:want * k].reshape(want, k).astype(np.uint64)
                fields = (bits << np.arange(k, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
            parts.append(fields + np.uint64(unzigzag(md)))
            got += want
            if status != OK:
                pos = len(data)
                break
            pos += nbytes
        blocks += 1 if got else 0
        done += got
        off = pos
    with np.errstate(over="ignore"):
        vals = np.cumsum(np.concatenate([np.array([unzigzag(first)], dtype=np.uint64)] + parts), dtype=np.uint64)
    keep = len(vals) if cap is None else min(cap, len(vals))
    out = vals[:keep]
    if w < 8:
        out = out & np.uint64((1 << (8 * w)) - 1)
    return out, (len(vals), off, N, blocks, status) + rep


def elements_bytes(data, w, cap=None):
    """-> (the bytes of the elements that a call stores, the result)"""
    vals, res = decode(data, w, cap)
    return vals.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :w].tobytes(), res


# ---- values that exercise the format ----
def random_values(rnd, n, bits=20, signed=True):
    """n values whose deltas need up to `bits` bits"""
    v, out = rnd.getrandbits(40), []
    for _ in range(n):
        out.append(v & M64)
        v += rnd.getrandbits(rnd.randint(0, bits)) - ((1 << (bits - 1)) if signed and bits else 0)
    return out


def mixed_width_block(rnd, V=32):
    """(values, B, M): one block of nine miniblocks' worth -- B = 9 x 32 is no multiple of 128, so M = 12 over B = 384: the widths 0, 1, 7, 8,
    31, 32, 33, 63 and 64 one after the other, then three more; min_delta is 0 so that a field is the delta itself"""
    widths = [0, 1, 7, 8, 31, 32, 33, 63, 64, 5, 0, 64]
    vals, v = [5], 5
    for k in widths:
        for t in range(V):
            f = 0 if k == 0 else (rnd.getrandbits(k) | (1 << (k - 1)) if t == 0 else rnd.getrandbits(k))
            v = (v + f) & M64
            vals.append(v)
    return vals, V * len(widths), len(widths), widths


def stops(B=128, M=4):
    """(name, bytes that follow whole blocks -- a block that stops --, status, values it still gives, bytes of it that are consumed or None for
    all): every row of the stop table for a block; `more` values are declared beyond the blocks in front"""
    V = B // M
    k = 5
    return [
        ("min_delta of eleven bytes", b"\xff" * 10 + b"\x01" + bytes(M), BAD_HEADER, 0, 0),
        ("width above 64", b"\x02" + bytes([k, 65] + [0] * (M - 2)) + bytes(V * k // 8), BAD_WIDTH, 0, 0),
        ("nothing", b"", TRUNCATED, 0, 0),
        ("min_delta cut", b"\x80\x80", TRUNCATED, 0, 0),
        ("width bytes cut", b"\x02" + bytes(M - 1), TRUNCATED, 0, 0),
        ("payload cut", b"\x02" + bytes([k] * M) + bytes(V * k // 8) + bytes(7), TRUNCATED, V + 7 * 8 // k, None),
    ]


def short_table(n=3000, seed=11):
    """-> (src, [(source offset, length, destination offset, cap, width)], destination size): many short segments of every kind, whole and cut,
    at every alignment"""
    rnd = random.Random(seed)
    src, segs, d_at = bytearray(), [], 1
    for i in range(n):
        w = rnd.choice(WIDTHS)
        kind = i % 10
        if kind == 0:
            data = b""
        elif kind == 1:
            data = encode(random_values(rnd, rnd.randrange(0, 3), 12))
        else:
            B, M = rnd.choice([(128, 4), (128, 1), (256, 4), (256, 8)])
            data = encode(random_values(rnd, rnd.randrange(1, 300), rnd.choice([0, 3, 12, 40, 64])), B, M)
            if kind == 2:
                data = data[:rnd.randrange(len(data))]
            elif kind == 3 and len(data) > 8:
                data = bytearray(data)
                data[rnd.randrange(4, len(data))] = 0xFF
                data = bytes(data)
            elif kind == 4:
                data += bytes(rnd.randrange(1, 9))
            elif kind == 5:   # a header that is none
                data = varint(rnd.choice([0, 64, 192, 65664])) + data[2:]   # (B = 128 and 256 are two bytes)
        count = decode(data, w)[1][0]
        cap = rnd.choice([count, count, count + 3, count // 2, 0])
        segs.append((len(src), len(data), d_at, cap, w))
        src += data + bytes(rnd.randrange(0, 3))
        d_at += min(cap, count) * w + rnd.randrange(0, 3)
    return bytes(src), segs, d_at + 16


def block_offsets(data):
    """the offsets of the blocks of a stream that decodes OK"""
    hdr, off = [], 0
    for _ in range(4):
        v, nb, _ = read_varint(data, off)
        hdr.append(v)
        off += nb
    B, M, N = hdr[:3]
    V, out, left = B // M, [], max(N, 1) - 1
    while left:
        out.append(off)
        off += read_varint(data, off)[1]
        need = min(M, (min(left, B) + V - 1) // V)
        off += M + sum(V * k // 8 for k in data[off:off + need])
        left -= min(left, B)
    return out


def encode_bits(bits, first=0, B=65536, M=4):
    """a long stream fast: the deltas are the 0s and 1s of the numpy array `bits`, every miniblock has width 1 and every min_delta is 0"""
    V = B // M
    out = [varint(B), varint(M), varint(len(bits) + 1), varint(zigzag(first))]
    for at in range(0, len(bits), B):
        blk = bits[at:at + B]
        need = (len(blk) + V - 1) // V
        out.append(b"\x00" + bytes([1] * need + [0xEE] * (M - need)))
        out.append(np.packbits(np.concatenate([blk, np.zeros(need * V - len(blk), dtype=np.uint8)]), bitorder="little").tobytes())
    return b"".join(out)
