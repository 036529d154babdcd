"""Fixed-width bit packing in numpy, from the definition in include/brotli/batch.h ("Bit-unpack on the device"): the reference of the bit-unpack
tests.

A segment is m fields of k bits (1 .. 64) read from a string of bits; element i is the field of bits i k .. i k + k - 1, as a little-endian
integer of w bytes (1, 2, 4, 8; k <= 8 w).  LSB-first: stream bit b is bit b % 8 of byte b // 8 and a field's first bit is the value's bit 0.
MSB-first: stream bit b is bit 7 - b % 8 of byte b // 8 and a field's first bit is the value's bit k - 1.  Signed: the value is sign-extended
from bit k - 1.  ceil(m k / 8) bytes are read; pad bits and bytes behind are ignored."""
import numpy as np

MSB_FIRST, SIGNED = 1, 2   # (BROTLI_AMD_BITUNPACK_MSB_FIRST, BROTLI_AMD_BITUNPACK_SIGNED)

# the two examples of the Parquet format text -- the values 0 .. 7 at k = 3 --, and the MSB-first one unpacked signed into w = 2
PINNED_VALUES, PINNED_BITS = list(range(8)), 3
PINNED_LSB = bytes.fromhex("88c6fa")
PINNED_MSB = bytes.fromhex("053977")
PINNED_MSB_SIGNED_W2 = bytes.fromhex("0000010002000300fcfffdfffeffffff")


def valid_shapes():
    """every (w, k) that goes together: 120 pairs"""
    return [(w, k) for w in (1, 2, 4, 8) for k in range(1, 8 * w + 1)]


def src_bytes(m, k):
    return (m * k + 7) // 8


def unpack(b, m, k, w, flags=0):
    """fields -> elements: unpackbits in the stream's bit order, (m, k), a weighted sum, the extension"""
    assert 1 <= k <= 8 * w and w in (1, 2, 4, 8) and flags in (0, 1, 2, 3)
    a = np.frombuffer(bytes(b), dtype=np.uint8)[:src_bytes(m, k)]
    assert len(a) == src_bytes(m, k)
    bits = np.unpackbits(a, bitorder="big" if flags & MSB_FIRST else "little")[:m * k].reshape(m, k).astype(np.uint64)
    place = np.arange(k, dtype=np.uint64)          # the value's bit that a field's t-th bit is
    if flags & MSB_FIRST:
        place = np.uint64(k - 1) - place
    v = (bits << place).sum(axis=1, dtype=np.uint64) if m else np.zeros(0, dtype=np.uint64)   # (disjoint bits: the sum is the or)
    if flags & SIGNED and k < 64:
        s = np.uint64(1 << (k - 1))
        v = (v ^ s) - s                              # (wraps: the extension to 64 bits)
    return v.astype("<u8").view(np.uint8).reshape(m, 8)[:, :w].tobytes()


def unpack_loop(b, m, k, w, flags=0):
    """the definition bit by bit (slow: for short inputs)"""
    src = bytes(b)
    out = bytearray()
    for i in range(m):
        v = 0
        for t in range(k):
            bit = i * k + t
            if flags & MSB_FIRST:
                v |= ((src[bit // 8] >> (7 - bit % 8)) & 1) << (k - 1 - t)
            else:
                v |= ((src[bit // 8] >> (bit % 8)) & 1) << t
        if flags & SIGNED and (v >> (k - 1)) & 1:
            v -= 1 << k
        out += (v & ((1 << (8 * w)) - 1)).to_bytes(w, "little")
    return bytes(out)


def pack(values, k, flags=0):
    """the low k bits of every value -> fields, the last byte padded with zero bits"""
    v = np.asarray(values).astype(np.uint64) if len(values) else np.zeros(0, dtype=np.uint64)
    place = np.arange(k, dtype=np.uint64)
    if flags & MSB_FIRST:
        place = np.uint64(k - 1) - place
    bits = ((v[:, None] >> place[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="big" if flags & MSB_FIRST else "little").tobytes()
