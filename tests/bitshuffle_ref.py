"""Bitshuffle in numpy, from the definition in include/brotli/batch.h ("Bit-unshuffle on the device"): the reference of the bit-unshuffle tests.

A segment of len bytes, a width w and a block size `block` in elements (0: one block; otherwise a multiple of 8): m = len // w elements in blocks
of `block`; a full block transposes c = block elements, the last, shorter one c = (m - b block) rounded down to a multiple of 8; what is behind
is copied.  A block's shuffled form is 8 w bit rows of c / 8 bytes; row 8 j + k holds bit k of byte j of every element, element i in bit i % 8
of byte i / 8."""
import numpy as np


def _blocks(n, w, block):
    """[(byte offset, transposed elements)] of the blocks of n bytes"""
    m = n // w
    if block == 0 or block >= m:
        return [(0, m // 8 * 8)]
    assert block % 8 == 0
    return [(b0 * w, block if m - b0 >= block else (m - b0) // 8 * 8) for b0 in range(0, m, block)]


def _full_blocks(n, w, block):
    """the number of full blocks in front of the last one, which _blocks handles alone (all full blocks at once: one numpy call)"""
    m = n // w
    return 0 if block == 0 or block >= m else m // block


def bitshuffle(b, w, block=0):
    """elements -> bit planes"""
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    out = a.copy()
    nb = _full_blocks(len(a), w, block)
    if nb:
        bits = np.unpackbits(a[:nb * block * w].reshape(nb, block, w), axis=2, bitorder="little")          # [b, i, 8 j + k]
        out[:nb * block * w] = np.packbits(bits.transpose(0, 2, 1), axis=2, bitorder="little").reshape(-1)   # [b, 8 j + k, i / 8]
    for o, c in _blocks(len(a), w, block)[nb:]:
        if c:
            bits = np.unpackbits(a[o:o + c * w].reshape(c, w), axis=1, bitorder="little")   # [i, 8 j + k]
            out[o:o + c * w] = np.packbits(bits.T, axis=1, bitorder="little").reshape(-1)     # row 8 j + k: element i in bit i % 8 of byte i / 8
    return out.tobytes()


def bitunshuffle(b, w, block=0):
    """bit planes -> elements"""
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    out = a.copy()
    nb = _full_blocks(len(a), w, block)
    if nb:
        rows = np.unpackbits(a[:nb * block * w].reshape(nb, 8 * w, block // 8), axis=2, bitorder="little")   # [b, 8 j + k, i]
        out[:nb * block * w] = np.packbits(rows.transpose(0, 2, 1), axis=2, bitorder="little").reshape(-1)
    for o, c in _blocks(len(a), w, block)[nb:]:
        if c:
            rows = np.unpackbits(a[o:o + c * w].reshape(8 * w, c // 8), axis=1, bitorder="little")   # [8 j + k, i]
            out[o:o + c * w] = np.packbits(rows.T, axis=1, bitorder="little").reshape(-1)
    return out.tobytes()


def bitunshuffle_loop(b, w, block=0):
    """the formula bit by bit (slow: for short inputs)"""
    src = bytes(b)
    dst = bytearray(src)
    for o, c in _blocks(len(src), w, block):
        for i in range(c):
            for j in range(w):
                v = 0
                for k in range(8):
                    v |= ((src[o + (8 * j + k) * (c // 8) + i // 8] >> (i % 8)) & 1) << k
                dst[o + i * w + j] = v
    return bytes(dst)
