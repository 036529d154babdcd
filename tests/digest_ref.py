"""References for the digests of batch.h (test_digest_cpu.py, test_gpu_digest.py): zlib for CRC-32, a table-driven loop for CRC-32C, and
x^(8 n) mod P by square and multiply -- none of it shares code with csrc/brotli_crc.h."""
import zlib

CRC32, CRC32C = 1, 2
POLY = {CRC32: 0xEDB88320, CRC32C: 0x82F63B78}
CHECK = {CRC32: 0xCBF43926, CRC32C: 0xE3069283}   # of b"123456789"

_TABLE = []
for _v in range(256):
    for _ in range(8):
        _v = (_v >> 1) ^ (POLY[CRC32C] if _v & 1 else 0)
    _TABLE.append(_v)


def crc32c(data):
    r = 0xFFFFFFFF
    for b in bytes(data):
        r = _TABLE[(r ^ b) & 0xFF] ^ (r >> 8)
    return r ^ 0xFFFFFFFF


def crc(kind, data):
    return zlib.crc32(bytes(data)) & 0xFFFFFFFF if kind == CRC32 else crc32c(data)


def mulmod(kind, a, b):
    """a b mod P in the reflected register: bit 31 is x^0"""
    r = 0
    for i in range(32):
        if (b >> (31 - i)) & 1:
            r ^= a
        a = (a >> 1) ^ (POLY[kind] if a & 1 else 0)
    return r


def xpow(kind, e):
    """x^e mod P"""
    r, sq = 0x80000000, 0x40000000
    while e:
        if e & 1:
            r = mulmod(kind, r, sq)
        sq = mulmod(kind, sq, sq)
        e >>= 1
    return r
