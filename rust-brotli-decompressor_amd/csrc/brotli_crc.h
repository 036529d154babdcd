// brotli_crc.h -- CRC-32 and CRC-32C of byte segments that are digested in PIECES: the arithmetic, once, for the host and the device.
//
// Both are reflected 32-bit CRCs with init and final XOR 0xFFFFFFFF: CRC-32 (0xEDB88320: zlib, gzip, PNG, the `crc` field of a Parquet page)
// and CRC-32C (0x82F63B78, Castagnoli: log and object stores).  "123456789" gives 0xCBF43926 and 0xE3069283; no bytes give 0.
//
// A CRC is linear over GF(2).  The RAW register -- no init, no final XOR -- after the bytes A then B is the register after A, multiplied by
// x^(8 |B|) mod P, XOR the register after B alone.  So a segment is cut into pieces that are digested independently, each from a raw
// register of 0, each then multiplied by x^(8 x the segment's bytes behind the piece), and XORed together in any order
// (csrc/brotli_crc_kernels.hip: a piece a lane).  The init value goes in ONCE per segment, as the start register of the piece that holds the
// segment's first byte, where the multiplication carries it along like a byte of data; the final XOR goes in once, with the piece that holds
// the last byte, behind which nothing is multiplied.  The same rule for whole standard CRCs: crc(A B) == shift(crc(A), |B|) ^ crc(B).
//
// In the reflected register bit 31 is the coefficient of x^0 and bit 0 that of x^31: x^0 is 0x80000000, and a multiplication by x is a
// shift to the right.  Words are taken from memory little-endian (gfx950, x86-64).
//
// One set of functions for the host (csrc/brotli_digest.cpp: BrotliAmdDebugDigestHost, BrotliAmdDebugDigestShift; tests/tools/digest_san.cpp)
// and the device.  They see the byte tables and the powers through pointers: the device hands them its copy in LDS.
#ifndef BROTLI_AMD_CRC_H_
#define BROTLI_AMD_CRC_H_

#include <stdint.h>

#include "brotli_seg_walk.h"   // a segment's units

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BROTLI_AMD_CRC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BROTLI_AMD_CRC_HD inline
#endif

#define BROTLI_AMD_CRC32_POLY 0xEDB88320u
#define BROTLI_AMD_CRC32C_POLY 0x82F63B78u

// One segment of a digest launch (csrc/brotli_crc_kernels.hip): len bytes at ptr, a device address of any alignment, len 0 included.  Nothing
// outside the 16-byte-aligned span around [ptr, ptr + len) is read.
typedef struct BrotliAmdCrcSeg {
  const uint8_t* ptr;
  uint64_t len;
} BrotliAmdCrcSeg;
#define BROTLI_AMD_CRC_RUN_UNITS 8u       // consecutive units that one lane takes through the tables
#define BROTLI_AMD_CRC_TILE_BYTES 32768u  // source bytes of one tile: the blocks of a launch take the segments' bytes tile by tile

// the polynomial of a digest kind (BROTLI_AMD_DIGEST_CRC32 = 1, BROTLI_AMD_DIGEST_CRC32C = 2: include/brotli/batch.h); 0: no such kind
BROTLI_AMD_CRC_HD constexpr uint32_t brotli_amd_crc_poly(uint32_t kind) { return kind == 1u ? BROTLI_AMD_CRC32_POLY : kind == 2u ? BROTLI_AMD_CRC32C_POLY : 0u; }

// a b mod P
BROTLI_AMD_CRC_HD constexpr uint32_t brotli_amd_crc_mul(uint32_t poly, uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 0; i < 32; i++) {   // bit 31 - i of b: the coefficient of x^i, with a = a x^i
    r ^= (b & 0x80000000u) ? a : 0u;
    b <<= 1;
    a = (a >> 1) ^ ((a & 1u) ? poly : 0u);
  }
  return r;
}

// What a polynomial needs.  t: slicing by 4 -- t[0][v] is the raw register after the byte v and t[k][v] the same k zero bytes later, so four
// bytes go through four lookups.  pw[j] = x^(8 2^j) mod P: a shift by any 64-bit number of bytes is at most 64 multiplications.
struct BrotliAmdCrcConsts {
  uint32_t t[4][256];
  uint32_t pw[64];
};

constexpr BrotliAmdCrcConsts brotli_amd_crc_make_consts(uint32_t poly) {
  BrotliAmdCrcConsts c = {};
  for (uint32_t v = 0; v < 256u; v++) {
    uint32_t r = v;
    for (int i = 0; i < 8; i++) r = (r >> 1) ^ ((r & 1u) ? poly : 0u);
    c.t[0][v] = r;
  }
  for (uint32_t k = 1; k < 4u; k++)
    for (uint32_t v = 0; v < 256u; v++) c.t[k][v] = (c.t[k - 1][v] >> 8) ^ c.t[0][c.t[k - 1][v] & 0xFFu];
  uint32_t p = 0x40000000u;   // x^1
  for (int i = 0; i < 3; i++) p = brotli_amd_crc_mul(poly, p, p);   // x^8
  for (uint32_t j = 0; j < 64u; j++) { c.pw[j] = p; p = brotli_amd_crc_mul(poly, p, p); }
  return c;
}

// crc x^(8 nbytes) mod P: what nbytes more bytes behind it make of a piece's raw register (and of a whole standard CRC, in the combine rule)
BROTLI_AMD_CRC_HD uint32_t brotli_amd_crc_shift(uint32_t poly, const uint32_t* pw, uint32_t crc, uint64_t nbytes) {
  for (uint32_t j = 0; nbytes != 0u; j++, nbytes >>= 1)
    if (nbytes & 1u) crc = brotli_amd_crc_mul(poly, crc, pw[j]);
  return crc;
}

// the raw register one byte, and four bytes (a little-endian word), later; t = BrotliAmdCrcConsts::t as 1024 words
BROTLI_AMD_CRC_HD uint32_t brotli_amd_crc_byte(const uint32_t* t, uint32_t reg, uint32_t byte) { return t[(reg ^ byte) & 0xFFu] ^ (reg >> 8); }
BROTLI_AMD_CRC_HD uint32_t brotli_amd_crc_word(const uint32_t* t, uint32_t reg, uint32_t w) {
  reg ^= w;
  return t[768u + (reg & 0xFFu)] ^ t[512u + ((reg >> 8) & 0xFFu)] ^ t[256u + ((reg >> 16) & 0xFFu)] ^ t[reg >> 24];
}

// ... and bytes [lo, hi) of the sixteen in w0..w3 later (0 <= lo < hi <= 16).  Bytes in front of lo and behind hi are not looked at: they are
// not the segment's.
BROTLI_AMD_CRC_HD uint32_t brotli_amd_crc_unit(const uint32_t* t, uint32_t reg, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t lo, uint32_t hi) {
  if (lo == 0u && hi == 16u)
    return brotli_amd_crc_word(t, brotli_amd_crc_word(t, brotli_amd_crc_word(t, brotli_amd_crc_word(t, reg, w0), w1), w2), w3);
  const uint32_t w[4] = {w0, w1, w2, w3};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < 4u; i++) {
    if (4u * i >= lo && 4u * i + 4u <= hi) { reg = brotli_amd_crc_word(t, reg, w[i]); continue; }
    for (uint32_t k = 0; k < 4u; k++)
      if (4u * i + k >= lo && 4u * i + k < hi) reg = brotli_amd_crc_byte(t, reg, (w[i] >> (8u * k)) & 0xFFu);
  }
  return reg;
}

// A segment's UNITS (csrc/brotli_seg_walk.h) are the 16-byte-aligned words of memory that [src, src + len) touches; unit k is the word at
// (src & ~15) + 16 k.
// One PIECE: units [u0, u1) of the segment (u0 < u1 <= its units), each fetched as ONE aligned 16-byte word by load(address, w) -> w[0..4).
// -> the piece's raw register (started with the init value where the piece holds the segment's first byte), and in *behind the segment's bytes
// behind the piece.
template <class Load>
BROTLI_AMD_CRC_HD uint32_t brotli_amd_crc_piece(const uint32_t* t, Load& load, uint64_t src, uint64_t len, uint64_t u0, uint64_t u1, uint64_t* behind) {
  const uint64_t base = src & ~(uint64_t)15, end = src + len;
  uint32_t reg = u0 == 0u ? 0xFFFFFFFFu : 0u;
  for (uint64_t u = u0; u < u1; u++) {
    const uint64_t W = base + 16u * u;
    uint32_t w[4];
    load(W, w);
    reg = brotli_amd_crc_unit(t, reg, w[0], w[1], w[2], w[3], W < src ? (uint32_t)(src - W) : 0u, W + 16u <= end ? 16u : (uint32_t)(end - W));
  }
  const uint64_t stop = base + 16u * u1;
  *behind = stop < end ? end - stop : 0u;
  return reg;
}

// What a piece adds to its segment's digest: the XOR of these over a segment's pieces, in any order, is the segment's standard CRC (a segment
// of no bytes has no piece, and its digest is 0).
BROTLI_AMD_CRC_HD uint32_t brotli_amd_crc_piece_term(uint32_t poly, const uint32_t* pw, uint32_t reg, uint64_t behind) {
  return behind != 0u ? brotli_amd_crc_shift(poly, pw, reg, behind) : reg ^ 0xFFFFFFFFu;
}

#endif  // BROTLI_AMD_CRC_H_
