// brotli_bitunshuffle.h -- bit planes back into elements: the arithmetic of one unit of work, once, for the host and the device.
//
// THE TRANSFORM (include/brotli/batch.h states it in the same terms).  A segment of len bytes, a width w (1, 2, 4 or 8) and a block size B in
// elements (0: the whole segment is one block; otherwise a multiple of 8): m = len / w elements.  The elements are cut into BLOCKS of B, at the
// same byte offsets in source and destination: block b starts at element b B and byte o = b B w.  A full block transposes c = B elements, the
// last, shorter one c = (m - b B) rounded down to a multiple of 8 (that can be 0); so the last m % 8 elements and the len % w bytes behind them
// are copied: dst[p] = src[p] for p >= 8 (m / 8) w.  Inside a block, for element i < c, byte j < w and bit k < 8 (bit 0 the least significant):
//     bit k of dst[o + i w + j]  =  bit (i % 8) of src[o + (8 j + k) (c / 8) + i / 8]
// The source of a block is 8 w bit ROWS of c / 8 bytes; row 8 j + k holds bit k of byte j of every element, element i in bit i % 8 of byte i / 8.
// Width 1 is a real transform.  Out of place: no destination range overlaps a source range or another destination range.
//
// A UNIT (csrc/brotli_seg_walk.h) is one aligned 16-byte word of DESTINATION memory that [dst, dst + len) touches; unit k is the word at
// (dst & ~15) + 16 k.  Every word of a segment is of one of three KINDS, decided by brotli_amd_bitunshuffle_word_kind -- the one function the
// kernel and the host hook ask:
//   SLOW   the word is produced by itself (brotli_amd_bitunshuffle_unit), byte by byte, bit by bit: eight single-byte loads a byte inside a
//          block, one for a copied byte.  Correct for every dst % 16, src % 16, w, B, position in a block, the copied tail, and a word that is
//          the first and the last of its segment.  It is the fallback and the edge.
//   FIRST  the word is the first of a FAST ITEM: a run of 32 elements i0 .. i0 + 31 (i0 a multiple of 32) of one block whose dst + o is a
//          multiple of 16 and whose c holds the whole run -- 32 w bytes, the 2 w neighbouring words that hold exactly these elements.  Whoever
//          takes this word takes the whole item (brotli_amd_bitunshuffle_item_w), also where it reaches into the next tile.
//   REST   a later word of a fast item: nothing to do, its FIRST word's taker stores it.
// THE FAST ITEM.  Per byte column j one dword from each of the rows 8 j .. 8 j + 7: the four row bytes at i0 / 8, fetched as the one or two
// aligned dwords around them (a row starts at every residue mod 4) and shifted together.  The eight dwords are four 8 x 8 bit matrices, one a
// byte lane; three rounds of masked swaps (0x0F0F0F0F, 0x33333333, 0x55555555) transpose all four at once, after which dword t holds byte j of
// the elements i0 + t, i0 + 8 + t, i0 + 16 + t, i0 + 24 + t.  The w columns are interleaved by unshuffle's 4 x 4 byte transposes and stored as
// 2 w aligned 16-byte words.  Width 8 goes column by column, so that eight loads are live, not sixty-four.  Neighbouring lanes take
// neighbouring items: a wave's load instruction reads 256 contiguous bytes of one row.
//
// LOADS.  Single bytes of [src, src + len), and aligned dwords that hold one.  STORES.  One aligned 16-byte store where the segment covers the
// word; at the segment's first and last word the edge store of csrc/brotli_seg_walk.h -- never a read-modify-write.
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugBitUnshuffleHost; tests/tools/bitunshuffle_san.cpp) and the
// device (csrc/brotli_bitunshuffle_kernels.hip).  Addresses are integers.
#ifndef BROTLI_AMD_BITUNSHUFFLE_H_
#define BROTLI_AMD_BITUNSHUFFLE_H_

#include <stdint.h>

#include "brotli_unshuffle.h"   // the loads and stores, perm / funnel, the 4 x 4 byte transpose; through it the segment walk and the edge store

#define BROTLI_AMD_BITUNSHUFFLE_HD BROTLI_AMD_UNSHUFFLE_HD

#define BROTLI_AMD_BITUNSHUFFLE_ITEM_ELEMS 32u   // elements of a fast item

enum { BROTLI_AMD_BITUNSHUFFLE_SLOW = 0, BROTLI_AMD_BITUNSHUFFLE_FIRST = 1, BROTLI_AMD_BITUNSHUFFLE_REST = 2 };

BROTLI_AMD_BITUNSHUFFLE_HD constexpr bool brotli_amd_bitunshuffle_block_ok(uint32_t B) { return (B & 7u) == 0u; }
BROTLI_AMD_BITUNSHUFFLE_HD constexpr uint32_t brotli_amd_bitunshuffle_log(uint32_t w) { return w == 1u ? 0u : w == 2u ? 1u : w == 4u ? 2u : 3u; }

// The block of element e (< m) of a segment of m elements cut into blocks of B: *b0 its first element, *c the elements it transposes.
// -> the element behind the block.
BROTLI_AMD_BITUNSHUFFLE_HD uint64_t brotli_amd_bitunshuffle_block(uint64_t m, uint32_t B, uint64_t e, uint64_t* b0, uint64_t* c) {
  if (B == 0u || B >= m) { *b0 = 0u; *c = m & ~(uint64_t)7; return m; }
  const uint64_t b = (e >> 32) == 0u ? (uint64_t)((uint32_t)e / B) : e / B;   // (a 32-bit division wherever it is one)
  const uint64_t at = b * B, left = m - at;
  *b0 = at;
  if (left >= B) { *c = B; return at + B; }
  *c = left & ~(uint64_t)7;
  return m;
}

// THE DECISION: the kind of unit k of the segment.  FIRST: *o is the block's byte offset, *c its transposed elements, *i0 the item's first element
// in the block.
BROTLI_AMD_BITUNSHUFFLE_HD uint32_t brotli_amd_bitunshuffle_word_kind(uint64_t dst, uint64_t len, uint32_t w, uint32_t B, uint64_t k, uint64_t* o, uint64_t* c,
                                                                      uint64_t* i0) {
  const uint32_t LOG = brotli_amd_bitunshuffle_log(w);
  const uint64_t Wd = (dst & ~(uint64_t)15) + 16u * k;
  if (Wd < dst) return BROTLI_AMD_BITUNSHUFFLE_SLOW;          // a first word that begins in front of the segment
  const uint64_t p = Wd - dst, m = len >> LOG;
  if ((p >> LOG) >= m) return BROTLI_AMD_BITUNSHUFFLE_SLOW;   // the left-over bytes
  uint64_t b0, cc;
  (void)brotli_amd_bitunshuffle_block(m, B, p >> LOG, &b0, &cc);
  const uint64_t oo = b0 << LOG;
  if (((dst + oo) & 15u) != 0u) return BROTLI_AMD_BITUNSHUFFLE_SLOW;   // the block's words do not hold whole runs of its elements
  const uint64_t i = (p - oo) >> LOG;                          // (p - oo is a multiple of 16, so of w: the word's first byte is element i's first)
  const uint64_t first = i & ~(uint64_t)(BROTLI_AMD_BITUNSHUFFLE_ITEM_ELEMS - 1u);
  if (first + BROTLI_AMD_BITUNSHUFFLE_ITEM_ELEMS > cc) return BROTLI_AMD_BITUNSHUFFLE_SLOW;   // no whole group of 32 left in the block
  *o = oo; *c = cc; *i0 = first;
  return i == first ? BROTLI_AMD_BITUNSHUFFLE_FIRST : BROTLI_AMD_BITUNSHUFFLE_REST;
}

// ---- the slow unit ----
// byte p (< w m) of the destination of a segment: eight row bytes, a bit of each.  The block of the element is (b0, c).
BROTLI_AMD_BITUNSHUFFLE_HD uint32_t brotli_amd_bitunshuffle_gather(uint64_t src, uint32_t w, uint64_t p, uint64_t b0, uint64_t c) {
  const uint32_t LOG = brotli_amd_bitunshuffle_log(w);
  const uint64_t i = (p >> LOG) - b0, rb = c >> 3;
  const uint32_t j = (uint32_t)p & (w - 1u), bit = (uint32_t)i & 7u;
  uint64_t A = src + (b0 << LOG) + (uint64_t)(8u * j) * rb + (i >> 3);
  uint32_t v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t k = 0; k < 8u; k++, A += rb) v |= ((brotli_amd_unshuffle_ld8(A) >> bit) & 1u) << k;
  return v;
}

// Unit k of a segment, whatever its kind would be: reads and writes as the head of this file says.  (another width: nothing is read or written)
BROTLI_AMD_BITUNSHUFFLE_HD void brotli_amd_bitunshuffle_unit(uint64_t src, uint64_t dst, uint64_t len, uint32_t w, uint32_t B, uint64_t k) {
  if (!brotli_amd_unshuffle_width_ok(w)) return;
  const uint32_t LOG = brotli_amd_bitunshuffle_log(w);
  const uint64_t Wd = (dst & ~(uint64_t)15) + 16u * k;
  const uint64_t lo = Wd > dst ? Wd : dst, hi = Wd + 16u < dst + len ? Wd + 16u : dst + len;   // the word's bytes that are the segment's
  const uint64_t m = len >> LOG, body = (m & ~(uint64_t)7) << LOG;                              // behind `body`: copied bytes
  uint64_t b0 = 0, c = 0, bend = 0;   // the block at hand: elements [b0, bend)
  bool have = false;
  BrotliAmdU4 v = {0u, 0u, 0u, 0u};
  for (uint32_t d = 0; d < 4u; d++) {
    uint32_t x = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t q = 0; q < 4u; q++) {
      const uint64_t a = Wd + 4u * d + q;
      if (a < lo || a >= hi) continue;
      const uint64_t p = a - dst;
      uint32_t byte;
      if (p >= body) {
        byte = brotli_amd_unshuffle_ld8(src + p);
      } else {
        const uint64_t e = p >> LOG;
        if (!have || e >= bend) { bend = brotli_amd_bitunshuffle_block(m, B, e, &b0, &c); have = true; }
        byte = e - b0 < c ? brotli_amd_bitunshuffle_gather(src, w, p, b0, c) : brotli_amd_unshuffle_ld8(src + p);
      }
      x |= byte << (8u * q);
    }
    v.x = d == 0u ? x : v.x; v.y = d == 1u ? x : v.y; v.z = d == 2u ? x : v.z; v.w = d == 3u ? x : v.w;
  }
  if (lo == Wd && hi == Wd + 16u) brotli_amd_unshuffle_st128(Wd, v);
  else brotli_amd_seg_store_edge(Wd, lo, hi, v);
}

// ---- the fast item ----
// eight dwords r[k], four 8 x 8 bit matrices (one a byte lane: row k, column s = bit s of the lane's byte of r[k]), transposed in place: bit k
// of a byte of r[s] becomes what bit s of that byte of r[k] was.  Three rounds of masked swaps; (a & M) | (b & ~M) is one v_bfi_b32.
BROTLI_AMD_BITUNSHUFFLE_HD void brotli_amd_bitunshuffle_swap(uint32_t* a, uint32_t* b, uint32_t sh, uint32_t M) {
  const uint32_t x = *a, y = *b;
  *a = (x & M) | ((y << sh) & ~M);
  *b = ((x >> sh) & M) | (y & ~M);
}
BROTLI_AMD_BITUNSHUFFLE_HD void brotli_amd_bitunshuffle_transpose8(uint32_t* r) {
  brotli_amd_bitunshuffle_swap(&r[0], &r[4], 4u, 0x0F0F0F0Fu); brotli_amd_bitunshuffle_swap(&r[1], &r[5], 4u, 0x0F0F0F0Fu);
  brotli_amd_bitunshuffle_swap(&r[2], &r[6], 4u, 0x0F0F0F0Fu); brotli_amd_bitunshuffle_swap(&r[3], &r[7], 4u, 0x0F0F0F0Fu);
  brotli_amd_bitunshuffle_swap(&r[0], &r[2], 2u, 0x33333333u); brotli_amd_bitunshuffle_swap(&r[1], &r[3], 2u, 0x33333333u);
  brotli_amd_bitunshuffle_swap(&r[4], &r[6], 2u, 0x33333333u); brotli_amd_bitunshuffle_swap(&r[5], &r[7], 2u, 0x33333333u);
  brotli_amd_bitunshuffle_swap(&r[0], &r[1], 1u, 0x55555555u); brotli_amd_bitunshuffle_swap(&r[2], &r[3], 1u, 0x55555555u);
  brotli_amd_bitunshuffle_swap(&r[4], &r[5], 1u, 0x55555555u); brotli_amd_bitunshuffle_swap(&r[6], &r[7], 1u, 0x55555555u);
}

// One byte column of an item: the four bytes at A of eight rows rb bytes apart, each as the aligned dwords around it -- the second one's address
// is the first's where the four bytes do not reach into it, so every dword loaded holds a byte of the row --, transposed: q[t] = the column's byte of elements t, 8 + t,
// 16 + t, 24 + t of the item.
BROTLI_AMD_BITUNSHUFFLE_HD void brotli_amd_bitunshuffle_column(uint64_t A, uint64_t rb, uint32_t* q) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t k = 0; k < 8u; k++, A += rb) {
    const uint64_t D = A & ~(uint64_t)3;
    const uint32_t sh = ((uint32_t)A & 3u) * 8u;
    const uint32_t d0 = brotli_amd_unshuffle_ld32(D);
    const uint32_t d1 = brotli_amd_unshuffle_ld32(sh != 0u ? D + 4u : D);   // (no branch: where the four bytes are one dword, that dword again)
    q[k] = brotli_amd_unshuffle_funnel(d1, d0, sh);
  }
  brotli_amd_bitunshuffle_transpose8(q);
}

// The item of elements i0 .. i0 + 31 of the block at byte offset o with c transposed elements (a FIRST word's *o, *c, *i0): 8 W row runs in,
// 2 W aligned words out.
template <uint32_t W>
BROTLI_AMD_BITUNSHUFFLE_HD void brotli_amd_bitunshuffle_item_w(uint64_t src, uint64_t dst, uint64_t o, uint64_t c, uint64_t i0) {
  const uint64_t rb = c >> 3;
  const uint64_t S = src + o + (i0 >> 3);   // the item's bytes of row 0
  const uint64_t D = dst + o + i0 * W;      // a multiple of 16
  uint32_t O[W <= 2u ? 8u * W : 1u];        // the item's dwords (widths 1 and 2)
  if constexpr (W == 1u) {
    uint32_t q[8], t[4], u[4];
    brotli_amd_bitunshuffle_column(S, rb, q);
    brotli_amd_unshuffle_transpose4(q[0], q[1], q[2], q[3], t);
    brotli_amd_unshuffle_transpose4(q[4], q[5], q[6], q[7], u);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t g = 0; g < 4u; g++) { O[2u * g] = t[g]; O[2u * g + 1u] = u[g]; }
  } else if constexpr (W == 2u) {
    uint32_t q0[8], q1[8];
    brotli_amd_bitunshuffle_column(S, rb, q0);
    brotli_amd_bitunshuffle_column(S + 8u * rb, rb, q1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t s = 0; s < 8u; s += 2u) {
      uint32_t t[4];
      brotli_amd_unshuffle_transpose4(q0[s], q1[s], q0[s + 1u], q1[s + 1u], t);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t g = 0; g < 4u; g++) O[4u * g + s / 2u] = t[g];
    }
  } else {
    // widths 4 and 8: all columns transposed first -- eight loads live at a time --, then the words as soon as their four dwords exist
    uint32_t q[W][8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < W; j++) brotli_amd_bitunshuffle_column(S + (uint64_t)(8u * j) * rb, rb, q[j]);
    if constexpr (W == 4u) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t s = 0; s < 8u; s += 4u) {   // elements 8 g + s .. 8 g + s + 3: word 2 g + s / 4
        uint32_t t[4][4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t i = 0; i < 4u; i++) brotli_amd_unshuffle_transpose4(q[0][s + i], q[1][s + i], q[2][s + i], q[3][s + i], t[i]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t g = 0; g < 4u; g++) brotli_amd_unshuffle_st128(D + 16u * (2u * g + s / 4u), BrotliAmdU4{t[0][g], t[1][g], t[2][g], t[3][g]});
      }
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t s = 0; s < 8u; s += 2u) {   // elements 8 g + s and 8 g + s + 1: word 4 g + s / 2
        uint32_t t0[4], u0[4], t1[4], u1[4];
        brotli_amd_unshuffle_transpose4(q[0][s], q[1][s], q[2][s], q[3][s], t0);
        brotli_amd_unshuffle_transpose4(q[4][s], q[5][s], q[6][s], q[7][s], u0);
        brotli_amd_unshuffle_transpose4(q[0][s + 1u], q[1][s + 1u], q[2][s + 1u], q[3][s + 1u], t1);
        brotli_amd_unshuffle_transpose4(q[4][s + 1u], q[5][s + 1u], q[6][s + 1u], q[7][s + 1u], u1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t g = 0; g < 4u; g++) brotli_amd_unshuffle_st128(D + 16u * (4u * g + s / 2u), BrotliAmdU4{t0[g], u0[g], t1[g], u1[g]});
      }
    }
  }
  if constexpr (W <= 2u)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 2u * W; i++) brotli_amd_unshuffle_st128(D + 16u * i, BrotliAmdU4{O[4u * i], O[4u * i + 1u], O[4u * i + 2u], O[4u * i + 3u]});
}

// ---- the work assignment ----
// The units [ka, kb) of a segment of width W, as ONE taker has them (a lane of the kernel in a tile inside one segment; the host hook): every
// SLOW word by itself, every item whose FIRST word is among them whole -- also where its later words lie behind kb --, no REST word.  Takers of
// disjoint ranges write disjoint bytes, and the takers of all units of a segment write all of it.  -> the fast items taken.
template <uint32_t W>
BROTLI_AMD_BITUNSHUFFLE_HD uint32_t brotli_amd_bitunshuffle_range_w(uint64_t src, uint64_t dst, uint64_t len, uint32_t B, uint64_t ka, uint64_t kb) {
  uint32_t items = 0;
  for (uint64_t k = ka; k < kb;) {
    uint64_t o = 0, c = 0, i0 = 0;
    const uint32_t kind = brotli_amd_bitunshuffle_word_kind(dst, len, W, B, k, &o, &c, &i0);
    if (kind == BROTLI_AMD_BITUNSHUFFLE_FIRST) {
      brotli_amd_bitunshuffle_item_w<W>(src, dst, o, c, i0);
      items++;
      k += 2u * W;   // (its later words)
    } else {
      if (kind == BROTLI_AMD_BITUNSHUFFLE_SLOW) brotli_amd_bitunshuffle_unit(src, dst, len, W, B, k);
      k++;
    }
  }
  return items;
}

// ... of any allowed width (another width: nothing is read or written)
BROTLI_AMD_BITUNSHUFFLE_HD uint32_t brotli_amd_bitunshuffle_range(uint64_t src, uint64_t dst, uint64_t len, uint32_t w, uint32_t B, uint64_t ka, uint64_t kb) {
  switch (w) {
    case 1u: return brotli_amd_bitunshuffle_range_w<1u>(src, dst, len, B, ka, kb);
    case 2u: return brotli_amd_bitunshuffle_range_w<2u>(src, dst, len, B, ka, kb);
    case 4u: return brotli_amd_bitunshuffle_range_w<4u>(src, dst, len, B, ka, kb);
    case 8u: return brotli_amd_bitunshuffle_range_w<8u>(src, dst, len, B, ka, kb);
    default: return 0u;
  }
}

// A SLOT is the 2 W words from unit 2 W s of a segment on: what a lane takes at a time in a tile inside one segment.  Where dst is a multiple of
// 16 and the blocks begin at multiples of 32 elements (B == 0, B a multiple of 32), a slot is exactly one item.  The slots of the units
// [ka, kb) are those from ka / (2 W) to (kb - 1) / (2 W); slot s has of them the units max(2 W s, ka) .. min(2 W (s + 1), kb).
template <uint32_t W>
BROTLI_AMD_BITUNSHUFFLE_HD uint32_t brotli_amd_bitunshuffle_slot_w(uint64_t src, uint64_t dst, uint64_t len, uint32_t B, uint64_t s, uint64_t ka, uint64_t kb) {
  const uint64_t a = 2u * W * s, b = a + 2u * W;
  return brotli_amd_bitunshuffle_range_w<W>(src, dst, len, B, a > ka ? a : ka, b < kb ? b : kb);
}

#endif  // BROTLI_AMD_BITUNSHUFFLE_H_
