// brotli_unvarint.h -- LEB128 varints back into elements: the arithmetic of one unit of work and the bookkeeping of one tile, once, for the host
// and the device.
//
// THE TRANSFORM (include/brotli/batch.h has it in full).  A segment of len bytes, a width w (1, 2, 4 or 8), flags and a capacity cap in elements.
// A byte with bit 7 clear ENDS a varint; varint i is the bytes behind the end in front of it (from the segment's first byte for i = 0) up to
// its own end, L_i of them.  Byte j contributes its low 7 bits at bit 7 j of a 64-bit value; what lies at and above bit 64 is dropped.  A
// varint of more than ten bytes is OVERLONG: its element is 0.  With BROTLI_AMD_UNVARINT_ZIGZAG v = (v >> 1) ^ (0 - (v & 1)).  Element i, the
// value truncated to w bytes, goes to dst + i w for i < min(m, cap), m being the number of ends.  Every segment has a result: count = m,
// consumed = the last end's position + 1 (0 where there is none), overlong = the overlong varints among all m.
//
// A UNIT is one aligned 16-byte word of SOURCE memory that [src, src + len) touches (the digests walk sources too); unit k is the word at
// Ws = (src & ~15) + 16 k.  It is fetched with ONE aligned 16-byte load and the bytes that are not the segment's read as 0.  A unit CONTRIBUTES
// the varints that END in it: its `ends` mask has bit i set where byte i of the word is the segment's and has bit 7 clear.
//
// THE VALUE of the varint that ends at byte i of a unit needs that byte and up to ten bytes in front of it, so the unit's word and the word in
// front of it -- the WINDOW, 32 bytes, the unit's at 16 .. 31 -- are enough: ten continuation bytes in front of an end say overlong, and no
// look-back goes further.  A byte in front of the segment's first reads as 0, which ends a varint: nothing reaches back across the segment's
// start.  The window's 7-bit groups are packed once into 224 bits; the varint that ends at byte q is the 7 L bits below bit 7 (q + 1) of them.
//
// STORES.  Element i as ONE store of w bytes where dst + i w is a multiple of w, byte by byte elsewhere; nothing beside the element's bytes.
//
// A TILE is tile_units consecutive units of all segments one after the other.  The index of a unit's first element is the number of ends in
// the segment's units in front of it: a running COUNT with restarts, which is undelta's running sum with a popcount for a sum.  So the three
// phases are undelta's (csrc/brotli_undelta.h), and its pair, combine, cont, nohead, last_piece and carry_in are used as they are:
//   1. the tile's summary: the ends in its last piece, and the two facts;
//   2. the carries: undelta's carry launch itself;
//   3. emit: the running count over the tile's units gives every unit its first index; the unit stores the elements whose ends lie in it, up
//      to cap.  The unit that is its segment's last knows count; consumed is a maximum and overlong a sum over the units, in any order.
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUnvarintHost; tests/tools/unvarint_san.cpp) and the device
// (csrc/brotli_unvarint_kernels.hip); only the cross-lane running count and the atomics are the device's own.  Addresses are integers.
#ifndef BROTLI_AMD_UNVARINT_H_
#define BROTLI_AMD_UNVARINT_H_

#include "brotli/batch.h"       // BrotliAmdUnvarintResult, BROTLI_AMD_UNVARINT_ZIGZAG
#include "brotli_device_abi.h"  // the segment of a launch: BrotliAmdUnvarintSeg
#include "brotli_seg_walk.h"    // the unit count, the search for a unit's segment
#include "brotli_undelta.h"     // the tile's record, the pair and its operator, the facts of a tile; the dword mask
#include "brotli_unshuffle.h"   // the memory helpers

#define BROTLI_AMD_UNVARINT_HD BROTLI_AMD_UNSHUFFLE_HD
#define BROTLI_AMD_UNVARINT_FLAGS BROTLI_AMD_UNVARINT_ZIGZAG   // the flag bits there are
#define BROTLI_AMD_UNVARINT_MAX_CAP ((uint64_t)1 << 56)        // (so that cap w cannot overflow)

// ---- the unit ----
// bit i: byte i of the four has bit 7 set
BROTLI_AMD_UNVARINT_HD uint32_t brotli_amd_unvarint_high_bits(uint32_t d) { return ((((d >> 7) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu; }
// ... of the sixteen
BROTLI_AMD_UNVARINT_HD uint32_t brotli_amd_unvarint_cont(BrotliAmdU4 v) {
  return brotli_amd_unvarint_high_bits(v.x) | (brotli_amd_unvarint_high_bits(v.y) << 4) | (brotli_amd_unvarint_high_bits(v.z) << 8) |
         (brotli_amd_unvarint_high_bits(v.w) << 12);
}
BROTLI_AMD_UNVARINT_HD uint32_t brotli_amd_unvarint_popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(x);
#else
  return (uint32_t)__builtin_popcount(x);
#endif
}

// Unit k of the segment [src, src + len): its word, what is not the segment's as 0; *ends: the bytes of the word that end a varint.
BROTLI_AMD_UNVARINT_HD BrotliAmdU4 brotli_amd_unvarint_fetch(uint64_t src, uint64_t len, uint64_t k, uint32_t* ends) {
  const uint64_t Ws = (src & ~(uint64_t)15) + 16u * k;
  const uint64_t lo = Ws > src ? Ws : src, hi = Ws + 16u < src + len ? Ws + 16u : src + len;   // the word's bytes that are the segment's
  BrotliAmdU4 v = brotli_amd_unshuffle_ld128(Ws);
  uint32_t inside = 0xFFFFu;
  if (lo != Ws || hi != Ws + 16u) {
    const uint32_t blo = (uint32_t)(lo - Ws), bhi = (uint32_t)(hi - Ws);
    v.x &= brotli_amd_undelta_dword_mask(0u, blo, bhi); v.y &= brotli_amd_undelta_dword_mask(1u, blo, bhi);
    v.z &= brotli_amd_undelta_dword_mask(2u, blo, bhi); v.w &= brotli_amd_undelta_dword_mask(3u, blo, bhi);
    inside = ((1u << bhi) - 1u) & ~((1u << blo) - 1u);
  }
  *ends = ~brotli_amd_unvarint_cont(v) & inside;
  return v;
}
// The unit's contribution: the varints that end in it.
BROTLI_AMD_UNVARINT_HD uint64_t brotli_amd_unvarint_total(uint32_t ends) { return brotli_amd_unvarint_popc(ends); }

// ---- the window: the word in front of a unit's (zeros in front of a segment's first unit) and the unit's ----
// the low 7 bits of eight bytes, packed into 56
BROTLI_AMD_UNVARINT_HD uint64_t brotli_amd_unvarint_pack7(uint32_t lo, uint32_t hi) {
  uint64_t x = ((uint64_t)hi << 32) | lo;
  x = (x & 0x007F007F007F007Full) | ((x & 0x7F007F007F007F00ull) >> 1);
  x = (x & 0x00003FFF00003FFFull) | ((x & 0x3FFF00003FFF0000ull) >> 2);
  return (x & 0x000000000FFFFFFFull) | ((x & 0x0FFFFFFF00000000ull) >> 4);
}
struct BrotliAmdUnvarintWindow {
  uint64_t p[4];   // the 7-bit groups of the 32 bytes: byte i's at bit 7 i
  uint32_t cont;   // bit i: byte i has bit 7 set
};
BROTLI_AMD_UNVARINT_HD BrotliAmdUnvarintWindow brotli_amd_unvarint_window(BrotliAmdU4 prev, BrotliAmdU4 cur) {
  const uint64_t c0 = brotli_amd_unvarint_pack7(prev.x, prev.y), c1 = brotli_amd_unvarint_pack7(prev.z, prev.w);
  const uint64_t c2 = brotli_amd_unvarint_pack7(cur.x, cur.y), c3 = brotli_amd_unvarint_pack7(cur.z, cur.w);
  BrotliAmdUnvarintWindow w;
  w.p[0] = c0 | (c1 << 56); w.p[1] = (c1 >> 8) | (c2 << 48); w.p[2] = (c2 >> 16) | (c3 << 40); w.p[3] = c3 >> 24;
  w.cont = brotli_amd_unvarint_cont(prev) | (brotli_amd_unvarint_cont(cur) << 16);
  return w;
}
// the 64 bits from bit `at` on (at + 64 <= 224 + 32)
BROTLI_AMD_UNVARINT_HD uint64_t brotli_amd_unvarint_bits(const BrotliAmdUnvarintWindow& w, uint32_t at) {
  const uint32_t i = at >> 6, s = at & 63u;
  return s ? (w.p[i] >> s) | (w.p[i + 1u] << (64u - s)) : w.p[i];
}
// The bytes of the varint that ends at byte q (16 .. 31) of the window: 1 .. 10, or more than 10 for an overlong one.
BROTLI_AMD_UNVARINT_HD uint32_t brotli_amd_unvarint_length(const BrotliAmdUnvarintWindow& w, uint32_t q) {
  const uint32_t stops = ~w.cont & ((1u << q) - 1u);   // the bytes in front of q that end a varint, or are none of the segment's
  return stops ? q - (31u - (uint32_t)__builtin_clz(stops)) : 32u;
}
// Its value, L (1 .. 10) being its length: the 7 L bits below bit 7 (q + 1); of ten bytes the lowest 64.
BROTLI_AMD_UNVARINT_HD uint64_t brotli_amd_unvarint_value(const BrotliAmdUnvarintWindow& w, uint32_t q, uint32_t L) {
  if (L == 10u) return brotli_amd_unvarint_bits(w, 7u * q - 63u);
  return brotli_amd_unvarint_bits(w, 7u * q - 57u) >> (64u - 7u * L);
}
BROTLI_AMD_UNVARINT_HD uint64_t brotli_amd_unvarint_unzigzag(uint64_t v) { return (v >> 1) ^ ((uint64_t)0 - (v & 1u)); }

// One element: the low `width` bytes of v, little-endian, at address a -- one store where a is a multiple of the width.
BROTLI_AMD_UNVARINT_HD void brotli_amd_unvarint_store(uint64_t a, uint32_t width, uint64_t v) {
  if ((a & (width - 1u)) == 0u) {
#if defined(__HIP_DEVICE_COMPILE__)
    switch (width) {
      case 1u: *(BROTLI_AMD_GLOBAL uint8_t*)a = (uint8_t)v; break;
      case 2u: *(BROTLI_AMD_GLOBAL uint16_t*)a = (uint16_t)v; break;
      case 4u: *(BROTLI_AMD_GLOBAL uint32_t*)a = (uint32_t)v; break;
      default: *(BROTLI_AMD_GLOBAL uint64_t*)a = v; break;
    }
#else
    memcpy(reinterpret_cast<void*>((uintptr_t)a), &v, width);   // (little-endian hosts)
#endif
    return;
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t j = 0; j < 8u; j++)
    if (j < width) *(BROTLI_AMD_GLOBAL uint8_t*)(uintptr_t)(a + j) = (uint8_t)(v >> (8u * j));
}

// What a unit adds to its segment's result beside its ends.
struct BrotliAmdUnvarintPart {
  uint64_t consumed;   // the position behind its last end (0: it has no end)
  uint32_t overlong;
};

// Unit k of the segment sg, `cur` and `ends` as fetched, `prev` the word of unit k - 1 as fetched (zeros for k == 0), `first` the index of the
// first varint that ends in the unit: the elements first .. in front of sg.cap are stored.  (A width that is none: nothing is written.)
BROTLI_AMD_UNVARINT_HD BrotliAmdUnvarintPart brotli_amd_unvarint_emit(const BrotliAmdUnvarintSeg& sg, uint64_t k, BrotliAmdU4 prev, BrotliAmdU4 cur,
                                                                      uint32_t ends, uint64_t first) {
  BrotliAmdUnvarintPart part = {0u, 0u};
  if (ends == 0u) return part;
  const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst;
  const uint64_t Ws = (src & ~(uint64_t)15) + 16u * k;
  part.consumed = Ws + (32u - (uint32_t)__builtin_clz(ends)) - src;
  const BrotliAmdUnvarintWindow w = brotli_amd_unvarint_window(prev, cur);
  const bool known = brotli_amd_unshuffle_width_ok(sg.width);
  uint64_t at = first;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < 16u; i++) {
    if (((ends >> i) & 1u) == 0u) continue;
    const uint32_t L = brotli_amd_unvarint_length(w, 16u + i);
    if (L > 10u) part.overlong++;
    if (at < sg.cap && known) {
      uint64_t v = 0u;
      if (L <= 10u) {
        v = brotli_amd_unvarint_value(w, 16u + i, L);
        if (sg.flags & BROTLI_AMD_UNVARINT_ZIGZAG) v = brotli_amd_unvarint_unzigzag(v);
      }
      brotli_amd_unvarint_store(dst + at * sg.width, sg.width, v);
    }
    at++;
  }
  return part;
}

// ---- the three phases over host memory, tile by tile (the device replaces the loops over a tile's units by its lanes) ----
// phase 1 of the tile [t0, t1) (t1: the tile's end or the end of all units): its summary
inline BrotliAmdUndeltaTile brotli_amd_unvarint_host_summary(const BrotliAmdUnvarintSeg* segs, const uint64_t* pre, uint32_t n, uint64_t t0, uint64_t t1) {
  uint32_t j = 0;
  const uint64_t from = brotli_amd_undelta_last_piece(pre, n, t0, t1, &j);
  BrotliAmdUndeltaTile s = {0u, brotli_amd_undelta_cont(pre, n, t0), brotli_amd_undelta_nohead(pre[j], t0)};
  for (uint64_t g = from; g < t1; g++) {
    uint32_t ends = 0;
    (void)brotli_amd_unvarint_fetch((uint64_t)(uintptr_t)segs[j].src, segs[j].len, g - pre[j], &ends);
    s.sum += brotli_amd_unvarint_total(ends);
  }
  return s;
}
// phase 3 of the tile [t0, t1) with its carry-in; results[0..n) start as zeros
inline void brotli_amd_unvarint_host_emit(const BrotliAmdUnvarintSeg* segs, const uint64_t* pre, uint32_t n, uint64_t t0, uint64_t t1, uint64_t carry_in,
                                          BrotliAmdUnvarintResult* results) {
  BrotliAmdUndeltaPair run = {carry_in, 0u};
  for (uint64_t g = t0; g < t1; g++) {
    const uint32_t j = brotli_amd_seg_find(pre, n, g);
    const uint64_t src = (uint64_t)(uintptr_t)segs[j].src, k = g - pre[j];
    uint32_t ends = 0, none = 0;
    const BrotliAmdU4 cur = brotli_amd_unvarint_fetch(src, segs[j].len, k, &ends);
    const BrotliAmdU4 prev = k ? brotli_amd_unvarint_fetch(src, segs[j].len, k - 1u, &none) : BrotliAmdU4{0u, 0u, 0u, 0u};
    if (k == 0u) run = BrotliAmdUndeltaPair{0u, 1u};
    const BrotliAmdUnvarintPart part = brotli_amd_unvarint_emit(segs[j], k, prev, cur, ends, run.sum);
    run = brotli_amd_undelta_combine(run, BrotliAmdUndeltaPair{brotli_amd_unvarint_total(ends), 0u});
    if (part.consumed > results[j].consumed) results[j].consumed = part.consumed;
    results[j].overlong += part.overlong;
    if (g + 1u == pre[j + 1u]) results[j].count = run.sum;   // the segment's last unit
  }
}

#endif  // BROTLI_AMD_UNVARINT_H_
