// brotli_bitunpack.h -- k-bit fields back into elements: the arithmetic of one unit of work, once, for the host and the device.
//
// THE TRANSFORM (include/brotli/batch.h states it in the same terms).  A segment has source bytes src[0, src_len), a count m of elements, a field
// width k (1 .. 64), an element width w (1, 2, 4 or 8, k <= 8 w) and flags.  The destination is exactly m w bytes: element i is a little-endian
// unsigned integer of w bytes at dst + i w.  The source is read as a string of bits, and element i is the field of bits i k .. i k + k - 1:
//   LSB-first (flags bit 0 clear)            stream bit b is bit b % 8 of src[b / 8] (bit 0 the least significant); the first bit of a field is
//                                            the value's bit 0
//   MSB-first (BROTLI_AMD_BITUNPACK_MSB_FIRST)  stream bit b is bit 7 - b % 8 of src[b / 8]; the first bit of a field is the value's bit k - 1
//   BROTLI_AMD_BITUNPACK_SIGNED              the value is sign-extended from bit k - 1 to 8 w bits; otherwise zero-extended
// k == 8 w is a copy LSB-first and a byte reversal per element MSB-first.  ceil(m k / 8) source bytes are read; the pad bits of the last one and
// the source bytes behind it are ignored.  Out of place: no destination range overlaps a source range or another destination range.
//
// A UNIT (csrc/brotli_seg_walk.h) is one aligned 16-byte word of DESTINATION memory that [dst, dst + m w) touches; unit u is the word at
// (dst & ~15) + 16 u.  Every word of a segment is of one of three KINDS, decided by brotli_amd_bitunpack_word_kind -- the one function the
// kernel and the host hook ask:
//   SLOW   the word is produced by itself (brotli_amd_bitunpack_unit), byte by byte: destination byte p is byte p % w of element p / w, whose
//          field is read as the single bytes that hold it.  Correct for every dst % 16 -- a dst that is no multiple of w included --, src % 16,
//          k, w and flags, and for a word that is the first and the last of its segment.  It is the fallback and the edge.
//   FIRST  the word is the first of a FAST ITEM: the 32 whole elements i0 .. i0 + 31, i0 a multiple of 32, where dst + i0 w is a multiple of
//          16 (so: where dst is one) and i0 + 32 <= m.  Whoever takes this word takes the whole item, also where it reaches into the next tile.
//   REST   a later word of a fast item: nothing to do, its FIRST word's taker stores it.
// THE FAST ITEM (brotli_amd_bitunpack_item<W, K>).  Its source is exactly the 4 k bytes from byte i0 k / 8 on, at any residue mod 4: the k + 1
// aligned dwords around them are shifted together into k dwords -- the one-dword-further load is guarded as brotli_amd_bitunshuffle_column
// guards its own: where the bytes do not reach into it, the dword in front again.  The item is a template on (W, K), so every dword index and
// every shift of the 32 fields is a constant: a field is one funnel shift of two neighbouring dwords and a mask, for K > 32 two of them (it may
// span three dwords).  MSB-first the dwords are byte-swapped first, which makes the stream big-endian dwords, and the fields are cut from the
// top.  Fields of more than 32 bits go in two halves of 16 elements, so that 33 dwords are live at a time and not 65.  The elements are put
// together W bytes each and stored as 2 W aligned 16-byte words, each as soon as its four dwords exist.  There is
// an item for every valid (W, K) -- 120 pairs --, both bit orders and both extensions.  Neighbouring lanes take neighbouring items: one load
// instruction of a wave reads 64 dwords 4 k bytes apart.
//
// LOADS.  Single bytes of [src, src + ceil(m k / 8)), and aligned dwords that hold one of them.  STORES.  One aligned 16-byte store where the
// segment covers the word; at the segment's first and last word the edge store of csrc/brotli_seg_walk.h -- never a read-modify-write.
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugBitUnpackHost; tests/tools/bitunpack_san.cpp) and the device
// (csrc/brotli_bitunpack_kernels.hip).  Addresses are integers.
#ifndef BROTLI_AMD_BITUNPACK_H_
#define BROTLI_AMD_BITUNPACK_H_

#include <stdint.h>

#include "brotli_unshuffle.h"   // the loads and stores, perm / funnel; through it the segment walk and the edge store

#define BROTLI_AMD_BITUNPACK_HD BROTLI_AMD_UNSHUFFLE_HD

#define BROTLI_AMD_BITUNPACK_ITEM_ELEMS 32u   // elements of a fast item
#define BROTLI_AMD_BITUNPACK_FLAG_MSB 1u      // (batch.h: BROTLI_AMD_BITUNPACK_MSB_FIRST)
#define BROTLI_AMD_BITUNPACK_FLAG_SIGNED 2u   // (batch.h: BROTLI_AMD_BITUNPACK_SIGNED)
#define BROTLI_AMD_BITUNPACK_FLAGS 3u         // the known flag bits
#define BROTLI_AMD_BITUNPACK_MAX_COUNT ((uint64_t)1 << 56)   // elements of a segment at the most: neither m k nor m w overflows

#if defined(__HIP_DEVICE_COMPILE__)
#define BROTLI_AMD_BITUNPACK_UNROLL _Pragma("unroll")
#else
#define BROTLI_AMD_BITUNPACK_UNROLL
#endif

enum { BROTLI_AMD_BITUNPACK_SLOW = 0, BROTLI_AMD_BITUNPACK_FIRST = 1, BROTLI_AMD_BITUNPACK_REST = 2 };

BROTLI_AMD_BITUNPACK_HD constexpr uint32_t brotli_amd_bitunpack_log(uint32_t w) { return w == 1u ? 0u : w == 2u ? 1u : w == 4u ? 2u : 3u; }
// a field width, an element width and flags that go together
BROTLI_AMD_BITUNPACK_HD constexpr bool brotli_amd_bitunpack_shape_ok(uint32_t k, uint32_t w, uint32_t flags) {
  return brotli_amd_unshuffle_width_ok(w) && k >= 1u && k <= 8u * w && (flags & ~BROTLI_AMD_BITUNPACK_FLAGS) == 0u;
}
// the source bytes that m fields of k bits are read from (m <= BROTLI_AMD_BITUNPACK_MAX_COUNT)
BROTLI_AMD_BITUNPACK_HD constexpr uint64_t brotli_amd_bitunpack_src_bytes(uint64_t m, uint32_t k) { return (m * k + 7u) >> 3; }
// what a segment table's `param` holds: k | flags << 8
BROTLI_AMD_BITUNPACK_HD constexpr uint32_t brotli_amd_bitunpack_param(uint32_t k, uint32_t flags) { return k | flags << 8; }

// THE DECISION: the kind of unit u of a segment of m elements of width w at dst.  FIRST: *i0 is the item's first element.
BROTLI_AMD_BITUNPACK_HD uint32_t brotli_amd_bitunpack_word_kind(uint64_t dst, uint64_t m, uint32_t w, uint64_t u, uint64_t* i0) {
  if ((dst & 15u) != 0u) return BROTLI_AMD_BITUNPACK_SLOW;   // no word holds whole runs of 32 / (2 w) elements from a multiple of 32 on
  const uint64_t i = (16u * u) >> brotli_amd_bitunpack_log(w);   // the word's first byte is element i's first
  const uint64_t first = i & ~(uint64_t)(BROTLI_AMD_BITUNPACK_ITEM_ELEMS - 1u);
  if (first + BROTLI_AMD_BITUNPACK_ITEM_ELEMS > m) return BROTLI_AMD_BITUNPACK_SLOW;   // no whole group of 32 left
  *i0 = first;
  return i == first ? BROTLI_AMD_BITUNPACK_FIRST : BROTLI_AMD_BITUNPACK_REST;
}

// ---- the slow unit ----
// Element i of the segment, extended to 64 bits: the nb <= 9 single bytes that hold its field, one after the other.
BROTLI_AMD_BITUNPACK_HD uint64_t brotli_amd_bitunpack_value(uint64_t src, uint64_t i, uint32_t k, uint32_t flags) {
  const uint64_t bit = i * k;
  const uint64_t A = src + (bit >> 3);
  const uint32_t off = (uint32_t)bit & 7u, nb = (off + k + 7u) >> 3;
  uint64_t v = 0;
  if ((flags & BROTLI_AMD_BITUNPACK_FLAG_MSB) == 0u) {
    // byte t holds the field's bits from 8 t - off on
    v = (uint64_t)brotli_amd_unshuffle_ld8(A) >> off;
    for (uint32_t t = 1; t < nb; t++) v |= (uint64_t)brotli_amd_unshuffle_ld8(A + t) << (8u * t - off);   // (8 t - off <= 63: t == 8 only where off != 0)
  } else {
    // the bytes as one big-endian number, the field r bits above its end: the last byte brings 8 - r bits (what falls off the top is in front
    // of the field)
    const uint32_t r = 8u * nb - off - k;
    for (uint32_t t = 0; t + 1u < nb; t++) v = (v << 8) | brotli_amd_unshuffle_ld8(A + t);
    v = (v << (8u - r)) | (brotli_amd_unshuffle_ld8(A + nb - 1u) >> r);
  }
  if (k < 64u) {
    v &= ((uint64_t)1 << k) - 1u;
    if ((flags & BROTLI_AMD_BITUNPACK_FLAG_SIGNED) != 0u) { const uint64_t s = (uint64_t)1 << (k - 1u); v = (v ^ s) - s; }
  }
  return v;
}

// Unit u of a segment, whatever its kind would be: reads and writes as the head of this file says.  (a shape that is not ok: nothing is read
// or written)
BROTLI_AMD_BITUNPACK_HD void brotli_amd_bitunpack_unit(uint64_t src, uint64_t dst, uint64_t m, uint32_t w, uint32_t k, uint32_t flags, uint64_t u) {
  if (!brotli_amd_bitunpack_shape_ok(k, w, flags)) return;
  const uint32_t LOG = brotli_amd_bitunpack_log(w);
  const uint64_t len = m << LOG;
  const uint64_t Wd = (dst & ~(uint64_t)15) + 16u * u;
  const uint64_t lo = Wd > dst ? Wd : dst, hi = Wd + 16u < dst + len ? Wd + 16u : dst + len;   // the word's bytes that are the segment's
  uint64_t at = ~(uint64_t)0, val = 0;   // the element at hand
  BrotliAmdU4 v = {0u, 0u, 0u, 0u};
  for (uint32_t d = 0; d < 4u; d++) {
    uint32_t x = 0;
    BROTLI_AMD_BITUNPACK_UNROLL
    for (uint32_t q = 0; q < 4u; q++) {
      const uint64_t a = Wd + 4u * d + q;
      if (a < lo || a >= hi) continue;
      const uint64_t p = a - dst, e = p >> LOG;
      if (e != at) { val = brotli_amd_bitunpack_value(src, e, k, flags); at = e; }
      x |= ((uint32_t)(val >> (8u * ((uint32_t)p & (w - 1u)))) & 0xFFu) << (8u * q);
    }
    v.x = d == 0u ? x : v.x; v.y = d == 1u ? x : v.y; v.z = d == 2u ? x : v.z; v.w = d == 3u ? x : v.w;
  }
  if (lo == Wd && hi == Wd + 16u) brotli_amd_unshuffle_st128(Wd, v);
  else brotli_amd_seg_store_edge(Wd, lo, hi, v);
}

// ---- the fast item ----
// n (1 .. 32) bits from bit P on of the LSB-first bit string in the dwords d: bit b is bit b % 32 of d[b / 32].  (P and n are constants where
// the loops around are unrolled, and d[P / 32 + 1] is touched only where the bits reach into it)
BROTLI_AMD_BITUNPACK_HD uint32_t brotli_amd_bitunpack_bits_lsb(const uint32_t* d, uint32_t P, uint32_t n) {
  const uint32_t q = P >> 5, off = P & 31u;
  uint32_t x = d[q] >> off;
  if (off + n > 32u) x |= d[q + 1u] << (32u - off);
  return n < 32u ? x & ((1u << n) - 1u) : x;
}
// ... of the MSB-first bit string in the byte-swapped dwords D: bit b is bit 31 - b % 32 of D[b / 32]; the first bit is the result's bit n - 1
BROTLI_AMD_BITUNPACK_HD uint32_t brotli_amd_bitunpack_bits_msb(const uint32_t* D, uint32_t P, uint32_t n) {
  const uint32_t q = P >> 5, off = P & 31u;
  uint32_t x;
  if (off + n <= 32u) x = D[q] >> (32u - off - n);
  else x = (D[q] << (off + n - 32u)) | (D[q + 1u] >> (64u - off - n));
  return n < 32u ? x & ((1u << n) - 1u) : x;
}

// the field of K bits from bit P on of an item's dwords, extended to 64 bits: *lo and *hi
template <uint32_t K, bool MSB>
BROTLI_AMD_BITUNPACK_HD void brotli_amd_bitunpack_field(const uint32_t* d, uint32_t P, bool is_signed, uint32_t* lo, uint32_t* hi) {
  if constexpr (K <= 32u) {
    const uint32_t s = is_signed ? 1u << (K - 1u) : 0u;
    const uint32_t x = ((MSB ? brotli_amd_bitunpack_bits_msb(d, P, K) : brotli_amd_bitunpack_bits_lsb(d, P, K)) ^ s) - s;
    *lo = x;
    *hi = is_signed ? (uint32_t)((int32_t)x >> 31) : 0u;
  } else {
    const uint32_t s = (K < 64u && is_signed) ? 1u << ((K - 33u) & 31u) : 0u;
    uint32_t h;
    if constexpr (MSB) { h = brotli_amd_bitunpack_bits_msb(d, P, K - 32u); *lo = brotli_amd_bitunpack_bits_msb(d, P + K - 32u, 32u); }
    else { *lo = brotli_amd_bitunpack_bits_lsb(d, P, 32u); h = brotli_amd_bitunpack_bits_lsb(d, P + 32u, K - 32u); }
    *hi = (h ^ s) - s;
  }
}

// The item of elements i0 .. i0 + 31 (a FIRST word's *i0) of fields of K bits into elements of W bytes: K + 1 aligned dwords in, 2 W aligned
// words out.
template <uint32_t W, uint32_t K, bool MSB>
BROTLI_AMD_BITUNPACK_HD void brotli_amd_bitunpack_item_order(uint64_t src, uint64_t dst, uint64_t i0, bool is_signed) {
  static_assert(K >= 1u && K <= 8u * W, "a field fits its element");
  const uint64_t S = src + (i0 >> 5) * (4u * K);   // the item's 4 K bytes
  const uint64_t A = S & ~(uint64_t)3;
  const uint32_t sh = ((uint32_t)S & 3u) * 8u;
  const uint64_t D = dst + i0 * W;   // a multiple of 16
  constexpr uint32_t PER = 16u / W;  // elements of a word
  // Fields of more than 32 bits go in two halves of 16 elements, so that at the most 33 dwords are live and not 65: half h holds the bits from
  // 16 K h on, which lie in the item's dwords Q0 .. Q1 (for an odd K the second half begins in the middle of one).
  constexpr uint32_t HALVES = K > 32u ? 2u : 1u, E = 32u / HALVES;
  BROTLI_AMD_BITUNPACK_UNROLL
  for (uint32_t h = 0; h < HALVES; h++) {
    const uint32_t P0 = h * E * K, Q0 = P0 >> 5, Q1 = (P0 + E * K - 1u) >> 5, N = Q1 - Q0 + 1u;
    uint32_t d[(E * K + 31u) / 32u + 1u];
    {
      uint32_t raw[(E * K + 31u) / 32u + 2u];
      BROTLI_AMD_BITUNPACK_UNROLL
      for (uint32_t q = 0; q < N; q++) raw[q] = brotli_amd_unshuffle_ld32(A + 4u * (Q0 + q));
      // (no branch: where the item's bytes end with its dword K - 1, that dword again)
      raw[N] = brotli_amd_unshuffle_ld32(Q1 + 1u < K || sh != 0u ? A + 4u * (Q1 + 1u) : A + 4u * Q1);
      BROTLI_AMD_BITUNPACK_UNROLL
      for (uint32_t q = 0; q < N; q++) {
        const uint32_t x = brotli_amd_unshuffle_funnel(raw[q + 1u], raw[q], sh);
        d[q] = MSB ? brotli_amd_unshuffle_perm(0u, x, 0x00010203u) : x;
      }
    }
    BROTLI_AMD_BITUNPACK_UNROLL
    for (uint32_t g = 0; g < E / PER; g++) {
      uint32_t o[4] = {0u, 0u, 0u, 0u};
      BROTLI_AMD_BITUNPACK_UNROLL
      for (uint32_t t = 0; t < PER; t++) {
        uint32_t lo, hi;
        brotli_amd_bitunpack_field<K, MSB>(d, (P0 & 31u) + (g * PER + t) * K, is_signed, &lo, &hi);
        if constexpr (W == 1u) o[t >> 2] |= (lo & 0xFFu) << (8u * (t & 3u));
        else if constexpr (W == 2u) o[t >> 1] |= (lo & 0xFFFFu) << (16u * (t & 1u));
        else if constexpr (W == 4u) o[t] = lo;
        else { o[2u * t] = lo; o[2u * t + 1u] = hi; }
      }
      brotli_amd_unshuffle_st128(D + 16u * (h * (E / PER) + g), BrotliAmdU4{o[0], o[1], o[2], o[3]});
    }
  }
}
template <uint32_t W, uint32_t K>
BROTLI_AMD_BITUNPACK_HD void brotli_amd_bitunpack_item(uint64_t src, uint64_t dst, uint64_t i0, uint32_t flags) {
  const bool is_signed = (flags & BROTLI_AMD_BITUNPACK_FLAG_SIGNED) != 0u;
  if ((flags & BROTLI_AMD_BITUNPACK_FLAG_MSB) != 0u) brotli_amd_bitunpack_item_order<W, K, true>(src, dst, i0, is_signed);
  else brotli_amd_bitunpack_item_order<W, K, false>(src, dst, i0, is_signed);
}

// ---- the work assignment ----
// The FAST ITEMS among the units [ka, kb) of a segment of fields of K bits and elements of W bytes, as ONE taker has them: every item whose
// FIRST word is among them whole -- also where its later words lie behind kb --, no REST word by itself.  -> the items taken.
template <uint32_t W, uint32_t K>
BROTLI_AMD_BITUNPACK_HD uint32_t brotli_amd_bitunpack_items_wk(uint64_t src, uint64_t dst, uint64_t m, uint32_t flags, uint64_t ka, uint64_t kb) {
  uint32_t items = 0;
  for (uint64_t u = ka; u < kb;) {
    uint64_t i0 = 0;
    if (brotli_amd_bitunpack_word_kind(dst, m, W, u, &i0) == BROTLI_AMD_BITUNPACK_FIRST) {
      brotli_amd_bitunpack_item<W, K>(src, dst, i0, flags);
      items++;
      u += 2u * W;   // (its later words)
    } else {
      u++;
    }
  }
  return items;
}
// The SLOW WORDS among the units [ka, kb), each by itself.
BROTLI_AMD_BITUNPACK_HD void brotli_amd_bitunpack_slow_words(uint64_t src, uint64_t dst, uint64_t m, uint32_t w, uint32_t k, uint32_t flags, uint64_t ka, uint64_t kb) {
  for (uint64_t u = ka; u < kb; u++) {
    uint64_t i0 = 0;
    if (brotli_amd_bitunpack_word_kind(dst, m, w, u, &i0) == BROTLI_AMD_BITUNPACK_SLOW) brotli_amd_bitunpack_unit(src, dst, m, w, k, flags, u);
  }
}
// The units [ka, kb) of a segment as one taker has them: the items and the slow words above.  Takers of disjoint ranges write disjoint bytes,
// and the takers of all units of a segment write all of it.  -> the fast items taken.
template <uint32_t W, uint32_t K>
BROTLI_AMD_BITUNPACK_HD uint32_t brotli_amd_bitunpack_range_wk(uint64_t src, uint64_t dst, uint64_t m, uint32_t flags, uint64_t ka, uint64_t kb) {
  const uint32_t items = brotli_amd_bitunpack_items_wk<W, K>(src, dst, m, flags, ka, kb);
  brotli_amd_bitunpack_slow_words(src, dst, m, W, K, flags, ka, kb);
  return items;
}

// f.template operator()<W, K>() for the one valid pair (w, k): the switch that a tile inside one segment goes through once.  (an invalid pair:
// f is not called)
#define BROTLI_AMD_BITUNPACK_CASE(Kc) case Kc: if constexpr (Kc <= 8u * W) f.template operator()<W, Kc>(); break;
#define BROTLI_AMD_BITUNPACK_CASE8(B) \
  BROTLI_AMD_BITUNPACK_CASE(B + 1u) BROTLI_AMD_BITUNPACK_CASE(B + 2u) BROTLI_AMD_BITUNPACK_CASE(B + 3u) BROTLI_AMD_BITUNPACK_CASE(B + 4u) \
  BROTLI_AMD_BITUNPACK_CASE(B + 5u) BROTLI_AMD_BITUNPACK_CASE(B + 6u) BROTLI_AMD_BITUNPACK_CASE(B + 7u) BROTLI_AMD_BITUNPACK_CASE(B + 8u)
template <uint32_t W, class F>
BROTLI_AMD_BITUNPACK_HD void brotli_amd_bitunpack_for_k(uint32_t k, F f) {
  switch (k) {
    BROTLI_AMD_BITUNPACK_CASE8(0u) BROTLI_AMD_BITUNPACK_CASE8(8u) BROTLI_AMD_BITUNPACK_CASE8(16u) BROTLI_AMD_BITUNPACK_CASE8(24u)
    BROTLI_AMD_BITUNPACK_CASE8(32u) BROTLI_AMD_BITUNPACK_CASE8(40u) BROTLI_AMD_BITUNPACK_CASE8(48u) BROTLI_AMD_BITUNPACK_CASE8(56u)
    default: break;
  }
}
#undef BROTLI_AMD_BITUNPACK_CASE8
#undef BROTLI_AMD_BITUNPACK_CASE
template <class F>
BROTLI_AMD_BITUNPACK_HD void brotli_amd_bitunpack_for_wk(uint32_t w, uint32_t k, F f) {
  switch (w) {
    case 1u: brotli_amd_bitunpack_for_k<1u>(k, f); break;
    case 2u: brotli_amd_bitunpack_for_k<2u>(k, f); break;
    case 4u: brotli_amd_bitunpack_for_k<4u>(k, f); break;
    case 8u: brotli_amd_bitunpack_for_k<8u>(k, f); break;
    default: break;
  }
}

// A SLOT is the 2 w words from unit 2 w s of a segment on: what a lane takes at a time in a tile inside one segment.  Where dst is a multiple of
// 16 a slot in front of the last m % 32 elements is exactly one item.  The slots of the units [ka, kb) are those from ka / (2 w) to
// (kb - 1) / (2 w); slot s has of them the units max(2 w s, ka) .. min(2 w (s + 1), kb).
template <uint32_t W, uint32_t K>
BROTLI_AMD_BITUNPACK_HD uint32_t brotli_amd_bitunpack_slot_wk(uint64_t src, uint64_t dst, uint64_t m, uint32_t flags, uint64_t s, uint64_t ka, uint64_t kb) {
  const uint64_t a = 2u * W * s, b = a + 2u * W;
  return brotli_amd_bitunpack_range_wk<W, K>(src, dst, m, flags, a > ka ? a : ka, b < kb ? b : kb);
}
// ... of its fast item alone (the kernel: its slow words are taken in front of the switch, so that the slow unit is there once)
template <uint32_t W, uint32_t K>
BROTLI_AMD_BITUNPACK_HD uint32_t brotli_amd_bitunpack_slot_items_wk(uint64_t src, uint64_t dst, uint64_t m, uint32_t flags, uint64_t s, uint64_t ka, uint64_t kb) {
  const uint64_t a = 2u * W * s, b = a + 2u * W;
  return brotli_amd_bitunpack_items_wk<W, K>(src, dst, m, flags, a > ka ? a : ka, b < kb ? b : kb);
}

// Slot s of any valid shape (another: nothing is read or written) -> the fast items taken
struct BrotliAmdBitUnpackSlot {
  uint64_t src, dst, m; uint32_t flags; uint64_t s, ka, kb; uint32_t* items;
  template <uint32_t W, uint32_t K> BROTLI_AMD_BITUNPACK_HD void operator()() const { *items = brotli_amd_bitunpack_slot_wk<W, K>(src, dst, m, flags, s, ka, kb); }
};
BROTLI_AMD_BITUNPACK_HD uint32_t brotli_amd_bitunpack_slot(uint64_t src, uint64_t dst, uint64_t m, uint32_t w, uint32_t k, uint32_t flags, uint64_t s, uint64_t ka,
                                                           uint64_t kb) {
  uint32_t items = 0;
  if ((flags & ~BROTLI_AMD_BITUNPACK_FLAGS) == 0u) brotli_amd_bitunpack_for_wk(w, k, BrotliAmdBitUnpackSlot{src, dst, m, flags, s, ka, kb, &items});
  return items;
}

// One word of a tile of SEVERAL segments -- unit u of its segment, the tile holding the segment's units [ka, kb) --, taken by itself whatever
// its kind: a lane there has a segment of its own, and with it a k of its own, so no item's code can be chosen for the wave.  The word that
// would be an item's FIRST also takes the item's words from kb on, which the next tile leaves to it as REST words; a word that would be a REST
// word is left alone where its FIRST word lies in front of ka.  So the rule of the ranges holds here too.
BROTLI_AMD_BITUNPACK_HD void brotli_amd_bitunpack_word_alone(uint64_t src, uint64_t dst, uint64_t m, uint32_t w, uint32_t k, uint32_t flags, uint64_t u, uint64_t ka,
                                                             uint64_t kb) {
  if (!brotli_amd_bitunpack_shape_ok(k, w, flags)) return;
  uint64_t i0 = 0;
  const uint32_t kind = brotli_amd_bitunpack_word_kind(dst, m, w, u, &i0);
  if (kind == BROTLI_AMD_BITUNPACK_SLOW) { brotli_amd_bitunpack_unit(src, dst, m, w, k, flags, u); return; }
  const uint64_t f = (i0 << brotli_amd_bitunpack_log(w)) >> 4;   // the item's FIRST word
  if (f < ka) return;                                           // (the tile in front has it)
  brotli_amd_bitunpack_unit(src, dst, m, w, k, flags, u);
  if (kind == BROTLI_AMD_BITUNPACK_FIRST)
    for (uint64_t x = u + 1u; x < u + 2u * w; x++) if (x >= kb) brotli_amd_bitunpack_unit(src, dst, m, w, k, flags, x);
}

#endif  // BROTLI_AMD_BITUNPACK_H_
