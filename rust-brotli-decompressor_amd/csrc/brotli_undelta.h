// brotli_undelta.h -- running sums of deltas back into values: the arithmetic of one unit of work and the bookkeeping of one tile, once, for the
// host and the device.
//
// THE TRANSFORM.  A segment of len bytes and a width w (1, 2, 4 or 8): m = len / w elements, read as little-endian unsigned integers of w bytes,
// and r = len % w bytes left over.  For k < m
//     dst_elem[k] = (src_elem[0] + ... + src_elem[k]) mod 2^(8 w)
// and the r left-over bytes behind the last whole element are copied unchanged (unshuffle's rule).  Width 1 is a running sum of bytes.
//
// A UNIT is one aligned 16-byte word of DESTINATION memory that [dst, dst + len) touches, as in csrc/brotli_unshuffle.h; unit k is the word at
// Wd = (dst & ~15) + 16 k, and its byte 0 is position p0 = Wd - dst of the segment (negative in a first unit that starts inside its word).
//
// WHICH ELEMENTS.  A unit CONTRIBUTES the elements that START in it: its SLOTS i = 0 .. 16 / w - 1 are the elements eb + i, eb = ceil(p0 / w),
// which start at byte off0 + i w of the word, off0 = eb w - p0 in [0, w).  A slot counts where 0 <= eb + i < m; the others read as 0.  So every
// element is counted exactly once, whatever dst % w is.  The slots' source bytes are the 16 bytes at src + eb w (any alignment): the one or two
// aligned 16-byte words around them, each loaded only where it holds a wanted byte and shifted together in registers.
// With off0 != 0 the word's first off0 bytes are the HIGH bytes of the element eb - 1, which started in the unit before -- and whose value is
// exactly the unit's carry-in (the sum of every element that started in front of the unit); the last slot hangs off0 bytes over the word's end,
// and the next unit writes those.
//
// A unit's work:  v = fetch (the slots, what does not count zeroed);  total(v) = its contribution;  finish(v, carry) = the running sums inside the
// word on top of the carry, the straddling element's bytes in front, the left-over bytes as they are, and the stores.
// LOADS stay inside the 16-byte-aligned span around [src, src + len).  STORES: one aligned 16-byte store where the segment covers the word; at
// the segment's first and last word aligned dwords and single bytes of [dst, dst + len) only -- never a read-modify-write.
// IN PLACE (dst == src, a multiple of w): off0 == 0 and src + eb w == Wd, so a unit reads exactly the bytes of the word it writes.
//
// A TILE is tile_units consecutive units of all segments one after the other (pre[]: the units in front of each segment).  Three phases, each
// complete before the next begins, so nothing ever waits for a neighbour:
//   1. the tile's summary: the sum of the contributions of its LAST PIECE -- the units of the segment still open at the tile's end, from
//      max(that segment's first unit, the tile's first) on --, and two facts: cont (the tile's first unit continues a segment begun earlier)
//      and nohead (no segment starts in the tile; nohead implies cont);
//   2. the carries: carry_out[t] = nohead[t] ? carry_in[t] + sum[t] : sum[t];  carry_in[t + 1] = cont[t + 1] ? carry_out[t] : 0;
//   3. apply: a segmented running sum of the contributions over the tile's units (a segment's first unit restarts from 0, the tile's first
//      starts from carry_in) gives every unit its carry; finish.
// Sums are kept in 64 bits and truncated to w bytes where they are used.
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUndeltaHost; tests/tools/undelta_san.cpp) and the device
// (csrc/brotli_undelta_kernels.hip); only the cross-lane running sum is the device's own.  Addresses are integers.
#ifndef BROTLI_AMD_UNDELTA_H_
#define BROTLI_AMD_UNDELTA_H_

#include "brotli_device_abi.h"  // the segment of a launch: BrotliAmdUnshuffleSeg (src, dst, len, width)
#include "brotli_seg_walk.h"    // the unit count, the search for a unit's segment
#include "brotli_unshuffle.h"   // the memory and register helpers

#define BROTLI_AMD_UNDELTA_HD BROTLI_AMD_UNSHUFFLE_HD

// what phase 1 leaves of a tile
struct BrotliAmdUndeltaTile {
  uint64_t sum;      // of the contributions of the tile's last piece
  uint32_t cont;     // the tile's first unit is not its segment's first
  uint32_t nohead;   // no segment's first unit lies in the tile
};

// ---- running sums with restarts: the pair (sum since the last restart, was there a restart) and its associative operator ----
struct BrotliAmdUndeltaPair { uint64_t sum; uint32_t head; };
// a, then b
BROTLI_AMD_UNDELTA_HD BrotliAmdUndeltaPair brotli_amd_undelta_combine(BrotliAmdUndeltaPair a, BrotliAmdUndeltaPair b) {
  return BrotliAmdUndeltaPair{b.head ? b.sum : a.sum + b.sum, a.head | b.head};
}
// phase 2's element of a tile: carry_out[t] = combine(.. carry_out[t - 1] .., this).sum
BROTLI_AMD_UNDELTA_HD BrotliAmdUndeltaPair brotli_amd_undelta_tile_pair(BrotliAmdUndeltaTile s) { return BrotliAmdUndeltaPair{s.sum, s.nohead ? 0u : 1u}; }
BROTLI_AMD_UNDELTA_HD uint64_t brotli_amd_undelta_carry_in(uint64_t carry_out_before, BrotliAmdUndeltaTile s) { return s.cont ? carry_out_before : 0u; }

// ---- a tile's part [lo, hi) among the segments whose prefix sum is pre[0..count] (the whole tile, or what one chunk of segments holds of it) ----
// the first unit of the part's last piece, and that piece's segment
BROTLI_AMD_UNDELTA_HD uint64_t brotli_amd_undelta_last_piece(const uint64_t* pre, uint32_t count, uint64_t lo, uint64_t hi, uint32_t* seg) {
  const uint32_t j = brotli_amd_seg_find(pre, count, hi - 1u);
  *seg = j;
  return pre[j] > lo ? pre[j] : lo;
}
// cont of the tile whose first unit t0 is the part's first
BROTLI_AMD_UNDELTA_HD uint32_t brotli_amd_undelta_cont(const uint64_t* pre, uint32_t count, uint64_t t0) {
  return pre[brotli_amd_seg_find(pre, count, t0)] < t0 ? 1u : 0u;
}
// nohead of the tile at t0 whose last unit belongs to the segment that begins at unit `first`
BROTLI_AMD_UNDELTA_HD uint32_t brotli_amd_undelta_nohead(uint64_t first, uint64_t t0) { return first < t0 ? 1u : 0u; }

// ---- the unit ----
// bytes [blo, bhi) of sixteen: the mask of dword i
BROTLI_AMD_UNDELTA_HD uint32_t brotli_amd_undelta_dword_mask(uint32_t i, uint32_t blo, uint32_t bhi) {
  const int32_t a0 = (int32_t)blo - (int32_t)(4u * i), z0 = (int32_t)bhi - (int32_t)(4u * i);
  const int32_t a = a0 < 0 ? 0 : a0, z = z0 > 4 ? 4 : z0;
  if (a >= z) return 0u;
  const uint32_t upto = z == 4 ? 0xFFFFFFFFu : (1u << (8 * z)) - 1u;
  return upto & ~((1u << (8 * a)) - 1u);
}

template <uint32_t W> struct BrotliAmdUndeltaGeom {
  static constexpr uint32_t LOG = W == 1u ? 0u : W == 2u ? 1u : W == 4u ? 2u : 3u;
  static constexpr uint32_t PER = 16u / W;   // slots of a word
};

// The slots of unit k: sixteen bytes, slot i at bytes [i W, i W + W); a slot that does not count is 0.
template <uint32_t W>
BROTLI_AMD_UNDELTA_HD BrotliAmdU4 brotli_amd_undelta_fetch_w(uint64_t src, uint64_t dst, uint64_t len, uint64_t k) {
  constexpr uint32_t LOG = BrotliAmdUndeltaGeom<W>::LOG, PER = BrotliAmdUndeltaGeom<W>::PER;
  const uint64_t Wd = (dst & ~(uint64_t)15) + 16u * k;
  const int64_t p0 = (int64_t)(Wd - dst);                  // -15 ..
  const int64_t eb = (p0 + (int64_t)(W - 1u)) >> LOG;      // ceil(p0 / W) (arithmetic shift)
  const int64_t m = (int64_t)(len >> LOG);
  const int64_t ea = eb > 0 ? eb : 0, ez = eb + (int64_t)PER < m ? eb + (int64_t)PER : m;   // the slots that count: elements [ea, ez)
  BrotliAmdU4 v = {0u, 0u, 0u, 0u};
  if (ea >= ez) return v;
  // (src + eb W lies below src in a first unit that starts inside its word: only used through the two bounds)
  v = brotli_amd_unshuffle_copy_word(src + (uint64_t)(eb * (int64_t)W), src + (uint64_t)ea * W, src + (uint64_t)ez * W);
  if (ea != eb || ez != eb + (int64_t)PER) {
    const uint32_t blo = (uint32_t)(ea - eb) * W, bhi = (uint32_t)(ez - eb) * W;
    v.x &= brotli_amd_undelta_dword_mask(0u, blo, bhi); v.y &= brotli_amd_undelta_dword_mask(1u, blo, bhi);
    v.z &= brotli_amd_undelta_dword_mask(2u, blo, bhi); v.w &= brotli_amd_undelta_dword_mask(3u, blo, bhi);
  }
  return v;
}

// The unit's contribution: the sum of its slots (mod 2^64: truncated to W bytes where it is used).
template <uint32_t W>
BROTLI_AMD_UNDELTA_HD uint64_t brotli_amd_undelta_total_w(BrotliAmdU4 v) {
  if constexpr (W == 8u) {
    return (((uint64_t)v.y << 32) | v.x) + (((uint64_t)v.w << 32) | v.z);
  } else if constexpr (W == 4u) {
    return (uint64_t)v.x + v.y + v.z + v.w;
  } else if constexpr (W == 2u) {
    return (uint64_t)((v.x & 0xFFFFu) + (v.x >> 16) + (v.y & 0xFFFFu) + (v.y >> 16) + (v.z & 0xFFFFu) + (v.z >> 16) + (v.w & 0xFFFFu) + (v.w >> 16));
  } else {
    // bytes 0 and 2, and 1 and 3, of every dword in 16-bit fields: eight bytes a field at the most, no field overflows
    const uint32_t t = (v.x & 0x00FF00FFu) + ((v.x >> 8) & 0x00FF00FFu) + (v.y & 0x00FF00FFu) + ((v.y >> 8) & 0x00FF00FFu) +
                       (v.z & 0x00FF00FFu) + ((v.z >> 8) & 0x00FF00FFu) + (v.w & 0x00FF00FFu) + ((v.w >> 8) & 0x00FF00FFu);
    return (uint64_t)((t & 0xFFFFu) + (t >> 16));
  }
}

// The running sums of the slots on top of `carry`, each truncated to W bytes, in the slots' places.
template <uint32_t W>
BROTLI_AMD_UNDELTA_HD BrotliAmdU4 brotli_amd_undelta_scan_w(BrotliAmdU4 v, uint64_t carry) {
  if constexpr (W == 8u) {
    const uint64_t a = ((((uint64_t)v.y << 32) | v.x)) + carry, b = a + (((uint64_t)v.w << 32) | v.z);
    return BrotliAmdU4{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
  } else if constexpr (W == 4u) {
    BrotliAmdU4 o;
    o.x = v.x + (uint32_t)carry; o.y = o.x + v.y; o.z = o.y + v.z; o.w = o.z + v.w;
    return o;
  } else if constexpr (W == 2u) {
    uint32_t d[4] = {v.x, v.y, v.z, v.w}, c = (uint32_t)carry;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 4u; i++) {
      const uint32_t lo = (d[i] + c) & 0xFFFFu;          // (no carry between the two fields: each is added on its own)
      c = (lo + (d[i] >> 16)) & 0xFFFFu;
      d[i] = lo | (c << 16);
    }
    return BrotliAmdU4{d[0], d[1], d[2], d[3]};
  } else {
    // a dword's bytes b0 .. b3 as 16-bit fields, so that no sum carries into its neighbour: even = (b0, b2), odd = (b1, b3);
    // (b0 + b1, b2 + b3) -> (p1, p3) -> (p0, p2); the carry is added to all four at once
    uint32_t d[4] = {v.x, v.y, v.z, v.w}, c = (uint32_t)carry & 0xFFu;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 4u; i++) {
      const uint32_t even = d[i] & 0x00FF00FFu, odd = (d[i] >> 8) & 0x00FF00FFu;
      const uint32_t pairs = even + odd;
      const uint32_t cc = c * 0x00010001u;
      const uint32_t p_odd = pairs + (pairs << 16);              // (p1, p3) in front of the carry: at most 4 x 255 a field
      const uint32_t p_even = even + (p_odd << 16) + cc;         // (p0, p2)
      const uint32_t q_odd = p_odd + cc;
      d[i] = (p_even & 0x00FF00FFu) | ((q_odd & 0x00FF00FFu) << 8);
      c = (q_odd >> 16) & 0xFFu;
    }
    return BrotliAmdU4{d[0], d[1], d[2], d[3]};
  }
}

// Unit k of a segment of width W, its slots v as fetched and its carry (the sum of the segment's elements that start in front of the unit): the
// word's bytes, stored as the head of this file says.
template <uint32_t W>
BROTLI_AMD_UNDELTA_HD void brotli_amd_undelta_finish_w(uint64_t src, uint64_t dst, uint64_t len, uint64_t k, BrotliAmdU4 v, uint64_t carry) {
  constexpr uint32_t LOG = BrotliAmdUndeltaGeom<W>::LOG;
  const uint64_t Wd = (dst & ~(uint64_t)15) + 16u * k;
  const uint64_t lo = Wd > dst ? Wd : dst, hi = Wd + 16u < dst + len ? Wd + 16u : dst + len;   // the word's bytes that are the segment's
  const uint32_t off0 = (uint32_t)(dst - Wd) & (W - 1u);   // eb W - p0: where the first slot starts in the word
  BrotliAmdU4 o = brotli_amd_undelta_scan_w<W>(v, carry);
  if constexpr (W != 1u) {
    if (off0 != 0u) {
      // the element that straddles the word's start has the carry's value: its high off0 bytes in front, the slots shifted up by off0
      const uint64_t c = carry << (64u - 8u * W);
      const uint32_t I[6] = {(uint32_t)c, (uint32_t)(c >> 32), o.x, o.y, o.z, o.w};
      o = brotli_amd_unshuffle_shift_bytes(I, 8u - off0);
    }
    // the left-over bytes behind the last element stay what they are
    const uint64_t body = (len >> LOG) << LOG;
    if (hi > dst + body) {
      uint32_t w4[4] = {o.x, o.y, o.z, o.w};
      const uint64_t from = dst + body > lo ? dst + body : lo;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t q = 0; q < 16u; q++) {
        const uint64_t a = Wd + q;
        if (a >= from && a < hi) w4[q >> 2] = (w4[q >> 2] & ~(0xFFu << (8u * (q & 3u)))) | (brotli_amd_unshuffle_ld8(src + (a - dst)) << (8u * (q & 3u)));
      }
      o.x = w4[0]; o.y = w4[1]; o.z = w4[2]; o.w = w4[3];
    }
  }
  if (lo == Wd && hi == Wd + 16u) brotli_amd_unshuffle_st128(Wd, o);
  else brotli_amd_seg_store_edge(Wd, lo, hi, o);
}

// ... of any allowed width (another width: nothing is read or written)
BROTLI_AMD_UNDELTA_HD BrotliAmdU4 brotli_amd_undelta_fetch(uint64_t src, uint64_t dst, uint64_t len, uint32_t width, uint64_t k) {
  switch (width) {
    case 1u: return brotli_amd_undelta_fetch_w<1u>(src, dst, len, k);
    case 2u: return brotli_amd_undelta_fetch_w<2u>(src, dst, len, k);
    case 4u: return brotli_amd_undelta_fetch_w<4u>(src, dst, len, k);
    case 8u: return brotli_amd_undelta_fetch_w<8u>(src, dst, len, k);
    default: return BrotliAmdU4{0u, 0u, 0u, 0u};
  }
}
BROTLI_AMD_UNDELTA_HD uint64_t brotli_amd_undelta_total(BrotliAmdU4 v, uint32_t width) {
  switch (width) {
    case 1u: return brotli_amd_undelta_total_w<1u>(v);
    case 2u: return brotli_amd_undelta_total_w<2u>(v);
    case 4u: return brotli_amd_undelta_total_w<4u>(v);
    case 8u: return brotli_amd_undelta_total_w<8u>(v);
    default: return 0u;
  }
}
BROTLI_AMD_UNDELTA_HD void brotli_amd_undelta_finish(uint64_t src, uint64_t dst, uint64_t len, uint32_t width, uint64_t k, BrotliAmdU4 v, uint64_t carry) {
  switch (width) {
    case 1u: brotli_amd_undelta_finish_w<1u>(src, dst, len, k, v, carry); break;
    case 2u: brotli_amd_undelta_finish_w<2u>(src, dst, len, k, v, carry); break;
    case 4u: brotli_amd_undelta_finish_w<4u>(src, dst, len, k, v, carry); break;
    case 8u: brotli_amd_undelta_finish_w<8u>(src, dst, len, k, v, carry); break;
    default: break;
  }
}

// ---- the three phases over host memory, tile by tile (the device replaces the loops over a tile's units by its lanes) ----
// phase 1 of the tile [t0, t1) (t1: the tile's end or the end of all units): its summary
inline BrotliAmdUndeltaTile brotli_amd_undelta_host_summary(const BrotliAmdUnshuffleSeg* segs, const uint64_t* pre, uint32_t n, uint64_t t0, uint64_t t1) {
  uint32_t j = 0;
  const uint64_t from = brotli_amd_undelta_last_piece(pre, n, t0, t1, &j);
  BrotliAmdUndeltaTile s = {0u, brotli_amd_undelta_cont(pre, n, t0), brotli_amd_undelta_nohead(pre[j], t0)};
  const uint64_t src = (uint64_t)(uintptr_t)segs[j].src, dst = (uint64_t)(uintptr_t)segs[j].dst;
  for (uint64_t g = from; g < t1; g++) s.sum += brotli_amd_undelta_total(brotli_amd_undelta_fetch(src, dst, segs[j].len, segs[j].width, g - pre[j]), segs[j].width);
  return s;
}
// phase 3 of the tile [t0, t1) with its carry-in
inline void brotli_amd_undelta_host_apply(const BrotliAmdUnshuffleSeg* segs, const uint64_t* pre, uint32_t n, uint64_t t0, uint64_t t1, uint64_t carry_in) {
  BrotliAmdUndeltaPair run = {carry_in, 0u};
  for (uint64_t g = t0; g < t1; g++) {
    const uint32_t j = brotli_amd_seg_find(pre, n, g);
    const uint64_t src = (uint64_t)(uintptr_t)segs[j].src, dst = (uint64_t)(uintptr_t)segs[j].dst, k = g - pre[j];
    const BrotliAmdU4 v = brotli_amd_undelta_fetch(src, dst, segs[j].len, segs[j].width, k);
    if (k == 0u) run = BrotliAmdUndeltaPair{0u, 1u};
    brotli_amd_undelta_finish(src, dst, segs[j].len, segs[j].width, k, v, run.sum);
    run = brotli_amd_undelta_combine(run, BrotliAmdUndeltaPair{brotli_amd_undelta_total(v, segs[j].width), 0u});
  }
}

#endif  // BROTLI_AMD_UNDELTA_H_
