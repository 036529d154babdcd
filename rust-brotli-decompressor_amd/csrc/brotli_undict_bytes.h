// brotli_undict_bytes.h -- dictionary-index runs and a dictionary of PLAIN byte arrays back into an Arrow string column, (offsets, data): the
// dictionary's length chain, the one function that turns an index into an entry, an item's offsets and bytes word by word of the destination,
// and the host's walk and items, once, for the host and the device.
//
// THE TRANSFORM (include/brotli/batch.h has it in full).  A segment is an unrle segment (csrc/brotli_unrle.h) whose values are INDICES into a
// dictionary of dict_len bytes at dict: entry e is a little-endian uint32 length L_e, then L_e bytes.  The dictionary is WALKED once a call,
// entry after entry, into starts[0 .. D]: starts[e] is the position of entry e's first value byte, and a sentinel behind the last entry makes
// L_e = starts[e + 1] - 4 - starts[e] hold for every e < D, a cut dictionary included.  Element i of the segment, i < m = min(count, cap), is
// entry idx_i where idx_i < D; an index at or above D gives an EMPTY element, is never made an address, and is counted (undict's bad and
// first_bad).  offsets[i] = offset_base + the bytes of the elements in front of i, for i = 0 .. m, and data is the elements' bytes one behind
// the other, cut at data_cap.
//
// The destination is cut into unrle's ITEMS.  An item's bytes are summed up first (its undelta tile record), the carry launch gives every item
// the bytes in front of it, and then the item is expanded by itself: ends(t), t = 0 .. its elements, are the offsets of its elements in the
// segment's data, and its offsets and its bytes are written WORD BY WORD OF THE DESTINATION -- the aligned 16-byte words that its range
// touches, each by one taker, whole words as one store and the range's head and tail as single elements or bytes.  Items of one segment write
// disjoint bytes, in any order, and so do the words of an item.
//
// LOADS.  What unrle loads of [src, src + len); single bytes of [dict, dict + dict_len) (the device's walk: the aligned 16-byte words that hold
// them, through LDS); starts[idx] and starts[idx + 1] for idx < D alone.
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUndictBytesHost; tests/tools/undict_bytes_san.cpp) and the device
// (csrc/brotli_undict_bytes_kernels.hip); the device replaces the loops over an item's elements and words by its lanes, and keeps ends and the
// entries' positions in LDS.  Addresses are integers.
#ifndef BROTLI_AMD_UNDICT_BYTES_H_
#define BROTLI_AMD_UNDICT_BYTES_H_

#include "brotli/batch.h"       // BrotliAmdUndictBytesResult, BROTLI_AMD_UNDICT_BYTES_*
#include "brotli_device_abi.h"  // the segment and the dictionary record of a launch
#include "brotli_undbp.h"       // an item's sum as a tile record: brotli_amd_undbp_tile
#include "brotli_undict.h"      // BROTLI_AMD_UNDICT_NONE, the walk's width
#include "brotli_unrle.h"       // the walk, a run, an element, the items

#define BROTLI_AMD_UNDICT_BYTES_HD BROTLI_AMD_UNSHUFFLE_HD
#define BROTLI_AMD_UNDICT_BYTES_FLAGS (BROTLI_AMD_UNDICT_BYTES_WIDTH_BYTE | BROTLI_AMD_UNDICT_BYTES_OFFSETS64 | BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY)   // a segment's
#define BROTLI_AMD_UNDICT_BYTES_MAX_CAP BROTLI_AMD_UNRLE_MAX_CAP
#define BROTLI_AMD_UNDICT_BYTES_MAX_DICT ((uint64_t)1 << 32)   // a dictionary's bytes are below it: entry positions are 32-bit

static_assert(BROTLI_AMD_UNDICT_BYTES_WIDTH_BYTE == BROTLI_AMD_UNRLE_WIDTH_BYTE, "the walk takes that flag as it is");
static_assert(sizeof(BrotliAmdUndictBytesResult) == 80u, "undict's seven fields, bytes, and the dictionary's three and a reserved word");

// ---- the dictionary's length chain ----
struct BrotliAmdUndictBytesDictResult {
  uint64_t entries;    // D
  uint64_t consumed;   // the bytes of the D entries
  uint32_t status;     // BROTLI_AMD_UNDICT_BYTES_DICT_*
  uint32_t reserved;
};
// the entries of starts[] that a dictionary of len bytes, bounded by `bound` entries, needs: an entry takes four bytes at the least
BROTLI_AMD_UNDICT_BYTES_HD uint64_t brotli_amd_undict_bytes_starts(uint64_t len, uint64_t bound) { return (bound < len / 4u ? bound : len / 4u) + 1u; }

// A dictionary of len < 2^32 bytes, entry after entry, up to `bound` entries -> its result.  rd.ensure(o) is called in front of a length at
// offset o, and rd.window gives the bytes from o on (unrle's readers).  put(e, s): starts[e] = s, for e = 0 .. D.
template <class Reader, class Put>
BROTLI_AMD_UNDICT_BYTES_HD BrotliAmdUndictBytesDictResult brotli_amd_undict_bytes_dict_walk(Reader& rd, uint64_t len, uint64_t bound, Put put) {
  uint64_t pos = 0, e = 0;
  uint32_t status = BROTLI_AMD_UNDICT_BYTES_DICT_OK;
  while (e < bound && pos < len) {
    const uint64_t left = len - pos;
    if (left < 4u) { status = BROTLI_AMD_UNDICT_BYTES_DICT_CUT; break; }
    uint32_t b8 = 0;
    rd.ensure(pos);
    const uint64_t L = rd.window(pos, left, &b8) & 0xFFFFFFFFull;
    if (L > left - 4u) { status = BROTLI_AMD_UNDICT_BYTES_DICT_CUT; break; }
    put(e, (uint32_t)(pos + 4u));
    pos += 4u + L; e++;
  }
  put(e, (uint32_t)(pos + 4u));   // the sentinel (modulo 2^32, as the difference is taken)
  return BrotliAmdUndictBytesDictResult{e, pos, status, 0u};
}

// ---- an index -> its entry ----
struct BrotliAmdUndictBytesEntry { uint32_t pos, len, bad; };
// Entry idx of the D entries whose positions are starts[0 .. D].  The comparison is one of 64 bits, and an index that fails it is never
// multiplied or added to anything: its entry is empty and it is bad.
BROTLI_AMD_UNDICT_BYTES_HD BrotliAmdUndictBytesEntry brotli_amd_undict_bytes_lookup(const uint32_t* starts, uint64_t D, uint64_t idx) {
  if (idx >= D) return BrotliAmdUndictBytesEntry{0u, 0u, 1u};
  const uint32_t a = starts[idx], b = starts[idx + 1u];
  return BrotliAmdUndictBytesEntry{a, b - 4u - a, 0u};
}

// ---- the offsets ----
BROTLI_AMD_UNDICT_BYTES_HD uint32_t brotli_amd_undict_bytes_offset_width(uint32_t flags) { return (flags & BROTLI_AMD_UNDICT_BYTES_OFFSETS64) != 0u ? 8u : 4u; }
// offsets[0], which the segment's first item writes whether it has elements or not
BROTLI_AMD_UNDICT_BYTES_HD void brotli_amd_undict_bytes_first_offset(const BrotliAmdUndictBytesSeg& sg) {
  if (sg.offsets != nullptr && (sg.flags & BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY) == 0u)
    brotli_amd_unvarint_store((uint64_t)(uintptr_t)sg.offsets, brotli_amd_undict_bytes_offset_width(sg.flags), sg.offset_base);
}
// An item of the elements [e0, e1) writes offsets[e0 + 1 .. e1], which lie in the SLOTS [*s0, *s1) of ow bytes from the address of the
// segment's offsets on; slot s holds offset_base + ends(s - *s0 + 1).
BROTLI_AMD_UNDICT_BYTES_HD void brotli_amd_undict_bytes_offset_slots(uint32_t flags, uint64_t e0, uint64_t e1, uint64_t* s0, uint64_t* s1) {
  const uint64_t shift = (flags & BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY) != 0u ? 0u : 1u;
  *s0 = e0 + shift; *s1 = e1 + shift;
}
// Word q of the aligned 16-byte words that the slots [s0, s1) at O touch: the slots whose first byte lies in it, as one 16-byte store where
// they fill it, single elements elsewhere (byte by byte where O is no multiple of ow).
template <class Ends>
BROTLI_AMD_UNDICT_BYTES_HD void brotli_amd_undict_bytes_offsets_word(uint64_t O, uint32_t ow, uint64_t base, uint64_t s0, uint64_t s1, Ends ends, uint64_t q) {
  const uint64_t lo = O + s0 * ow, hi = O + s1 * ow, A = (lo & ~(uint64_t)15) + 16u * q;
  const uint64_t sa = A <= lo ? s0 : (A - O + ow - 1u) / ow, sb = A + 16u >= hi ? s1 : (A + 16u - O + ow - 1u) / ow;
  if ((O & (ow - 1u)) == 0u && (sb - sa) * ow == 16u) {
    uint64_t v[4] = {0u, 0u, 0u, 0u};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < 4u; u++)
      if (u < 16u / ow) v[u] = base + ends((uint32_t)(sa + u - s0) + 1u);
    const BrotliAmdU4 w = ow == 8u ? BrotliAmdU4{(uint32_t)v[0], (uint32_t)(v[0] >> 32), (uint32_t)v[1], (uint32_t)(v[1] >> 32)}
                                   : BrotliAmdU4{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]};
    brotli_amd_unshuffle_st128(A, w);
    return;
  }
  for (uint64_t s = sa; s < sb; s++) brotli_amd_unvarint_store(O + s * ow, ow, base + ends((uint32_t)(s - s0) + 1u));
}

// ---- the bytes ----
// The part [*lo, *hi) of an item's bytes [first, last) -- offsets in the segment's data -- that a capacity of data_cap bytes leaves.
BROTLI_AMD_UNDICT_BYTES_HD void brotli_amd_undict_bytes_data_range(uint64_t first, uint64_t last, uint64_t data_cap, uint64_t* lo, uint64_t* hi) {
  *lo = first < data_cap ? first : data_cap;
  *hi = last < data_cap ? last : data_cap;
}
// Word q of the aligned 16-byte words that [data + lo, data + hi) touches, lo < hi being the item's range: ends(t), t = 0 .. m, are the
// offsets of the item's m elements and of its end, pos(t) is the position of element t's bytes in the dictionary at address dict.  The word's
// first element is found by a binary search; it is put together from consecutive elements' bytes, empty elements skipped, and stored once --
// as single bytes where the range does not fill it.
template <class Ends, class Pos>
BROTLI_AMD_UNDICT_BYTES_HD void brotli_amd_undict_bytes_data_word(uint64_t data, uint64_t dict, uint32_t m, uint64_t lo, uint64_t hi, Ends ends, Pos pos, uint64_t q) {
  const uint64_t A = ((data + lo) & ~(uint64_t)15) + 16u * q;
  const uint64_t p0 = A > data + lo ? A - data : lo, p1 = A + 16u < data + hi ? A + 16u - data : hi;
  uint32_t t = 0, b = m;   // the last element that begins at or in front of p0 (ends(0) <= lo, and p0 < hi <= ends(m))
  while (b - t > 1u) { const uint32_t mid = (t + b) >> 1; if (ends(mid) <= p0) t = mid; else b = mid; }
  uint64_t start = ends(t), end = ends(t + 1u), wlo = 0, whi = 0;
  for (uint64_t p = p0; p < p1;) {
    while (end <= p) { t++; start = end; end = ends(t + 1u); }
    const uint64_t stop = end < p1 ? end : p1;
    for (uint64_t s = dict + pos(t) + (p - start); p < stop; p++, s++) {
      const uint64_t byte = brotli_amd_unshuffle_ld8(s);
      const uint32_t at = (uint32_t)(data + p - A);
      if (at < 8u) wlo |= byte << (8u * at); else whi |= byte << (8u * (at - 8u));
    }
  }
  if (p1 - p0 == 16u) {
    brotli_amd_unshuffle_st128(A, BrotliAmdU4{(uint32_t)wlo, (uint32_t)(wlo >> 32), (uint32_t)whi, (uint32_t)(whi >> 32)});
    return;
  }
  for (uint64_t p = p0; p < p1; p++) {
    const uint32_t at = (uint32_t)(data + p - A);
    brotli_amd_unvarint_store(data + p, 1u, (at < 8u ? wlo >> (8u * at) : whi >> (8u * (at - 8u))) & 0xFFu);
  }
}

// ---- the walks and an item over host memory (the device replaces the loops over an item's elements and words by its lanes) ----
// what the RLE walk leaves of a segment's result: what the items add to, and what its dictionary's walk found (zeros for a segment that only
// counts)
BROTLI_AMD_UNDICT_BYTES_HD BrotliAmdUndictBytesResult brotli_amd_undict_bytes_result(const BrotliAmdUnrleResult& r, BrotliAmdUndictBytesDictResult dict) {
  return BrotliAmdUndictBytesResult{r.count, r.consumed, r.runs, r.status, r.bits, 0u, BROTLI_AMD_UNDICT_NONE, 0u, dict.entries, dict.consumed, dict.status, 0u};
}
// starts[0 .. brotli_amd_undict_bytes_starts(len, bound))
inline BrotliAmdUndictBytesDictResult brotli_amd_undict_bytes_host_dict(uint64_t dict, uint64_t len, uint64_t bound, uint32_t* starts) {
  BrotliAmdUnrleDirect rd = {dict};
  return brotli_amd_undict_bytes_dict_walk(rd, len, bound, [&](uint64_t e, uint32_t s) { starts[e] = s; });
}
// ckpts[0 .. brotli_amd_unrle_items(sg.cap, item_elems)) start as BROTLI_AMD_UNRLE_NONE
inline BrotliAmdUndictBytesResult brotli_amd_undict_bytes_host_walk(const BrotliAmdUndictBytesSeg& sg, BrotliAmdUndictBytesDictResult dict, uint32_t item_elems,
                                                                    BrotliAmdUnrleCheckpoint* ckpts) {
  BrotliAmdUnrleDirect rd = {(uint64_t)(uintptr_t)sg.src};
  const BrotliAmdUnrleResult r = brotli_amd_unrle_walk(rd, sg.len, sg.cap, BROTLI_AMD_UNDICT_WALK_WIDTH, sg.bits, sg.flags & BROTLI_AMD_UNRLE_FLAGS, item_elems,
                                                       [&](uint64_t j0, uint64_t j1, uint64_t off, uint64_t first) {
    for (uint64_t j = j0; j < j1; j++) ckpts[j] = BrotliAmdUnrleCheckpoint{off, first};
  });
  return brotli_amd_undict_bytes_result(r, dict);
}
// item j's bytes as its tile record; its bad elements go into res->bad and res->first_bad (items in any order give the same)
inline BrotliAmdUndeltaTile brotli_amd_undict_bytes_host_count(const BrotliAmdUndictBytesSeg& sg, const uint32_t* starts, BrotliAmdUndictBytesResult* res,
                                                               BrotliAmdUnrleCheckpoint cp, uint64_t j, uint32_t item_elems) {
  uint64_t sum = 0;
  brotli_amd_unrle_host_item_each((uint64_t)(uintptr_t)sg.src, sg.len, sg.cap, res->count, res->bits, cp, j, item_elems, [&](uint64_t e, uint64_t idx) {
    const BrotliAmdUndictBytesEntry en = brotli_amd_undict_bytes_lookup(starts, res->dict_entries, idx);
    sum += en.len;
    if (en.bad) { res->bad++; if (e < res->first_bad) res->first_bad = e; }
  });
  return brotli_amd_undbp_tile(j, 0u, sum);
}
// Item j's offsets and bytes on top of its carry-in, the bytes of the elements in front of it; the item that holds the segment's last
// delivered element writes res->bytes.  ends[0 .. item_elems] and pos[0 .. item_elems) are the caller's room; words(count, each) calls each(q)
// for q = 0 .. count - 1 in the order the caller wants.
template <class Words>
inline void brotli_amd_undict_bytes_host_expand(const BrotliAmdUndictBytesSeg& sg, uint64_t dict, const uint32_t* starts, BrotliAmdUndictBytesResult* res,
                                                BrotliAmdUnrleCheckpoint cp, uint64_t j, uint32_t item_elems, uint64_t carry_in, uint64_t* ends, uint32_t* pos,
                                                Words words) {
  if (j == 0u) brotli_amd_undict_bytes_first_offset(sg);
  uint64_t e0, e1;
  brotli_amd_unrle_item_range(res->count, sg.cap, j, item_elems, &e0, &e1);
  if (cp.off == BROTLI_AMD_UNRLE_NONE || e0 >= e1) return;
  const uint32_t m = (uint32_t)(e1 - e0);
  ends[0] = carry_in;
  brotli_amd_unrle_host_item_each((uint64_t)(uintptr_t)sg.src, sg.len, sg.cap, res->count, res->bits, cp, j, item_elems, [&](uint64_t e, uint64_t idx) {
    const BrotliAmdUndictBytesEntry en = brotli_amd_undict_bytes_lookup(starts, res->dict_entries, idx);
    pos[e - e0] = en.pos;
    ends[e - e0 + 1u] = ends[e - e0] + en.len;
  });
  auto end_of = [&](uint32_t t) { return ends[t]; };
  auto pos_of = [&](uint32_t t) { return pos[t]; };
  if (sg.offsets != nullptr) {
    const uint64_t O = (uint64_t)(uintptr_t)sg.offsets;
    const uint32_t ow = brotli_amd_undict_bytes_offset_width(sg.flags);
    uint64_t s0, s1;
    brotli_amd_undict_bytes_offset_slots(sg.flags, e0, e1, &s0, &s1);
    words(brotli_amd_seg_units(O + s0 * ow, (s1 - s0) * ow), [&](uint64_t q) { brotli_amd_undict_bytes_offsets_word(O, ow, sg.offset_base, s0, s1, end_of, q); });
  }
  uint64_t lo, hi;
  brotli_amd_undict_bytes_data_range(ends[0], ends[m], sg.data_cap, &lo, &hi);
  if (sg.data != nullptr && lo < hi) {
    const uint64_t data = (uint64_t)(uintptr_t)sg.data;
    words(brotli_amd_seg_units(data + lo, hi - lo), [&](uint64_t q) { brotli_amd_undict_bytes_data_word(data, dict, m, lo, hi, end_of, pos_of, q); });
  }
  if (e1 == (res->count < sg.cap ? res->count : sg.cap)) res->bytes = ends[m];
}

#endif  // BROTLI_AMD_UNDICT_BYTES_H_
