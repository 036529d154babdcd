// brotli_undba.h -- Parquet's DELTA_BYTE_ARRAY back into an Arrow string column, (offsets, data): the two streams of a segment as undbp's,
// the test of an element against the one in front of it, an item's elements, what an item behind the first bad element takes for its
// carry-in, what the segment's last item leaves, where a byte of the data comes from in each of the three phases of the prefix copies, and
// the host's phases, once, for the host and the device.
//
// THE TRANSFORM (include/brotli/batch.h has it in full).  A segment of len bytes is a DELTA_BINARY_PACKED stream P of prefix lengths, a
// stream S of suffix lengths from P's `consumed` on, and the suffix bytes behind S.  Both streams are undbp's (csrc/brotli_undbp.h): its walk,
// its items of item_deltas deltas, its checkpoints and groups; the items' sums with undelta's carry launch over them give every item the two
// values in front of its first delta.  Both streams are cut with one cap and one item size, so item j of P and item j of S are the same
// ELEMENTS: element 0 in item 0, and element d + 1 for every delta d of the item, below m = min(count_p, count_s, cap).  Element i has p_i and
// s_i, the low 32 bits of its two values as signed int32, and is BAD where p_i < 0, s_i < 0 or p_i > D_(i-1) = p_(i-1) + s_(i-1): a test that
// needs the element in front alone, which at an item's first element is the carry-in.  first_bad is the minimum over all items; elements from
// it on are empty, the others have L_i = D_i.  An item sums L and s up to ITS first bad element (two more tile records); an item behind
// first_bad takes for its carry-in what the item of first_bad has in front of it and in it (brotli_amd_undba_sum_in).  The offsets are
// undlba's stores (csrc/brotli_undlba.h).
//
// THE PREFIX COPIES.  Inside an item r_e = min(p_first, .., p_e).  PHASE A, items in any order: element e's bytes [p_e, L_e) are its suffix,
// and its bytes [r_e, p_e) are element e - 1's, which lie in the item: the running string is kept up to `cap` bytes (LDS on the device), and a
// byte beyond that is found by walking back to the element whose suffix holds it (brotli_amd_undba_back_byte) -- from the SOURCE, so nothing
// that this phase stores is loaded again.  It records the item's last element (BrotliAmdUndbaLast).  PHASE B, a segment's items one after the
// other: the last element of item j gets its bytes [0, r_last) from the last element of item j - 1; the carried string is kept up to `cap`
// bytes, and a byte beyond that is loaded from the item whose phase A stored it (brotli_amd_undba_far_byte), never from what this phase
// stored.  PHASE C, items in any order: every other element e of an item j >= 1 gets its bytes [0, r_e) from the last element of item j - 1.
// Every store is cut at keep = min(bytes, data_cap): a copy's source lies in front of its destination, so what is stored was stored from.
//
// LOADS.  What undbp loads of [src, src + len); suffix bytes in front of src + len, one by one; bytes of the data below `keep`.
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUndbaHost; tests/tools/undba_san.cpp) and the device
// (csrc/brotli_undba_kernels.hip); the device replaces the loops over an item's groups and over a string's bytes by its lanes.
#ifndef BROTLI_AMD_UNDBA_H_
#define BROTLI_AMD_UNDBA_H_

#include "brotli/batch.h"       // BrotliAmdUndbaResult, BROTLI_AMD_UNDBA_*
#include "brotli_device_abi.h"  // BrotliAmdUndbaSeg, BrotliAmdUndbaLast
#include "brotli_undlba.h"      // the offsets' stores; an item's values on the host
#include <vector>

#define BROTLI_AMD_UNDBA_HD BROTLI_AMD_UNSHUFFLE_HD
#define BROTLI_AMD_UNDBA_FLAGS (BROTLI_AMD_UNDBA_OFFSETS64 | BROTLI_AMD_UNDBA_ENDS_ONLY)   // a segment's
#define BROTLI_AMD_UNDBA_MAX_CAP BROTLI_AMD_UNDBP_MAX_CAP
#define BROTLI_AMD_UNDBA_NONE (~(uint64_t)0)   // first_bad where no element was bad

static_assert(sizeof(BrotliAmdUndbaResult) == 128u, "undbp's seven fields and data_status, the same with bad_kind, and first_bad, bytes, suffix_bytes, data_avail");
static_assert(BROTLI_AMD_UNDBA_OFFSETS64 == BROTLI_AMD_UNDLBA_OFFSETS64 && BROTLI_AMD_UNDBA_ENDS_ONLY == BROTLI_AMD_UNDLBA_ENDS_ONLY &&
                  BROTLI_AMD_UNDBA_SKIP == BROTLI_AMD_UNDLBA_SKIP, "undlba's flags, and its stores of the offsets");

// ---- the result of the two walks: what the items add to ----
BROTLI_AMD_UNDBA_HD BrotliAmdUndbaResult brotli_amd_undba_result(const BrotliAmdUndbpResult& p, const BrotliAmdUndbpResult& s, uint64_t len) {
  const uint32_t differ = p.count != s.count && p.status == BROTLI_AMD_UNDBP_OK && s.status == BROTLI_AMD_UNDBP_OK ? BROTLI_AMD_UNDBA_DATA_COUNTS_DIFFER : 0u;
  return BrotliAmdUndbaResult{p.count, p.consumed, p.declared, p.blocks, p.status, p.block_values, p.miniblocks, BROTLI_AMD_UNDBA_DATA_OK | differ,
                              s.count, s.consumed, s.declared, s.blocks, s.status, s.block_values, s.miniblocks, BROTLI_AMD_UNDBA_BAD_NONE,
                              BROTLI_AMD_UNDBA_NONE, 0u, 0u, len - p.consumed - s.consumed};
}
// ... and the walks' own parts of it again
BROTLI_AMD_UNDBA_HD BrotliAmdUndbpResult brotli_amd_undba_walked_p(const BrotliAmdUndbaResult& r) {
  return BrotliAmdUndbpResult{r.count_p, r.consumed_p, r.declared_p, r.blocks_p, r.status_p, r.block_values_p, r.miniblocks_p};
}
BROTLI_AMD_UNDBA_HD BrotliAmdUndbpResult brotli_amd_undba_walked_s(const BrotliAmdUndbaResult& r) {
  return BrotliAmdUndbpResult{r.count_s, r.consumed_s, r.declared_s, r.blocks_s, r.status_s, r.block_values_s, r.miniblocks_s};
}
// the two streams as undbp's walk and items take them (they write nothing): S begins where P's walk stopped, whatever its status is
BROTLI_AMD_UNDBA_HD BrotliAmdUndbpSeg brotli_amd_undba_seg_p(const BrotliAmdUndbaSeg& sg) {
  return BrotliAmdUndbpSeg{sg.src, nullptr, sg.len, sg.cap, sg.first_item, 8u, 0u};
}
BROTLI_AMD_UNDBA_HD BrotliAmdUndbpSeg brotli_amd_undba_seg_s(const BrotliAmdUndbaSeg& sg, uint64_t consumed_p) {   // (the walk's: consumed_p <= len)
  return BrotliAmdUndbpSeg{sg.src + consumed_p, nullptr, sg.len - consumed_p, sg.cap, sg.first_item, 8u, 0u};
}

// ---- the elements ----
BROTLI_AMD_UNDBA_HD uint64_t brotli_amd_undba_m(uint64_t count_p, uint64_t count_s, uint64_t cap) {
  const uint64_t c = count_p < count_s ? count_p : count_s;
  return c < cap ? c : cap;
}
// the elements [*lo, *hi) of item j: element 0 and those of the deltas [0, item_deltas) in item 0, those of its own deltas in every other one
BROTLI_AMD_UNDBA_HD void brotli_amd_undba_item_elems(uint64_t m, uint64_t j, uint32_t item_deltas, uint64_t* lo, uint64_t* hi) {
  const uint64_t first = j == 0u ? 0u : j * item_deltas + 1u, end = (j + 1u) * item_deltas + 1u;
  *lo = first < m ? first : m;
  *hi = end < m ? end : m;
}
// the item that holds element e
BROTLI_AMD_UNDBA_HD uint64_t brotli_amd_undba_item_of(uint64_t e, uint32_t item_deltas) { return e == 0u ? 0u : (e - 1u) / item_deltas; }
// Which rule an element breaks, d_prev being D of the element in front of it (0 in front of element 0): the first of the three, or none.
BROTLI_AMD_UNDBA_HD uint32_t brotli_amd_undba_bad_kind(int32_t p, int32_t s, int64_t d_prev) {
  if (p < 0) return BROTLI_AMD_UNDBA_BAD_PREFIX_NEGATIVE;
  if (s < 0) return BROTLI_AMD_UNDBA_BAD_SUFFIX_NEGATIVE;
  return (int64_t)p > d_prev ? BROTLI_AMD_UNDBA_BAD_PREFIX_LONG : BROTLI_AMD_UNDBA_BAD_NONE;
}
BROTLI_AMD_UNDBA_HD int64_t brotli_amd_undba_d(uint64_t vp, uint64_t vs) { return (int64_t)(int32_t)(uint32_t)vp + (int64_t)(int32_t)(uint32_t)vs; }
// What an item whose first element is `lo` has in front of it, of L or of s: its own carry-in, or, behind first_bad, what the item of first_bad
// has in front of it and in it up to first_bad (its carry-in and its own tile record's sum).
BROTLI_AMD_UNDBA_HD uint64_t brotli_amd_undba_sum_in(uint64_t first_bad, uint64_t lo, uint64_t own_carry, uint64_t bad_carry, uint64_t bad_sum) {
  return lo > first_bad ? bad_carry + bad_sum : own_carry;
}

// ---- the segment's last item (brotli_amd_undlba_last_item over m) leaves: bytes, suffix_bytes and the bits of data_status ----
BROTLI_AMD_UNDBA_HD void brotli_amd_undba_finish(BrotliAmdUndbaResult* res, uint64_t bytes, uint64_t suffix_bytes) {
  res->bytes = bytes;
  res->suffix_bytes = suffix_bytes;
  res->data_status |= (suffix_bytes > res->data_avail ? BROTLI_AMD_UNDBA_DATA_SHORT : 0u) | (res->first_bad != BROTLI_AMD_UNDBA_NONE ? BROTLI_AMD_UNDBA_DATA_BAD : 0u);
}
// the bytes of the data that are stored
BROTLI_AMD_UNDBA_HD uint64_t brotli_amd_undba_keep(const BrotliAmdUndbaSeg& sg, uint64_t bytes) {
  return sg.data == nullptr ? 0u : bytes < sg.data_cap ? bytes : sg.data_cap;
}

// ---- where a byte comes from ----
// suffix byte q of the `avail` that begin at the address suffixes: one at or behind the segment's end reads as 0 and is not loaded
BROTLI_AMD_UNDBA_HD uint32_t brotli_amd_undba_suffix_byte(uint64_t suffixes, uint64_t avail, uint64_t q) {
  return q < avail ? brotli_amd_unshuffle_ld8(suffixes + q) : 0u;
}
// Byte k of the item's element idx, k < p[idx], without the running string: back through the item to the element f whose suffix holds it --
// p[f] <= k --, q being the suffix bytes in front of element idx.  There is one: r <= k.  p and s are the item's elements' (LDS on the device).
BROTLI_AMD_UNDBA_HD uint32_t brotli_amd_undba_back_byte(const uint32_t* p, const uint32_t* s, uint32_t idx, uint64_t q, uint32_t k, uint64_t suffixes, uint64_t avail) {
  uint32_t f = idx;
  while (f != 0u) {
    f--;
    q -= s[f];
    if (p[f] <= k) return brotli_amd_undba_suffix_byte(suffixes, avail, q + (k - p[f]));
  }
  return 0u;   // (not reached)
}
// phase A: byte k, r <= k < L, of element idx; cur: the running string, of which the bytes below cap are kept
BROTLI_AMD_UNDBA_HD uint32_t brotli_amd_undba_a_byte(const uint32_t* p, const uint32_t* s, const uint8_t* cur, uint32_t cap, uint32_t idx, uint64_t q, uint32_t k, uint64_t suffixes,
                                                     uint64_t avail) {
  const uint32_t pe = p[idx];
  if (k >= pe) return brotli_amd_undba_suffix_byte(suffixes, avail, q + (k - pe));
  return k < cap ? cur[k] : brotli_amd_undba_back_byte(p, s, idx, q, k, suffixes, avail);
}
// phase B: byte k, k < lasts[j].r, of the last element of item j without the carried string: it is the last element of the item f < j whose
// phase A stored it -- lasts[f].r <= k --; item 0's r is 0.  data: the segment's; a byte at or behind keep was not stored and is not loaded.
BROTLI_AMD_UNDBA_HD uint32_t brotli_amd_undba_far_byte(const BrotliAmdUndbaLast* lasts, uint64_t j, uint32_t k, uint64_t data, uint64_t keep) {
  uint64_t f = j - 1u;
  while (f != 0u && k < lasts[f].r) f--;
  const uint64_t at = lasts[f].at + k;
  return at < keep ? brotli_amd_unshuffle_ld8(data + at) : 0u;
}
// How many of the n bytes that begin at byte `at` of the data are stored: every loop over an element's bytes ends there, so that the work
// follows min(bytes, data_cap) and never a declared length (two elements of 2^31 - 1 bytes over ten bytes of source are a legal page).
BROTLI_AMD_UNDBA_HD uint64_t brotli_amd_undba_stored(uint64_t at, uint64_t n, uint64_t keep) {
  return at >= keep ? 0u : n < keep - at ? n : keep - at;
}
// a byte of the data, where it is kept
BROTLI_AMD_UNDBA_HD void brotli_amd_undba_put(uint64_t data, uint64_t keep, uint64_t at, uint32_t byte) {
  if (at < keep) brotli_amd_unvarint_store(data + at, 1u, byte);
}

// ---- the walks and an item over host memory ----
// ckpts_p and ckpts_s [0 .. brotli_amd_undbp_items(sg.cap, item_deltas)) start as BROTLI_AMD_UNDBP_NONE (both NULL: a counting walk)
inline BrotliAmdUndbaResult brotli_amd_undba_host_walk(const BrotliAmdUndbaSeg& sg, uint32_t item_deltas, BrotliAmdUndbpCheckpoint* ckpts_p, BrotliAmdUndbpCheckpoint* ckpts_s,
                                                       uint64_t* first_p, uint64_t* first_s) {
  const BrotliAmdUndbpResult p = brotli_amd_undbp_host_walk(brotli_amd_undba_seg_p(sg), item_deltas, ckpts_p, first_p);
  const BrotliAmdUndbpResult s = brotli_amd_undbp_host_walk(brotli_amd_undba_seg_s(sg, p.consumed), item_deltas, ckpts_s, first_s);
  return brotli_amd_undba_result(p, s, sg.len);
}
// item j's deltas of both streams as tile records: undbp's
inline void brotli_amd_undba_host_sum(const BrotliAmdUndbaSeg& sg, const BrotliAmdUndbaResult& res, BrotliAmdUndbpCheckpoint cp_p, BrotliAmdUndbpCheckpoint cp_s, uint64_t first_p,
                                      uint64_t first_s, uint64_t j, uint32_t item_deltas, BrotliAmdUndeltaTile* tile_p, BrotliAmdUndeltaTile* tile_s) {
  *tile_p = brotli_amd_undbp_host_sum(brotli_amd_undba_seg_p(sg), brotli_amd_undba_walked_p(res), cp_p, first_p, j, item_deltas);
  *tile_s = brotli_amd_undbp_host_sum(brotli_amd_undba_seg_s(sg, res.consumed_p), brotli_amd_undba_walked_s(res), cp_s, first_s, j, item_deltas);
}
// An item's elements [lo, lo + p.size()): the two int32 of each, and D of the element in front of the first (0 in front of element 0).
struct BrotliAmdUndbaHostItem {
  uint64_t lo = 0;
  int64_t d_in = 0;
  std::vector<int32_t> p, s;
};
inline BrotliAmdUndbaHostItem brotli_amd_undba_host_item(const BrotliAmdUndbaSeg& sg, const BrotliAmdUndbaResult& res, BrotliAmdUndbpCheckpoint cp_p, BrotliAmdUndbpCheckpoint cp_s,
                                                         uint64_t first_p, uint64_t first_s, uint64_t j, uint32_t item_deltas, uint64_t value_in_p, uint64_t value_in_s) {
  BrotliAmdUndbaHostItem it;
  uint64_t hi, a, b;
  brotli_amd_undba_item_elems(brotli_amd_undba_m(res.count_p, res.count_s, sg.cap), j, item_deltas, &it.lo, &hi);
  it.d_in = j == 0u ? 0 : brotli_amd_undba_d(value_in_p, value_in_s);
  it.p.assign(hi - it.lo, 0);
  it.s.assign(hi - it.lo, 0);
  const BrotliAmdUndbpSeg sp = brotli_amd_undba_seg_p(sg), ss = brotli_amd_undba_seg_s(sg, res.consumed_p);
  const BrotliAmdUndlbaSeg lp = {sp.src, nullptr, sp.len, sp.cap, 0u, 0u, 0u, nullptr, 0u, 0u}, ls = {ss.src, nullptr, ss.len, ss.cap, 0u, 0u, 0u, nullptr, 0u, 0u};
  brotli_amd_undlba_host_each(lp, brotli_amd_undlba_result(brotli_amd_undba_walked_p(res), sp.len), cp_p, first_p, j, item_deltas, value_in_p, &a, &b,
                              [&](uint64_t e, uint64_t v) { if (e >= it.lo && e < hi) it.p[e - it.lo] = (int32_t)(uint32_t)v; });
  brotli_amd_undlba_host_each(ls, brotli_amd_undlba_result(brotli_amd_undba_walked_s(res), ss.len), cp_s, first_s, j, item_deltas, value_in_s, &a, &b,
                              [&](uint64_t e, uint64_t v) { if (e >= it.lo && e < hi) it.s[e - it.lo] = (int32_t)(uint32_t)v; });
  return it;
}
// The item's sums of L and of s up to its first bad element as tile records; that element goes into res->first_bad (items in any order give
// the same).
inline void brotli_amd_undba_host_lengths(const BrotliAmdUndbaHostItem& it, uint64_t j, BrotliAmdUndbaResult* res, BrotliAmdUndeltaTile* tile_l, BrotliAmdUndeltaTile* tile_s) {
  uint64_t sum_l = 0, sum_s = 0;
  int64_t d = it.d_in;
  for (size_t x = 0; x < it.p.size(); x++) {
    if (brotli_amd_undba_bad_kind(it.p[x], it.s[x], d) != BROTLI_AMD_UNDBA_BAD_NONE) {
      if (it.lo + x < res->first_bad) res->first_bad = it.lo + x;
      break;
    }
    d = (int64_t)it.p[x] + it.s[x];
    sum_l += (uint64_t)d; sum_s += (uint64_t)it.s[x];
  }
  *tile_l = brotli_amd_undbp_tile(j, 0u, sum_l);
  *tile_s = brotli_amd_undbp_tile(j, 0u, sum_s);
}
// The item's elements as the data phases take them: p and s of the elements below first_bad, 0 and 0 from it on.
struct BrotliAmdUndbaHostLens { std::vector<uint32_t> p, s; };
inline BrotliAmdUndbaHostLens brotli_amd_undba_host_lens(const BrotliAmdUndbaHostItem& it, uint64_t first_bad) {
  BrotliAmdUndbaHostLens got;
  got.p.assign(it.p.size(), 0u); got.s.assign(it.p.size(), 0u);
  for (size_t x = 0; x < it.p.size() && it.lo + x < first_bad; x++) { got.p[x] = (uint32_t)it.p[x]; got.s[x] = (uint32_t)it.s[x]; }
  return got;
}
// Item j's offsets on top of bytes_in (and suffix_in), by brotli_amd_undba_sum_in; the item of first_bad writes bad_kind, the segment's last
// item bytes, suffix_bytes and data_status.
inline void brotli_amd_undba_host_expand(const BrotliAmdUndbaSeg& sg, BrotliAmdUndbaResult* res, const BrotliAmdUndbaHostItem& it, uint64_t j, uint32_t item_deltas, uint64_t bytes_in,
                                         uint64_t suffix_in) {
  if (j == 0u) brotli_amd_undlba_first_offset(sg);
  const uint32_t ow = brotli_amd_undlba_offset_width(sg.flags);
  const uint64_t ends = brotli_amd_undlba_ends_at(sg), m = brotli_amd_undba_m(res->count_p, res->count_s, sg.cap);
  uint64_t run = bytes_in, run_s = suffix_in;
  int64_t d = it.d_in;
  for (size_t x = 0; x < it.p.size(); x++) {
    const uint64_t e = it.lo + x;
    if (e == res->first_bad) res->bad_kind = brotli_amd_undba_bad_kind(it.p[x], it.s[x], d);
    d = (int64_t)it.p[x] + it.s[x];
    if (e < res->first_bad) { run += (uint64_t)d; run_s += (uint64_t)it.s[x]; }
    if (sg.offsets != nullptr) brotli_amd_unvarint_store(ends + e * ow, ow, sg.offset_base + run);
  }
  uint64_t a, b;
  brotli_amd_undbp_item_range(m, m, j, item_deltas, &a, &b);
  if (brotli_amd_undlba_last_item(m, m, j, a, b)) brotli_amd_undba_finish(res, run, run_s);
}
// PHASE A over the item's n elements (p, s), whose bytes begin at bytes_in in the data and whose suffixes at suffix_in behind `suffixes`; cur:
// cap bytes.  -> the item's last element.
inline BrotliAmdUndbaLast brotli_amd_undba_host_a(uint64_t data, uint64_t keep, uint64_t suffixes, uint64_t avail, const uint32_t* p, const uint32_t* s, uint32_t n, uint64_t bytes_in,
                                                  uint64_t suffix_in, uint8_t* cur, uint32_t cap) {
  BrotliAmdUndbaLast last = {bytes_in, 0u, 0u};
  uint64_t at = bytes_in, q = suffix_in;
  uint32_t r = ~0u;
  for (uint32_t x = 0; x < n; x++) {
    const uint32_t len = p[x] + s[x];
    r = r < p[x] ? r : p[x];
    for (uint64_t k64 = r, end = brotli_amd_undba_stored(at, len, keep); k64 < end; k64++) {
      const uint32_t k = (uint32_t)k64;
      const uint32_t byte = brotli_amd_undba_a_byte(p, s, cur, cap, x, q, k, suffixes, avail);
      brotli_amd_undba_put(data, keep, at + k, byte);
      if (k >= p[x] && k < cap) cur[k] = (uint8_t)byte;
    }
    last = BrotliAmdUndbaLast{at, len, r};
    at += len; q += s[x];
  }
  return last;
}
// PHASE B over one segment's items, one after the other; cur: cap bytes.
inline void brotli_amd_undba_host_b(uint64_t data, uint64_t keep, const BrotliAmdUndbaLast* lasts, uint64_t items, uint8_t* cur, uint32_t cap) {
  for (uint64_t j = 0; j < items; j++) {
    const BrotliAmdUndbaLast me = lasts[j];
    const uint32_t r = j != 0u ? me.r : 0u;
    for (uint32_t k = 0, stored = (uint32_t)brotli_amd_undba_stored(me.at, r, keep); k < stored; k++) brotli_amd_undba_put(data, keep, me.at + k, k < cap ? cur[k] : brotli_amd_undba_far_byte(lasts, j, k, data, keep));
    // what phase A stored of this element goes behind what was carried into it
    for (uint32_t k = r; k < me.len && k < cap; k++) cur[k] = me.at + k < keep ? (uint8_t)brotli_amd_unshuffle_ld8(data + me.at + k) : 0u;
  }
}
// PHASE C over the n elements of an item j >= 1 but its last: their bytes [0, r_e) from the last element of item j - 1.
inline void brotli_amd_undba_host_c(uint64_t data, uint64_t keep, BrotliAmdUndbaLast before, const uint32_t* p, const uint32_t* s, uint32_t n, uint64_t bytes_in) {
  uint64_t at = bytes_in;
  uint32_t r = ~0u;
  for (uint32_t x = 0; x + 1u < n; x++) {
    r = r < p[x] ? r : p[x];
    for (uint32_t k = 0, stored = (uint32_t)brotli_amd_undba_stored(at, r, keep); k < stored; k++)
      brotli_amd_undba_put(data, keep, at + k, brotli_amd_unshuffle_ld8(data + before.at + k));
    at += p[x] + s[x];
  }
}
#endif  // BROTLI_AMD_UNDBA_H_
