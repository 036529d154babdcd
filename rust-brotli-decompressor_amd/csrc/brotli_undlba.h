// brotli_undlba.h -- Parquet's DELTA_LENGTH_BYTE_ARRAY back into an Arrow string column, (offsets, data): the step from a value to a length,
// the tile record of an item's bytes, where an element's end goes, what the segment's last item leaves, and the host's phases, once, for the
// host and the device.
//
// THE TRANSFORM (include/brotli/batch.h has it in full).  A segment of len bytes is a DELTA_BINARY_PACKED stream of N values and, directly
// behind it -- at `consumed` --, the elements' bytes back to back.  The stream is undbp's (csrc/brotli_undbp.h): its walk, its items of
// item_deltas deltas, its checkpoints, its groups, and the items' sums with undelta's carry launch over them give every item the value in front
// of its first delta.  Element i of the segment, i < m = min(count, cap), has the LENGTH L_i: the low 32 bits of v_i as a signed int32; a
// negative one gives an EMPTY element and is counted (bad, first_bad).  An item's good lengths are summed up (a second tile record), the carry
// launch over those gives every item the bytes in front of it, and then the item writes the ENDS of its elements: offsets[e + 1] = offset_base
// + the lengths up to and with e.  Item 0 has element 0 and offsets[0] as well.  The item that holds the segment's last delivered element knows
// the segment's bytes: it writes them, data_status, and the segment's copy -- min(bytes, data_avail, data_cap) bytes from src + consumed to
// data --, which the ragged copy (csrc/brotli_copy_kernels.hip) takes.  Items of one segment write disjoint bytes.
//
// LOADS.  What undbp loads of [src, src + len), and the copy's source inside it.  STORES.  An offset as one store of its width where its
// address is a multiple of it, byte by byte elsewhere (the device puts a lane's neighbouring offsets together into aligned 16-byte stores).
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUndlbaHost; tests/tools/undlba_san.cpp) and the device
// (csrc/brotli_undlba_kernels.hip); the device replaces the loops over an item's groups by its lanes.  Addresses are integers.
#ifndef BROTLI_AMD_UNDLBA_H_
#define BROTLI_AMD_UNDLBA_H_

#include "brotli/batch.h"       // BrotliAmdUndlbaResult, BROTLI_AMD_UNDLBA_*
#include "brotli_device_abi.h"  // the segment of a launch: BrotliAmdUndlbaSeg; a copy: BrotliAmdCopySeg
#include "brotli_undbp.h"       // the walk, an item's blocks, a group, the tile record

#define BROTLI_AMD_UNDLBA_HD BROTLI_AMD_UNSHUFFLE_HD
#define BROTLI_AMD_UNDLBA_FLAGS (BROTLI_AMD_UNDLBA_OFFSETS64 | BROTLI_AMD_UNDLBA_ENDS_ONLY)   // a segment's
#define BROTLI_AMD_UNDLBA_MAX_CAP BROTLI_AMD_UNDBP_MAX_CAP
#define BROTLI_AMD_UNDLBA_NONE (~(uint64_t)0)   // first_bad where no element was bad

static_assert(sizeof(BrotliAmdUndlbaResult) == 80u, "undbp's seven fields, data_status, and bad, first_bad, bytes, data_avail");

// ---- a value -> its length ----
struct BrotliAmdUndlbaLength { uint32_t len, bad; };
// Parquet's INT32 arithmetic: the low 32 bits of the value, signed.  A negative length is never added to anything: the element is empty and bad.
BROTLI_AMD_UNDLBA_HD BrotliAmdUndlbaLength brotli_amd_undlba_length(uint64_t v) {
  const uint32_t low = (uint32_t)v;
  return (low >> 31) != 0u ? BrotliAmdUndlbaLength{0u, 1u} : BrotliAmdUndlbaLength{low, 0u};
}

// ---- the result ----
// what the walk leaves of a segment of len bytes: what the items add to
BROTLI_AMD_UNDLBA_HD BrotliAmdUndlbaResult brotli_amd_undlba_result(const BrotliAmdUndbpResult& r, uint64_t len) {
  return BrotliAmdUndlbaResult{r.count, r.consumed, r.declared, r.blocks, r.status, r.block_values, r.miniblocks, BROTLI_AMD_UNDLBA_DATA_OK,
                               0u, BROTLI_AMD_UNDLBA_NONE, 0u, len - r.consumed};
}
// ... and the walk's own part of it again
BROTLI_AMD_UNDLBA_HD BrotliAmdUndbpResult brotli_amd_undlba_walked(const BrotliAmdUndlbaResult& r) {
  return BrotliAmdUndbpResult{r.count, r.consumed, r.declared, r.blocks, r.status, r.block_values, r.miniblocks};
}
// the segment as undbp's walk and items take it (they write nothing)
BROTLI_AMD_UNDLBA_HD BrotliAmdUndbpSeg brotli_amd_undlba_lengths_seg(const BrotliAmdUndlbaSeg& sg) {
  return BrotliAmdUndbpSeg{sg.src, nullptr, sg.len, sg.cap, sg.first_item, 8u, 0u};
}

// ---- the tile record of an item's bytes: the first item of a segment is a head ----
BROTLI_AMD_UNDLBA_HD BrotliAmdUndeltaTile brotli_amd_undlba_tile(uint64_t j, uint64_t bytes) { return brotli_amd_undbp_tile(j, 0u, bytes); }

// ---- the offsets ----
BROTLI_AMD_UNDLBA_HD uint32_t brotli_amd_undlba_offset_width(uint32_t flags) { return (flags & BROTLI_AMD_UNDLBA_OFFSETS64) != 0u ? 8u : 4u; }
// offsets[0], which the segment's first item writes whether it has elements or not
BROTLI_AMD_UNDLBA_HD void brotli_amd_undlba_first_offset(const BrotliAmdUndlbaSeg& sg) {
  if (sg.offsets != nullptr && (sg.flags & BROTLI_AMD_UNDLBA_ENDS_ONLY) == 0u)
    brotli_amd_unvarint_store((uint64_t)(uintptr_t)sg.offsets, brotli_amd_undlba_offset_width(sg.flags), sg.offset_base);
}
// the address of the END of element 0 -- offsets[1] --; that of element e lies e offset widths behind it
BROTLI_AMD_UNDLBA_HD uint64_t brotli_amd_undlba_ends_at(const BrotliAmdUndlbaSeg& sg) {
  return (uint64_t)(uintptr_t)sg.offsets + ((sg.flags & BROTLI_AMD_UNDLBA_ENDS_ONLY) != 0u ? 0u : brotli_amd_undlba_offset_width(sg.flags));
}

// ---- the segment's last item ----
// whether item j, of the deltas [a, b) by brotli_amd_undbp_item_range, holds the last of the segment's min(count, cap) elements; a segment
// without elements has its first item for it
BROTLI_AMD_UNDLBA_HD bool brotli_amd_undlba_last_item(uint64_t count, uint64_t cap, uint64_t j, uint64_t a, uint64_t b) {
  const uint64_t m = count < cap ? count : cap, dn = m != 0u ? m - 1u : 0u;
  return dn == 0u ? j == 0u : a < b && b == dn;
}
// What that item leaves, `bytes` being the good lengths of all delivered elements: the result's bytes and data_status, and the segment's copy.
BROTLI_AMD_UNDLBA_HD void brotli_amd_undlba_finish(const BrotliAmdUndlbaSeg& sg, BrotliAmdUndlbaResult* res, uint64_t bytes, BrotliAmdCopySeg* copy) {
  const uint64_t consumed = res->consumed, avail = sg.len - consumed;   // (the walk's: consumed <= len)
  res->bytes = bytes;
  res->data_status = bytes <= avail ? BROTLI_AMD_UNDLBA_DATA_OK : BROTLI_AMD_UNDLBA_DATA_SHORT;
  uint64_t keep = bytes < avail ? bytes : avail;
  keep = keep < sg.data_cap ? keep : sg.data_cap;
  *copy = BrotliAmdCopySeg{sg.src + consumed, sg.data, sg.data != nullptr ? keep : 0u};
}

// ---- the walk and an item over host memory (the device replaces the loops over an item's groups by its lanes) ----
// ckpts[0 .. brotli_amd_undbp_items(sg.cap, item_deltas)) start as BROTLI_AMD_UNDBP_NONE
inline BrotliAmdUndlbaResult brotli_amd_undlba_host_walk(const BrotliAmdUndlbaSeg& sg, uint32_t item_deltas, BrotliAmdUndbpCheckpoint* ckpts, uint64_t* first) {
  return brotli_amd_undlba_result(brotli_amd_undbp_host_walk(brotli_amd_undlba_lengths_seg(sg), item_deltas, ckpts, first), sg.len);
}
// item j's deltas as its tile record: undbp's
inline BrotliAmdUndeltaTile brotli_amd_undlba_host_sum(const BrotliAmdUndlbaSeg& sg, const BrotliAmdUndlbaResult& res, BrotliAmdUndbpCheckpoint cp, uint64_t first, uint64_t j,
                                                       uint32_t item_deltas) {
  return brotli_amd_undbp_host_sum(brotli_amd_undlba_lengths_seg(sg), brotli_amd_undlba_walked(res), cp, first, j, item_deltas);
}
// each(e, v) for the elements of item j, value_in being the value in front of its first delta: element 0 in a segment's first item, then the
// one behind each of its deltas -> the item's deltas [*a, *b)
template <class Each>
inline void brotli_amd_undlba_host_each(const BrotliAmdUndlbaSeg& sg, const BrotliAmdUndlbaResult& res, BrotliAmdUndbpCheckpoint cp, uint64_t first, uint64_t j,
                                        uint32_t item_deltas, uint64_t value_in, uint64_t* a, uint64_t* b, Each each) {
  brotli_amd_undbp_item_range(res.count, sg.cap, j, item_deltas, a, b);
  if (cp.off == BROTLI_AMD_UNDBP_NONE) return;
  uint64_t v = value_in;
  if (j == 0u) {
    if (res.count == 0u || sg.cap == 0u) return;
    v += first;
    each((uint64_t)0, v);
  }
  if (*a >= *b) return;
  const uint64_t src = (uint64_t)(uintptr_t)sg.src;
  BrotliAmdUnrleDirect rd = {src};
  brotli_amd_undbp_item_blocks(rd, sg.len, res.block_values / res.miniblocks, res.miniblocks, cp, *a, *b, [&](uint64_t lo, uint64_t hi, uint64_t pos, uint32_t k, uint64_t md, uint64_t m0) {
    for (uint64_t d = lo; d < hi; d++) {
      v += md + brotli_amd_undbp_field(src + pos, k, (uint32_t)(d - m0));
      each(d + 1u, v);
    }
  });
}
// item j's good lengths as its tile record; its bad elements go into res->bad and res->first_bad (items in any order give the same)
inline BrotliAmdUndeltaTile brotli_amd_undlba_host_lengths(const BrotliAmdUndlbaSeg& sg, BrotliAmdUndlbaResult* res, BrotliAmdUndbpCheckpoint cp, uint64_t first, uint64_t j,
                                                           uint32_t item_deltas, uint64_t value_in) {
  uint64_t a, b, sum = 0;
  brotli_amd_undlba_host_each(sg, *res, cp, first, j, item_deltas, value_in, &a, &b, [&](uint64_t e, uint64_t v) {
    const BrotliAmdUndlbaLength L = brotli_amd_undlba_length(v);
    sum += L.len;
    if (L.bad != 0u) { res->bad++; if (e < res->first_bad) res->first_bad = e; }
  });
  return brotli_amd_undlba_tile(j, sum);
}
// Item j's offsets on top of bytes_in, the bytes of the elements in front of it; the segment's last item writes the result's bytes and
// data_status, and *copy.
inline void brotli_amd_undlba_host_expand(const BrotliAmdUndlbaSeg& sg, BrotliAmdUndlbaResult* res, BrotliAmdUndbpCheckpoint cp, uint64_t first, uint64_t j,
                                          uint32_t item_deltas, uint64_t value_in, uint64_t bytes_in, BrotliAmdCopySeg* copy) {
  if (j == 0u) brotli_amd_undlba_first_offset(sg);
  const uint32_t ow = brotli_amd_undlba_offset_width(sg.flags);
  const uint64_t ends = brotli_amd_undlba_ends_at(sg);
  uint64_t a, b, run = bytes_in;
  brotli_amd_undlba_host_each(sg, *res, cp, first, j, item_deltas, value_in, &a, &b, [&](uint64_t e, uint64_t v) {
    run += brotli_amd_undlba_length(v).len;
    if (sg.offsets != nullptr) brotli_amd_unvarint_store(ends + e * ow, ow, sg.offset_base + run);
  });
  if (brotli_amd_undlba_last_item(res->count, sg.cap, j, a, b)) brotli_amd_undlba_finish(sg, res, run, copy);
}
// the data: a copy, byte by byte (the device's is the ragged copy)
inline void brotli_amd_undlba_host_copy(const BrotliAmdCopySeg& copy) {
  const uint64_t src = (uint64_t)(uintptr_t)copy.src, dst = (uint64_t)(uintptr_t)copy.dst;
  for (uint64_t p = 0; p < copy.len; p++) brotli_amd_unvarint_store(dst + p, 1u, brotli_amd_unshuffle_ld8(src + p));
}

#endif  // BROTLI_AMD_UNDLBA_H_
