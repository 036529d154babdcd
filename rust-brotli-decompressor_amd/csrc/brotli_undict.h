// brotli_undict.h -- dictionary-index runs back into VALUES: the load of one dictionary entry, the one function that turns an index into a value,
// and the host's walk and item, once, for the host and the device.
//
// THE TRANSFORM (include/brotli/batch.h has it in full).  A segment is an unrle segment (csrc/brotli_unrle.h) whose values are INDICES into a
// dictionary of D entries of w bytes (1, 2, 4 or 8) at dict, any alignment.  Element i of the destination, i < min(count, cap), is the entry
// that index i names, copied as it is; an index at or above D gives 0, is never made an address, and is counted: the segment's result has
// unrle's five fields, then `bad`, the delivered elements with such an index, and `first_bad`, the smallest of them.  The field width is bound
// by 32 alone -- the walk is unrle's, called with an element width of 8 --, so a dictionary of bytes may be addressed by fields of 12 bits.
//
// LOADS.  What unrle loads of [src, src + len); an entry as ONE load of w bytes where dict + idx w is a multiple of w -- where dict is --, byte
// by byte elsewhere: the store rule's mirror.  Nothing outside [dict, dict + D w) is read.  STORES: unrle's.
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUndictHost; tests/tools/undict_san.cpp) and the device
// (csrc/brotli_undict_kernels.hip); the device replaces the loop over an item's elements by its lanes, and the sums over an item's bad
// elements by a reduction in the wave and one atomic add and one atomic minimum.  Addresses are integers.
#ifndef BROTLI_AMD_UNDICT_H_
#define BROTLI_AMD_UNDICT_H_

#include "brotli/batch.h"       // BrotliAmdUndictResult, BROTLI_AMD_UNDICT_*
#include "brotli_device_abi.h"  // the segment of a launch: BrotliAmdUndictSeg
#include "brotli_unrle.h"       // the walk, a run, an element, the items

#define BROTLI_AMD_UNDICT_HD BROTLI_AMD_UNSHUFFLE_HD
#define BROTLI_AMD_UNDICT_FLAGS BROTLI_AMD_UNDICT_WIDTH_BYTE   // the flag bits there are
#define BROTLI_AMD_UNDICT_MAX_CAP BROTLI_AMD_UNRLE_MAX_CAP
#define BROTLI_AMD_UNDICT_MAX_ENTRIES ((uint64_t)1 << 56)      // (so that D w cannot overflow)
#define BROTLI_AMD_UNDICT_WALK_WIDTH 8u                        // the element width the walk is told: only k <= 32 binds
#define BROTLI_AMD_UNDICT_NONE (~(uint64_t)0)                  // first_bad where there is no bad element

static_assert(BROTLI_AMD_UNDICT_WIDTH_BYTE == BROTLI_AMD_UNRLE_WIDTH_BYTE, "the walk takes the flags as they are");
static_assert(sizeof(BrotliAmdUndictResult) == 48u, "unrle's five fields, bad and first_bad");

// ---- one entry ----
// The w bytes at address a, little-endian: one load where a is a multiple of w, single bytes elsewhere.
BROTLI_AMD_UNDICT_HD uint64_t brotli_amd_undict_load(uint64_t a, uint32_t w) {
  if ((a & (w - 1u)) == 0u) {
#if defined(__HIP_DEVICE_COMPILE__)
    switch (w) {
      case 1u: return *(const BROTLI_AMD_GLOBAL uint8_t*)a;
      case 2u: return *(const BROTLI_AMD_GLOBAL uint16_t*)a;
      case 4u: return *(const BROTLI_AMD_GLOBAL uint32_t*)a;
      default: return *(const BROTLI_AMD_GLOBAL uint64_t*)a;
    }
#else
    uint64_t v = 0;
    memcpy(&v, reinterpret_cast<const void*>((uintptr_t)a), w);   // (little-endian hosts)
    return v;
#endif
  }
  uint64_t v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t j = 0; j < 8u; j++)
    if (j < w) v |= (uint64_t)brotli_amd_unshuffle_ld8(a + j) << (8u * j);
  return v;
}

// ---- an index -> its value ----
struct BrotliAmdUndictValue { uint64_t value; uint32_t bad; };
// Entry idx of the `entries` entries of w bytes at dict.  The comparison is one of 64 bits, and an index that fails it is never multiplied or
// added to anything: its value is 0 and it is bad.  (idx < 2^32 and entries <= 2^56, so idx w cannot overflow.)
BROTLI_AMD_UNDICT_HD BrotliAmdUndictValue brotli_amd_undict_lookup(uint64_t dict, uint64_t entries, uint32_t w, uint64_t idx) {
  if (idx >= entries) return BrotliAmdUndictValue{0u, 1u};
  return BrotliAmdUndictValue{brotli_amd_undict_load(dict + idx * w, w), 0u};
}

// ---- the walk and an item over host memory ----
// ckpts[0 .. brotli_amd_unrle_items(sg.cap, item_elems)) start as BROTLI_AMD_UNRLE_NONE
inline BrotliAmdUndictResult brotli_amd_undict_host_walk(const BrotliAmdUndictSeg& sg, uint32_t item_elems, BrotliAmdUnrleCheckpoint* ckpts) {
  BrotliAmdUnrleDirect rd = {(uint64_t)(uintptr_t)sg.src};
  const BrotliAmdUnrleResult r = brotli_amd_unrle_walk(rd, sg.len, sg.cap, BROTLI_AMD_UNDICT_WALK_WIDTH, sg.bits, sg.flags, item_elems,
                                                       [&](uint64_t j0, uint64_t j1, uint64_t off, uint64_t first) {
    for (uint64_t j = j0; j < j1; j++) ckpts[j] = BrotliAmdUnrleCheckpoint{off, first};
  });
  return BrotliAmdUndictResult{r.count, r.consumed, r.runs, r.status, r.bits, 0u, BROTLI_AMD_UNDICT_NONE};
}
// item j of the segment, res being the walk's result and cp the item's checkpoint: its elements are stored, and its bad ones go into res->bad
// and res->first_bad (items in any order give the same)
inline void brotli_amd_undict_host_item(const BrotliAmdUndictSeg& sg, BrotliAmdUndictResult* res, BrotliAmdUnrleCheckpoint cp, uint64_t j, uint32_t item_elems) {
  const uint64_t dst = (uint64_t)(uintptr_t)sg.dst, dict = (uint64_t)(uintptr_t)sg.dict;
  brotli_amd_unrle_host_item_each((uint64_t)(uintptr_t)sg.src, sg.len, sg.cap, res->count, res->bits, cp, j, item_elems, [&](uint64_t e, uint64_t idx) {
    const BrotliAmdUndictValue v = brotli_amd_undict_lookup(dict, sg.dict_entries, sg.width, idx);
    brotli_amd_unvarint_store(dst + e * sg.width, sg.width, v.value);
    if (v.bad) { res->bad++; if (e < res->first_bad) res->first_bad = e; }
  });
}

#endif  // BROTLI_AMD_UNDICT_H_
