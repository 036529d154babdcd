// brotli_unnull.h -- dense values spread over nulls by DEFINITION LEVELS: the prefix rule, the present mask of a lane's slots, the step from a
// rank to a value, a validity byte and the bookkeeping of an item, once, for the host and the device.
//
// THE TRANSFORM (include/brotli/batch.h has it in full).  A segment's LEVELS are unrle runs (csrc/brotli_unrle.h) of fields of k bits; slot i
// of the destination, i < m = min(count, cap), is PRESENT where level_i == level, compared unmasked, and null elsewhere.  A present slot's RANK
// r_i is the number of present slots in front of it, and its value is the w bytes at values + r_i w where r_i < V; a present slot of rank
// >= V is MISSING: its value is 0, nothing is read through that rank, and it is counted.  A null slot's value is 0.  Bit i & 7 of byte i >> 3
// at valid -- Arrow's layout -- says whether slot i is present; exactly ceil(m / 8) bytes are written, the last one's bits at and above m as 0.
// With BROTLI_AMD_UNNULL_LENGTH_PREFIX the segment's first four bytes are the runs' length L, little-endian, and the runs are [4, 4 + L); with
// BROTLI_AMD_UNNULL_VALUES_FOLLOW the values are what lies behind the runs in the same segment.
//
// The walk, the checkpoints and the runs that cover an item are unrle's.  An ITEM is item_elems slots, a multiple of 8 -- so an item owns
// whole validity bytes --, and a LANE of an item has 16 neighbouring slots: their present mask (inside an RLE run one compare), the mask's
// popcount, and, on top of the ranks in front of the lane, the value of every slot.  An item's popcount is an undelta tile record -- a head for
// a segment's first item, a continuation otherwise, as undbp's sums are --, and undelta's carry launch gives every item the present slots in
// front of it.
//
// LOADS.  What unrle loads of the runs; a value as undict's entry (csrc/brotli_undict.h: brotli_amd_undict_lookup with the rank as the index).
// STORES.  unrle's for the slots; single bytes of the bitmap (the device gathers a lane's two bytes across lanes into aligned 16-byte stores).
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUnnullHost; tests/tools/unnull_san.cpp) and the device
// (csrc/brotli_unnull_kernels.hip); the device replaces the loop over an item's lanes by its lanes and the running rank by a scan in the wave.
// A segment's present and missing slots are written once, by the item that holds its last delivered slot: no atomics.  Addresses are integers.
#ifndef BROTLI_AMD_UNNULL_H_
#define BROTLI_AMD_UNNULL_H_

#include <algorithm>

#include "brotli/batch.h"       // BrotliAmdUnnullResult, BROTLI_AMD_UNNULL_*
#include "brotli_device_abi.h"  // the segment of a launch: BrotliAmdUnnullSeg
#include "brotli_undbp.h"       // an item's sum as a tile record: brotli_amd_undbp_tile
#include "brotli_undict.h"      // a rank -> its value: brotli_amd_undict_lookup
#include "brotli_unrle.h"       // the walk, a run, an element, the items

#define BROTLI_AMD_UNNULL_HD BROTLI_AMD_UNSHUFFLE_HD
#define BROTLI_AMD_UNNULL_FLAGS (BROTLI_AMD_UNNULL_LENGTH_PREFIX | BROTLI_AMD_UNNULL_VALUES_FOLLOW)   // the flag bits there are
#define BROTLI_AMD_UNNULL_MAX_CAP BROTLI_AMD_UNRLE_MAX_CAP
#define BROTLI_AMD_UNNULL_MAX_VALUES ((uint64_t)1 << 56)   // (so that V w cannot overflow)
#define BROTLI_AMD_UNNULL_WALK_WIDTH 8u                    // the element width the walk is told: only k <= 32 binds
#define BROTLI_AMD_UNNULL_LANE_SLOTS 16u                   // neighbouring slots of a lane: two validity bytes

static_assert(sizeof(BrotliAmdUnnullResult) == 56u, "unrle's five fields, present, missing and values");
static_assert(BROTLI_AMD_UNNULL_BAD_LENGTH == BROTLI_AMD_UNRLE_BAD_WIDTH + 1u, "a status of its own behind unrle's");

// an item's slots are whole validity bytes
BROTLI_AMD_UNNULL_HD bool brotli_amd_unnull_item_ok(uint32_t item_elems) { return item_elems != 0u && item_elems % 8u == 0u; }

// ---- the prefix rule ----
// where a segment's runs lie: [off, off + len) of it; status BROTLI_AMD_UNNULL_BAD_LENGTH: nowhere
struct BrotliAmdUnnullRuns { uint64_t off, len; uint32_t status; };
// rd reads the segment of len bytes from its first byte on (ensure and window: brotli_amd_unrle_walk's reader)
template <class Reader>
BROTLI_AMD_UNNULL_HD BrotliAmdUnnullRuns brotli_amd_unnull_prefix(Reader& rd, uint64_t len, uint32_t flags) {
  if ((flags & BROTLI_AMD_UNNULL_LENGTH_PREFIX) == 0u) return BrotliAmdUnnullRuns{0u, len, BROTLI_AMD_UNRLE_OK};
  if (len < 4u) return BrotliAmdUnnullRuns{0u, 0u, BROTLI_AMD_UNNULL_BAD_LENGTH};
  uint32_t b8;
  rd.ensure(0u);
  const uint64_t L = rd.window(0u, len, &b8) & 0xFFFFFFFFull;
  if (L > len - 4u) return BrotliAmdUnnullRuns{0u, 0u, BROTLI_AMD_UNNULL_BAD_LENGTH};
  return BrotliAmdUnnullRuns{4u, L, BROTLI_AMD_UNRLE_OK};
}
// the offset of the runs alone (what an item needs beside their length, which the walk leaves it)
BROTLI_AMD_UNNULL_HD uint64_t brotli_amd_unnull_runs_off(uint32_t flags) { return (flags & BROTLI_AMD_UNNULL_LENGTH_PREFIX) != 0u ? 4u : 0u; }

// The segment's result out of where its runs lie and what their walk said (r: over the runs alone): consumed counts from the segment's first
// byte, and `values` is the V that is used -- the argument's, or with VALUES_FOLLOW the whole elements behind runs that ended well.
BROTLI_AMD_UNNULL_HD BrotliAmdUnnullResult brotli_amd_unnull_result(const BrotliAmdUnnullSeg& sg, BrotliAmdUnnullRuns runs, BrotliAmdUnrleResult r) {
  if (runs.status != BROTLI_AMD_UNRLE_OK) return BrotliAmdUnnullResult{0u, 0u, 0u, runs.status, sg.bits, 0u, 0u, (sg.flags & BROTLI_AMD_UNNULL_VALUES_FOLLOW) != 0u ? 0u : sg.values_count};
  BrotliAmdUnnullResult res = {r.count, runs.off + r.consumed, r.runs, r.status, r.bits, 0u, 0u, sg.values_count};
  if ((sg.flags & BROTLI_AMD_UNNULL_VALUES_FOLLOW) != 0u) res.values = r.status == BROTLI_AMD_UNRLE_OK ? (sg.len - res.consumed) / sg.width : 0u;
  return res;
}
// the address of the dense values (not looked at where the result's `values` is 0)
BROTLI_AMD_UNNULL_HD uint64_t brotli_amd_unnull_values_at(const BrotliAmdUnnullSeg& sg, const BrotliAmdUnnullResult& res) {
  return (sg.flags & BROTLI_AMD_UNNULL_VALUES_FOLLOW) != 0u ? (uint64_t)(uintptr_t)sg.src + res.consumed : (uint64_t)(uintptr_t)sg.values;
}

// ---- the mask of a lane ----
// The present bits of the n (1 .. 16) values from value i0 on of ONE run of the runs at address src -- `payload` is the run's payload offset
// for a packed run and BROTLI_AMD_UNRLE_NONE for an RLE run, whose value is `value` --, bit 0 being value i0's.  Inside an RLE run: one
// compare, and no field is extracted.
BROTLI_AMD_UNNULL_HD uint32_t brotli_amd_unnull_run_mask(uint64_t src, uint64_t payload, uint32_t value, uint32_t k, uint32_t level, uint64_t i0, uint32_t n) {
  if (payload == BROTLI_AMD_UNRLE_NONE) return value == level ? (1u << n) - 1u : 0u;
  uint32_t mask = 0;
  for (uint32_t t = 0; t < n; t++) mask |= (brotli_amd_unrle_element(src, payload, value, k, i0 + t) == (uint64_t)level ? 1u : 0u) << t;
  return mask;
}
BROTLI_AMD_UNNULL_HD uint32_t brotli_amd_unnull_popcount(uint32_t mask) { return (uint32_t)__builtin_popcount(mask); }

// ---- a rank -> its value ----
// Slot t of a lane whose present mask is `mask` and whose first present slot has rank rank0: a null slot is 0; a present one is the value of
// rank rank0 + (the lane's present slots in front of it), by undict's bounds-checked entry load -- bad: the slot is missing.
BROTLI_AMD_UNNULL_HD BrotliAmdUndictValue brotli_amd_unnull_slot(uint64_t values, uint64_t V, uint32_t w, uint64_t rank0, uint32_t mask, uint32_t t) {
  if (((mask >> t) & 1u) == 0u) return BrotliAmdUndictValue{0u, 0u};
  return brotli_amd_undict_lookup(values, V, w, rank0 + brotli_amd_unnull_popcount(mask & ((1u << t) - 1u)));
}

// ---- a validity byte ----
// byte j (0 or 1) of a lane's mask: slots 8 j .. 8 j + 7 of the lane, LSB-first; the slots that a lane does not have are 0 in its mask
BROTLI_AMD_UNNULL_HD uint32_t brotli_amd_unnull_valid_byte(uint32_t mask, uint32_t j) { return (mask >> (8u * j)) & 0xFFu; }

// ---- the items ----
// An item's slots [e0, e1) are unrle's elements (brotli_amd_unrle_item_range); its validity bytes are [e0 / 8, ceil(e1 / 8)).

// ---- the segment's sums ----
// What the item that holds the segment's last delivered slot knows: the delivered slots that are there are its carry-in and its own, and their
// ranks are 0 .. present - 1, so exactly those at or above V are missing.
BROTLI_AMD_UNNULL_HD void brotli_amd_unnull_totals(uint64_t carry_in, uint64_t item_present, uint64_t V, uint64_t* present, uint64_t* missing) {
  *present = carry_in + item_present;
  *missing = *present > V ? *present - V : 0u;
}

// ---- the walk and an item over host memory ----
// ckpts[0 .. brotli_amd_unrle_items(sg.cap, item_elems)) start as BROTLI_AMD_UNRLE_NONE; *runs: where the segment's runs lie
inline BrotliAmdUnnullResult brotli_amd_unnull_host_walk(const BrotliAmdUnnullSeg& sg, uint32_t item_elems, BrotliAmdUnrleCheckpoint* ckpts, BrotliAmdUnnullRuns* runs) {
  BrotliAmdUnrleDirect whole = {(uint64_t)(uintptr_t)sg.src};
  *runs = brotli_amd_unnull_prefix(whole, sg.len, sg.flags);
  BrotliAmdUnrleResult r = {0u, 0u, 0u, BROTLI_AMD_UNRLE_OK, sg.bits};
  if (runs->status == BROTLI_AMD_UNRLE_OK) {
    BrotliAmdUnrleDirect rd = {(uint64_t)(uintptr_t)sg.src + runs->off};
    r = brotli_amd_unrle_walk(rd, runs->len, sg.cap, BROTLI_AMD_UNNULL_WALK_WIDTH, sg.bits, 0u, item_elems, [&](uint64_t j0, uint64_t j1, uint64_t off, uint64_t first) {
      for (uint64_t j = j0; j < j1; j++) ckpts[j] = BrotliAmdUnrleCheckpoint{off, first};
    });
  }
  return brotli_amd_unnull_result(sg, *runs, r);
}
// the present masks of item j's lanes, 16 slots each: masks[0 .. ceil(item_elems / 16)) start as 0
inline void brotli_amd_unnull_host_masks(const BrotliAmdUnnullSeg& sg, BrotliAmdUnnullRuns runs, const BrotliAmdUnnullResult& res, BrotliAmdUnrleCheckpoint cp, uint64_t j,
                                         uint32_t item_elems, uint32_t* masks) {
  const uint64_t src = (uint64_t)(uintptr_t)sg.src + runs.off;
  uint64_t e0, e1;
  brotli_amd_unrle_item_range(res.count, sg.cap, j, item_elems, &e0, &e1);
  if (cp.off == BROTLI_AMD_UNRLE_NONE || e0 >= e1) return;
  BrotliAmdUnrleDirect rd = {src};
  BrotliAmdUnrleWalk st = {cp.off, cp.first};
  for (uint64_t e = e0; e < e1;) {
    const BrotliAmdUnrleRun run = brotli_amd_unrle_run(rd, runs.len, res.bits, st);
    if (run.kind == BROTLI_AMD_UNRLE_STOP) return;   // (not below count)
    const uint64_t run_end = st.elems + run.count, payload = run.kind == BROTLI_AMD_UNRLE_RLE ? BROTLI_AMD_UNRLE_NONE : run.payload;
    while (e < run_end && e < e1) {   // the part of one lane that lies in this run
      const uint64_t lane = (e - e0) / BROTLI_AMD_UNNULL_LANE_SLOTS, lane_end = e0 + (lane + 1u) * BROTLI_AMD_UNNULL_LANE_SLOTS;
      const uint64_t stop = std::min(std::min(run_end, e1), lane_end);
      masks[lane] |= brotli_amd_unnull_run_mask(src, payload, run.value, res.bits, sg.level, e - st.elems, (uint32_t)(stop - e)) << (uint32_t)(e - (lane_end - BROTLI_AMD_UNNULL_LANE_SLOTS));
      e = stop;
    }
    st.off = run.next; st.elems = run_end;
    if (run.status != BROTLI_AMD_UNRLE_OK) return;
  }
}
// what item j leaves for the carry launch: its present slots
inline BrotliAmdUndeltaTile brotli_amd_unnull_host_count(const BrotliAmdUnnullSeg& sg, BrotliAmdUnnullRuns runs, const BrotliAmdUnnullResult& res, BrotliAmdUnrleCheckpoint cp,
                                                         uint64_t j, uint32_t item_elems, uint32_t* masks) {
  brotli_amd_unnull_host_masks(sg, runs, res, cp, j, item_elems, masks);
  uint64_t sum = 0;
  for (uint32_t l = 0; l < (item_elems + BROTLI_AMD_UNNULL_LANE_SLOTS - 1u) / BROTLI_AMD_UNNULL_LANE_SLOTS; l++) sum += brotli_amd_unnull_popcount(masks[l]);
  return brotli_amd_undbp_tile(j, 0u, sum);
}
// item j's slots and validity bytes on top of its carry-in, the present slots in front of it; the item that holds the segment's last
// delivered slot writes res's present and missing (items in any order give the same)
inline void brotli_amd_unnull_host_expand(const BrotliAmdUnnullSeg& sg, BrotliAmdUnnullRuns runs, BrotliAmdUnnullResult* res, BrotliAmdUnrleCheckpoint cp, uint64_t j,
                                          uint32_t item_elems, uint64_t carry_in, uint32_t* masks) {
  uint64_t e0, e1;
  brotli_amd_unrle_item_range(res->count, sg.cap, j, item_elems, &e0, &e1);
  if (cp.off == BROTLI_AMD_UNRLE_NONE || e0 >= e1) return;
  brotli_amd_unnull_host_masks(sg, runs, *res, cp, j, item_elems, masks);
  const uint64_t dst = (uint64_t)(uintptr_t)sg.dst, valid = (uint64_t)(uintptr_t)sg.valid, values = brotli_amd_unnull_values_at(sg, *res);
  uint64_t rank0 = carry_in;
  for (uint64_t la = e0; la < e1; la += BROTLI_AMD_UNNULL_LANE_SLOTS) {
    const uint32_t mask = masks[(la - e0) / BROTLI_AMD_UNNULL_LANE_SLOTS], m = (uint32_t)std::min<uint64_t>(BROTLI_AMD_UNNULL_LANE_SLOTS, e1 - la);
    for (uint32_t t = 0; t < m; t++) {
      const BrotliAmdUndictValue v = brotli_amd_unnull_slot(values, res->values, sg.width, rank0, mask, t);
      brotli_amd_unvarint_store(dst + (la + t) * sg.width, sg.width, v.value);
    }
    if (valid != 0u)
      for (uint32_t b = 0; 8u * b < m; b++) brotli_amd_unvarint_store(valid + (la >> 3) + b, 1u, brotli_amd_unnull_valid_byte(mask, b));
    rank0 += brotli_amd_unnull_popcount(mask);
  }
  if (e1 == (res->count < sg.cap ? res->count : sg.cap)) brotli_amd_unnull_totals(carry_in, rank0 - carry_in, res->values, &res->present, &res->missing);
}

#endif  // BROTLI_AMD_UNNULL_H_
