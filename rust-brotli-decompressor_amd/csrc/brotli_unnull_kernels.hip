// brotli_unnull_kernels.hip -- four launches in stream order that spread the dense values of n independent segments over their nulls by
// definition levels, and give every segment its slots, its validity bitmap and its result (gfx950, wave64).  The transform, the prefix rule, a
// lane's present mask, the step from a rank to a value and the bookkeeping of an item are csrc/brotli_unnull.h; the grammar, one run and the
// checkpoints are unrle's (csrc/brotli_unrle.h).  No block ever waits for another block's result -- no look-back, no flags, no spins, no grid
// barrier, no atomics on the bitmap.
//   1. brotli_amd_unnull_walk_kernel    ONE WAVE A SEGMENT: with a length prefix the wave reads its four bytes through the stage of
//                                       csrc/brotli_wave_stage.h, then unrle's walk as it is over the runs.  It writes the segment's result --
//                                       present 0, missing 0, the V that is used --, the runs' length, the checkpoint of every item and the
//                                       segment's entry of the items' prefix array.
//   2. brotli_amd_unnull_count_kernel   ONE WAVE AN ITEM, over the items of all segments in one flat list, on unrle's collection of the runs
//                                       that cover the item.  A lane forms the present mask of its 16 NEIGHBOURING slots -- inside an RLE run
//                                       one compare, no field is extracted --, and the wave's popcount is the item's undelta tile record.
//   3. brotli_amd_undelta_carry_kernel  undelta's carry launch itself (csrc/brotli_undelta_kernels.hip), over those records: a running sum
//                                       with restarts at the segments' first items -> every item's carry-in, the present slots in front of it.
//   4. brotli_amd_unnull_expand_kernel  the same item function; a scan over the lanes' popcounts and the carry-in give a lane its first rank.
//                                       Its present slots have consecutive ranks, so neighbouring lanes read neighbouring values: the loads
//                                       go in groups of kGroup, none waiting for another, and a rank at or above V is never made an address.
//                                       Slots are put together into aligned 16-byte stores, single ones at the edges.  A lane has two
//                                       validity bytes; the lanes' bytes are gathered across the wave, a lane an aligned 16-byte word of the
//                                       bitmap, stored whole where the item covers it and byte by byte at the item's two ends.  The item
//                                       that holds the segment's last delivered slot writes the result's present and missing: its carry-in
//                                       and its own popcount are all of them.  (One atomicAdd an item, as first built, cost 3 ms on one
//                                       segment of 65 536 items: they all hit one address.  profiles/unnull.txt.)
// THE SCRATCH behind the table: the n results, the n lengths of the runs, the items' prefix array (n + 1 entries), and for every item a
// checkpoint -- set to BROTLI_AMD_UNRLE_NONE in front of the walk --, a tile record and a carry.  A call that only counts has no items and is
// the first launch alone.
// The collection of an item's runs into LDS and a lane's way through them are csrc/brotli_run_items.h.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_run_items.h"    // the run batch, the walk's frame, the scratch and the launcher
#include "brotli_seg_walk.h"
#include "brotli_unnull.h"
#include "brotli_wave_stage.h"   // the wave's view of its source through LDS, same(), Word16, wave_grid

namespace {

constexpr uint32_t kThreads = brotli_amd_wave::kSegThreads, kWaves = brotli_amd_wave::kSegWaves;
constexpr uint32_t kChunk = BROTLI_AMD_UNRLE_WALK_CHUNK, kItem = BROTLI_AMD_UNRLE_ITEM_ELEMS;
constexpr uint32_t kPerLane = kItem / 64u;   // neighbouring slots of a lane
constexpr uint32_t kBatch = brotli_amd_wave::kRunBatch;
#ifndef BROTLI_AMD_UNNULL_GROUP
#define BROTLI_AMD_UNNULL_GROUP 4u
#endif
constexpr uint32_t kGroup = BROTLI_AMD_UNNULL_GROUP;   // slots of a lane whose value loads are in flight together (4, 8 or 16: profiles/unnull.txt)

static_assert(kChunk == brotli_amd_wave::kStageChunk, "the chunk the stage has");
static_assert(kPerLane == BROTLI_AMD_UNNULL_LANE_SLOTS && kPerLane % kGroup == 0u, "a lane's slots are two validity bytes and whole 16-byte words, in whole groups");
static_assert(kItem / 8u == 128u, "an item's validity bytes: eight 16-byte words, nine where the bitmap is not aligned");

using brotli_amd_wave::RunBatch;
using brotli_amd_wave::RunCursor;
using brotli_amd_wave::same;
using brotli_amd_wave::Stage;
using brotli_amd_wave::Word16;

typedef BrotliAmdUnnullSeg Seg;
typedef BrotliAmdUnnullResult Result;
typedef BrotliAmdUnrleCheckpoint Checkpoint;
typedef BrotliAmdUndeltaTile Tile;

// ---- launch 1 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_unnull_walk_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* __restrict__ results,
                                                                          uint64_t* __restrict__ run_lens, uint64_t* __restrict__ pre, Checkpoint* __restrict__ ckpts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  struct Walked { BrotliAmdUnnullRuns runs; BrotliAmdUnrleResult r; };
  brotli_amd_wave::walk_segments(
      stage, segs, n, items, pre, ckpts,
      [](const Seg& sg, Stage& whole, auto mark) {
        Walked got = {brotli_amd_unnull_prefix(whole, sg.len, sg.flags), {0u, 0u, 0u, BROTLI_AMD_UNRLE_OK, sg.bits}};
        if (got.runs.status == BROTLI_AMD_UNRLE_OK) {   // (the same in every lane)
          Stage rd(whole.lds, (uint64_t)(uintptr_t)sg.src + got.runs.off, got.runs.len, whole.lane);
          got.r = brotli_amd_unrle_walk(rd, got.runs.len, sg.cap, BROTLI_AMD_UNNULL_WALK_WIDTH, sg.bits, 0u, kItem, mark);
        }
        return got;
      },
      [&](uint64_t i, const Seg& sg, const Walked& got) {
        results[i] = brotli_amd_unnull_result(sg, got.runs, got.r);   // (what the items add to)
        run_lens[i] = got.runs.len;
      });
}

// ---- launches 2 and 4 ----
// The present mask of this lane's slots [la, lb) of an item that ends at slot e1, whose runs -- len bytes at address src, fields of k bits --
// are walked from the checkpoint cp on: bit t is slot la + t's.  batch: the wave's room for a batch of runs.
__device__ __forceinline__ uint32_t item_mask(uint8_t* lds, RunBatch batch, uint64_t src, uint64_t len, uint32_t k, uint32_t level,
                                              Checkpoint cp, uint64_t e1, uint64_t la, uint64_t lb, uint32_t lane) {
  Stage rd(lds, src, len, lane);
  BrotliAmdUnrleWalk st = {cp.off, cp.first};
  uint32_t mask = 0;
  bool more = true;
  while (more && st.elems < e1) {
    batch.collect(rd, len, k, st, more, e1, lane);
    // this lane's slots among the batch's: run after run, each part's bits at once
    const uint64_t a = la > batch.lo ? la : batch.lo, b = lb < st.elems ? lb : st.elems;
    if (a < b) {
      RunCursor<false> run(batch, a);
      uint64_t e = a;
      while (e < b) {
        run.seek(e);
        const uint64_t stop = b < run.end ? b : run.end;
        mask |= brotli_amd_unnull_run_mask(src, batch.payload[run.r], batch.value[run.r], k, level, e - run.first, (uint32_t)(stop - e)) << (uint32_t)(e - la);
        e = stop;
      }
    }
  }
  return mask;
}

__global__ __launch_bounds__(kThreads) void brotli_amd_unnull_count_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, const Result* __restrict__ results,
                                                                           const uint64_t* __restrict__ run_lens, const uint64_t* __restrict__ pre,
                                                                           const Checkpoint* __restrict__ ckpts, Tile* __restrict__ tiles) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  __shared__ uint64_t run_first[kWaves][kBatch + 1u];   // the first slot of every run of the batch; behind the last: the batch's end
  __shared__ uint64_t run_payload[kWaves][kBatch];      // (BROTLI_AMD_UNRLE_NONE: an RLE run)
  __shared__ uint32_t run_value[kWaves][kBatch];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    const Checkpoint cp = ckpts[g];
    const uint32_t i = brotli_amd_seg_find(pre, n, g);
    const uint64_t j = g - pre[i];
    uint32_t sum = 0;
    if (cp.off != BROTLI_AMD_UNRLE_NONE) {   // (beyond count otherwise; the same in every lane)
      const Seg sg = segs[i];
      uint64_t e0, e1;
      brotli_amd_unrle_item_range(results[i].count, sg.cap, j, kItem, &e0, &e1);
      if (e0 < e1) {
        const uint64_t la = e0 + (uint64_t)kPerLane * lane, lb = la + kPerLane < e1 ? la + kPerLane : e1;   // this lane's slots
        sum = brotli_amd_unnull_popcount(item_mask(stage[wave], RunBatch(run_first[wave], run_payload[wave], run_value[wave]),
                                                   (uint64_t)(uintptr_t)sg.src + brotli_amd_unnull_runs_off(sg.flags), run_lens[i], results[i].bits, sg.level, cp, e1, la, lb, lane));
#pragma unroll
        for (uint32_t off = 32; off != 0u; off >>= 1) sum += (uint32_t)__shfl_down((int)sum, off, 64);
      }
    }
    if (lane == 0u) tiles[g] = brotli_amd_undbp_tile(j, 0u, sum);
  }
}

// The slots [g0, g0 + kGroup) below m of a lane whose m slots (1 .. 16) begin at address at0 and whose present mask is `mask`, the first
// present one of rank rank0: their values out of the V dense ones of W bytes at `values`, and stored -- single slots in front of `head` and
// from `tail` on, whole 16-byte words between.  (undict's store rule, in lines of its own as there: one helper for both measured slower in
// both, profiles/run_items.txt.)
template <uint32_t W>
__device__ __forceinline__ void gather_and_store(uint64_t values, uint64_t V, uint64_t rank0, uint32_t mask, uint64_t at0, uint32_t m, uint32_t head, uint32_t tail,
                                                 uint32_t g0, Word16* word) {
  constexpr uint32_t per_word = 16u / W;
  uint64_t val[kGroup];
  // the loads, none of which waits for another (a slot at or above m has no bit; a missing one is 0)
#pragma unroll
  for (uint32_t u = 0; u < kGroup; u++) val[u] = brotli_amd_unnull_slot(values, V, W, rank0, mask, g0 + u).value;
#pragma unroll
  for (uint32_t u = 0; u < kGroup; u++) {
    const uint32_t t = g0 + u;
    if (t >= m) {
    } else if (t < head || t >= tail) {
      brotli_amd_unvarint_store(at0 + (uint64_t)t * W, W, val[u]);
    } else {
      const uint32_t pos = (t - head) & (per_word - 1u);
      word->put(pos * W, W, val[u]);
      if (pos == per_word - 1u) { brotli_amd_unshuffle_st128(at0 + (uint64_t)(t - pos) * W, word->word()); *word = Word16(); }
    }
  }
}

__global__ __launch_bounds__(kThreads) void brotli_amd_unnull_expand_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* results,
                                                                            const uint64_t* __restrict__ run_lens, const uint64_t* __restrict__ pre,
                                                                            const Checkpoint* __restrict__ ckpts, const uint64_t* __restrict__ carries) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  __shared__ uint64_t run_first[kWaves][kBatch + 1u];
  __shared__ uint64_t run_payload[kWaves][kBatch];
  __shared__ uint32_t run_value[kWaves][kBatch];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    const Checkpoint cp = ckpts[g];
    if (cp.off == BROTLI_AMD_UNRLE_NONE) continue;   // (beyond count; the same in every lane)
    const uint32_t i = brotli_amd_seg_find(pre, n, g);
    const Seg sg = segs[i];
    const Result res = results[i];   // (what the walk left: present and missing are not looked at)
    const uint32_t w = sg.width;
    uint64_t e0, e1;
    brotli_amd_unrle_item_range(res.count, sg.cap, g - pre[i], kItem, &e0, &e1);
    if (e0 >= e1) continue;
    const uint64_t la = e0 + (uint64_t)kPerLane * lane, lb = la + kPerLane < e1 ? la + kPerLane : e1;   // this lane's slots
    const uint32_t m = la < lb ? (uint32_t)(lb - la) : 0u;
    const uint32_t mask = item_mask(stage[wave], RunBatch(run_first[wave], run_payload[wave], run_value[wave]), (uint64_t)(uintptr_t)sg.src + brotli_amd_unnull_runs_off(sg.flags),
                                    run_lens[i], res.bits, sg.level, cp, e1, la, lb, lane);
    // this lane's first rank: the item's carry-in and the present slots of the lanes below
    const uint32_t pc = brotli_amd_unnull_popcount(mask);
    uint32_t inc = pc;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
      const uint32_t q = (uint32_t)__shfl_up((int)inc, off, 64);
      if (lane >= off) inc += q;
    }
    const uint64_t rank0 = carries[g] + (inc - pc);
    // group after group of the lane's slots: a group's loads together, then its stores
    if (m != 0u) {
      const uint64_t values = brotli_amd_unnull_values_at(sg, res), V = res.values;
      const uint64_t at0 = (uint64_t)(uintptr_t)sg.dst + la * w;
      const uint32_t per_word = 16u / w, to_word = ((16u - ((uint32_t)at0 & 15u)) & 15u) / w;
      const uint32_t head = (at0 & (w - 1u)) != 0u || to_word > m ? m : to_word, tail = head + (m - head) / per_word * per_word;
      Word16 word;
#pragma unroll 1
      for (uint32_t g0 = 0; g0 < m; g0 += kGroup) {
        switch (w) {   // (the same in every lane)
          case 1u: gather_and_store<1u>(values, V, rank0, mask, at0, m, head, tail, g0, &word); break;
          case 2u: gather_and_store<2u>(values, V, rank0, mask, at0, m, head, tail, g0, &word); break;
          case 4u: gather_and_store<4u>(values, V, rank0, mask, at0, m, head, tail, g0, &word); break;
          default: gather_and_store<8u>(values, V, rank0, mask, at0, m, head, tail, g0, &word); break;
        }
      }
    }
    // the bitmap: lane q takes the q-th aligned 16-byte word that the item's validity bytes touch, and gathers its bytes from the lanes' masks
    if (sg.valid != nullptr) {   // (the same in every lane)
      const uint64_t vb0 = (uint64_t)(uintptr_t)sg.valid + (e0 >> 3);
      const uint32_t nbytes = (uint32_t)((e1 - e0 + 7u) >> 3), skew = (uint32_t)vb0 & 15u;
      const uint64_t A = (vb0 & ~(uint64_t)15) + 16u * lane;
      Word16 vw;
      uint32_t inside = 0;
#pragma unroll
      for (uint32_t q = 0; q < 16u; q++) {
        const uint32_t bi = 16u * lane + q - skew;   // the validity byte of the item at A + q (wraps below 0: not inside)
        const uint32_t from = (uint32_t)__shfl((int)mask, (int)((bi >> 1) & 63u), 64);   // (every lane takes part)
        if (bi < nbytes) { vw.put(q, 1u, brotli_amd_unnull_valid_byte(from, bi & 1u)); inside |= 1u << q; }
      }
      if (inside == 0xFFFFu) {
        brotli_amd_unshuffle_st128(A, vw.word());
      } else if (inside != 0u) {
#pragma unroll
        for (uint32_t q = 0; q < 16u; q++)
          if (((inside >> q) & 1u) != 0u) brotli_amd_unvarint_store(A + q, 1u, (q < 8u ? vw.lo >> (8u * q) : vw.hi >> (8u * (q - 8u))) & 0xFFu);
      }
    }
    // the segment's present and missing slots: the item that holds its last delivered slot has them all
    if (e1 == (res.count < sg.cap ? res.count : sg.cap)) {   // (the same in every lane)
      uint32_t present = pc;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) present += __shfl_xor(present, off);
      if (lane == 0u) brotli_amd_unnull_totals(carries[g], present, res.values, &results[i].present, &results[i].missing);
    }
  }
}

}  // namespace

// the scratch of a launch over `units` units of n segments -- a unit a segment and a unit an item --: the results first, then the runs' lengths,
// the items' prefix array, the checkpoints, the tile records and the carries
extern "C" uint64_t brotli_amd_unnull_scratch_bytes(uint64_t units, uint32_t n) {
  return brotli_amd_wave::ItemScratch<Result, Checkpoint, true, true>::bytes(units - n, n);
}

// units: n + the items of all segments (the host has the table); d_scratch: brotli_amd_unnull_scratch_bytes of device memory, 16-byte aligned;
// ev[0..4], where not NULL, are recorded in front of, between and behind the four launches
extern "C" hipError_t brotli_amd_launch_unnull(const void* d_table, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  return brotli_amd_wave::launch_walk_count_carry_expand<Seg, Result, Checkpoint>(brotli_amd_unnull_walk_kernel, brotli_amd_unnull_count_kernel, brotli_amd_unnull_expand_kernel, d_table,
                                                                                  n, units, d_scratch, stream, ev);
}
