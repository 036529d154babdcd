// brotli_undbp_kernels.hip -- four launches in stream order that turn the DELTA_BINARY_PACKED streams of n independent segments, of any
// alignment and length, back into elements of 1, 2, 4 or 8 bytes, and give every segment its result (gfx950, wave64).  The transform, a varint,
// a block, a group and the bookkeeping of an item are csrc/brotli_undbp.h.  No block ever waits for another block's result -- no look-back, no
// flags, no spins, no grid barrier.
//   1. brotli_amd_undbp_walk_kernel    ONE WAVE A SEGMENT, the waves striding over the table, on unrle's walk: where a block lies depends on
//                                      every block header in front of it, so a segment's headers are one taker's.  The wave stages the source
//                                      through LDS (csrc/brotli_wave_stage.h) and reads the stream header and every block's min_delta and
//                                      width bytes, eight of them a round trip, every lane the same; it never reads a payload: a block's
//                                      payloads make the stage jump.  It writes the segment's result and first value, the checkpoint of every
//                                      item (the lanes striding over the items that begin in one block), and the segment's entry of the items'
//                                      prefix array.
//   2. brotli_amd_undbp_sum_kernel     ONE WAVE AN ITEM, over the items of all segments in one flat list, so one long segment is taken by every
//                                      CU.  The item's segment is found by the search of csrc/brotli_seg_walk.h in the prefix array.  From its
//                                      checkpoint the wave reads the few block headers that cover the item again and gives each lane ONE GROUP
//                                      of 32 fields: its address, k and min_delta.  The lanes' sums together are the item's undelta tile record.
//   3. brotli_amd_undelta_carry_kernel undelta's carry launch itself (csrc/brotli_undelta_kernels.hip), over those records: a running sum with
//                                      restarts at the segments' first items -> every item's carry-in, the value in front of its first delta.
//   4. brotli_amd_undbp_expand_kernel  the same item function; a running sum over the lanes' group sums and the carry-in give a lane the value in
//                                      front of its group, and it sums its 32 deltas up one after the other.  A lane's elements are 32
//                                      NEIGHBOURS, one element behind its group because element 0 is `first`: it puts them together into
//                                      aligned 16-byte stores wherever it has a whole word, whatever that shift and dst's alignment are, and
//                                      stores the few at its two ends one by one.
// THE SCRATCH behind the table: the n results, the n first values, the items' prefix array (n + 1 entries), and for every item a checkpoint --
// set to BROTLI_AMD_UNDBP_NONE in front of the walk --, a tile record and a carry.  A call that only counts has no items and is the first
// launch alone.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_run_items.h"    // the walk's frame, the scratch and the launcher
#include "brotli_seg_walk.h"
#include "brotli_undbp.h"
#include "brotli_undbp_groups.h"   // an item's groups, a group a lane
#include "brotli_wave_stage.h"

namespace {

constexpr uint32_t kThreads = brotli_amd_wave::kSegThreads, kWaves = brotli_amd_wave::kSegWaves;
constexpr uint32_t kChunk = brotli_amd_wave::kStageChunk, kItem = BROTLI_AMD_UNDBP_ITEM_DELTAS, kGroup = BROTLI_AMD_UNDBP_GROUP;

static_assert(kItem == 64u * kGroup, "a group a lane");

using brotli_amd_wave::same;
using brotli_amd_wave::Stage;
using brotli_amd_wave::Word16;

typedef BrotliAmdUndbpSeg Seg;
typedef BrotliAmdUndbpResult Result;
typedef BrotliAmdUndbpCheckpoint Checkpoint;
typedef BrotliAmdUndeltaTile Tile;

// ---- launch 1 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undbp_walk_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* __restrict__ results,
                                                                         uint64_t* __restrict__ firsts, uint64_t* __restrict__ pre, Checkpoint* __restrict__ ckpts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  struct Walked { Result res; uint64_t first; };
  brotli_amd_wave::walk_segments(
      stage, segs, n, items, pre, ckpts,
      [](const Seg& sg, Stage& rd, auto mark) {
        Walked got = {{}, 0u};
        got.res = brotli_amd_undbp_walk(rd, sg.len, sg.cap, kItem, &got.first, mark);
        return got;
      },
      [&](uint64_t i, const Seg&, const Walked& got) {
        results[i] = got.res;
        firsts[i] = got.first;
      });
}

// ---- launches 2 and 4 ----
// (a lane's group and the item function: csrc/brotli_undbp_groups.h)
typedef brotli_amd_wave::DbpGroup Group;
using brotli_amd_wave::dbp_item_groups;

__global__ __launch_bounds__(kThreads) void brotli_amd_undbp_sum_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, const Result* __restrict__ results,
                                                                        const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ pre,
                                                                        const Checkpoint* __restrict__ ckpts, Tile* __restrict__ tiles) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    uint32_t i; uint64_t j, a; Group grp;
    uint64_t sum = 0;
    if (dbp_item_groups<kItem>(stage[wave], segs, n, results, pre, ckpts, g, lane, &i, &j, &a, &grp)) {
      sum = brotli_amd_undbp_group_sum(grp.at, grp.k, grp.min_delta, grp.nf);
#pragma unroll
      for (uint32_t off = 32; off != 0u; off >>= 1) sum += (uint64_t)__shfl_down((unsigned long long)sum, off, 64);
    }
    if (lane == 0u) tiles[g] = brotli_amd_undbp_tile(j, j == 0u ? firsts[i] : 0u, sum);
  }
}

__global__ __launch_bounds__(kThreads) void brotli_amd_undbp_expand_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, const Result* __restrict__ results,
                                                                           const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ pre,
                                                                           const Checkpoint* __restrict__ ckpts, const uint64_t* __restrict__ carries) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    uint32_t i; uint64_t j, a = 0; Group grp;
    const bool deltas = dbp_item_groups<kItem>(stage[wave], segs, n, results, pre, ckpts, g, lane, &i, &j, &a, &grp);
    if (ckpts[g].off == BROTLI_AMD_UNDBP_NONE) continue;
    const Seg sg = segs[i];
    if (j == 0u && (results[i].count == 0u || sg.cap == 0u)) continue;
    if (j != 0u && !deltas) continue;
    // the value in front of this lane's group: the item's carry-in, `first` in a segment's first item, the groups of the lanes below
    const uint64_t sum = brotli_amd_undbp_group_sum(grp.at, grp.k, grp.min_delta, grp.nf);
    uint64_t inc = sum;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
      const uint64_t q = (uint64_t)__shfl_up((unsigned long long)inc, off, 64);
      if (lane >= off) inc += q;
    }
    uint64_t v = carries[g] + (j == 0u ? firsts[i] : 0u) + (inc - sum);
    // this lane's elements [e, e1): the one behind each of its deltas, and element 0 in front of them for the first lane of a first item
    bool lead = j == 0u && lane == 0u;
    const uint32_t w = sg.width, per_word = 16u / w;
    const uint64_t dst = (uint64_t)(uintptr_t)sg.dst, e0 = a + (uint64_t)kGroup * lane + 1u;
    uint64_t e = lead ? 0u : e0;
    const uint64_t e1 = e0 + grp.nf;
    uint32_t t = 0;
    auto next = [&]() {   // the elements one after the other
      if (lead) { lead = false; return v; }
      v += grp.min_delta + brotli_amd_undbp_field(grp.at, grp.k, t++);
      return v;
    };
    while (e < e1) {
      const uint64_t at = dst + e * w;
      if ((at & 15u) == 0u && e + per_word <= e1) {
        Word16 word;
        for (uint32_t q = 0; q < per_word; q++) word.put(q * w, w, next());
        brotli_amd_unshuffle_st128(at, word.word());
        e += per_word;
      } else {
        brotli_amd_unvarint_store(at, w, next());
        e++;
      }
    }
  }
}

}  // namespace

extern "C" uint32_t brotli_amd_undbp_item_deltas(void) { return kItem; }
extern "C" uint32_t brotli_amd_undbp_walk_chunk(void) { return kChunk; }
// the scratch of a launch over `units` units of n segments -- a unit a segment and a unit an item --: the results first, then the first values,
// the items' prefix array, the checkpoints, the tile records and the carries
extern "C" uint64_t brotli_amd_undbp_scratch_bytes(uint64_t units, uint32_t n) {
  return brotli_amd_wave::ItemScratch<Result, Checkpoint, true, true>::bytes(units - n, n);
}

// units: n + the items of all segments (the host has the table); d_scratch: brotli_amd_undbp_scratch_bytes of device memory, 16-byte aligned;
// ev[0..4], where not NULL, are recorded in front of, between and behind the four launches
extern "C" hipError_t brotli_amd_launch_undbp(const void* d_table, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  return brotli_amd_wave::launch_walk_count_carry_expand<Seg, Result, Checkpoint>(brotli_amd_undbp_walk_kernel, brotli_amd_undbp_sum_kernel, brotli_amd_undbp_expand_kernel, d_table, n,
                                                                                  units, d_scratch, stream, ev);
}
