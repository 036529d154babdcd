// brotli_undict_kernels.hip -- two launches in stream order that turn the dictionary-index runs of n independent segments, of any alignment and
// length, into the VALUES their indices name in each segment's dictionary, and give every segment its result (gfx950, wave64).  The transform,
// an entry's load and the one function that turns an index into a value are csrc/brotli_undict.h; the grammar, one run, one element and the
// bookkeeping of an item are unrle's (csrc/brotli_unrle.h).  No block ever waits for another block's result.
//   1. brotli_amd_undict_walk_kernel    unrle's walk as it is (brotli_amd_unrle_walk through the stage of csrc/brotli_wave_stage.h), told an
//                                       element width of 8 so that only k <= 32 binds.  It writes the segment's result -- bad 0, first_bad none --,
//                                       the checkpoint of every item and the segment's entry of the items' prefix array.
//   2. brotli_amd_undict_expand_kernel  ONE WAVE AN ITEM, over the items of all segments in one flat list, on unrle's collection of the runs that
//                                       cover the item and its lane search.  A lane has 16 NEIGHBOURING elements and takes them in groups of
//                                       kGroup: it forms all of a group's indices first, then looks them up -- independent loads through the
//                                       caches, issued together; inside an RLE run one lookup serves every element of the run that the lane
//                                       holds --, then puts the aligned 16-byte words together and stores them, element by element at the
//                                       edges.  (All 16 at once cost 242 VGPRs and two waves a SIMD, and measured slower: DESIGN.md, section 8.)
//                                       An index at or above the
//                                       dictionary's entries is never made an address.  The lanes' bad elements are summed up in the wave; an
//                                       item that has some adds them to its segment's result with one atomicAdd and one atomicMin.
// THE SCRATCH behind the table: the n results, the items' prefix array (n + 1 entries), the checkpoints -- one an item, set to
// BROTLI_AMD_UNRLE_NONE in front of the walk.  A call that only counts has no items and is the first launch alone.
// The collection of an item's runs into LDS and a lane's way through them are csrc/brotli_run_items.h.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_run_items.h"    // the run batch, the walk's frame, the scratch and the launcher
#include "brotli_seg_walk.h"
#include "brotli_undict.h"
#include "brotli_wave_stage.h"   // the wave's view of its source through LDS, same(), Word16, wave_grid

namespace {

constexpr uint32_t kThreads = brotli_amd_wave::kSegThreads, kWaves = brotli_amd_wave::kSegWaves;
constexpr uint32_t kChunk = BROTLI_AMD_UNRLE_WALK_CHUNK, kItem = BROTLI_AMD_UNRLE_ITEM_ELEMS;
constexpr uint32_t kPerLane = kItem / 64u;   // neighbouring elements of a lane
constexpr uint32_t kBatch = brotli_amd_wave::kRunBatch;
#ifndef BROTLI_AMD_UNDICT_GROUP
#define BROTLI_AMD_UNDICT_GROUP 4u
#endif
constexpr uint32_t kGroup = BROTLI_AMD_UNDICT_GROUP;   // elements of a lane whose lookups are in flight together (4, 8 or 16: profiles/undict.txt)

static_assert(kChunk == brotli_amd_wave::kStageChunk, "the chunk the stage has");
static_assert(kPerLane == 16u && kPerLane % kGroup == 0u, "a lane's elements are whole 16-byte words at every width, in whole groups");

using brotli_amd_wave::RunBatch;
using brotli_amd_wave::RunCursor;
using brotli_amd_wave::same;
using brotli_amd_wave::Stage;
using brotli_amd_wave::Word16;

typedef BrotliAmdUndictSeg Seg;
typedef BrotliAmdUndictResult Result;
typedef BrotliAmdUnrleCheckpoint Checkpoint;

// ---- launch 1 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undict_walk_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* __restrict__ results,
                                                                          uint64_t* __restrict__ pre, Checkpoint* __restrict__ ckpts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  brotli_amd_wave::walk_segments(
      stage, segs, n, items, pre, ckpts,
      [](const Seg& sg, Stage& rd, auto mark) { return brotli_amd_unrle_walk(rd, sg.len, sg.cap, BROTLI_AMD_UNDICT_WALK_WIDTH, sg.bits, sg.flags, kItem, mark); },
      [&](uint64_t i, const Seg&, const BrotliAmdUnrleResult& res) {
        results[i] = Result{res.count, res.consumed, res.runs, res.status, res.bits, 0u, BROTLI_AMD_UNDICT_NONE};   // (what the items add to)
      });
}

// ---- launch 2 ----
// What a lane carries from one group of its elements to the next: the word being put together, and the last element's value and badness.
struct LaneCarry { Word16 word; uint64_t val = 0; uint32_t bad = 0; };

// The elements [g0, g0 + kGroup) below m of a lane whose m elements (1 .. 16) begin at address at0, their indices in idx: looked up in the D
// entries of W bytes at dict, and stored -- single elements in front of `head` and from `tail` on, whole 16-byte words between (unnull has
// the same rule in lines of its own: through one helper for both, this kernel's 8-byte gathers measured 3 % slower, profiles/run_items.txt).
// Bit u of `fresh` says that element g0 + u needs a lookup of its own; the others have the value of the element in front of them.  -> the
// bad elements' bits
template <uint32_t W>
__device__ __forceinline__ uint32_t lookup_and_store(uint64_t dict, uint64_t D, uint64_t at0, uint32_t m, uint32_t head, uint32_t tail, uint32_t g0,
                                                     const uint32_t (&idx)[kGroup], uint32_t fresh, LaneCarry* carry) {
  constexpr uint32_t per_word = 16u / W;
  uint64_t val[kGroup];
  uint32_t bad = 0;
  // the loads, none of which waits for another
#pragma unroll
  for (uint32_t u = 0; u < kGroup; u++) {
    val[u] = 0u;
    if (((fresh >> u) & 1u) != 0u) {
      const BrotliAmdUndictValue v = brotli_amd_undict_lookup(dict, D, W, idx[u]);
      val[u] = v.value; bad |= v.bad << u;
    }
  }
#pragma unroll
  for (uint32_t u = 0; u < kGroup; u++)
    if (g0 + u < m && ((fresh >> u) & 1u) == 0u) {
      val[u] = u ? val[u - 1u] : carry->val;
      bad |= (u ? (bad >> (u - 1u)) & 1u : carry->bad) << u;
    }
#pragma unroll
  for (uint32_t u = 0; u < kGroup; u++) {
    const uint32_t t = g0 + u;
    if (t >= m) {
    } else if (t < head || t >= tail) {
      brotli_amd_unvarint_store(at0 + (uint64_t)t * W, W, val[u]);
    } else {
      const uint32_t pos = (t - head) & (per_word - 1u);
      carry->word.put(pos * W, W, val[u]);
      if (pos == per_word - 1u) { brotli_amd_unshuffle_st128(at0 + (uint64_t)(t - pos) * W, carry->word.word()); carry->word = Word16(); }
    }
  }
  carry->val = val[kGroup - 1u]; carry->bad = (bad >> (kGroup - 1u)) & 1u;
  return bad;
}

__global__ __launch_bounds__(kThreads) void brotli_amd_undict_expand_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* results,
                                                                            const uint64_t* __restrict__ pre, const Checkpoint* __restrict__ ckpts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  __shared__ uint64_t run_first[kWaves][kBatch + 1u];   // the first element of every run of the batch; behind the last: the batch's end
  __shared__ uint64_t run_payload[kWaves][kBatch];      // (BROTLI_AMD_UNRLE_NONE: an RLE run)
  __shared__ uint32_t run_value[kWaves][kBatch];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  RunBatch batch(run_first[wave], run_payload[wave], run_value[wave]);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    const Checkpoint cp = ckpts[g];
    if (cp.off == BROTLI_AMD_UNRLE_NONE) continue;   // (beyond count; the same in every lane)
    const uint32_t i = brotli_amd_seg_find(pre, n, g);
    const Seg sg = segs[i];
    const uint64_t count = results[i].count;
    const uint32_t k = results[i].bits, w = sg.width;
    const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst, dict = (uint64_t)(uintptr_t)sg.dict, D = sg.dict_entries;
    uint64_t e0, e1;
    brotli_amd_unrle_item_range(count, sg.cap, g - pre[i], kItem, &e0, &e1);
    if (e0 >= e1) continue;
    const uint64_t la = e0 + (uint64_t)kPerLane * lane, lb = la + kPerLane < e1 ? la + kPerLane : e1;   // this lane's elements
    Stage rd(stage[wave], src, sg.len, lane);
    BrotliAmdUnrleWalk st = {cp.off, cp.first};
    uint32_t lane_bad = 0;                       // this lane's bad elements,
    uint64_t lane_first = BROTLI_AMD_UNDICT_NONE;   // and the first of them
    bool more = true;
    while (more && st.elems < e1) {
      batch.collect(rd, sg.len, k, st, more, e1, lane);
      // this lane's elements among the batch's
      const uint64_t a = la > batch.lo ? la : batch.lo, b = lb < st.elems ? lb : st.elems;
      if (a >= b) continue;
      RunCursor<true> run(batch, a);
      // group after group of the lane's elements: all of a group's indices first, then its lookups together, then its stores
      const uint32_t m = (uint32_t)(b - a);
      const uint64_t at0 = dst + a * w;
      const uint32_t per_word = 16u / w, to_word = ((16u - ((uint32_t)at0 & 15u)) & 15u) / w;
      const uint32_t head = (at0 & (w - 1u)) != 0u || to_word > m ? m : to_word, tail = head + (m - head) / per_word * per_word;
      LaneCarry carry;
      uint32_t bad = 0;
#pragma unroll 1
      for (uint32_t g0 = 0; g0 < m; g0 += kGroup) {
        uint32_t idx[kGroup], fresh = 0;
#pragma unroll
        for (uint32_t u = 0; u < kGroup; u++) {
          idx[u] = 0u;
          if (g0 + u < m) {
            const uint64_t e = a + g0 + u;
            const bool moved = run.seek(e) || g0 + u == 0u;
            idx[u] = (uint32_t)brotli_amd_unrle_element(src, run.payload, run.value, k, e - run.first);
            if (moved || run.payload != BROTLI_AMD_UNRLE_NONE) fresh |= 1u << u;   // (inside an RLE run: the lookup of the element in front)
          }
        }
        uint32_t group_bad;
        switch (w) {   // (the same in every lane)
          case 1u: group_bad = lookup_and_store<1u>(dict, D, at0, m, head, tail, g0, idx, fresh, &carry); break;
          case 2u: group_bad = lookup_and_store<2u>(dict, D, at0, m, head, tail, g0, idx, fresh, &carry); break;
          case 4u: group_bad = lookup_and_store<4u>(dict, D, at0, m, head, tail, g0, idx, fresh, &carry); break;
          default: group_bad = lookup_and_store<8u>(dict, D, at0, m, head, tail, g0, idx, fresh, &carry); break;
        }
        bad |= group_bad << g0;
      }
      if (bad != 0u) {
        const uint64_t at = a + (uint32_t)__builtin_ctz(bad);
        lane_bad += (uint32_t)__builtin_popcount(bad);
        lane_first = at < lane_first ? at : lane_first;
      }
    }
    // the item's bad elements: summed up in the wave, then one add and one minimum
    if (__ballot(lane_bad != 0u) != 0ull) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        lane_bad += __shfl_xor(lane_bad, off);
        const uint64_t other = __shfl_xor((unsigned long long)lane_first, off);
        lane_first = other < lane_first ? other : lane_first;
      }
      if (lane == 0u) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&results[i].bad), (unsigned long long)lane_bad);
        atomicMin(reinterpret_cast<unsigned long long*>(&results[i].first_bad), (unsigned long long)lane_first);
      }
    }
  }
}

}  // namespace

// the scratch of a launch over `units` units of n segments -- a unit a segment and a unit an item --: the results first, then the items' prefix
// array and the checkpoints
extern "C" uint64_t brotli_amd_undict_scratch_bytes(uint64_t units, uint32_t n) {
  return brotli_amd_wave::ItemScratch<Result, Checkpoint, false, false>::bytes(units - n, n);
}

// units: n + the items of all segments (the host has the table); d_scratch: brotli_amd_undict_scratch_bytes of device memory, 16-byte aligned;
// ev[0..2], where not NULL, are recorded in front of, between and behind the two launches
extern "C" hipError_t brotli_amd_launch_undict(const void* d_table, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  return brotli_amd_wave::launch_walk_expand<Seg, Result, Checkpoint>(brotli_amd_undict_walk_kernel, brotli_amd_undict_expand_kernel, d_table, n, units, d_scratch, stream, ev);
}
