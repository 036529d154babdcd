// brotli_unrle_kernels.hip -- two launches in stream order that turn the runs of the RLE / bit-packed hybrid of n independent segments, of any
// alignment and length, back into elements of 1, 2, 4 or 8 bytes, and give every segment its result (gfx950, wave64).  The transform, one run,
// one element and the bookkeeping of an item are csrc/brotli_unrle.h.  No block ever waits for another block's result.
//   1. brotli_amd_unrle_walk_kernel    ONE WAVE A SEGMENT, the waves striding over the table.  Where a header lies depends on every header in
//                                      front of it, so a segment's headers are one taker's.  The wave stages the source through LDS in aligned
//                                      chunks of BROTLI_AMD_UNRLE_WALK_CHUNK bytes, one 16-byte load a lane, two chunks resident and the third
//                                      in flight in registers, and takes the runs one after the other out of LDS (brotli_amd_unrle_walk, every
//                                      lane the same).  It never reads a packed payload: a run that passes the resident chunks makes the stage
//                                      jump.  It writes the segment's result, the checkpoint of every item of the segment (the lanes striding
//                                      over the items that begin in one run), and the segment's entry of the items' prefix array.
//   2. brotli_amd_unrle_expand_kernel  ONE WAVE AN ITEM, over the items of all segments in one flat list: work is split by the DESTINATION,
//                                      so one segment with a gigabyte of destination is expanded by every CU.  The item's segment is found by
//                                      the search of csrc/brotli_seg_walk.h in the prefix array.  The wave starts at its checkpoint and
//                                      collects the runs that cover its item through the same stage, up to 64 at a time, wave-uniform, into
//                                      LDS with their first elements; a lane takes 16 NEIGHBOURING elements and finds the run of its first
//                                      one by a search in that batch, so runs of 8 values or of 1 do not leave lanes idle.  Its stores are
//                                      16 bytes wide where dst + i w is a multiple of 16 and the lane has the word's elements, and element by
//                                      element elsewhere.
// THE SCRATCH behind the table: the n results, the items' prefix array (n + 1 entries), the checkpoints -- one an item, set to
// BROTLI_AMD_UNRLE_NONE in front of the walk.  A call that only counts has no items and is the first launch alone.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_run_items.h"    // the run batch, the walk's frame, the scratch and the launcher
#include "brotli_seg_walk.h"
#include "brotli_unrle.h"
#include "brotli_wave_stage.h"   // the wave's view of its source through LDS, same(), Word16, wave_grid

namespace {

constexpr uint32_t kThreads = brotli_amd_wave::kSegThreads, kWaves = brotli_amd_wave::kSegWaves;
constexpr uint32_t kChunk = BROTLI_AMD_UNRLE_WALK_CHUNK, kItem = BROTLI_AMD_UNRLE_ITEM_ELEMS;
constexpr uint32_t kPerLane = kItem / 64u;   // neighbouring elements of a lane
constexpr uint32_t kBatch = brotli_amd_wave::kRunBatch;

static_assert(kChunk == brotli_amd_wave::kStageChunk, "the chunk the stage has");
static_assert(kPerLane * 64u == kItem && kPerLane % 16u == 0u, "a lane's elements are whole 16-byte words at every width");

using brotli_amd_wave::RunBatch;
using brotli_amd_wave::RunCursor;
using brotli_amd_wave::same;
using brotli_amd_wave::Stage;
using brotli_amd_wave::Word16;

typedef BrotliAmdUnrleSeg Seg;
typedef BrotliAmdUnrleResult Result;
typedef BrotliAmdUnrleCheckpoint Checkpoint;

// ---- launch 1 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_unrle_walk_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* __restrict__ results,
                                                                         uint64_t* __restrict__ pre, Checkpoint* __restrict__ ckpts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  brotli_amd_wave::walk_segments(
      stage, segs, n, items, pre, ckpts,
      [](const Seg& sg, Stage& rd, auto mark) { return brotli_amd_unrle_walk(rd, sg.len, sg.cap, sg.width, sg.bits, sg.flags, kItem, mark); },
      [&](uint64_t i, const Seg&, const Result& res) { results[i] = res; });
}

// ---- launch 2 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_unrle_expand_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, const Result* __restrict__ results,
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
    const Result res = results[i];
    const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst;
    const uint32_t k = res.bits, w = sg.width, per_word = 16u / w;
    uint64_t e0, e1;
    brotli_amd_unrle_item_range(res.count, sg.cap, g - pre[i], kItem, &e0, &e1);
    if (e0 >= e1) continue;
    const uint64_t la = e0 + (uint64_t)kPerLane * lane, lb = la + kPerLane < e1 ? la + kPerLane : e1;   // this lane's elements
    Stage rd(stage[wave], src, sg.len, lane);
    BrotliAmdUnrleWalk st = {cp.off, cp.first};
    bool more = true;
    while (more && st.elems < e1) {
      batch.collect(rd, sg.len, k, st, more, e1, lane);
      // this lane's elements among the batch's
      const uint64_t a = la > batch.lo ? la : batch.lo, b = lb < st.elems ? lb : st.elems;
      if (a >= b) continue;
      RunCursor<true> run(batch, a);
      auto element = [&](uint64_t e) {
        run.seek(e);
        return brotli_amd_unrle_element(src, run.payload, run.value, k, e - run.first);
      };
      for (uint64_t e = a; e < b;) {
        const uint64_t at = dst + e * w;
        if ((at & 15u) == 0u && e + per_word <= b) {
          Word16 word;
          for (uint32_t t = 0; t < per_word; t++) word.put(t * w, w, element(e + t));
          brotli_amd_unshuffle_st128(at, word.word());
          e += per_word;
        } else {
          brotli_amd_unvarint_store(at, w, element(e));
          e++;
        }
      }
    }
  }
}

}  // namespace

extern "C" uint32_t brotli_amd_unrle_item_elems(void) { return kItem; }
extern "C" uint32_t brotli_amd_unrle_walk_chunk(void) { return kChunk; }
// the scratch of a launch over `units` units of n segments -- a unit a segment and a unit an item --: the results first, then the items' prefix
// array and the checkpoints
extern "C" uint64_t brotli_amd_unrle_scratch_bytes(uint64_t units, uint32_t n) {
  return brotli_amd_wave::ItemScratch<Result, Checkpoint, false, false>::bytes(units - n, n);
}

// units: n + the items of all segments (the host has the table); d_scratch: brotli_amd_unrle_scratch_bytes of device memory, 16-byte aligned;
// ev[0..2], where not NULL, are recorded in front of, between and behind the two launches
extern "C" hipError_t brotli_amd_launch_unrle(const void* d_table, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  return brotli_amd_wave::launch_walk_expand<Seg, Result, Checkpoint>(brotli_amd_unrle_walk_kernel, brotli_amd_unrle_expand_kernel, d_table, n, units, d_scratch, stream, ev);
}
