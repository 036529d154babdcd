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
#include "brotli_seg_walk.h"
#include "brotli_unrle.h"
#include "brotli_wave_stage.h"   // the wave's view of its source through LDS, same(), Word16, wave_grid

namespace {

constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS, kWaves = kThreads / 64u;
constexpr uint32_t kChunk = BROTLI_AMD_UNRLE_WALK_CHUNK, kItem = BROTLI_AMD_UNRLE_ITEM_ELEMS;
constexpr uint32_t kPerLane = kItem / 64u;   // neighbouring elements of a lane
constexpr uint32_t kBatch = 64;              // runs collected at a time

static_assert(kChunk == brotli_amd_wave::kStageChunk, "the chunk the stage has");
static_assert(kPerLane * 64u == kItem && kPerLane % 16u == 0u, "a lane's elements are whole 16-byte words at every width");

using brotli_amd_wave::lds_sync;
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
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + wave; i < n; i += (uint64_t)gridDim.x * kWaves) {
    const Seg sg = segs[i];
    Stage rd(stage[wave], (uint64_t)(uintptr_t)sg.src, sg.len, lane);
    Checkpoint* mine = ckpts + sg.first_item;
    const Result res = brotli_amd_unrle_walk(rd, sg.len, sg.cap, sg.width, sg.bits, sg.flags, kItem, [&](uint64_t j0, uint64_t j1, uint64_t off, uint64_t first) {
      for (uint64_t j = j0 + lane; j < j1; j += 64u) mine[j] = Checkpoint{off, first};
    });
    if (lane == 0u) {
      results[i] = res;
      pre[i] = sg.first_item;
      if (i + 1u == n) pre[n] = items;
    }
  }
}

// ---- launch 2 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_unrle_expand_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, const Result* __restrict__ results,
                                                                           const uint64_t* __restrict__ pre, const Checkpoint* __restrict__ ckpts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  __shared__ uint64_t run_first[kWaves][kBatch + 1u];   // the first element of every run of the batch; behind the last: the batch's end
  __shared__ uint64_t run_payload[kWaves][kBatch];      // (BROTLI_AMD_UNRLE_NONE: an RLE run)
  __shared__ uint32_t run_value[kWaves][kBatch];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  uint64_t* const first = run_first[wave];
  uint64_t* const payload = run_payload[wave];
  uint32_t* const value = run_value[wave];
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    const Checkpoint cp = ckpts[g];
    if (cp.off == BROTLI_AMD_UNRLE_NONE) continue;   // (beyond count; the same in every lane)
    const uint32_t i = brotli_amd_seg_find(pre, n, g);
    const Seg sg = segs[i];
    const Result res = results[i];
    const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst;
    const uint32_t k = res.bits, w = sg.width, per_word = 16u / w;
    const uint64_t end = res.count < sg.cap ? res.count : sg.cap, e0 = (g - pre[i]) * kItem;
    if (e0 >= end) continue;
    const uint64_t e1 = e0 + kItem < end ? e0 + kItem : end;
    const uint64_t la = e0 + (uint64_t)kPerLane * lane, lb = la + kPerLane < e1 ? la + kPerLane : e1;   // this lane's elements
    Stage rd(stage[wave], src, sg.len, lane);
    BrotliAmdUnrleWalk st = {cp.off, cp.first};
    bool more = true;
    while (more && st.elems < e1) {
      // the next runs, up to kBatch of them: every lane walks, lane 0 keeps
      const uint64_t batch_lo = st.elems;
      uint32_t nr = 0;
      lds_sync();   // (the batch before is done with)
      while (more && nr < kBatch && st.elems < e1) {
        rd.ensure(st.off);
        const BrotliAmdUnrleRun run = brotli_amd_unrle_run(rd, sg.len, k, st);
        if (run.kind == BROTLI_AMD_UNRLE_STOP) { more = false; break; }   // (not below count)
        if (lane == 0u) {
          first[nr] = st.elems;
          payload[nr] = run.kind == BROTLI_AMD_UNRLE_RLE ? BROTLI_AMD_UNRLE_NONE : run.payload;
          value[nr] = run.value;
        }
        nr++;
        st.off = run.next; st.elems += run.count;
        more = run.status == BROTLI_AMD_UNRLE_OK;
      }
      if (lane == 0u) first[nr] = st.elems;
      lds_sync();
      // this lane's elements among the batch's
      const uint64_t a = la > batch_lo ? la : batch_lo, b = lb < st.elems ? lb : st.elems;
      if (a >= b) continue;
      uint32_t r = 0;
      { uint32_t hi = nr; while (hi - r > 1u) { const uint32_t m = (r + hi) >> 1; if (first[m] <= a) r = m; else hi = m; } }
      uint64_t r_first = first[r], r_end = first[r + 1u], r_payload = payload[r];
      uint32_t r_value = value[r];
      auto element = [&](uint64_t e) {
        while (e >= r_end) { r++; r_first = r_end; r_end = first[r + 1u]; r_payload = payload[r]; r_value = value[r]; }
        return brotli_amd_unrle_element(src, r_payload, r_value, k, e - r_first);
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

constexpr uint64_t pre_bytes(uint32_t n) { return (((uint64_t)n + 1u) * sizeof(uint64_t) + 15u) & ~(uint64_t)15; }

}  // namespace

extern "C" uint32_t brotli_amd_unrle_item_elems(void) { return kItem; }
extern "C" uint32_t brotli_amd_unrle_walk_chunk(void) { return kChunk; }
// the scratch of a launch over `units` units of n segments -- a unit a segment and a unit an item --: the results first, then the items' prefix
// array and the checkpoints
extern "C" uint64_t brotli_amd_unrle_scratch_bytes(uint64_t units, uint32_t n) {
  return (uint64_t)n * sizeof(Result) + pre_bytes(n) + (units - n) * sizeof(Checkpoint);
}

// units: n + the items of all segments (the host has the table); d_scratch: brotli_amd_unrle_scratch_bytes of device memory, 16-byte aligned;
// ev[0..2], where not NULL, are recorded in front of, between and behind the two launches
extern "C" hipError_t brotli_amd_launch_unrle(const void* d_table, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  if (n == 0u) return hipSuccess;
  const BrotliAmdUnrleSeg* d_segs = static_cast<const BrotliAmdUnrleSeg*>(d_table);
  const uint64_t items = units - n;
  Result* results = static_cast<Result*>(d_scratch);
  uint64_t* pre = reinterpret_cast<uint64_t*>(results + n);
  Checkpoint* ckpts = reinterpret_cast<Checkpoint*>(reinterpret_cast<uint8_t*>(pre) + pre_bytes(n));
  hipError_t e = hipSuccess;
  uint32_t grid = 0;
  if (items != 0u && (e = hipMemsetAsync(ckpts, 0xFF, (size_t)items * sizeof(Checkpoint), stream)) != hipSuccess) return e;
  if ((e = brotli_amd_wave::wave_grid(n, kWaves, &grid)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(brotli_amd_unrle_walk_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, items, results, pre, ckpts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
  if (items != 0u) {
    if ((e = brotli_amd_wave::wave_grid(items, kWaves, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(brotli_amd_unrle_expand_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, items, results, pre, ckpts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
  return hipSuccess;
}
