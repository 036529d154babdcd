// brotli_undict_bytes_kernels.hip -- five launches in stream order that turn the dictionary-index runs of n independent segments, of any
// alignment and length, and their dictionaries of PLAIN byte arrays into Arrow string columns -- offsets and bytes --, and give every segment
// its result (gfx950, wave64).  The transform, the dictionary's length chain, the one function that turns an index into an entry and the
// destination's words are csrc/brotli_undict_bytes.h; the grammar, one run, one element and the bookkeeping of an item are unrle's
// (csrc/brotli_unrle.h).  No block ever waits for another block's result -- no flags, no spins, no atomics on offsets or data.
//   1. brotli_amd_undict_bytes_dict_kernel     ONE WAVE A DICTIONARY, the waves striding over the call's table of distinct dictionaries: the
//                                              wave stages the dictionary's bytes through the stage of csrc/brotli_wave_stage.h, follows the
//                                              length chain and writes starts[0 .. D] and the dictionary's result.  A serial chain.
//   2. brotli_amd_undict_bytes_walk_kernel     unrle's walk as it is, told an element width of 8; it writes the segment's result -- bad 0,
//                                              first_bad none, bytes 0, and what its dictionary's walk found --, the checkpoint of every item
//                                              and the segment's entry of the items' prefix array.
//   3. brotli_amd_undict_bytes_count_kernel    ONE WAVE AN ITEM, on unrle's collection of the runs that cover the item.  A lane forms the
//                                              indices of its 16 neighbouring elements and looks each up -- starts[idx] and starts[idx + 1]
//                                              together; inside an RLE run one lookup serves every element of the run that the lane holds --,
//                                              and the wave's sum of the lengths is the item's undelta tile record.  The wave's bad elements go
//                                              to the segment's result with one atomicAdd and one atomicMin.
//   4. brotli_amd_undelta_carry_kernel         undelta's carry launch itself (csrc/brotli_undelta_kernels.hip): every item's carry-in, the bytes
//                                              of the segment's elements in front of it.
//   5. brotli_amd_undict_bytes_expand_kernel   the same item function; a lane writes its elements' lengths and positions to LDS, a scan over
//                                              the lanes' sums on top of the carry-in turns the lengths into the item's offsets, ends[0 .. m].
//                                              Then the lanes stride over the aligned 16-byte words of the item's offsets and over those of its
//                                              bytes (csrc/brotli_undict_bytes.h: a binary search of ends a word, one store a word).  The item
//                                              that holds the segment's last delivered element writes the result's bytes.
// A measuring call has no destinations, and every store of launch 5 but that of `bytes` is predicated off.
// THE SCRATCH behind the table: the n results, the items' prefix array, and for every item a checkpoint, a tile record and a carry
// (csrc/brotli_run_items.h); behind them a result for every dictionary, and starts[] of all dictionaries.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_run_items.h"    // the run batch, the walk's frame, the scratch and the walk's launch
#include "brotli_seg_walk.h"
#include "brotli_undict_bytes.h"
#include "brotli_wave_stage.h"   // the wave's view of its source through LDS, same(), wave_grid

namespace {

constexpr uint32_t kThreads = brotli_amd_wave::kSegThreads, kWaves = brotli_amd_wave::kSegWaves;
constexpr uint32_t kChunk = BROTLI_AMD_UNRLE_WALK_CHUNK, kItem = BROTLI_AMD_UNRLE_ITEM_ELEMS;
constexpr uint32_t kPerLane = kItem / 64u;   // neighbouring elements of a lane
constexpr uint32_t kBatch = brotli_amd_wave::kRunBatch;

static_assert(kChunk == brotli_amd_wave::kStageChunk, "the chunk the stage has");
static_assert(kPerLane == 16u, "the padding of the items' LDS arrays: one entry behind every lane's sixteen");

using brotli_amd_wave::lds_sync;
using brotli_amd_wave::RunBatch;
using brotli_amd_wave::RunCursor;
using brotli_amd_wave::same;
using brotli_amd_wave::Stage;

typedef BrotliAmdUndictBytesSeg Seg;
typedef BrotliAmdUndictBytesResult Result;
typedef BrotliAmdUndictBytesDict Dict;
typedef BrotliAmdUndictBytesDictResult DictResult;
typedef BrotliAmdUnrleCheckpoint Checkpoint;
typedef BrotliAmdUndeltaTile Tile;
typedef brotli_amd_wave::ItemScratch<Result, Checkpoint, false, true> Scratch;

// ---- launch 1 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undict_bytes_dict_kernel(const Dict* __restrict__ dicts, uint32_t nd, uint32_t* __restrict__ starts,
                                                                                DictResult* __restrict__ dict_results) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + wave; i < nd; i += (uint64_t)gridDim.x * kWaves) {
    const Dict d = dicts[i];
    Stage rd(stage[wave], (uint64_t)(uintptr_t)d.dict, d.len, lane);
    uint32_t* mine = starts + d.first_start;
    const DictResult got = brotli_amd_undict_bytes_dict_walk(rd, d.len, d.bound, [&](uint64_t e, uint32_t s) { if (lane == 0u) mine[e] = s; });
    if (lane == 0u) dict_results[i] = got;
  }
}

// ---- launch 2 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undict_bytes_walk_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* __restrict__ results,
                                                                                uint64_t* __restrict__ pre, const DictResult* __restrict__ dict_results,
                                                                                Checkpoint* __restrict__ ckpts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  brotli_amd_wave::walk_segments(
      stage, segs, n, items, pre, ckpts,
      [](const Seg& sg, Stage& rd, auto mark) {
        return brotli_amd_unrle_walk(rd, sg.len, sg.cap, BROTLI_AMD_UNDICT_WALK_WIDTH, sg.bits, sg.flags & BROTLI_AMD_UNRLE_FLAGS, kItem, mark);
      },
      [&](uint64_t i, const Seg& sg, const BrotliAmdUnrleResult& res) {
        results[i] = brotli_amd_undict_bytes_result(res, sg.dict != BROTLI_AMD_UNDICT_BYTES_NO_DICT ? dict_results[sg.dict] : DictResult{0u, 0u, 0u, 0u});   // (what the items add to)
      });
}

// ---- launches 3 and 5 ----
// The entries of this lane's elements [la, lb) of an item that ends at element e1, whose runs -- len bytes at address src, fields of k bits --
// are walked from the checkpoint cp on: each(t, entry) for element la + t.  Every lane of the wave calls it (the runs are collected together).
template <class Each>
__device__ __forceinline__ void item_entries(uint8_t* lds, RunBatch batch, uint64_t src, uint64_t len, uint32_t k, const uint32_t* __restrict__ starts, uint64_t D,
                                             Checkpoint cp, uint64_t e1, uint64_t la, uint64_t lb, uint32_t lane, Each each) {
  Stage rd(lds, src, len, lane);
  BrotliAmdUnrleWalk st = {cp.off, cp.first};
  bool more = true;
  while (more && st.elems < e1) {
    batch.collect(rd, len, k, st, more, e1, lane);
    // this lane's elements among the batch's
    const uint64_t a = la > batch.lo ? la : batch.lo, b = lb < st.elems ? lb : st.elems;
    if (a >= b) continue;
    RunCursor<true> run(batch, a);
    BrotliAmdUndictBytesEntry en = {0u, 0u, 0u};
    for (uint64_t e = a; e < b; e++) {
      const bool moved = run.seek(e) || e == a;
      if (moved || run.payload != BROTLI_AMD_UNRLE_NONE)   // (inside an RLE run: the lookup of the element in front)
        en = brotli_amd_undict_bytes_lookup(starts, D, brotli_amd_unrle_element(src, run.payload, run.value, k, e - run.first));
      each((uint32_t)(e - la), en);
    }
  }
}

__global__ __launch_bounds__(kThreads) void brotli_amd_undict_bytes_count_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* results,
                                                                                 const uint64_t* __restrict__ pre, const Dict* __restrict__ dicts,
                                                                                 const uint32_t* __restrict__ starts, const Checkpoint* __restrict__ ckpts,
                                                                                 Tile* __restrict__ tiles) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  __shared__ uint64_t run_first[kWaves][kBatch + 1u];   // the first element of every run of the batch; behind the last: the batch's end
  __shared__ uint64_t run_payload[kWaves][kBatch];      // (BROTLI_AMD_UNRLE_NONE: an RLE run)
  __shared__ uint32_t run_value[kWaves][kBatch];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    const Checkpoint cp = ckpts[g];
    const uint32_t i = brotli_amd_seg_find(pre, n, g);
    const uint64_t j = g - pre[i];
    uint64_t sum = 0;
    if (cp.off != BROTLI_AMD_UNRLE_NONE) {   // (beyond count otherwise; the same in every lane)
      const Seg sg = segs[i];
      uint64_t e0, e1;
      brotli_amd_unrle_item_range(results[i].count, sg.cap, j, kItem, &e0, &e1);
      if (e0 < e1) {
        const uint64_t la = e0 + (uint64_t)kPerLane * lane, lb = la + kPerLane < e1 ? la + kPerLane : e1;   // this lane's elements
        uint32_t lane_bad = 0;                          // this lane's bad elements,
        uint64_t lane_first = BROTLI_AMD_UNDICT_NONE;   // and the first of them
        item_entries(stage[wave], RunBatch(run_first[wave], run_payload[wave], run_value[wave]), (uint64_t)(uintptr_t)sg.src, sg.len, results[i].bits,
                     starts + dicts[sg.dict].first_start, results[i].dict_entries, cp, e1, la, lb, lane, [&](uint32_t t, const BrotliAmdUndictBytesEntry& en) {
          sum += en.len;
          if (en.bad != 0u) { lane_bad++; if (la + t < lane_first) lane_first = la + t; }
        });
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor((unsigned long long)sum, off);
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
    if (lane == 0u) tiles[g] = brotli_amd_undbp_tile(j, 0u, sum);
  }
}

// An item's arrays in LDS have one entry of padding behind every lane's sixteen, so that the lanes' neighbouring entries lie in different banks.
__device__ __forceinline__ uint32_t slot(uint32_t t) { return t + (t >> 4); }
constexpr uint32_t kEnds = kItem + 1u + (kItem >> 4) + 1u, kPos = kItem + (kItem >> 4);

__global__ __launch_bounds__(kThreads) void brotli_amd_undict_bytes_expand_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* results,
                                                                                  const uint64_t* __restrict__ pre, const Dict* __restrict__ dicts,
                                                                                  const uint32_t* __restrict__ starts, const Checkpoint* __restrict__ ckpts,
                                                                                  const uint64_t* __restrict__ carries) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  __shared__ uint64_t run_first[kWaves][kBatch + 1u];
  __shared__ uint64_t run_payload[kWaves][kBatch];
  __shared__ uint32_t run_value[kWaves][kBatch];
  __shared__ uint64_t item_ends[kWaves][kEnds];   // ends(t) at slot(t): first an element's length at slot(t + 1), then the running sum
  __shared__ uint32_t item_pos[kWaves][kPos];     // the position of element t's bytes in its dictionary, at slot(t)
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  uint64_t* ends = item_ends[wave];
  uint32_t* pos = item_pos[wave];
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    const Checkpoint cp = ckpts[g];
    const uint32_t i = brotli_amd_seg_find(pre, n, g);
    const uint64_t j = g - pre[i];
    const Seg sg = segs[i];
    if (j == 0u && lane == 0u) brotli_amd_undict_bytes_first_offset(sg);
    if (cp.off == BROTLI_AMD_UNRLE_NONE) continue;   // (beyond count; the same in every lane)
    const uint64_t count = results[i].count;
    uint64_t e0, e1;
    brotli_amd_unrle_item_range(count, sg.cap, j, kItem, &e0, &e1);
    if (e0 >= e1) continue;
    const uint32_t m = (uint32_t)(e1 - e0);
    const uint64_t la = e0 + (uint64_t)kPerLane * lane, lb = la + kPerLane < e1 ? la + kPerLane : e1;   // this lane's elements
    const Dict dict = dicts[sg.dict];
    lds_sync();   // (the item before is done with the arrays)
    uint64_t lane_sum = 0;
    item_entries(stage[wave], RunBatch(run_first[wave], run_payload[wave], run_value[wave]), (uint64_t)(uintptr_t)sg.src, sg.len, results[i].bits,
                 starts + dict.first_start, results[i].dict_entries, cp, e1, la, lb, lane, [&](uint32_t t, const BrotliAmdUndictBytesEntry& en) {
      const uint32_t at = kPerLane * lane + t;
      pos[slot(at)] = en.pos;
      ends[slot(at + 1u)] = en.len;
      lane_sum += en.len;
    });
    // this lane's first offset: the item's carry-in and the bytes of the lanes below
    uint64_t inc = lane_sum;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
      const uint64_t q = __shfl_up((unsigned long long)inc, off, 64);
      if (lane >= off) inc += q;
    }
    uint64_t run = carries[g] + (inc - lane_sum);
    if (lane == 0u) ends[0] = run;
    for (uint32_t at = kPerLane * lane; at < m && at < kPerLane * (lane + 1u); at++) {   // (a lane's own entries: no other lane has written them)
      run += ends[slot(at + 1u)];
      ends[slot(at + 1u)] = run;
    }
    lds_sync();
    auto end_of = [&](uint32_t t) { return ends[slot(t)]; };
    auto pos_of = [&](uint32_t t) { return pos[slot(t)]; };
    if (sg.offsets != nullptr) {   // (the same in every lane)
      const uint64_t O = (uint64_t)(uintptr_t)sg.offsets;
      const uint32_t ow = brotli_amd_undict_bytes_offset_width(sg.flags);
      uint64_t s0, s1;
      brotli_amd_undict_bytes_offset_slots(sg.flags, e0, e1, &s0, &s1);
      const uint64_t words = brotli_amd_seg_units(O + s0 * ow, (s1 - s0) * ow);
      for (uint64_t q = lane; q < words; q += 64u) brotli_amd_undict_bytes_offsets_word(O, ow, sg.offset_base, s0, s1, end_of, q);
    }
    const uint64_t last = end_of(m);
    uint64_t lo, hi;
    brotli_amd_undict_bytes_data_range(end_of(0u), last, sg.data_cap, &lo, &hi);
    if (sg.data != nullptr && lo < hi) {   // (the same in every lane)
      const uint64_t data = (uint64_t)(uintptr_t)sg.data, words = brotli_amd_seg_units(data + lo, hi - lo);
      for (uint64_t q = lane; q < words; q += 64u) brotli_amd_undict_bytes_data_word(data, (uint64_t)(uintptr_t)dict.dict, m, lo, hi, end_of, pos_of, q);
    }
    // the segment's bytes: the item that holds its last delivered element has them all
    if (lane == 0u && e1 == (count < sg.cap ? count : sg.cap)) results[i].bytes = last;
  }
}

}  // namespace

// The scratch of a launch over `units` units of n segments -- a unit a segment and a unit an item --, nd distinct dictionaries and `starts`
// entry positions of them together: the results first, then the items' prefix array, the checkpoints, the tile records and the carries, the
// dictionaries' results, the positions.
extern "C" uint64_t brotli_amd_undict_bytes_scratch_bytes(uint64_t units, uint32_t n, uint32_t nd, uint64_t starts) {
  return brotli_amd_wave::pad16(Scratch::bytes(units - n, n)) + brotli_amd_wave::pad16((uint64_t)nd * sizeof(DictResult)) + starts * sizeof(uint32_t);
}

// d_table: the n segments; d_dicts: the nd dictionary records; units: n + the items of all segments (the host has the table); d_scratch:
// brotli_amd_undict_bytes_scratch_bytes of device memory, 16-byte aligned; ev[0..5], where not NULL, are recorded in front of, between and
// behind the five launches.  A call without items is the RLE walk alone.
extern "C" hipError_t brotli_amd_launch_undict_bytes(const void* d_table, uint32_t n, uint64_t units, const void* d_dicts, uint32_t nd, void* d_scratch, hipStream_t stream,
                                                     const hipEvent_t* ev) {
  if (n == 0u) return hipSuccess;
  const Seg* d_segs = static_cast<const Seg*>(d_table);
  const Dict* dicts = static_cast<const Dict*>(d_dicts);
  const uint64_t items = units - n;
  const Scratch s(d_scratch, items, n);
  DictResult* dict_results = reinterpret_cast<DictResult*>(static_cast<uint8_t*>(d_scratch) + brotli_amd_wave::pad16(Scratch::bytes(items, n)));
  uint32_t* starts = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(dict_results) + brotli_amd_wave::pad16((uint64_t)nd * sizeof(DictResult)));
  hipError_t e = hipSuccess;
  uint32_t grid = 0;
  if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
  if (nd != 0u) {
    if ((e = brotli_amd_wave::wave_grid(nd, kWaves, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(brotli_amd_undict_bytes_dict_kernel, dim3(grid), dim3(kThreads), 0, stream, dicts, nd, starts, dict_results);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = brotli_amd_wave::launch_walk(brotli_amd_undict_bytes_walk_kernel, d_segs, n, items, s.ckpts, stream, ev ? ev + 1 : nullptr, s.results, s.pre,
                                        static_cast<const DictResult*>(dict_results))) != hipSuccess)
    return e;
  if (items != 0u) {
    if ((e = brotli_amd_wave::wave_grid(items, kWaves, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(brotli_amd_undict_bytes_count_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, items, s.results, static_cast<const uint64_t*>(s.pre), dicts,
                       static_cast<const uint32_t*>(starts), static_cast<const Checkpoint*>(s.ckpts), s.tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[3], stream)) != hipSuccess) return e;
  if (items != 0u && (e = brotli_amd_launch_tile_carries(s.tiles, s.carries, items, stream)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[4], stream)) != hipSuccess) return e;
  if (items != 0u) {
    hipLaunchKernelGGL(brotli_amd_undict_bytes_expand_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, items, s.results, static_cast<const uint64_t*>(s.pre), dicts,
                       static_cast<const uint32_t*>(starts), static_cast<const Checkpoint*>(s.ckpts), static_cast<const uint64_t*>(s.carries));
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[5], stream)) != hipSuccess) return e;
  return hipSuccess;
}
