// brotli_undlba_kernels.hip -- seven launches in stream order that turn the DELTA_LENGTH_BYTE_ARRAY bodies of n independent segments, of any
// alignment and length, into Arrow string columns -- offsets and bytes --, and give every segment its result (gfx950, wave64).  The transform,
// the step from a value to a length and what a segment's last item leaves are csrc/brotli_undlba.h; the grammar, a block, a group and the
// bookkeeping of an item are undbp's (csrc/brotli_undbp.h, csrc/brotli_undbp_groups.h).  No block ever waits for another block's result -- no
// flags, no spins, no atomics on offsets or data.
//   1. brotli_amd_undlba_walk_kernel     undbp's walk as it is, ONE WAVE A SEGMENT: the segment's result -- undbp's seven fields, data_avail,
//                                        bad 0, first_bad none, bytes 0 --, its first value, the checkpoint of every item and the segment's
//                                        entry of the items' prefix array.
//   2. brotli_amd_undlba_sum_kernel      ONE WAVE AN ITEM, undbp's item function and group sum: a lane a group of 32 fields, the item's sum an
//                                        undelta tile record.
//   3. brotli_amd_undelta_carry_kernel   undelta's carry launch itself (csrc/brotli_undelta_kernels.hip): the value in front of every item's
//                                        first delta.
//   4. brotli_amd_undlba_lengths_kernel  the same item function; the lanes redo their 32 values on top of the carry-in and turn each into
//                                        (L, bad).  The wave's sum of good lengths is the item's second tile record; its bad elements go to
//                                        the segment's result with one atomicAdd and one atomicMin.
//   5. brotli_amd_undelta_carry_kernel   the carry launch again, over the byte sums: the bytes in front of every item.
//   6. brotli_amd_undlba_expand_kernel   the same item function; a scan over the lanes' byte sums on top of the carry-in gives a lane its first
//                                        offset.  A lane's entries are 32 NEIGHBOURS: it puts them together into aligned 16-byte stores
//                                        wherever it has a whole word, at either offset width and any alignment of the offsets, and stores the
//                                        few at its two ends one by one.  The item that holds the segment's last delivered element writes the
//                                        result's bytes and data_status and the segment's entry of the table of copies.
//   7. brotli_amd_ragged_copy_kernel     the ragged copy itself (csrc/brotli_copy_kernels.hip) over that table: the work is split by bytes, so
//                                        one segment's data is every CU's.
// A measuring call has no destinations: every store of launch 6 but those of the result and the table is predicated off, and the table's
// lengths are 0.  A call that only counts has no items and is the first launch alone.
// THE SCRATCH behind the table: the n results, the n first values, the items' prefix array, and for every item a checkpoint, a tile record and
// a carry (csrc/brotli_run_items.h); behind them a second tile record and a second carry an item, and the n entries of the table of copies,
// which is zeroed in front of the launches.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_run_items.h"      // the walk's frame, the scratch and the walk's launch
#include "brotli_seg_walk.h"
#include "brotli_undbp_groups.h"   // an item's groups, a group a lane
#include "brotli_undlba.h"
#include "brotli_wave_stage.h"

// (csrc/brotli_copy_kernels.hip)
extern "C" hipError_t brotli_amd_launch_ragged_copy_sized(const BrotliAmdCopySeg* d_segs, uint32_t n, uint64_t max_bytes, hipStream_t stream);

namespace {

constexpr uint32_t kThreads = brotli_amd_wave::kSegThreads, kWaves = brotli_amd_wave::kSegWaves;
constexpr uint32_t kChunk = brotli_amd_wave::kStageChunk, kItem = BROTLI_AMD_UNDBP_ITEM_DELTAS, kGroup = BROTLI_AMD_UNDBP_GROUP;

static_assert(kItem == 64u * kGroup, "a group a lane");

using brotli_amd_wave::dbp_item_groups;
using brotli_amd_wave::same;
using brotli_amd_wave::Stage;
using brotli_amd_wave::Word16;

typedef BrotliAmdUndlbaSeg Seg;
typedef BrotliAmdUndlbaResult Result;
typedef BrotliAmdUndbpCheckpoint Checkpoint;
typedef BrotliAmdUndeltaTile Tile;
typedef brotli_amd_wave::DbpGroup Group;
typedef brotli_amd_wave::ItemScratch<Result, Checkpoint, true, true> Scratch;

// ---- launch 1 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undlba_walk_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* __restrict__ results,
                                                                          uint64_t* __restrict__ firsts, uint64_t* __restrict__ pre, Checkpoint* __restrict__ ckpts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  struct Walked { BrotliAmdUndbpResult res; uint64_t first; };
  brotli_amd_wave::walk_segments(
      stage, segs, n, items, pre, ckpts,
      [](const Seg& sg, Stage& rd, auto mark) {
        Walked got = {{}, 0u};
        got.res = brotli_amd_undbp_walk(rd, sg.len, sg.cap, kItem, &got.first, mark);
        return got;
      },
      [&](uint64_t i, const Seg& sg, const Walked& got) {
        results[i] = brotli_amd_undlba_result(got.res, sg.len);   // (what the items add to)
        firsts[i] = got.first;
      });
}

// ---- launch 2 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undlba_sum_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, const Result* __restrict__ results,
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

// ---- launches 4 and 6 ----
// The value in front of this lane's group: the item's carry-in, `first` in a segment's first item, the groups of the lanes below.
__device__ __forceinline__ uint64_t value_in_front(const Group& grp, uint64_t carry, uint64_t first, uint32_t lane) {
  const uint64_t sum = brotli_amd_undbp_group_sum(grp.at, grp.k, grp.min_delta, grp.nf);
  uint64_t inc = sum;
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint64_t q = (uint64_t)__shfl_up((unsigned long long)inc, off, 64);
    if (lane >= off) inc += q;
  }
  return carry + first + (inc - sum);
}
// Whether item j of segment i has elements, by its checkpoint: the segment's first item has element 0, every other one those of its deltas.
// (The same in every lane.)
__device__ __forceinline__ bool item_taken(const Checkpoint* __restrict__ ckpts, uint64_t g, uint64_t j, uint64_t count, uint64_t cap, bool deltas) {
  if (ckpts[g].off == BROTLI_AMD_UNDBP_NONE) return false;
  return j == 0u ? count != 0u && cap != 0u : deltas;
}

__global__ __launch_bounds__(kThreads) void brotli_amd_undlba_lengths_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* results,
                                                                             const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ pre,
                                                                             const Checkpoint* __restrict__ ckpts, const uint64_t* __restrict__ carries,
                                                                             Tile* __restrict__ byte_tiles) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    uint32_t i; uint64_t j, a = 0; Group grp;
    const bool deltas = dbp_item_groups<kItem>(stage[wave], segs, n, static_cast<const Result*>(results), pre, ckpts, g, lane, &i, &j, &a, &grp);
    uint64_t bytes = 0;
    if (item_taken(ckpts, g, j, results[i].count, segs[i].cap, deltas)) {
      uint64_t v = value_in_front(grp, carries[g], j == 0u ? firsts[i] : 0u, lane);
      const uint64_t e0 = a + (uint64_t)kGroup * lane + 1u;   // the element behind this lane's first delta
      uint32_t lane_bad = 0;                          // this lane's bad elements,
      uint64_t lane_first = BROTLI_AMD_UNDLBA_NONE;   // and the first of them
      auto take = [&](uint64_t e, uint64_t value) {
        const BrotliAmdUndlbaLength L = brotli_amd_undlba_length(value);
        bytes += L.len;
        if (L.bad != 0u) { lane_bad++; if (e < lane_first) lane_first = e; }
      };
      if (j == 0u && lane == 0u) take(0u, v);   // element 0 is `first`
      for (uint32_t t = 0; t < grp.nf; t++) {
        v += grp.min_delta + brotli_amd_undbp_field(grp.at, grp.k, t);
        take(e0 + t, v);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) bytes += __shfl_xor((unsigned long long)bytes, off);
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
    if (lane == 0u) byte_tiles[g] = brotli_amd_undlba_tile(j, bytes);
  }
}

__global__ __launch_bounds__(kThreads) void brotli_amd_undlba_expand_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* results,
                                                                            const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ pre,
                                                                            const Checkpoint* __restrict__ ckpts, const uint64_t* __restrict__ carries,
                                                                            const uint64_t* __restrict__ byte_carries, BrotliAmdCopySeg* __restrict__ copies) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < items; g += (uint64_t)gridDim.x * kWaves) {
    uint32_t i; uint64_t j, a = 0; Group grp;
    const bool deltas = dbp_item_groups<kItem>(stage[wave], segs, n, static_cast<const Result*>(results), pre, ckpts, g, lane, &i, &j, &a, &grp);
    const Seg sg = segs[i];
    const uint64_t count = results[i].count;
    if (j == 0u && lane == 0u) brotli_amd_undlba_first_offset(sg);
    uint64_t a_, b_;   // the item's deltas, whatever its checkpoint is
    brotli_amd_undbp_item_range(count, sg.cap, j, kItem, &a_, &b_);
    uint64_t total = byte_carries[g];   // the bytes up to and with this item's elements
    if (item_taken(ckpts, g, j, count, sg.cap, deltas)) {
      const uint64_t v0 = value_in_front(grp, carries[g], j == 0u ? firsts[i] : 0u, lane);
      const bool lead0 = j == 0u && lane == 0u;
      // this lane's bytes, and with those of the lanes below and the carry-in its first offset
      uint64_t v = v0, mine = 0;
      if (lead0) mine += brotli_amd_undlba_length(v).len;
      for (uint32_t t = 0; t < grp.nf; t++) {
        v += grp.min_delta + brotli_amd_undbp_field(grp.at, grp.k, t);
        mine += brotli_amd_undlba_length(v).len;
      }
      uint64_t inc = mine;
#pragma unroll
      for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint64_t q = (uint64_t)__shfl_up((unsigned long long)inc, off, 64);
        if (lane >= off) inc += q;
      }
      uint64_t run = total + (inc - mine);
      total += (uint64_t)__shfl((unsigned long long)inc, 63, 64);
      if (sg.offsets != nullptr) {   // (the same in every lane)
        // this lane's elements [e, e1): the one behind each of its deltas, and element 0 in front of them for the first lane of a first item;
        // the end of element e is entry e from `ends` on
        bool lead = lead0;
        const uint32_t w = brotli_amd_undlba_offset_width(sg.flags), per_word = 16u / w;
        const uint64_t ends = brotli_amd_undlba_ends_at(sg), e0 = a_ + (uint64_t)kGroup * lane + 1u;
        uint64_t e = lead ? 0u : e0;
        const uint64_t e1 = e0 + grp.nf;
        uint32_t t = 0;
        v = v0;
        auto next = [&]() {   // the ends one after the other
          if (lead) lead = false;
          else v += grp.min_delta + brotli_amd_undbp_field(grp.at, grp.k, t++);
          run += brotli_amd_undlba_length(v).len;
          return sg.offset_base + run;
        };
        while (e < e1) {
          const uint64_t at = ends + e * w;
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
    if (lane == 0u && brotli_amd_undlba_last_item(count, sg.cap, j, a_, b_)) brotli_amd_undlba_finish(sg, &results[i], total, &copies[i]);
  }
}

// the second tile records, the second carries and the table of copies behind the scratch of csrc/brotli_run_items.h
struct Behind {
  Tile* byte_tiles;
  uint64_t* byte_carries;
  BrotliAmdCopySeg* copies;
  static uint64_t bytes(uint64_t items, uint32_t n) { return items * (sizeof(Tile) + sizeof(uint64_t)) + brotli_amd_wave::pad16((uint64_t)n * sizeof(BrotliAmdCopySeg)); }
  Behind(void* d_scratch, uint64_t items, uint32_t n) {
    uint8_t* at = static_cast<uint8_t*>(d_scratch) + brotli_amd_wave::pad16(Scratch::bytes(items, n));
    byte_tiles = reinterpret_cast<Tile*>(at); at += items * sizeof(Tile);
    byte_carries = reinterpret_cast<uint64_t*>(at); at += items * sizeof(uint64_t);
    copies = reinterpret_cast<BrotliAmdCopySeg*>(at);
  }
};

}  // namespace

// the scratch of a launch over `units` units of n segments -- a unit a segment and a unit an item
extern "C" uint64_t brotli_amd_undlba_scratch_bytes(uint64_t units, uint32_t n) {
  return brotli_amd_wave::pad16(Scratch::bytes(units - n, n)) + Behind::bytes(units - n, n);
}

// d_table: the n segments; units: n + the items of all segments (the host has the table); max_bytes: what the segments' copies add up to at
// the most; d_scratch: brotli_amd_undlba_scratch_bytes of device memory, 16-byte aligned; ev[0..7], where not NULL, are recorded in front of,
// between and behind the seven launches.  A call without items is the walk alone.
extern "C" hipError_t brotli_amd_launch_undlba(const void* d_table, uint32_t n, uint64_t units, uint64_t max_bytes, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  if (n == 0u) return hipSuccess;
  const Seg* d_segs = static_cast<const Seg*>(d_table);
  const uint64_t items = units - n;
  const Scratch s(d_scratch, items, n);
  const Behind b(d_scratch, items, n);
  hipError_t e = hipSuccess;
  uint32_t grid = 0;
  if (items != 0u && (e = hipMemsetAsync(b.copies, 0, (size_t)n * sizeof(BrotliAmdCopySeg), stream)) != hipSuccess) return e;
  if ((e = brotli_amd_wave::launch_walk(brotli_amd_undlba_walk_kernel, d_segs, n, items, s.ckpts, stream, ev, s.results, s.column, s.pre)) != hipSuccess) return e;
  const Result* results = s.results;
  const uint64_t *firsts = s.column, *pre = s.pre, *carries = s.carries, *byte_carries = b.byte_carries;
  const Checkpoint* ckpts = s.ckpts;
  if (items != 0u) {
    if ((e = brotli_amd_wave::wave_grid(items, kWaves, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(brotli_amd_undlba_sum_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, items, results, firsts, pre, ckpts, s.tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
  if (items != 0u && (e = brotli_amd_launch_tile_carries(s.tiles, s.carries, items, stream)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[3], stream)) != hipSuccess) return e;
  if (items != 0u) {
    hipLaunchKernelGGL(brotli_amd_undlba_lengths_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, items, s.results, firsts, pre, ckpts, carries, b.byte_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[4], stream)) != hipSuccess) return e;
  if (items != 0u && (e = brotli_amd_launch_tile_carries(b.byte_tiles, b.byte_carries, items, stream)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[5], stream)) != hipSuccess) return e;
  if (items != 0u) {
    hipLaunchKernelGGL(brotli_amd_undlba_expand_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, items, s.results, firsts, pre, ckpts, carries, byte_carries, b.copies);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[6], stream)) != hipSuccess) return e;
  // (a measuring call: every length of the table is 0, and a block finds that out)
  if (items != 0u && (e = brotli_amd_launch_ragged_copy_sized(b.copies, n, max_bytes != 0u ? max_bytes : 1u, stream)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[7], stream)) != hipSuccess) return e;
  return hipSuccess;
}
