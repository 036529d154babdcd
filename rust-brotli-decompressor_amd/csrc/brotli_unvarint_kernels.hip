// brotli_unvarint_kernels.hip -- three launches in stream order that turn the LEB128 varints of n independent segments, of any alignment and
// length, back into elements of 1, 2, 4 or 8 bytes, and give every segment its result: the number of varints, the bytes they take and the
// overlong ones among them (gfx950, wave64).  The transform, what one unit of work reads and writes, and the bookkeeping of a tile are
// csrc/brotli_unvarint.h.
//
// Work is split by BYTES, not by segments: the segment walk of csrc/brotli_seg_walk.h over the words of SOURCE memory, in tiles of
// BROTLI_AMD_UNVARINT_TILE_BYTES, in phases 1 and 3.  Where an element goes depends on how many varints end in front of it, so a long segment's
// tiles need the counts of the tiles in front of them.  That is undelta's running sum with a popcount for a sum, and the skeleton is undelta's
// (csrc/brotli_undelta_kernels.hip): no block ever waits for another block's result.
//   1. brotli_amd_unvarint_count_kernel  every tile's summary: the ends in its last piece (striped over the threads) and the two facts.
//   2. undelta's carry launch itself      (brotli_amd_launch_tile_carries): the summaries -> carry_in[].
//   3. brotli_amd_unvarint_emit_kernel    every tile: a thread takes kUnitsPerThread NEIGHBOURING units, 64 bytes, and a running count with
//                                         restarts over the units -- serial in the thread, __shfl_up in the wave, LDS across the waves, keyed by
//                                         the unit-to-segment search -- gives every unit the index of its first element; the tile's first piece
//                                         starts from carry_in.  The thread then stores the elements whose ends lie in its bytes, up to cap: the
//                                         direct form, every thread its own run of elements.
// THE RESULTS lie behind the table and start as zeros.  The lane that holds a segment's last unit stores count.  consumed is a maximum and overlong
// a sum over the units, in any order: atomicMax / atomicAdd on the segment's result.  In a tile that lies inside one segment -- every tile of a
// long one -- they are reduced across the wave's lanes first and then WAIT in the wave, across the block's tiles, until the segment changes or the
// kernel ends: a segment of a gigabyte gets a few thousand atomics, not one a unit (the digest kernel's add_terms lesson).  Elsewhere a lane adds
// what its units found, neighbouring units of one segment together.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_seg_walk.h"
#include "brotli_unvarint.h"

// (csrc/brotli_undelta_kernels.hip)
extern "C" hipError_t brotli_amd_launch_tile_carries(const BrotliAmdUndeltaTile* tiles, uint64_t* carries, uint64_t ntiles, hipStream_t stream);

namespace {

constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS, kChunkSegs = BROTLI_AMD_SEG_CHUNK_SEGS;
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kUnitsPerThread = 4;
constexpr uint32_t kTileUnits = kThreads * kUnitsPerThread;

static_assert(kTileUnits * 16u == BROTLI_AMD_UNVARINT_TILE_BYTES, "the tile the header names");

typedef BrotliAmdUnvarintSeg Seg;
typedef BrotliAmdUndeltaPair Pair;
typedef unsigned long long Word;   // a result's field as the atomics take it

__device__ __forceinline__ Pair shfl_up_pair(Pair p, uint32_t off) {
  return Pair{(uint64_t)__shfl_up((unsigned long long)p.sum, off, 64), (uint32_t)__shfl_up((int)p.head, off, 64)};
}
// the running combination over the wave's lanes, this lane's included
__device__ __forceinline__ Pair wave_scan(Pair p, uint32_t lane) {
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const Pair q = shfl_up_pair(p, off);
    if (lane >= off) p = brotli_amd_undelta_combine(q, p);
  }
  return p;
}

// the address whose words are a segment's units
struct SrcOf { __device__ __forceinline__ const uint8_t* operator()(const Seg& sg) const { return sg.src; } };

// what a unit found into its segment's result (the fields are 64 bits wide; nothing is added where there is nothing)
__device__ __forceinline__ void add_part(BrotliAmdUnvarintResult* r, uint64_t consumed, uint64_t overlong) {
  if (consumed != 0u) atomicMax(reinterpret_cast<Word*>(&r->consumed), (Word)consumed);
  if (overlong != 0u) atomicAdd(reinterpret_cast<Word*>(&r->overlong), (Word)overlong);
}

// ---- phase 1 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_unvarint_count_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t units,
                                                                             BrotliAmdUndeltaTile* __restrict__ tiles) {
  __shared__ uint64_t pre[kChunkSegs + 1];   // units in front of each segment of the chunk (in front of the chunk included); [kChunkSegs]: behind its last
  __shared__ uint64_t scan[kThreads];
  __shared__ uint32_t wsum[kWaves];
  const uint32_t tid = threadIdx.x;
  brotli_amd_seg_walk<kTileUnits>(segs, n, pre, scan, SrcOf(), [&](const uint64_t* pre, const Seg* segs, uint32_t, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t tile) {
    if (lo == t0 && tid == 0u) tiles[tile].cont = brotli_amd_undelta_cont(pre, kChunkSegs, t0);
    const uint64_t tile_end = t0 + kTileUnits < units ? t0 + kTileUnits : units;
    if (hi != tile_end) return;   // (the tile's end lies in a later chunk's segments)
    uint32_t j = 0;
    const uint64_t from = brotli_amd_undelta_last_piece(pre, kChunkSegs, lo, hi, &j);
    const Seg sg = segs[j];
    const uint64_t first = pre[j], src = (uint64_t)(uintptr_t)sg.src;
    // this thread's share of the piece: at most kUnitsPerThread units, striped (a count has no order)
    uint32_t ends[kUnitsPerThread];
#pragma unroll
    for (uint32_t it = 0; it < kUnitsPerThread; it++) {
      const uint64_t g = from + it * kThreads + tid;
      ends[it] = 0u;
      if (g < hi) (void)brotli_amd_unvarint_fetch(src, sg.len, g - first, &ends[it]);
    }
    uint32_t c = 0;
#pragma unroll
    for (uint32_t it = 0; it < kUnitsPerThread; it++) c += brotli_amd_unvarint_popc(ends[it]);
#pragma unroll
    for (uint32_t off = 32; off != 0u; off >>= 1) c += (uint32_t)__shfl_down((int)c, off, 64);
    __syncthreads();   // (the part before is done with wsum[])
    if ((tid & 63u) == 0u) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0u) {
      uint64_t s = 0;
#pragma unroll
      for (uint32_t w = 0; w < kWaves; w++) s += wsum[w];
      tiles[tile].sum = s;
      tiles[tile].nohead = brotli_amd_undelta_nohead(first, t0);
    }
  });
}

// ---- phase 3 ----
// What a wave keeps between its block's tiles: what the tiles inside one segment found, reduced across its lanes (the same in every lane).
struct Waiting {
  bool any = false;
  uint32_t seg = 0;   // (the segment's number in the whole table, so it may wait across chunks of segments)
  uint64_t consumed = 0, overlong = 0;
};
__device__ __forceinline__ void settle(Waiting& wt, uint32_t lane, BrotliAmdUnvarintResult* results) {
  if (wt.any && lane == 0u) add_part(results + wt.seg, wt.consumed, wt.overlong);
  wt = Waiting();
}

__global__ __launch_bounds__(kThreads) void brotli_amd_unvarint_emit_kernel(const Seg* __restrict__ segs, uint32_t n, const uint64_t* __restrict__ carries,
                                                                            BrotliAmdUnvarintResult* __restrict__ results) {
  __shared__ uint64_t pre[kChunkSegs + 1];
  __shared__ uint64_t scan[kThreads];
  __shared__ uint64_t wsum[kWaves];
  __shared__ uint32_t whead[kWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  Waiting wt;
  brotli_amd_seg_walk<kTileUnits>(segs, n, pre, scan, SrcOf(), [&](const uint64_t* pre, const Seg* segs, uint32_t c0, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t tile) {
    // (a part that does not begin the tile begins a chunk of segments: its first unit is a segment's first)
    const uint64_t carry_in = lo == t0 ? carries[tile] : 0u;
    const uint32_t ja = brotli_amd_seg_find(pre, kChunkSegs, lo), jb = brotli_amd_seg_find(pre, kChunkSegs, hi - 1u);
    BrotliAmdU4 v[kUnitsPerThread];
    uint64_t k[kUnitsPerThread];
    uint32_t seg[kUnitsPerThread], ends[kUnitsPerThread];
    Pair mine = {0u, 0u};   // this thread's units together
#pragma unroll
    for (uint32_t i = 0; i < kUnitsPerThread; i++) {
      const uint64_t g = t0 + kUnitsPerThread * tid + i;
      v[i] = BrotliAmdU4{0u, 0u, 0u, 0u}; ends[i] = 0u; k[i] = ~(uint64_t)0; seg[i] = ja;
      if (g >= lo && g < hi) {
        if (ja != jb) seg[i] = brotli_amd_seg_find(pre, kChunkSegs, g);   // (one segment's tile -- the rule for a long one -- is searched for once)
        const Seg sg = segs[seg[i]];
        k[i] = g - pre[seg[i]];
        v[i] = brotli_amd_unvarint_fetch((uint64_t)(uintptr_t)sg.src, sg.len, k[i], &ends[i]);
        mine = brotli_amd_undelta_combine(mine, Pair{brotli_amd_unvarint_total(ends[i]), k[i] == 0u ? 1u : 0u});
      }
    }
    const Pair inc = wave_scan(mine, lane);
    __syncthreads();   // (the part before is done with wsum[])
    if (lane == 63u) { wsum[wave] = inc.sum; whead[wave] = inc.head; }
    __syncthreads();
    Pair run = {carry_in, 0u};   // what lies in front of this thread's first unit
#pragma unroll
    for (uint32_t w = 0; w < kWaves; w++)
      if (w < wave) run = brotli_amd_undelta_combine(run, Pair{wsum[w], whead[w]});
    Pair ex = shfl_up_pair(inc, 1u);
    if (lane == 0u) ex = Pair{0u, 0u};
    run = brotli_amd_undelta_combine(run, ex);
    // what this thread's units found, neighbouring units of one segment together
    bool have = false;
    uint32_t found_seg = 0;
    uint64_t consumed = 0, overlong = 0;
#pragma unroll
    for (uint32_t i = 0; i < kUnitsPerThread; i++) {
      if (k[i] == ~(uint64_t)0) continue;
      const Seg sg = segs[seg[i]];
      if (k[i] == 0u) run.sum = 0u;   // a segment's first unit restarts
      BrotliAmdU4 prev = {0u, 0u, 0u, 0u};
      if (k[i] != 0u) {   // the word in front: the neighbour's where this thread holds it (i - 1 is then this segment's unit k - 1)
        uint32_t none = 0;
        if (i != 0u && k[i != 0u ? i - 1u : 0u] + 1u == k[i]) prev = v[i != 0u ? i - 1u : 0u];
        else prev = brotli_amd_unvarint_fetch((uint64_t)(uintptr_t)sg.src, sg.len, k[i] - 1u, &none);
      }
      const BrotliAmdUnvarintPart part = brotli_amd_unvarint_emit(sg, k[i], prev, v[i], ends[i], run.sum);
      run.sum += brotli_amd_unvarint_total(ends[i]);
      if (k[i] + 1u == pre[seg[i] + 1u] - pre[seg[i]]) results[c0 + seg[i]].count = run.sum;   // the segment's last unit
      if (have && found_seg != c0 + seg[i]) { add_part(results + found_seg, consumed, overlong); consumed = 0u; overlong = 0u; }
      have = true; found_seg = c0 + seg[i];
      consumed = part.consumed > consumed ? part.consumed : consumed;
      overlong += part.overlong;
    }
    if (ja == jb) {   // one segment's: across the wave's lanes, and it waits
      if (wt.any && wt.seg != c0 + ja) settle(wt, lane, results);
#pragma unroll
      for (uint32_t off = 32; off != 0u; off >>= 1) {
        const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)consumed, off, 64);
        consumed = other > consumed ? other : consumed;
        overlong += (uint64_t)__shfl_xor((unsigned long long)overlong, off, 64);
      }
      wt.any = true; wt.seg = c0 + ja;
      wt.consumed = consumed > wt.consumed ? consumed : wt.consumed;
      wt.overlong += overlong;
    } else if (have) {
      add_part(results + found_seg, consumed, overlong);
    }
  });
  settle(wt, lane, results);
}

}  // namespace

extern "C" uint32_t brotli_amd_unvarint_tile_bytes(void) { return BROTLI_AMD_UNVARINT_TILE_BYTES; }
// the scratch of a launch over `units` units of n segments: the segments' results first, then the tiles' summaries and their carries, which
// start at a multiple of 16 bytes as they do where nothing lies in front of them
static constexpr uint64_t results_bytes(uint32_t n) { return ((uint64_t)n * sizeof(BrotliAmdUnvarintResult) + 15u) & ~(uint64_t)15; }
extern "C" uint64_t brotli_amd_unvarint_scratch_bytes(uint64_t units, uint32_t n) {
  return results_bytes(n) + ((units + kTileUnits - 1u) / kTileUnits) * (sizeof(BrotliAmdUndeltaTile) + sizeof(uint64_t));
}

// units: the units of all segments' SOURCES together (brotli_amd_seg_units: the host has the table); d_scratch: brotli_amd_unvarint_scratch_bytes
// of device memory, 16-byte aligned -- the results in it are zeroed here, on `stream`; ev[0..3], where not NULL, are recorded in front of, between
// and behind the three launches
extern "C" hipError_t brotli_amd_launch_unvarint(const void* d_table, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  if (n == 0u) return hipSuccess;
  const BrotliAmdUnvarintSeg* d_segs = static_cast<const BrotliAmdUnvarintSeg*>(d_table);
  const uint64_t ntiles = (units + kTileUnits - 1u) / kTileUnits;
  BrotliAmdUnvarintResult* results = static_cast<BrotliAmdUnvarintResult*>(d_scratch);
  BrotliAmdUndeltaTile* tiles = reinterpret_cast<BrotliAmdUndeltaTile*>(static_cast<uint8_t*>(d_scratch) + results_bytes(n));
  uint64_t* carries = reinterpret_cast<uint64_t*>(tiles + ntiles);
  hipError_t e = hipMemsetAsync(results, 0, (size_t)n * sizeof(BrotliAmdUnvarintResult), stream);
  if (e != hipSuccess || units == 0u) return e;
  uint32_t grid = 0;
  if ((e = brotli_amd_seg_grid(units, kTileUnits, &grid)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(brotli_amd_unvarint_count_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, units, tiles);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
  if ((e = brotli_amd_launch_tile_carries(tiles, carries, ntiles, stream)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(brotli_amd_unvarint_emit_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, carries, results);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[3], stream)) != hipSuccess) return e;
  return hipSuccess;
}
