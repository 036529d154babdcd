// brotli_undelta_kernels.hip -- three launches in stream order that turn the deltas of n independent segments, of any alignment, length and width
// (1, 2, 4, 8), back into values: a wrapping running sum per segment (gfx950, wave64).  The transform, what one unit of work reads and writes,
// and the bookkeeping of a tile are csrc/brotli_undelta.h.
//
// Work is split by BYTES, not by segments: the segment walk of csrc/brotli_seg_walk.h over the words of DESTINATION memory, in tiles of
// BROTLI_AMD_UNDELTA_TILE_BYTES, in phases 1 and 3.  A running sum is not local, so a long segment's
// tiles need the sums of the tiles in front of them.  No block ever waits for another block's result -- no look-back, no flags, no spins, no
// grid barrier: blocks take tiles in turns, so the owner of a tile in front need not even be resident.  Instead:
//   1. brotli_amd_undelta_sum_kernel    every tile's summary: the sum of its last piece (striped over the threads: a sum has no order) and the
//                                       two facts.  A tile of short segments reads a few units, a tile inside a long one all of its source.
//   2. brotli_amd_undelta_carry_kernel  ONE block: a running sum with restarts over the summaries, kCarrySpan tiles a pass -> carry_in[].
//   3. brotli_amd_undelta_apply_kernel  every tile: a thread takes kUnitsPerThread NEIGHBOURING units, fetches them, and a running sum with
//                                       restarts over the contributions -- serial in the thread, __shfl_up in the wave, LDS across the waves,
//                                       keyed by the unit-to-segment search, so a tile of many short segments is one pass -- gives every unit
//                                       its carry; the tile's first piece starts from carry_in.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_seg_walk.h"
#include "brotli_undelta.h"

namespace {

constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS, kChunkSegs = BROTLI_AMD_SEG_CHUNK_SEGS;
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kUnitsPerThread = 4;
constexpr uint32_t kTileUnits = kThreads * kUnitsPerThread;
constexpr uint32_t kCarryThreads = 1024;        // phase 2: kCarryPerThread neighbouring tiles a thread and pass
constexpr uint32_t kCarryPerThread = 4;
constexpr uint32_t kCarrySpan = kCarryThreads * kCarryPerThread;

static_assert(kTileUnits * 16u == BROTLI_AMD_UNDELTA_TILE_BYTES, "the tile the header names");

typedef BrotliAmdUnshuffleSeg Seg;
typedef BrotliAmdUndeltaPair Pair;

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
struct DstOf { __device__ __forceinline__ const uint8_t* operator()(const Seg& sg) const { return sg.dst; } };

// ---- phase 1 ----
// the sum of the contributions of the units [from, hi) of one segment of width W whose first unit is `first`: this thread's share (at most
// kUnitsPerThread units, striped)
template <uint32_t W>
__device__ __forceinline__ uint64_t piece_sum(const Seg& sg, uint64_t first, uint64_t from, uint64_t hi, uint32_t tid) {
  const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst;
  BrotliAmdU4 v[kUnitsPerThread];
#pragma unroll
  for (uint32_t it = 0; it < kUnitsPerThread; it++) {
    const uint64_t g = from + it * kThreads + tid;
    v[it] = BrotliAmdU4{0u, 0u, 0u, 0u};
    if (g < hi) v[it] = brotli_amd_undelta_fetch_w<W>(src, dst, sg.len, g - first);
  }
  uint64_t c = 0;
#pragma unroll
  for (uint32_t it = 0; it < kUnitsPerThread; it++) c += brotli_amd_undelta_total_w<W>(v[it]);
  return c;
}

__global__ __launch_bounds__(kThreads) void brotli_amd_undelta_sum_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t units,
                                                                          BrotliAmdUndeltaTile* __restrict__ tiles) {
  __shared__ uint64_t pre[kChunkSegs + 1];   // units in front of each segment of the chunk (in front of the chunk included); [kChunkSegs]: behind its last
  __shared__ uint64_t scan[kThreads];
  __shared__ uint64_t wsum[kWaves];
  const uint32_t tid = threadIdx.x;
  brotli_amd_seg_walk<kTileUnits>(segs, n, pre, scan, DstOf(), [&](const uint64_t* pre, const Seg* segs, uint32_t, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t tile) {
    if (lo == t0 && tid == 0u) tiles[tile].cont = brotli_amd_undelta_cont(pre, kChunkSegs, t0);
    const uint64_t tile_end = t0 + kTileUnits < units ? t0 + kTileUnits : units;
    if (hi != tile_end) return;   // (the tile's end lies in a later chunk's segments)
    uint32_t j = 0;
    const uint64_t from = brotli_amd_undelta_last_piece(pre, kChunkSegs, lo, hi, &j);
    const Seg sg = segs[j];
    const uint64_t first = pre[j];
    uint64_t c = 0;
    switch (sg.width) {
      case 1u: c = piece_sum<1u>(sg, first, from, hi, tid); break;
      case 2u: c = piece_sum<2u>(sg, first, from, hi, tid); break;
      case 4u: c = piece_sum<4u>(sg, first, from, hi, tid); break;
      case 8u: c = piece_sum<8u>(sg, first, from, hi, tid); break;
      default: break;   // (the host lets no other width through)
    }
#pragma unroll
    for (uint32_t off = 32; off != 0u; off >>= 1) c += (uint64_t)__shfl_down((unsigned long long)c, off, 64);
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

// ---- phase 2 ----
__global__ __launch_bounds__(kCarryThreads) void brotli_amd_undelta_carry_kernel(const BrotliAmdUndeltaTile* __restrict__ tiles, uint64_t* __restrict__ carries,
                                                                                 uint64_t ntiles) {
  __shared__ uint64_t wsum[kCarryThreads / 64u];
  __shared__ uint32_t whead[kCarryThreads / 64u];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const BrotliAmdUndeltaTile none = {0u, 0u, 1u};   // behind the last tile: passes everything through
  Pair out = {0u, 0u};                              // carry_out of the tile in front of the pass
  BrotliAmdUndeltaTile cur[kCarryPerThread], next[kCarryPerThread];
#pragma unroll
  for (uint32_t i = 0; i < kCarryPerThread; i++) next[i] = kCarryPerThread * tid + i < ntiles ? tiles[kCarryPerThread * tid + i] : none;
  for (uint64_t at = 0; at < ntiles; at += kCarrySpan) {
    const uint64_t t = at + kCarryPerThread * tid;   // this thread's first tile
    Pair mine = {0u, 0u};                            // this thread's tiles together
#pragma unroll
    for (uint32_t i = 0; i < kCarryPerThread; i++) {
      cur[i] = next[i];
      next[i] = t + kCarrySpan + i < ntiles ? tiles[t + kCarrySpan + i] : none;   // (the next pass's, on its way during this pass)
      mine = brotli_amd_undelta_combine(mine, brotli_amd_undelta_tile_pair(cur[i]));
    }
    const Pair inc = wave_scan(mine, lane);
    if (lane == 63u) { wsum[wave] = inc.sum; whead[wave] = inc.head; }
    __syncthreads();
    Pair before = out;   // carry_out of the tile in front of this wave's first
#pragma unroll
    for (uint32_t w = 0; w < kCarryThreads / 64u; w++) {
      if (w == wave) before = out;
      out = brotli_amd_undelta_combine(out, Pair{wsum[w], whead[w]});
    }
    Pair ex = shfl_up_pair(inc, 1u);
    if (lane == 0u) ex = Pair{0u, 0u};
    Pair run = brotli_amd_undelta_combine(before, ex);   // carry_out of the tile in front of this thread's first
#pragma unroll
    for (uint32_t i = 0; i < kCarryPerThread; i++) {
      if (t + i < ntiles) carries[t + i] = brotli_amd_undelta_carry_in(run.sum, cur[i]);
      run = brotli_amd_undelta_combine(run, brotli_amd_undelta_tile_pair(cur[i]));
    }
    __syncthreads();   // (before the next pass writes wsum[])
  }
}

// ---- phase 3 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undelta_apply_kernel(const Seg* __restrict__ segs, uint32_t n, const uint64_t* __restrict__ carries) {
  __shared__ uint64_t pre[kChunkSegs + 1];
  __shared__ uint64_t scan[kThreads];
  __shared__ uint64_t wsum[kWaves];
  __shared__ uint32_t whead[kWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  brotli_amd_seg_walk<kTileUnits>(segs, n, pre, scan, DstOf(), [&](const uint64_t* pre, const Seg* segs, uint32_t, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t tile) {
    // (a part that does not begin the tile begins a chunk of segments: its first unit is a segment's first)
    const uint64_t carry_in = lo == t0 ? carries[tile] : 0u;
    const uint32_t ja = brotli_amd_seg_find(pre, kChunkSegs, lo), jb = brotli_amd_seg_find(pre, kChunkSegs, hi - 1u);
    BrotliAmdU4 v[kUnitsPerThread];
    uint64_t c[kUnitsPerThread], k[kUnitsPerThread];
    uint32_t seg[kUnitsPerThread];
    Pair mine = {0u, 0u};   // this thread's units together
#pragma unroll
    for (uint32_t i = 0; i < kUnitsPerThread; i++) {
      const uint64_t g = t0 + kUnitsPerThread * tid + i;
      v[i] = BrotliAmdU4{0u, 0u, 0u, 0u}; c[i] = 0u; k[i] = ~(uint64_t)0; seg[i] = ja;
      if (g >= lo && g < hi) {
        if (ja != jb) seg[i] = brotli_amd_seg_find(pre, kChunkSegs, g);   // (one segment's tile -- the rule for a long one -- is searched for once)
        const Seg sg = segs[seg[i]];
        k[i] = g - pre[seg[i]];
        v[i] = brotli_amd_undelta_fetch((uint64_t)(uintptr_t)sg.src, (uint64_t)(uintptr_t)sg.dst, sg.len, sg.width, k[i]);
        c[i] = brotli_amd_undelta_total(v[i], sg.width);
        mine = brotli_amd_undelta_combine(mine, Pair{c[i], k[i] == 0u ? 1u : 0u});
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
#pragma unroll
    for (uint32_t i = 0; i < kUnitsPerThread; i++) {
      if (k[i] == ~(uint64_t)0) continue;
      const Seg sg = segs[seg[i]];
      if (k[i] == 0u) run.sum = 0u;   // a segment's first unit restarts
      brotli_amd_undelta_finish((uint64_t)(uintptr_t)sg.src, (uint64_t)(uintptr_t)sg.dst, sg.len, sg.width, k[i], v[i], run.sum);
      run.sum += c[i];
    }
  });
}

}  // namespace

extern "C" uint32_t brotli_amd_undelta_tile_bytes(void) { return BROTLI_AMD_UNDELTA_TILE_BYTES; }
extern "C" uint32_t brotli_amd_undelta_carry_span(void) { return kCarrySpan; }
// the scratch of a launch over `units` units: the tiles' summaries, then their carries
extern "C" uint64_t brotli_amd_undelta_scratch_bytes(uint64_t units) {
  return ((units + kTileUnits - 1u) / kTileUnits) * (sizeof(BrotliAmdUndeltaTile) + sizeof(uint64_t));
}

// The carry launch alone, for every call whose tiles leave BrotliAmdUndeltaTile records (undelta's sums, unvarint's counts of ends): ONE block turns
// tiles[0..ntiles) into carries[0..ntiles) on `stream`.
extern "C" hipError_t brotli_amd_launch_tile_carries(const BrotliAmdUndeltaTile* tiles, uint64_t* carries, uint64_t ntiles, hipStream_t stream) {
  hipLaunchKernelGGL(brotli_amd_undelta_carry_kernel, dim3(1), dim3(kCarryThreads), 0, stream, tiles, carries, ntiles);
  return hipGetLastError();
}

// units: the units of all segments together (brotli_amd_seg_units: the host has the table); d_scratch: brotli_amd_undelta_scratch_bytes
// of device memory, 16-byte aligned; ev[0..3], where not NULL, are recorded in front of, between and behind the three launches
extern "C" hipError_t brotli_amd_launch_undelta(const void* d_table, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  if (n == 0u || units == 0u) return hipSuccess;
  const BrotliAmdUnshuffleSeg* d_segs = static_cast<const BrotliAmdUnshuffleSeg*>(d_table);
  const uint64_t ntiles = (units + kTileUnits - 1u) / kTileUnits;
  uint32_t grid = 0;
  hipError_t e = brotli_amd_seg_grid(units, kTileUnits, &grid);
  if (e != hipSuccess) return e;
  BrotliAmdUndeltaTile* tiles = static_cast<BrotliAmdUndeltaTile*>(d_scratch);
  uint64_t* carries = reinterpret_cast<uint64_t*>(tiles + ntiles);
  if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(brotli_amd_undelta_sum_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, units, tiles);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
  if ((e = brotli_amd_launch_tile_carries(tiles, carries, ntiles, stream)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(brotli_amd_undelta_apply_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, carries);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[3], stream)) != hipSuccess) return e;
  return hipSuccess;
}
