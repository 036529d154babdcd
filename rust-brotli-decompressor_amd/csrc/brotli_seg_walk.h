// brotli_seg_walk.h -- the segment walk: how a launch over a table of n independent segments of any alignment and length shares its work among
// its blocks, once, for the four kernels that take such a table (the ragged copy, the digests, unshuffle, undelta) and for the host.
//
// Work is split by BYTES, not by segments.  A segment's UNITS are the 16-byte-aligned words of memory it touches -- of destination memory for
// the copy, unshuffle and undelta, of source memory for the digests.  The units of all segments, one after the other, are cut into TILES of
// tile_units, and the blocks take the tiles in turns: tile t is block t % grid's.  One long segment among a thousand short ones is spread over
// every block, and a thousand short ones are a dozen tiles.
//
// The launch gets the segment table alone, so no block knows beforehand where its tiles lie: every block builds the prefix sum of the
// segments' unit counts in LDS, for a CHUNK of kChunkSegs segments at a time, and a lane finds the segment of a unit by a binary search in it.
// pre[j] is the number of units in front of segment j of the chunk (the chunks in front included), pre[kChunkSegs] the chunk's end.
//
// A PART is what one chunk's segments hold of one tile: the units [lo, hi) of the tile at t0.  A tile may begin in one chunk and go on in the
// next; it stays its block's, which then comes by it once per chunk, a part each time.  A chunk may have no units at all; it has no parts.
// The parts of all blocks are disjoint and cover every unit (tests/test_seg_walk_cpu.py, through BrotliAmdDebugSegWalkParts).
#ifndef BROTLI_AMD_SEG_WALK_H_
#define BROTLI_AMD_SEG_WALK_H_

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BROTLI_AMD_SEG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BROTLI_AMD_SEG_HD inline
#endif
// (global-memory instructions, not flat ones: the addresses are computed as integers, so the address space is said where they are used)
#if defined(__HIP_DEVICE_COMPILE__)
#define BROTLI_AMD_GLOBAL __attribute__((address_space(1)))
#else
#define BROTLI_AMD_GLOBAL
#endif

#define BROTLI_AMD_SEG_THREADS 256u      // threads of a block of a walking kernel
#define BROTLI_AMD_SEG_CHUNK_SEGS 1024u  // segments whose prefix sum lies in LDS at a time: four a thread

// the units of the len bytes at addr
BROTLI_AMD_SEG_HD uint64_t brotli_amd_seg_units(uint64_t addr, uint64_t len) { return len ? ((addr + len + 15u) >> 4) - (addr >> 4) : 0u; }

// the segment of unit g in the prefix sum pre[0..count] of unit counts: pre[j] <= g < pre[j + 1] (pre[0] <= g < pre[count]; a segment without
// units is never the answer)
BROTLI_AMD_SEG_HD uint32_t brotli_amd_seg_find(const uint64_t* pre, uint32_t count, uint64_t g) {
  uint32_t a = 0, b = count;
  while (b - a > 1u) { const uint32_t m = (a + b) >> 1; if (pre[m] <= g) a = m; else b = m; }
  return a;
}

// sixteen bytes a lane: as plain words for the host and the device, and as the vector of one 16-byte load or store of the device's compiler
struct BrotliAmdU4 { uint32_t x, y, z, w; };
#if defined(__HIPCC__)
typedef uint32_t BrotliAmdV4 __attribute__((ext_vector_type(4)));
#endif

// A segment's first and last unit are EDGES.  Bytes [lo, hi) of the word at W (lo, hi inside [W, W + 16], not the whole word): aligned dwords
// where the segment has all four bytes, single bytes elsewhere -- never a read-modify-write: what lies next to them is not this segment's.
// (V4: BrotliAmdU4 or BrotliAmdV4)
template <class V4>
BROTLI_AMD_SEG_HD void brotli_amd_seg_store_edge(uint64_t W, uint64_t lo, uint64_t hi, V4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < 4u; i++) {
    const uint64_t A = W + 4u * i;
    if (A >= lo && A + 4u <= hi) {
#if defined(__HIP_DEVICE_COMPILE__)
      *(BROTLI_AMD_GLOBAL uint32_t*)A = w[i];
#else
      memcpy(reinterpret_cast<void*>((uintptr_t)A), &w[i], 4);
#endif
      continue;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 4u; j++)
      if (A + j >= lo && A + j < hi) *(BROTLI_AMD_GLOBAL uint8_t*)(uintptr_t)(A + j) = (uint8_t)(w[i] >> (8u * j));
  }
}

// One block's tiles among the units [base, end) of one chunk of segments: part(lo, hi, t0, tile) for what the chunk holds of each.  `tile` is
// the block's next tile, grid() the number of blocks -- a callable, so that the device reads gridDim.x where the loop uses it, as undelta's
// kernels did before the walk was shared: handed over as a value, the same loop costs undelta's sum kernel one percent (profiles/seg_walk.txt).
// -> the block's next tile behind the chunk (one that goes on behind `end` stays the block's).
template <class Grid, class Part>
BROTLI_AMD_SEG_HD uint64_t brotli_amd_seg_chunk_tiles(uint32_t tile_units, uint64_t base, uint64_t end, uint64_t tile, Grid grid, Part part) {
  while (tile * tile_units < end) {
    const uint64_t t0 = tile * tile_units, t1 = t0 + tile_units;
    const uint64_t lo = t0 > base ? t0 : base, hi = t1 < end ? t1 : end;   // the tile's units among this chunk's segments
    if (lo < hi) part(lo, hi, t0, tile);   // (not: a tile that began in the chunk before, and this chunk has no units)
    if (t1 > end) break;   // (the tile goes on in the next chunk's segments)
    tile += grid();
  }
  return tile;
}

// The walk of every block of a grid on the host, over the segments' unit counts alone, chunk after chunk as the device goes:
// part(block, tile, lo, hi) for every part (BrotliAmdDebugSegWalkParts, tests/tools/seg_walk_san.cpp).  It shares brotli_amd_seg_chunk_tiles
// with the device walk, not the chunk loop: the device's prefix sum in LDS and its chunk bookkeeping are the GPU tests' to check.
template <class Part>
inline void brotli_amd_seg_walk_model(const uint64_t* units, uint32_t n, uint32_t tile_units, uint32_t grid, Part part) {
  for (uint32_t block = 0; block < grid; block++) {
    uint64_t base = 0, tile = block;
    for (uint32_t c0 = 0; c0 < n;) {
      uint64_t end = base;
      for (const uint32_t c1 = n - c0 < BROTLI_AMD_SEG_CHUNK_SEGS ? n : c0 + BROTLI_AMD_SEG_CHUNK_SEGS; c0 < c1; c0++) end += units[c0];
      tile = brotli_amd_seg_chunk_tiles(tile_units, base, end, tile, [grid] { return grid; }, [&](uint64_t lo, uint64_t hi, uint64_t, uint64_t t) { part(block, t, lo, hi); });
      base = end;
    }
  }
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

// The walk of one block of BROTLI_AMD_SEG_THREADS threads over segs[0..n): part(pre, the chunk's segments, c0, lo, hi, t0, tile) for every part
// [lo, hi) of every tile of this block, c0 being the chunk's first segment.  addr(segment) is the address whose words are the segment's units.
// pre[BROTLI_AMD_SEG_CHUNK_SEGS + 1] and scan[BROTLI_AMD_SEG_THREADS] are the kernel's LDS.  Every thread makes the same walk; a part may
// synchronise the block.
template <uint32_t kTileUnits, class Seg, class Addr, class Part>
__device__ __forceinline__ void brotli_amd_seg_walk(const Seg* __restrict__ segs, uint32_t n, uint64_t* pre, uint64_t* scan, Addr addr, Part part) {
  constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS, kChunkSegs = BROTLI_AMD_SEG_CHUNK_SEGS;
  const uint32_t tid = threadIdx.x;
  uint64_t base = 0;              // units of the segments in front of the chunk
  uint64_t tile = blockIdx.x;     // this block's next tile
  for (uint32_t c0 = 0; c0 < n; c0 += kChunkSegs) {
    const uint32_t cnt = n - c0 < kChunkSegs ? n - c0 : kChunkSegs;
    uint64_t u[4], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t j = 4u * tid + k;
      u[k] = j < cnt ? brotli_amd_seg_units((uint64_t)(uintptr_t)addr(segs[c0 + j]), segs[c0 + j].len) : 0u;
      sum += u[k];
    }
    __syncthreads();   // (the chunk before is done with pre[])
    scan[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < kThreads; off <<= 1) {
      const uint64_t v = tid >= off ? scan[tid - off] : 0u;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    uint64_t at = base + scan[tid] - sum;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) { pre[4u * tid + k] = at; at += u[k]; }
    const uint64_t end = base + scan[kThreads - 1u];
    if (tid == 0u) pre[kChunkSegs] = end;
    __syncthreads();
    const Seg* chunk = segs + c0;
    tile = brotli_amd_seg_chunk_tiles(kTileUnits, base, end, tile, [] { return (uint32_t)gridDim.x; },
                                      [&](uint64_t lo, uint64_t hi, uint64_t t0, uint64_t t) { part(pre, chunk, c0, lo, hi, t0, t); });
    base = end;
  }
}

// The grid of a walking kernel over `units` units (0: unknown, a full grid): four blocks of four waves a CU, and no more blocks than there are tiles.
inline hipError_t brotli_amd_seg_grid(uint64_t units, uint32_t tile_units, uint32_t* grid) {
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  uint64_t g = (uint64_t)(cus > 0 ? cus : 1) * 4u;
  const uint64_t tiles = (units + tile_units - 1u) / tile_units;
  if (units != 0u && tiles < g) g = tiles;
  *grid = (uint32_t)g;
  return hipSuccess;
}

// ---- the shell of a kernel of ONE launch whose units are the words of DESTINATION memory (unshuffle, bit-unshuffle, bit-unpack) ----
// The body of such a kernel of BROTLI_AMD_SEG_THREADS threads with tiles of kUnitsPerThread units a thread: the LDS of the walk, the walk over the
// segments' dst, and each part split.  A part that lies inside one segment -- every tile of a long one -- is searched for once:
// one_segment(sg, first, lo, hi, t0, tid), `first` being the segment's first unit.  Elsewhere a lane takes a word after a search each:
// word_alone(sg, first, end, g, lo, hi) for unit g of the segment whose units are [first, end).  The part is always_inline, and so should a
// callable be that is too large for the inliner's liking (bit-unpack's): a call would put a stack into scratch memory.
template <uint32_t kUnitsPerThread, class Seg, class One, class Alone>
__device__ __forceinline__ void brotli_amd_seg_dst_kernel(const Seg* __restrict__ segs, uint32_t n, One one_segment, Alone word_alone) {
  constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS, kChunkSegs = BROTLI_AMD_SEG_CHUNK_SEGS;
  __shared__ uint64_t pre[kChunkSegs + 1];   // units in front of each segment of the chunk (in front of the chunk included); [kChunkSegs]: behind its last
  __shared__ uint64_t scan[kThreads];
  const uint32_t tid = threadIdx.x;
  brotli_amd_seg_walk<kThreads * kUnitsPerThread>(segs, n, pre, scan, [](const Seg& sg) { return sg.dst; },
                                                  [&](const uint64_t* pre, const Seg* segs, uint32_t, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t)
                                                      __attribute__((always_inline)) {
    const uint32_t ja = brotli_amd_seg_find(pre, kChunkSegs, lo), jb = brotli_amd_seg_find(pre, kChunkSegs, hi - 1u);
    if (ja == jb) {   // one segment's: the rule for a long one
      const Seg sg = segs[ja];
      one_segment(sg, pre[ja], lo, hi, t0, tid);
    } else {
      for (uint32_t it = 0; it < kUnitsPerThread; it++) {
        const uint64_t g = t0 + it * kThreads + tid;
        if (g >= lo && g < hi) {
          const uint32_t j = brotli_amd_seg_find(pre, kChunkSegs, g);
          const Seg sg = segs[j];
          word_alone(sg, pre[j], pre[j + 1u], g, lo, hi);
        }
      }
    }
  });
}

// ... and its launch over `units` units (the units of all segments together: the host has the table -- a launch of a few short segments has a
// few blocks, not a device full of blocks that find nothing to do).  The signature is every filter's launcher's: no scratch is used here, and
// ev[0..1], where not NULL, are recorded in front of and behind the launch.
template <class Seg>
inline hipError_t brotli_amd_seg_launch(void (*kernel)(const Seg*, uint32_t), uint32_t tile_units, const void* d_segs, uint32_t n, uint64_t units,
                                        hipStream_t stream, const hipEvent_t* ev) {
  if (n == 0u || units == 0u) return hipSuccess;
  uint32_t grid = 0;
  hipError_t e = brotli_amd_seg_grid(units, tile_units, &grid);
  if (e != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(BROTLI_AMD_SEG_THREADS), 0, stream, static_cast<const Seg*>(d_segs), n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return ev ? hipEventRecord(ev[1], stream) : hipSuccess;
}
#endif  // __HIPCC__

#endif  // BROTLI_AMD_SEG_WALK_H_
