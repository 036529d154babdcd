// brotli_unshuffle_kernels.hip -- one launch that turns the byte planes of n independent segments, of any alignment, length and width
// (1, 2, 4, 8), back into elements (gfx950, wave64).  The transform, and what one unit of work reads and writes, is csrc/brotli_unshuffle.h.
//
// Work is split by BYTES, not by segments: the segment walk of csrc/brotli_seg_walk.h over the words of DESTINATION memory, in tiles of
// BROTLI_AMD_UNSHUFFLE_TILE_BYTES.  A tile that lies inside one segment -- every tile of a long one -- is searched for once, and its width is
// then the same for every lane, so the unit's code is chosen once per tile.
//
// A lane produces one word: w runs of 16 / w (+ 1) plane bytes, each loaded as the aligned dwords around it.  Neighbouring lanes read
// neighbouring runs of the same plane, so a wave's load instruction reads one contiguous stretch of 64 x 16 / w bytes of a plane.  Width 8,
// whose runs would be two bytes, takes two neighbouring words a lane in a tile that lies inside one segment.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_seg_walk.h"
#include "brotli_unshuffle.h"

namespace {

constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS;
constexpr uint32_t kUnitsPerThread = 4;
constexpr uint32_t kTileUnits = kThreads * kUnitsPerThread;

static_assert(kTileUnits * 16u == BROTLI_AMD_UNSHUFFLE_TILE_BYTES, "the tile the header names");

// the units [lo, hi) of the tile at t0 that are this thread's, all of one segment of width W whose first unit is `first`.  Width 8: two neighbouring
// units a time (brotli_unshuffle.h: brotli_amd_unshuffle_two_units_w), so that a plane's run is four bytes, not two
template <uint32_t W>
__device__ __forceinline__ void tile_of_one(const BrotliAmdUnshuffleSeg& sg, uint64_t first, uint64_t t0, uint64_t lo, uint64_t hi, uint32_t tid) {
  const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst;
  if constexpr (W == 8u) {
#pragma unroll
    for (uint32_t it = 0; it < kUnitsPerThread / 2u; it++) {
      const uint64_t g = t0 + 2u * (it * kThreads + tid);
      if (g >= lo && g + 1u < hi) brotli_amd_unshuffle_two_units_w<W>(src, dst, sg.len, g - first, hi - first);
      else if (g >= lo && g < hi) brotli_amd_unshuffle_unit_w<W>(src, dst, sg.len, g - first);
      else if (g + 1u >= lo && g + 1u < hi) brotli_amd_unshuffle_unit_w<W>(src, dst, sg.len, g + 1u - first);
    }
  } else {
#pragma unroll
    for (uint32_t it = 0; it < kUnitsPerThread; it++) {
      const uint64_t g = t0 + it * kThreads + tid;
      if (g >= lo && g < hi) brotli_amd_unshuffle_unit_w<W>(src, dst, sg.len, g - first);
    }
  }
}

__global__ __launch_bounds__(kThreads) void brotli_amd_unshuffle_kernel(const BrotliAmdUnshuffleSeg* __restrict__ segs, uint32_t n) {
  brotli_amd_seg_dst_kernel<kUnitsPerThread>(segs, n, [](const BrotliAmdUnshuffleSeg& sg, uint64_t first, uint64_t lo, uint64_t hi, uint64_t t0, uint32_t tid) {
    switch (sg.width) {
      case 1u: tile_of_one<1u>(sg, first, t0, lo, hi, tid); break;
      case 2u: tile_of_one<2u>(sg, first, t0, lo, hi, tid); break;
      case 4u: tile_of_one<4u>(sg, first, t0, lo, hi, tid); break;
      case 8u: tile_of_one<8u>(sg, first, t0, lo, hi, tid); break;
      default: break;   // (the host lets no other width through)
    }
  }, [](const BrotliAmdUnshuffleSeg& sg, uint64_t first, uint64_t, uint64_t g, uint64_t, uint64_t) {
    brotli_amd_unshuffle_unit((uint64_t)(uintptr_t)sg.src, (uint64_t)(uintptr_t)sg.dst, sg.len, sg.width, g - first);
  });
}

}  // namespace

extern "C" uint32_t brotli_amd_unshuffle_tile_bytes(void) { return BROTLI_AMD_UNSHUFFLE_TILE_BYTES; }

extern "C" hipError_t brotli_amd_launch_unshuffle(const void* d_segs, uint32_t n, uint64_t units, void*, hipStream_t stream, const hipEvent_t* ev) {
  return brotli_amd_seg_launch(brotli_amd_unshuffle_kernel, kTileUnits, d_segs, n, units, stream, ev);
}
