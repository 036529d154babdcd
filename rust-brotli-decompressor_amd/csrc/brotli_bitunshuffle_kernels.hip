// brotli_bitunshuffle_kernels.hip -- one launch that turns the bit planes of n independent segments, of any alignment, length, width (1, 2, 4, 8)
// and block size, back into elements (gfx950, wave64).  The transform, the kinds of a word and what a unit and an item read and write is
// csrc/brotli_bitunshuffle.h.
//
// Work is split by BYTES, not by segments: the segment walk of csrc/brotli_seg_walk.h over the words of DESTINATION memory, in tiles of
// BROTLI_AMD_BITUNSHUFFLE_TILE_BYTES.  A tile that lies inside one segment -- every tile of a long one -- is searched for once, and its width is
// then the same for every lane, so the code is chosen once per tile; its lanes take SLOTS of 2 w words, neighbouring lanes neighbouring slots.
// Where the segment's blocks are aligned a slot is one fast item: eight loads a byte column, each of which reads, over the wave, 256 contiguous
// bytes of one bit row.  A fast item is 2 w words, so the tile is four times the unshuffle's: at width 8 it still has a slot for every thread.
// A tile of several segments takes its words one by one, after a search each.
#include <hip/hip_runtime.h>

#include "brotli_bitunshuffle.h"
#include "brotli_device_abi.h"
#include "brotli_seg_walk.h"

namespace {

constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS;
constexpr uint32_t kUnitsPerThread = 16;
constexpr uint32_t kTileUnits = kThreads * kUnitsPerThread;

static_assert(kTileUnits * 16u == BROTLI_AMD_BITUNSHUFFLE_TILE_BYTES, "the tile the header names");
static_assert(kUnitsPerThread % 16u == 0u, "a whole number of slots a thread at every width");

// the units [lo, hi) of a tile, all of one segment of width W whose first unit is `first`: the segment's slots that hold them, in turns
template <uint32_t W>
__device__ __forceinline__ void tile_of_one(const BrotliAmdUnshuffleSeg& sg, uint64_t first, uint64_t lo, uint64_t hi, uint32_t tid) {
  const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst;
  const uint64_t ka = lo - first, kb = hi - first;
  for (uint64_t s = ka / (2u * W) + tid; 2u * W * s < kb; s += kThreads) (void)brotli_amd_bitunshuffle_slot_w<W>(src, dst, sg.len, sg.param, s, ka, kb);
}

__global__ __launch_bounds__(kThreads) void brotli_amd_bitunshuffle_kernel(const BrotliAmdUnshuffleSeg* __restrict__ segs, uint32_t n) {
  brotli_amd_seg_dst_kernel<kUnitsPerThread>(segs, n, [](const BrotliAmdUnshuffleSeg& sg, uint64_t first, uint64_t lo, uint64_t hi, uint64_t, uint32_t tid) {
    switch (sg.width) {
      case 1u: tile_of_one<1u>(sg, first, lo, hi, tid); break;
      case 2u: tile_of_one<2u>(sg, first, lo, hi, tid); break;
      case 4u: tile_of_one<4u>(sg, first, lo, hi, tid); break;
      case 8u: tile_of_one<8u>(sg, first, lo, hi, tid); break;
      default: break;   // (the host lets no other width through)
    }
  }, [](const BrotliAmdUnshuffleSeg& sg, uint64_t first, uint64_t, uint64_t g, uint64_t, uint64_t) {
    const uint64_t k = g - first;
    (void)brotli_amd_bitunshuffle_range((uint64_t)(uintptr_t)sg.src, (uint64_t)(uintptr_t)sg.dst, sg.len, sg.width, sg.param, k, k + 1u);
  });
}

}  // namespace

extern "C" uint32_t brotli_amd_bitunshuffle_tile_bytes(void) { return BROTLI_AMD_BITUNSHUFFLE_TILE_BYTES; }

extern "C" hipError_t brotli_amd_launch_bitunshuffle(const void* d_segs, uint32_t n, uint64_t units, void*, hipStream_t stream, const hipEvent_t* ev) {
  return brotli_amd_seg_launch(brotli_amd_bitunshuffle_kernel, kTileUnits, d_segs, n, units, stream, ev);
}
