// brotli_bitunpack_kernels.hip -- one launch that turns the k-bit fields of n independent segments, of any alignment, count, field width
// (1 .. 64), element width (1, 2, 4, 8), bit order and extension, back into elements (gfx950, wave64).  The transform, the kinds of a word and
// what a unit and an item read and write is csrc/brotli_bitunpack.h.
//
// Work is split by BYTES, not by segments: the segment walk of csrc/brotli_seg_walk.h over the words of DESTINATION memory -- a segment's `len`
// is its destination's m w bytes --, in tiles of BROTLI_AMD_BITUNPACK_TILE_BYTES.  A tile that lies inside one segment -- every tile of a long
// one -- is searched for once, and its w and k are then the same for every lane, so the item's code is chosen once per tile, by a switch over
// the 120 pairs; its lanes take SLOTS of 2 w words, neighbouring lanes neighbouring slots.  Where the segment's destination is 16-byte aligned
// a slot is one fast item: k + 1 dword loads, each of which reads, over the wave, 64 dwords 4 k bytes apart.  The words that are no item's --
// all of them where the destination is not aligned, the last m % 32 elements' elsewhere -- are taken in front of the switch, a word a lane, so that
// the slow unit exists once in the kernel and not once per pair.  A tile of several segments takes its words one by one, after a search each,
// all of them the slow way: every lane there has a k of its own.
#include <hip/hip_runtime.h>

#include "brotli_bitunpack.h"
#include "brotli_device_abi.h"
#include "brotli_seg_walk.h"

namespace {

constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS;
constexpr uint32_t kUnitsPerThread = 16;
constexpr uint32_t kTileUnits = kThreads * kUnitsPerThread;

static_assert(kTileUnits * 16u == BROTLI_AMD_BITUNPACK_TILE_BYTES, "the tile the header names");
static_assert(kUnitsPerThread % 16u == 0u, "a whole number of slots a thread at every width");

// the fast items of the units [ka, kb) of one segment: the segment's slots that hold them, in turns
struct TileItems {
  uint64_t src, dst, m; uint32_t flags; uint64_t ka, kb; uint32_t tid;
  template <uint32_t W, uint32_t K> __device__ __forceinline__ void operator()() const {
    for (uint64_t s = ka / (2u * W) + tid; 2u * W * s < kb; s += kThreads) (void)brotli_amd_bitunpack_slot_items_wk<W, K>(src, dst, m, flags, s, ka, kb);
  }
};

// (both callables always_inline, as the shell's part is: the 120 items make them too large for the inliner's liking, and a call would need a stack)
__global__ __launch_bounds__(kThreads) void brotli_amd_bitunpack_kernel(const BrotliAmdUnshuffleSeg* __restrict__ segs, uint32_t n) {
  brotli_amd_seg_dst_kernel<kUnitsPerThread>(segs, n, [](const BrotliAmdUnshuffleSeg& sg, uint64_t first, uint64_t lo, uint64_t hi, uint64_t, uint32_t tid)
                                                          __attribute__((always_inline)) {
    const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst;
    const uint32_t w = sg.width, k = sg.param & 0xFFu, flags = sg.param >> 8;
    if (!brotli_amd_bitunpack_shape_ok(k, w, flags)) return;   // (the host lets no other shape through)
    const uint32_t LOG = brotli_amd_bitunpack_log(w);
    const uint64_t m = sg.len >> LOG, ka = lo - first, kb = hi - first;
    // the words that are no item's first: all of them where the destination is not aligned, those behind the whole groups of 32 elsewhere
    const bool items = (dst & 15u) == 0u;
    const uint64_t tail = ((m & ~(uint64_t)(BROTLI_AMD_BITUNPACK_ITEM_ELEMS - 1u)) << LOG) >> 4;
    for (uint64_t u = (items && tail > ka ? tail : ka) + tid; u < kb; u += kThreads) brotli_amd_bitunpack_slow_words(src, dst, m, w, k, flags, u, u + 1u);
    if (items) brotli_amd_bitunpack_for_wk(w, k, TileItems{src, dst, m, flags, ka, kb < tail ? kb : tail, tid});
  }, [](const BrotliAmdUnshuffleSeg& sg, uint64_t first, uint64_t end, uint64_t g, uint64_t lo, uint64_t hi) __attribute__((always_inline)) {
    const uint32_t w = sg.width;
    brotli_amd_bitunpack_word_alone((uint64_t)(uintptr_t)sg.src, (uint64_t)(uintptr_t)sg.dst, sg.len >> brotli_amd_bitunpack_log(w), w, sg.param & 0xFFu,
                                    sg.param >> 8, g - first, (lo > first ? lo : first) - first, (hi < end ? hi : end) - first);
  });
}

}  // namespace

extern "C" uint32_t brotli_amd_bitunpack_tile_bytes(void) { return BROTLI_AMD_BITUNPACK_TILE_BYTES; }

extern "C" hipError_t brotli_amd_launch_bitunpack(const void* d_segs, uint32_t n, uint64_t units, void*, hipStream_t stream, const hipEvent_t* ev) {
  return brotli_amd_seg_launch(brotli_amd_bitunpack_kernel, kTileUnits, d_segs, n, units, stream, ev);
}
