// brotli_wave_stage.h -- what one wave of a walk over a segment's bytes has for itself (device only; gfx950, wave64): its view of the source
// through LDS, the way a value that is the same in every lane stays in scalar registers, and sixteen bytes of neighbouring elements put together.
// Shared by the kernels whose segments are WALKED, header after header, by one taker: csrc/brotli_unrle_kernels.hip and
// csrc/brotli_undbp_kernels.hip.
#ifndef BROTLI_AMD_WAVE_STAGE_H_
#define BROTLI_AMD_WAVE_STAGE_H_

#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"   // BROTLI_AMD_UNRLE_WALK_CHUNK
#include "brotli_seg_walk.h"     // brotli_amd_seg_units
#include "brotli_unshuffle.h"    // the memory and register helpers

namespace brotli_amd_wave {

constexpr uint32_t kStageChunk = BROTLI_AMD_UNRLE_WALK_CHUNK;
static_assert(kStageChunk == 64u * 16u, "one 16-byte load a lane");

// LDS operations of one wave execute in order; this only stops the compiler from moving accesses across it
__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// What is the same in every lane but comes out of a lane's registers or out of LDS goes through v_readfirstlane, so that the compiler keeps it,
// and everything computed from it -- a walk's offsets and counts, its branches, the addresses of the table's entries --, in scalar registers.
__device__ __forceinline__ uint32_t same(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// A wave's view of a segment's bytes through LDS: chunk c is the kStageChunk bytes from (src & ~15) + kStageChunk c on, of which the wave loads
// the words that the segment touches (the others read as 0).  Chunks cur and cur + 1 are resident, at (c & 1) kStageChunk; chunk cur + 2 is in
// flight.  What a walk reads at a time -- a run's header and repeated value, a varint's first or last bytes, eight width bytes -- is 9 bytes at
// the most, so with the first byte in chunk cur all of them are resident: ensure(off) takes the three aligned dwords around them out of LDS at
// once -- one round trip a read, not one a byte -- and window() hands them over.  ensure() only ever goes forward or jumps.
struct Stage {
  uint8_t* lds;      // this wave's 2 kStageChunk bytes
  uint64_t base;     // src & ~15
  uint64_t words;    // the segment's units
  uint32_t skew;     // src & 15
  uint32_t lane;
  uint64_t cur;
  BrotliAmdU4 ahead;
  uint64_t lo;       // the bytes at the offsets off .. off + 7 of the last ensure(off),
  uint32_t hi;       // and at off + 8 (.. off + 11 where off lies at a dword's first byte)

  __device__ __forceinline__ Stage(uint8_t* lds_, uint64_t src, uint64_t len, uint32_t lane_)
      : lds(lds_), base(src & ~(uint64_t)15), words(brotli_amd_seg_units(src, len)), skew((uint32_t)src & 15u), lane(lane_), cur((uint64_t)1 << 62),
        ahead{0u, 0u, 0u, 0u}, lo(0u), hi(0u) {}
  __device__ __forceinline__ BrotliAmdU4 load(uint64_t chunk) const {
    const uint64_t w = chunk * 64u + lane;
    return w < words ? brotli_amd_unshuffle_ld128(base + 16u * w) : BrotliAmdU4{0u, 0u, 0u, 0u};
  }
  __device__ __forceinline__ void put(uint64_t chunk, BrotliAmdU4 v) {
    *reinterpret_cast<BrotliAmdV4*>(lds + ((uint32_t)chunk & 1u) * kStageChunk + 16u * lane) = BrotliAmdV4{v.x, v.y, v.z, v.w};
  }
  __device__ __forceinline__ uint32_t dword(uint32_t p) const { return *reinterpret_cast<const uint32_t*>(lds + (p & (2u * kStageChunk - 1u))); }   // (p: a multiple of 4)
  __device__ __forceinline__ void ensure(uint64_t off) {
    const uint64_t c = (skew + off) / kStageChunk;
    if (c != cur) {
      lds_sync();   // (the reads of what is replaced are done)
      if (c == cur + 1u) {
        put(c + 1u, ahead);
      } else {   // the stage jumps
        put(c, load(c));
        put(c + 1u, load(c + 1u));
      }
      cur = c;
      ahead = load(c + 2u);
      lds_sync();
    }
    const uint32_t p = (uint32_t)off + skew, a = p & ~3u, sh = (p & 3u) * 8u;
    const uint32_t w0 = same(dword(a)), w1 = same(dword(a + 4u)), w2 = same(dword(a + 8u));
    lo = brotli_amd_unshuffle_funnel(w1, w0, sh) | (uint64_t)brotli_amd_unshuffle_funnel(w2, w1, sh) << 32;
    hi = w2 >> sh;
  }
  // the bytes from `off` on, which ensure() was called for
  __device__ __forceinline__ uint64_t window(uint64_t, uint64_t, uint32_t* b8) const { *b8 = hi & 0xFFu; return lo; }
};

// sixteen bytes of neighbouring elements, put together
struct Word16 {
  uint64_t lo = 0, hi = 0;
  __device__ __forceinline__ void put(uint32_t pos, uint32_t width, uint64_t v) {   // the low `width` bytes of v at byte pos (a multiple of width)
    if (width < 8u) v &= ((uint64_t)1 << (8u * width)) - 1u;
    if (pos < 8u) lo |= v << (8u * pos); else hi |= v << (8u * (pos - 8u));
  }
  __device__ __forceinline__ BrotliAmdU4 word() const { return BrotliAmdU4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)}; }
};

// the blocks of a launch of one wave a piece of work, `waves` of them a block: no more than there is work, eight a CU at the most
inline hipError_t wave_grid(uint64_t pieces, uint32_t waves, uint32_t* grid) {
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  const uint64_t full = (uint64_t)(cus > 0 ? cus : 1) * 8u, need = (pieces + waves - 1u) / waves;
  *grid = (uint32_t)(need < full ? need : full);
  return hipSuccess;
}

}  // namespace brotli_amd_wave

#endif  // BROTLI_AMD_WAVE_STAGE_H_
