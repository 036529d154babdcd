// brotli_crc_kernels.hip -- one launch that gives the CRC-32 or CRC-32C of n independent byte segments of any alignment and any length
// (gfx950, wave64).  The arithmetic, and why a segment may be digested in pieces, is csrc/brotli_crc.h.
//
// Work is split by BYTES, not by segments: the segment walk of csrc/brotli_seg_walk.h over the words of SOURCE memory, in tiles of
// BROTLI_AMD_CRC_TILE_BYTES.  A tile that lies inside one segment is searched for once.
//
// A lane takes a RUN of kRunUnits consecutive units -- 128 bytes -- through the byte tables, which the block keeps in LDS.  What belongs to one
// segment in a run is a PIECE (brotli_crc.h).  Every unit is ONE aligned 16-byte load of a word that holds a byte of the segment, so no load
// leaves the 16-byte-aligned span around [ptr, ptr + len).
//
// EDGES.  Of a segment's first and last word only the bytes inside [ptr, ptr + len) go through the tables, one by one -- neither the bytes in
// front (no masking: they are not looked at) nor the bytes behind.  The init value 0xFFFFFFFF is put in ONCE per segment, as the start register
// of the piece that holds its first byte; the final XOR is put in once, by the piece that holds its last byte.  (Not: the combine rule over
// whole standard CRCs.)
//
// A piece's register is multiplied by x^(8 x the segment's bytes behind the piece) and XORed into the segment's word, which the host zeroed:
//   - in a tile that lies inside one segment and ends in front of that segment's last word -- every tile of a long segment but its last --
//     the runs are whole and follow each other: a lane multiplies by x^(8 x 128 x the lanes behind it in its wave), a constant it computed
//     once, the wave XORs across its lanes (__shfl_xor), and the wave's sum waits in a register of one of its lanes, with the bytes behind
//     it; when every lane holds one (and at the end) each lane does the long multiplication for its own.  So the multiplication by an
//     arbitrary power, 32 steps for every set bit of the count, is paid once per 8 KiB, not once per 128 bytes;
//   - everywhere else -- short segments, a long one's last tile -- a lane does the multiplication for each of its pieces.
// Either way, where the terms of a wave's lanes are all one segment's they are XORed across the lanes first and go in by ONE atomicXor: a long
// segment gets one atomic per 512 KiB (measured on one segment of 1 GiB: 1.75 ms with an atomic per waiting sum).
// Plain atomicXor on global memory: XOR commutes, so the words do not depend on which block took which tile, or when.
#include <hip/hip_runtime.h>

#include "brotli_crc.h"
#include "brotli_seg_walk.h"

namespace {

constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS, kChunkSegs = BROTLI_AMD_SEG_CHUNK_SEGS;
constexpr uint32_t kRunUnits = BROTLI_AMD_CRC_RUN_UNITS;   // consecutive units a lane: 128 bytes, one cache line's worth
constexpr uint32_t kTileUnits = kThreads * kRunUnits;
constexpr uint64_t kRunBytes = 16u * kRunUnits, kWaveBytes = 64u * kRunBytes;

static_assert(kTileUnits * 16u == BROTLI_AMD_CRC_TILE_BYTES, "the tile the header names");

// [kind - 1]: built by the compiler (brotli_crc.h)
__device__ const BrotliAmdCrcConsts kConsts[2] = {brotli_amd_crc_make_consts(BROTLI_AMD_CRC32_POLY), brotli_amd_crc_make_consts(BROTLI_AMD_CRC32C_POLY)};

struct LoadGlobal {
  __device__ __forceinline__ void operator()(uint64_t W, uint32_t* w) const {
    const BrotliAmdV4 v = *(const BROTLI_AMD_GLOBAL BrotliAmdV4*)W;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  }
};

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off);
  return v;
}

// What a wave keeps between tiles: the sums of its whole runs in tiles inside one segment, one a lane, each waiting for its long multiplication.
// (seg: the segment's number in the whole table, so a sum may wait across chunks of segments)
struct Waiting {
  uint32_t count = 0;   // (the same in every lane)
  uint32_t sum = 0, seg = 0;
  uint64_t behind = 0;
};

// The terms of a wave's lanes (have: this lane has one, for segment seg) into the segments' words: where they are all one segment's -- the rule: a
// long one's -- XORed across the lanes first and one atomic, so that a segment of a gigabyte does not queue a hundred thousand atomics on one word.
// (Every lane of the wave calls this.)
__device__ __forceinline__ void add_terms(uint32_t* out, bool have, uint32_t seg, uint32_t term, uint32_t lane) {
  const unsigned long long with = __ballot(have);
  if (with == 0ull) return;
  const uint32_t ref = __shfl(seg, __ffsll(with) - 1);
  if (__ballot(have && seg != ref) == 0ull) {
    const uint32_t sum = wave_xor(have ? term : 0u);
    if (lane == 0u) atomicXor(out + ref, sum);
  } else if (have) atomicXor(out + seg, term);
}

__device__ __forceinline__ void settle(Waiting& wt, uint32_t lane, uint32_t poly, const uint32_t* pw, uint32_t* out) {
  const bool have = lane < wt.count;
  add_terms(out, have, wt.seg, have ? brotli_amd_crc_shift(poly, pw, wt.sum, wt.behind) : 0u, lane);
  wt.count = 0;
}

__global__ __launch_bounds__(kThreads) void brotli_amd_crc_kernel(const BrotliAmdCrcSeg* __restrict__ segs, uint32_t n, uint32_t kind, uint32_t* __restrict__ out) {
  __shared__ uint32_t tab[1024];             // the byte tables of the launch's polynomial
  __shared__ uint32_t pw[64];
  __shared__ uint64_t pre[kChunkSegs + 1];   // units in front of each segment of the chunk (in front of the chunk included); [kChunkSegs]: behind its last
  __shared__ uint64_t scan[kThreads];
  const uint32_t tid = threadIdx.x;
  const uint32_t poly = brotli_amd_crc_poly(kind);
  const BrotliAmdCrcConsts& c = kConsts[kind - 1u];
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) tab[k * 256u + tid] = c.t[k][tid];
  if (tid < 64u) pw[tid] = c.pw[tid];
  __syncthreads();
  // x^(8 x the bytes of the lanes behind this one in its wave)
  const uint32_t lane_pow = brotli_amd_crc_shift(poly, pw, 0x80000000u, (uint64_t)(63u - (tid & 63u)) * kRunBytes);
  const uint32_t lane = tid & 63u;
  const LoadGlobal load;
  Waiting wt;
  // every thread digests its own run of every part
  brotli_amd_seg_walk<kTileUnits>(segs, n, pre, scan, [](const BrotliAmdCrcSeg& sg) { return sg.ptr; },
                                  [&](const uint64_t* pre, const BrotliAmdCrcSeg* segs, uint32_t c0, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t) {
    const uint64_t t1 = t0 + kTileUnits;
    const uint32_t ja = brotli_amd_seg_find(pre, kChunkSegs, lo), jb = brotli_amd_seg_find(pre, kChunkSegs, hi - 1u);
    const uint64_t g0 = t0 + (uint64_t)tid * kRunUnits;   // this lane's run
    bool whole = false;
    if (ja == jb && hi == t1) {   // one segment's, up to the tile's end: do its bytes go on behind the tile?
      const BrotliAmdCrcSeg sg = segs[ja];
      const uint64_t src = (uint64_t)(uintptr_t)sg.ptr, first = pre[ja];
      const uint64_t stop = (src & ~(uint64_t)15) + 16u * (t1 - first);   // the address behind the tile's last word
      if (stop < src + sg.len) {   // (the last byte, with the final XOR, is never in such a tile)
        whole = true;
        // the rule for a long segment: whole runs, one behind the other (a lane in front of the segment's first unit has nothing)
        const uint64_t W0 = (src & ~(uint64_t)15) + 16u * (g0 - first);   // (only used where g0 + k >= lo)
        BrotliAmdV4 v[kRunUnits];
#pragma unroll
        for (uint32_t k = 0; k < kRunUnits; k++) {
          v[k] = BrotliAmdV4{0u, 0u, 0u, 0u};
          if (g0 + k >= lo) v[k] = *(const BROTLI_AMD_GLOBAL BrotliAmdV4*)(W0 + 16u * k);
        }
        uint32_t reg = 0u;
#pragma unroll
        for (uint32_t k = 0; k < kRunUnits; k++) {
          if (g0 + k < lo) continue;
          uint32_t from = 0u;
          if (g0 + k == first) { reg = 0xFFFFFFFFu; from = (uint32_t)(src & 15u); }   // the segment's first byte: the init value, once
          reg = brotli_amd_crc_unit(tab, reg, v[k].x, v[k].y, v[k].z, v[k].w, from, 16u);
        }
        const uint32_t sum = wave_xor(brotli_amd_crc_mul(poly, reg, lane_pow));
        const uint64_t wave_stop = stop - (uint64_t)(3u - (tid >> 6)) * kWaveBytes;
        if (wave_stop > src) {   // (else the whole wave lies in front of the segment)
          if (lane == wt.count) { wt.sum = sum; wt.seg = c0 + ja; wt.behind = src + sg.len - wave_stop; }
          if (++wt.count == 64u) settle(wt, lane, poly, pw, out);
        }
      }
    }
    if (!whole) {
      // pieces: what of this lane's run belongs to one segment, segment by segment; the last one waits for the wave
      uint64_t g = g0 > lo ? g0 : lo;
      const uint64_t gend = g0 + kRunUnits < hi ? g0 + kRunUnits : hi;
      bool have = false;
      uint32_t term = 0u, term_seg = 0u;
      if (g < gend) {
        uint32_t j = ja == jb ? ja : brotli_amd_seg_find(pre, kChunkSegs, g);
        while (g < gend) {
          while (pre[j + 1u] <= g) j++;   // (segments without units lie between)
          if (have) atomicXor(out + term_seg, term);
          const BrotliAmdCrcSeg sg = segs[j];
          const uint64_t first = pre[j], u1 = (gend < pre[j + 1u] ? gend : pre[j + 1u]) - first;
          uint64_t behind = 0;
          const uint32_t reg = brotli_amd_crc_piece(tab, load, (uint64_t)(uintptr_t)sg.ptr, sg.len, g - first, u1, &behind);
          term = brotli_amd_crc_piece_term(poly, pw, reg, behind); term_seg = c0 + j; have = true;
          g = first + u1;
        }
      }
      add_terms(out, have, term_seg, term, lane);
    }
  });
  settle(wt, lane, poly, pw, out);
}

}  // namespace

extern "C" uint32_t brotli_amd_crc_tile_bytes(void) { return BROTLI_AMD_CRC_TILE_BYTES; }

// units: the units of all segments together (brotli_amd_seg_units: the host has the table); d_out: n words, zeroed on `stream` in front of the launch
extern "C" hipError_t brotli_amd_launch_crc(const BrotliAmdCrcSeg* d_segs, uint32_t n, uint32_t kind, uint64_t units, uint32_t* d_out, hipStream_t stream) {
  if (n == 0u || units == 0u) return hipSuccess;   // (segments without bytes: the zeroed words are their digests)
  if (brotli_amd_crc_poly(kind) == 0u) return hipErrorInvalidValue;
  uint32_t grid = 0;
  const hipError_t e = brotli_amd_seg_grid(units, kTileUnits, &grid);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(brotli_amd_crc_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, kind, d_out);
  return hipGetLastError();
}
