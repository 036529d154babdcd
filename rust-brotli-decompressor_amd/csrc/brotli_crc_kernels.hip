// brotli_crc_kernels.hip -- one launch that gives the CRC-32 or CRC-32C of n independent byte segments of any alignment and any length
// (gfx950, wave64).  The arithmetic, and why a segment may be digested in pieces, is csrc/brotli_crc.h.
//
// Work is split by BYTES, not by segments, the way csrc/brotli_copy_kernels.hip splits a copy (read the two side by side: the chunk loop and
// the tile walk are that file's).  A segment's UNITS are the 16-byte-aligned words of SOURCE memory it touches; the units of all segments, one
// after the other, are cut into tiles of kTileUnits (BROTLI_AMD_CRC_TILE_BYTES of source), and the blocks take the tiles in turns.  A lane
// finds the segment of a unit by a binary search in the prefix sum of the segments' unit counts, which every block builds in LDS for kChunkSegs
// segments at a time; a tile that lies inside one segment is searched for once.
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

#include <algorithm>

#include "brotli_crc.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kRunUnits = BROTLI_AMD_CRC_RUN_UNITS;   // consecutive units a lane: 128 bytes, one cache line's worth
constexpr uint32_t kTileUnits = kThreads * kRunUnits;
constexpr uint32_t kChunkSegs = kThreads * 4;   // segments whose prefix sum lies in LDS at a time: four a thread
constexpr uint64_t kRunBytes = 16u * kRunUnits, kWaveBytes = 64u * kRunBytes;
#if defined(__HIP_DEVICE_COMPILE__)
#define BROTLI_AMD_GLOBAL __attribute__((address_space(1)))
#else
#define BROTLI_AMD_GLOBAL
#endif
typedef uint32_t v4u __attribute__((ext_vector_type(4)));   // sixteen bytes a lane

static_assert(kTileUnits * 16u == BROTLI_AMD_CRC_TILE_BYTES, "the tile the header names");

// [kind - 1]: built by the compiler (brotli_crc.h)
__device__ const BrotliAmdCrcConsts kConsts[2] = {brotli_amd_crc_make_consts(BROTLI_AMD_CRC32_POLY), brotli_amd_crc_make_consts(BROTLI_AMD_CRC32C_POLY)};

struct LoadGlobal {
  __device__ __forceinline__ void operator()(uint64_t W, uint32_t* w) const {
    const v4u v = *(const BROTLI_AMD_GLOBAL v4u*)W;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  }
};

// the segment of unit g: pre[j] <= g < pre[j + 1] (pre[0] <= g < pre[kChunkSegs]; a segment without units is never the answer)
__device__ __forceinline__ uint32_t find_seg(const uint64_t* pre, uint64_t g) {
  uint32_t a = 0, b = kChunkSegs;
  while (b - a > 1u) { const uint32_t m = (a + b) >> 1; if (pre[m] <= g) a = m; else b = m; }
  return a;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off);
  return v;
}

// What a wave keeps between tiles: the sums of its whole runs in tiles inside one segment, one a lane, each waiting for its long multiplication.
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

// This block's tiles among the units [base, end) of one chunk of segments (pre[]: the units in front of each, segs / out: the chunk's first):
// every thread of the block makes the same walk and digests its own run.  -> the block's next tile (one that goes on behind `end` stays the block's).
__device__ __forceinline__ uint64_t take_tiles(const uint64_t* pre, const BrotliAmdCrcSeg* segs, uint32_t* out, uint64_t base, uint64_t end, uint64_t tile,
                                               uint32_t grid, uint32_t tid, uint32_t poly, const uint32_t* tab, const uint32_t* pw, uint32_t lane_pow,
                                               Waiting& wt) {
  const uint32_t lane = tid & 63u;
  const LoadGlobal load;
  while (tile * kTileUnits < end) {
    const uint64_t t0 = tile * kTileUnits, t1 = t0 + kTileUnits;
    const uint64_t lo = t0 > base ? t0 : base, hi = t1 < end ? t1 : end;   // the tile's units among this chunk's segments
    if (lo < hi) {   // (not: a tile that began in the chunk before, and this chunk has no units)
      const uint32_t ja = find_seg(pre, lo), jb = find_seg(pre, hi - 1u);
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
          v4u v[kRunUnits];
#pragma unroll
          for (uint32_t k = 0; k < kRunUnits; k++) {
            v[k] = v4u{0u, 0u, 0u, 0u};
            if (g0 + k >= lo) v[k] = *(const BROTLI_AMD_GLOBAL v4u*)(W0 + 16u * k);
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
            if (lane == wt.count) { wt.sum = sum; wt.seg = ja; wt.behind = src + sg.len - wave_stop; }
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
          uint32_t j = ja == jb ? ja : find_seg(pre, g);
          while (g < gend) {
            while (pre[j + 1u] <= g) j++;   // (segments without units lie between)
            if (have) atomicXor(out + term_seg, term);
            const BrotliAmdCrcSeg sg = segs[j];
            const uint64_t first = pre[j], u1 = (gend < pre[j + 1u] ? gend : pre[j + 1u]) - first;
            uint64_t behind = 0;
            const uint32_t reg = brotli_amd_crc_piece(tab, load, (uint64_t)(uintptr_t)sg.ptr, sg.len, g - first, u1, &behind);
            term = brotli_amd_crc_piece_term(poly, pw, reg, behind); term_seg = j; have = true;
            g = first + u1;
          }
        }
        add_terms(out, have, term_seg, term, lane);
      }
    }
    if (t1 > end) break;   // (the tile goes on in the next chunk's segments)
    tile += grid;
  }
  return tile;
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
  Waiting wt;
  uint64_t base = 0;              // units of the segments in front of the chunk
  uint64_t tile = blockIdx.x;     // this block's next tile
  for (uint32_t c0 = 0; c0 < n; c0 += kChunkSegs) {
    const uint32_t cnt = n - c0 < kChunkSegs ? n - c0 : kChunkSegs;
    uint64_t u[4], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t j = 4u * tid + k;
      u[k] = j < cnt ? brotli_amd_crc_seg_units((uint64_t)(uintptr_t)segs[c0 + j].ptr, segs[c0 + j].len) : 0u;
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
    tile = take_tiles(pre, segs + c0, out + c0, base, end, tile, gridDim.x, tid, poly, tab, pw, lane_pow, wt);
    // (the waiting sums name their segments by the chunk's numbering)
    settle(wt, tid & 63u, poly, pw, out + c0);
    base = end;
  }
}

}  // namespace

extern "C" uint32_t brotli_amd_crc_tile_bytes(void) { return BROTLI_AMD_CRC_TILE_BYTES; }

// units: the units of all segments together (brotli_amd_crc_seg_units: the host has the table); d_out: n words, zeroed on `stream` in front of the launch
extern "C" hipError_t brotli_amd_launch_crc(const BrotliAmdCrcSeg* d_segs, uint32_t n, uint32_t kind, uint64_t units, uint32_t* d_out, hipStream_t stream) {
  if (n == 0u || units == 0u) return hipSuccess;   // (segments without bytes: the zeroed words are their digests)
  if (brotli_amd_crc_poly(kind) == 0u) return hipErrorInvalidValue;
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  // four blocks of four waves a CU, and no more blocks than there are tiles
  const uint64_t grid = std::min<uint64_t>((uint64_t)(cus > 0 ? cus : 1) * 4u, (units + kTileUnits - 1u) / kTileUnits);
  hipLaunchKernelGGL(brotli_amd_crc_kernel, dim3((uint32_t)grid), dim3(kThreads), 0, stream, d_segs, n, kind, d_out);
  return hipGetLastError();
}
