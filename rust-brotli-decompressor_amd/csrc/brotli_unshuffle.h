// brotli_unshuffle.h -- byte planes back into elements: the arithmetic of one unit of work, once, for the host and the device.
//
// THE TRANSFORM.  A segment of len bytes and a width w (1, 2, 4 or 8): m = len / w elements, r = len % w bytes left over.  The source holds
// plane 0 -- byte 0 of every element --, then plane 1, ..., plane w - 1, then the r left-over bytes.  For p < w m:
//     dst[p] = src[(p % w) m + p / w]
// and for w m <= p < len: dst[p] = src[p] (Blosc's rule; Parquet's BYTE_STREAM_SPLIT never has r != 0).  Width 1 is a copy.  Out of place: no
// destination range overlaps a source range or another destination range.
//
// A UNIT (csrc/brotli_seg_walk.h) is one aligned 16-byte word of DESTINATION memory that [dst, dst + len) touches; unit k is the word at (dst & ~15) + 16 k.  The word
// starts at position p0 = W - dst of the segment (negative in a first unit that starts inside its word).  Its bytes belong to the elements
// e0 = floor(p0 / w) .. e0 + 16 / w (the last one only where p0 is no multiple of w), so the unit needs of every plane j one RUN of 16 / w
// (+ 1) bytes at src + j m + e0.  A run is fetched as the ALIGNED DWORDS around it, shifted together in registers; the w runs are interleaved by
// byte permutes into the 16 + w bytes of the elements e0 .., and the word is bytes [p0 mod w, p0 mod w + 16) of those.
//
// LOADS.  Of a run only the bytes of elements inside [0, m) are wanted.  Where a run and the dwords around it lie wholly inside their plane -- all
// but the first and last units of a long segment -- they are loaded without conditions; elsewhere a dword is loaded only where it holds a wanted
// byte: a byte of [src, src + w m).  So no load leaves the 16-byte-aligned span around [src, src + len) (it may touch any byte inside it: a
// plane's start j m takes every residue).  The r left-over bytes are loaded as single bytes where a unit holds one.
// STORES.  One aligned 16-byte store where the segment covers the word; at the segment's first and last word aligned dwords and single bytes
// of [dst, dst + len) only -- never a read-modify-write: what lies next to them is not this segment's.  A unit may hold the last element
// bytes AND the first left-over bytes, and may be the first and the last unit of a short segment at once.
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUnshuffleHost; tests/tools/unshuffle_san.cpp) and the device
// (csrc/brotli_unshuffle_kernels.hip).  Addresses are integers.
#ifndef BROTLI_AMD_UNSHUFFLE_H_
#define BROTLI_AMD_UNSHUFFLE_H_

#include <stdint.h>
#include <string.h>

#include "brotli_seg_walk.h"   // a segment's units, the search for a unit's segment, the edge store, BrotliAmdU4, BROTLI_AMD_GLOBAL

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BROTLI_AMD_UNSHUFFLE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BROTLI_AMD_UNSHUFFLE_HD inline
#endif

// ---- memory: aligned dwords, aligned 16-byte words, single bytes (the edge store: csrc/brotli_seg_walk.h) ----
BROTLI_AMD_UNSHUFFLE_HD uint32_t brotli_amd_unshuffle_ld32(uint64_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const BROTLI_AMD_GLOBAL uint32_t*)a;
#else
  uint32_t v; memcpy(&v, reinterpret_cast<const void*>((uintptr_t)a), 4); return v;
#endif
}
BROTLI_AMD_UNSHUFFLE_HD uint32_t brotli_amd_unshuffle_ld8(uint64_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const BROTLI_AMD_GLOBAL uint8_t*)a;
#else
  return *reinterpret_cast<const uint8_t*>((uintptr_t)a);
#endif
}
BROTLI_AMD_UNSHUFFLE_HD BrotliAmdU4 brotli_amd_unshuffle_ld128(uint64_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  const BrotliAmdV4 v = *(const BROTLI_AMD_GLOBAL BrotliAmdV4*)a;
  return BrotliAmdU4{v.x, v.y, v.z, v.w};
#else
  BrotliAmdU4 v; memcpy(&v, reinterpret_cast<const void*>((uintptr_t)a), 16); return v;
#endif
}
BROTLI_AMD_UNSHUFFLE_HD void brotli_amd_unshuffle_st128(uint64_t a, BrotliAmdU4 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *(BROTLI_AMD_GLOBAL BrotliAmdV4*)a = BrotliAmdV4{v.x, v.y, v.z, v.w};
#else
  memcpy(reinterpret_cast<void*>((uintptr_t)a), &v, 16);
#endif
}

// ---- registers ----
// v_perm_b32: byte i of the result is byte sel[i] of the eight bytes hi : lo (0..3: lo, 4..7: hi); a selector of 0x0C gives 0
BROTLI_AMD_UNSHUFFLE_HD uint32_t brotli_amd_unshuffle_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t both = ((uint64_t)hi << 32) | lo;
  uint32_t v = 0;
  for (uint32_t i = 0; i < 4u; i++) {
    const uint32_t c = (sel >> (8u * i)) & 0xFFu;
    if (c < 8u) v |= (uint32_t)((both >> (8u * c)) & 0xFFu) << (8u * i);
  }
  return v;
#endif
}
// the dword that starts sh bits (0, 8, 16, 24) into lo, of hi : lo (v_alignbyte_b32)
BROTLI_AMD_UNSHUFFLE_HD uint32_t brotli_amd_unshuffle_funnel(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, sh >> 3);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
#endif
}

// a0 b0 a1 b1 / a2 b2 a3 b3 of the bytes a0..a3 and b0..b3
#define BROTLI_AMD_UNSHUFFLE_ZIP_LO 0x05010400u
#define BROTLI_AMD_UNSHUFFLE_ZIP_HI 0x07030602u
// a0 a1 b0 b1 / a2 a3 b2 b3
#define BROTLI_AMD_UNSHUFFLE_PAIR_LO 0x05040100u
#define BROTLI_AMD_UNSHUFFLE_PAIR_HI 0x07060302u

// four dwords as a 4 x 4 matrix of bytes, transposed: t[i] = byte i of r0, r1, r2, r3
BROTLI_AMD_UNSHUFFLE_HD void brotli_amd_unshuffle_transpose4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t* t) {
  const uint32_t a = brotli_amd_unshuffle_perm(r1, r0, BROTLI_AMD_UNSHUFFLE_ZIP_LO), a2 = brotli_amd_unshuffle_perm(r1, r0, BROTLI_AMD_UNSHUFFLE_ZIP_HI);
  const uint32_t b = brotli_amd_unshuffle_perm(r3, r2, BROTLI_AMD_UNSHUFFLE_ZIP_LO), b2 = brotli_amd_unshuffle_perm(r3, r2, BROTLI_AMD_UNSHUFFLE_ZIP_HI);
  t[0] = brotli_amd_unshuffle_perm(b, a, BROTLI_AMD_UNSHUFFLE_PAIR_LO); t[1] = brotli_amd_unshuffle_perm(b, a, BROTLI_AMD_UNSHUFFLE_PAIR_HI);
  t[2] = brotli_amd_unshuffle_perm(b2, a2, BROTLI_AMD_UNSHUFFLE_PAIR_LO); t[3] = brotli_amd_unshuffle_perm(b2, a2, BROTLI_AMD_UNSHUFFLE_PAIR_HI);
}

// bytes [s, s + 16) of the 24 bytes in i[0..6) (s in 0..7)
BROTLI_AMD_UNSHUFFLE_HD BrotliAmdU4 brotli_amd_unshuffle_shift_bytes(const uint32_t* i, uint32_t s) {
  const uint32_t sh = (s & 3u) * 8u;
  BrotliAmdU4 v;
  if (s < 4u) {
    v.x = brotli_amd_unshuffle_funnel(i[1], i[0], sh); v.y = brotli_amd_unshuffle_funnel(i[2], i[1], sh);
    v.z = brotli_amd_unshuffle_funnel(i[3], i[2], sh); v.w = brotli_amd_unshuffle_funnel(i[4], i[3], sh);
  } else {
    v.x = brotli_amd_unshuffle_funnel(i[2], i[1], sh); v.y = brotli_amd_unshuffle_funnel(i[3], i[2], sh);
    v.z = brotli_amd_unshuffle_funnel(i[4], i[3], sh); v.w = brotli_amd_unshuffle_funnel(i[5], i[4], sh);
  }
  return v;
}

// ---- the work ----
BROTLI_AMD_UNSHUFFLE_HD constexpr bool brotli_amd_unshuffle_width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }

// The run of plane bytes at address A (any alignment) of which the bytes in [need_lo, need_hi) are wanted: ND aligned dwords around it,
// each loaded only where it holds a wanted byte, shifted together -- r[i] = bytes [4 i, 4 i + 4) of the run (what was not loaded reads as 0).
template <uint32_t ND>
BROTLI_AMD_UNSHUFFLE_HD void brotli_amd_unshuffle_run(uint64_t A, uint64_t need_lo, uint64_t need_hi, uint32_t* r) {
  const uint64_t D = A & ~(uint64_t)3;
  const uint32_t sh = ((uint32_t)A & 3u) * 8u;
  uint32_t d[ND + 1u];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < ND; i++) {
    d[i] = 0u;
    if (D + 4u * i < need_hi && D + 4u * i + 4u > need_lo) d[i] = brotli_amd_unshuffle_ld32(D + 4u * i);
  }
  d[ND] = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < ND; i++) r[i] = brotli_amd_unshuffle_funnel(d[i + 1u], d[i], sh);
}

// ... where every byte of the run and of the ND dwords around it is known to lie inside the segment: no conditions
template <uint32_t ND>
BROTLI_AMD_UNSHUFFLE_HD void brotli_amd_unshuffle_run_inside(uint64_t A, uint32_t* r) {
  const uint64_t D = A & ~(uint64_t)3;
  const uint32_t sh = ((uint32_t)A & 3u) * 8u;
  uint32_t d[ND + 1u];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < ND; i++) d[i] = brotli_amd_unshuffle_ld32(D + 4u * i);
  d[ND] = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < ND; i++) r[i] = brotli_amd_unshuffle_funnel(d[i + 1u], d[i], sh);
}

// width 1: the source of a word is shifted against it by (src - dst) mod 16 -- the one or two ALIGNED 16-byte words of source that hold the
// wanted bytes, shifted together
BROTLI_AMD_UNSHUFFLE_HD BrotliAmdU4 brotli_amd_unshuffle_copy_word(uint64_t S, uint64_t need_lo, uint64_t need_hi) {
  const uint32_t s = (uint32_t)S & 15u;
  const uint64_t SA = S - s;
  BrotliAmdU4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
  if (need_lo < SA + 16u) a = brotli_amd_unshuffle_ld128(SA);
  if (s != 0u && SA + 16u < need_hi) b = brotli_amd_unshuffle_ld128(SA + 16u);
  uint32_t t0, t1, t2, t3, t4;
  switch (s >> 2) {
    case 0: t0 = a.x; t1 = a.y; t2 = a.z; t3 = a.w; t4 = b.x; break;
    case 1: t0 = a.y; t1 = a.z; t2 = a.w; t3 = b.x; t4 = b.y; break;
    case 2: t0 = a.z; t1 = a.w; t2 = b.x; t3 = b.y; t4 = b.z; break;
    default: t0 = a.w; t1 = b.x; t2 = b.y; t3 = b.z; t4 = b.w; break;
  }
  const uint32_t sh = (s & 3u) * 8u;
  BrotliAmdU4 v;
  v.x = brotli_amd_unshuffle_funnel(t1, t0, sh); v.y = brotli_amd_unshuffle_funnel(t2, t1, sh);
  v.z = brotli_amd_unshuffle_funnel(t3, t2, sh); v.w = brotli_amd_unshuffle_funnel(t4, t3, sh);
  return v;
}

// Unit k of a segment of width W (1, 2, 4, 8): reads and writes as the head of this file says.
template <uint32_t W>
BROTLI_AMD_UNSHUFFLE_HD void brotli_amd_unshuffle_unit_w(uint64_t src, uint64_t dst, uint64_t len, uint64_t k) {
  constexpr uint32_t LOG = W == 1u ? 0u : W == 2u ? 1u : W == 4u ? 2u : 3u;
  constexpr uint32_t PER = 16u / W;                 // whole elements in a word
  constexpr uint32_t ND = (PER + 1u + 6u) / 4u;     // dwords around a run of PER + 1 bytes at any alignment
  const uint64_t Wd = (dst & ~(uint64_t)15) + 16u * k;
  const uint64_t lo = Wd > dst ? Wd : dst, hi = Wd + 16u < dst + len ? Wd + 16u : dst + len;   // the word's bytes that are the segment's
  BrotliAmdU4 v;
  if constexpr (W == 1u) {
    const uint64_t S = src + (Wd - dst);   // (wraps to below src in a first unit that starts inside its word: only used through need_lo / need_hi)
    v = brotli_amd_unshuffle_copy_word(S, S + (lo - Wd), S + (hi - Wd));
  } else {
    const uint64_t m = len >> LOG, body = m << LOG;
    const int64_t p0 = (int64_t)(Wd - dst);          // the segment's position of the word's byte 0: -15 ..
    const int64_t e0 = p0 >> LOG;                    // (floor: arithmetic shift)
    const uint32_t s = (uint32_t)p0 & (W - 1u);      // p0 == e0 W + s
    // the elements wanted: e0 .. e0 + PER (the last only where s != 0), inside [0, m)
    const int64_t ea = e0 > 0 ? e0 : 0;
    int64_t eb = e0 + (int64_t)PER + (s != 0u ? 1 : 0);
    if (eb > (int64_t)m) eb = (int64_t)m;
    uint32_t I[6] = {0u, 0u, 0u, 0u, 0u, 0u};        // the elements e0 .. interleaved: byte i W + j = byte i of plane j's run
    if (ea < eb) {
      uint32_t r[W][ND];
      // INSIDE: every plane's run lies in front of the plane's last 4 ND bytes, so the ND dwords around it hold bytes of [src, src + w m) only
      // (the dword in front holds the run's first byte) -- the rule for all but the first and last units of a long segment
      if (e0 >= 0 && (uint64_t)e0 + 4u * ND <= m) {
        uint64_t A = src + (uint64_t)e0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < W; j++, A += m) brotli_amd_unshuffle_run_inside<ND>(A, r[j]);
      } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < W; j++) {
          const uint64_t P = src + (uint64_t)j * m;
          brotli_amd_unshuffle_run<ND>(P + (uint64_t)e0, P + (uint64_t)ea, P + (uint64_t)eb, r[j]);
        }
      }
      if constexpr (W == 2u) {
        I[0] = brotli_amd_unshuffle_perm(r[1][0], r[0][0], BROTLI_AMD_UNSHUFFLE_ZIP_LO); I[1] = brotli_amd_unshuffle_perm(r[1][0], r[0][0], BROTLI_AMD_UNSHUFFLE_ZIP_HI);
        I[2] = brotli_amd_unshuffle_perm(r[1][1], r[0][1], BROTLI_AMD_UNSHUFFLE_ZIP_LO); I[3] = brotli_amd_unshuffle_perm(r[1][1], r[0][1], BROTLI_AMD_UNSHUFFLE_ZIP_HI);
        I[4] = brotli_amd_unshuffle_perm(r[1][2], r[0][2], BROTLI_AMD_UNSHUFFLE_ZIP_LO);
      } else if constexpr (W == 4u) {
        brotli_amd_unshuffle_transpose4(r[0][0], r[1][0], r[2][0], r[3][0], I);
        I[4] = brotli_amd_unshuffle_perm(r[1][1], r[0][1], 0x0C0C0400u) | brotli_amd_unshuffle_perm(r[3][1], r[2][1], 0x04000C0Cu);
      } else {
        uint32_t t[4], u[4];
        brotli_amd_unshuffle_transpose4(r[0][0], r[1][0], r[2][0], r[3][0], t);
        brotli_amd_unshuffle_transpose4(r[4][0], r[5][0], r[6][0], r[7][0], u);
        I[0] = t[0]; I[1] = u[0]; I[2] = t[1]; I[3] = u[1]; I[4] = t[2]; I[5] = u[2];
      }
    }
    v = brotli_amd_unshuffle_shift_bytes(I, s);
    // the left-over bytes behind the last element stay where they are
    if (hi > dst + body) {
      uint32_t w4[4] = {v.x, v.y, v.z, v.w};
      const uint64_t from = dst + body > lo ? dst + body : lo;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t q = 0; q < 16u; q++) {
        const uint64_t a = Wd + q;
        if (a >= from && a < hi) w4[q >> 2] = (w4[q >> 2] & ~(0xFFu << (8u * (q & 3u)))) | (brotli_amd_unshuffle_ld8(src + (a - dst)) << (8u * (q & 3u)));
      }
      v.x = w4[0]; v.y = w4[1]; v.z = w4[2]; v.w = w4[3];
    }
  }
  if (lo == Wd && hi == Wd + 16u) brotli_amd_unshuffle_st128(Wd, v);
  else brotli_amd_seg_store_edge(Wd, lo, hi, v);
}

// Units k and k + 1 of a segment of `units` units (k + 1 only where it is one): what one lane takes in a tile that lies inside one segment.
// Width 8 has runs of two or three bytes a unit, so there a lane that finds both words INSIDE (as above) fetches runs of four or five bytes
// once -- still two dwords a plane -- and produces 32 bytes from them; everything else is the two units one after the other.
template <uint32_t W>
BROTLI_AMD_UNSHUFFLE_HD void brotli_amd_unshuffle_two_units_w(uint64_t src, uint64_t dst, uint64_t len, uint64_t k, uint64_t units) {
  if constexpr (W == 8u) {
    const uint64_t Wd = (dst & ~(uint64_t)15) + 16u * k;
    const uint64_t m = len >> 3;
    const uint64_t e0 = (Wd - dst) >> 3;   // (only used where Wd >= dst)
    if (k + 1u < units && Wd >= dst && e0 + 8u <= m) {
      const uint32_t s = (uint32_t)(Wd - dst) & 7u;
      uint32_t r[8][2];
      uint64_t A = src + e0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t j = 0; j < 8u; j++, A += m) brotli_amd_unshuffle_run_inside<2u>(A, r[j]);
      uint32_t t[4], u[4], I[10];
      brotli_amd_unshuffle_transpose4(r[0][0], r[1][0], r[2][0], r[3][0], t);
      brotli_amd_unshuffle_transpose4(r[4][0], r[5][0], r[6][0], r[7][0], u);
      I[0] = t[0]; I[1] = u[0]; I[2] = t[1]; I[3] = u[1]; I[4] = t[2]; I[5] = u[2]; I[6] = t[3]; I[7] = u[3];
      I[8] = brotli_amd_unshuffle_perm(r[1][1], r[0][1], 0x0C0C0400u) | brotli_amd_unshuffle_perm(r[3][1], r[2][1], 0x04000C0Cu);
      I[9] = brotli_amd_unshuffle_perm(r[5][1], r[4][1], 0x0C0C0400u) | brotli_amd_unshuffle_perm(r[7][1], r[6][1], 0x04000C0Cu);
      brotli_amd_unshuffle_st128(Wd, brotli_amd_unshuffle_shift_bytes(I, s));
      brotli_amd_unshuffle_st128(Wd + 16u, brotli_amd_unshuffle_shift_bytes(I + 4, s));
      return;
    }
  }
  brotli_amd_unshuffle_unit_w<W>(src, dst, len, k);
  if (k + 1u < units) brotli_amd_unshuffle_unit_w<W>(src, dst, len, k + 1u);
}

BROTLI_AMD_UNSHUFFLE_HD void brotli_amd_unshuffle_two_units(uint64_t src, uint64_t dst, uint64_t len, uint32_t width, uint64_t k, uint64_t units) {
  switch (width) {
    case 1u: brotli_amd_unshuffle_two_units_w<1u>(src, dst, len, k, units); break;
    case 2u: brotli_amd_unshuffle_two_units_w<2u>(src, dst, len, k, units); break;
    case 4u: brotli_amd_unshuffle_two_units_w<4u>(src, dst, len, k, units); break;
    case 8u: brotli_amd_unshuffle_two_units_w<8u>(src, dst, len, k, units); break;
    default: break;
  }
}

// ... of any allowed width (another width: nothing is read or written)
BROTLI_AMD_UNSHUFFLE_HD void brotli_amd_unshuffle_unit(uint64_t src, uint64_t dst, uint64_t len, uint32_t width, uint64_t k) {
  switch (width) {
    case 1u: brotli_amd_unshuffle_unit_w<1u>(src, dst, len, k); break;
    case 2u: brotli_amd_unshuffle_unit_w<2u>(src, dst, len, k); break;
    case 4u: brotli_amd_unshuffle_unit_w<4u>(src, dst, len, k); break;
    case 8u: brotli_amd_unshuffle_unit_w<8u>(src, dst, len, k); break;
    default: break;
  }
}

#endif  // BROTLI_AMD_UNSHUFFLE_H_
