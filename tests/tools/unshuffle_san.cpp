// unshuffle_san.cpp -- the unshuffle unit function (csrc/brotli_unshuffle.h) under AddressSanitizer and UBSan, as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I rust-brotli-decompressor_amd/csrc tests/tools/unshuffle_san.cpp
// Every width; every length 0..160 at every pair of skews for lengths up to 48 and at 32 pairs beyond, the lengths 16 w k + d, 1023 .. 1025 and
// the tile's edges at 8 pairs, against a bytewise loop of its own.  Every source and every destination lies in a heap block of EXACTLY the
// sixteen-byte words its span touches: a load or a store one word too far would be reported; the destination's bytes beside the segment must
// keep their pattern.  Exits 0 when everything agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_device_abi.h"
#include "brotli_unshuffle.h"
#include "san_block.h"

static uint32_t g_seed = 2026u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static int one(uint32_t w, size_t len, uint32_t ss, uint32_t ds) {
  SanBlock sb(len, ss), db(len, ds);
  sb.fill_random(rnd);
  db.fill_pattern();
  const uint64_t src = sb.addr(), dst = db.addr();
  const uint64_t units = brotli_amd_seg_units(dst, len);
  if (units != db.span / 16u) { std::fprintf(stderr, "units %llu of a span of %zu\n", (unsigned long long)units, db.span); return 1; }
  // as a lane takes them in a tile inside one segment: two units a step (width 8 has a path of its own for two whole words), pairs that begin at
  // an even or an odd unit; otherwise unit by unit, the last first (the units do not depend on their order)
  if (rnd() & 1u) {
    const uint64_t odd = (ss ^ ds) & 1u;
    for (uint64_t k = odd; k < units; k += 2u) brotli_amd_unshuffle_two_units(src, dst, len, w, k, units);
    if (odd && units) brotli_amd_unshuffle_unit(src, dst, len, w, 0);
  } else {
    for (uint64_t k = units; k-- > 0;) brotli_amd_unshuffle_unit(src, dst, len, w, k);
  }
  const size_t m = len / w;
  const uint8_t* s = sb.at();
  size_t i = 0;
  uint8_t is = 0, must = 0;
  if (!db.holds([&](size_t p) { return p < w * m ? s[(p % w) * m + p / w] : s[p]; }, &i, &is, &must)) {
    std::fprintf(stderr, "width %u length %zu skews %u %u: byte %zu is %02x, not %02x\n", w, len, ss, ds, i, is, must);
    return 1;
  }
  return 0;
}

int main() {
  unsigned long long segments = 0;
  for (uint32_t w : {1u, 2u, 4u, 8u}) {
    for (size_t len = 0; len <= 160; len++) {
      if (len <= 48) {
        for (uint32_t ss = 0; ss < 16u; ss++)
          for (uint32_t ds = 0; ds < 16u; ds++) { if (int e = one(w, len, ss, ds)) return e; segments++; }
      } else {
        for (uint32_t k = 0; k < 16u; k++) {
          if (int e = one(w, len, k, k)) return e;
          if (int e = one(w, len, rnd() & 15u, rnd() & 15u)) return e;
          segments += 2;
        }
      }
    }
    std::vector<size_t> lens = {1023, 1024, 1025, BROTLI_AMD_UNSHUFFLE_TILE_BYTES - 1u, BROTLI_AMD_UNSHUFFLE_TILE_BYTES, BROTLI_AMD_UNSHUFFLE_TILE_BYTES + w + 1u};
    for (size_t k = 1; k <= 5; k++)
      for (int d = -1; d <= (int)w; d++) lens.push_back(16u * w * k + d);
    for (size_t len : lens)
      for (uint32_t k = 0; k < 8u; k++) { if (int e = one(w, len, k < 2u ? 15u * k : rnd() & 15u, k < 2u ? 15u - 15u * k : rnd() & 15u)) return e; segments++; }
    // a width that is none: nothing is read or written
    if (int e = one(1u, 0, 3, 5)) return e;
  }
  uint8_t guard[32];
  for (int i = 0; i < 32; i++) guard[i] = (uint8_t)i;
  brotli_amd_unshuffle_unit((uint64_t)(uintptr_t)guard, (uint64_t)(uintptr_t)guard + 16u, 16, 3u, 0);
  for (int i = 0; i < 32; i++) if (guard[i] != (uint8_t)i) return 1;
  std::printf("%llu segments\n", segments);
  return 0;
}
