// bitunshuffle_san.cpp -- the bit-unshuffle functions (csrc/brotli_bitunshuffle.h) under AddressSanitizer and UBSan, as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I rust-brotli-decompressor_amd/csrc tests/tools/bitunshuffle_san.cpp
// Every width and the block sizes 0, 8, 24, 32, 40, 2048 and one larger than the segment; every length 0..160 at every pair of skews for lengths up
// to 40 and at 8 pairs beyond, the lengths 8 w q + d, 1023 .. 1025 and the tile's edges at 6 pairs, against a loop of its own that goes byte by
// byte and bit by bit.  The work is taken as the kernel's lanes take it in a tile inside one segment: tile after tile, slot after slot
// (brotli_amd_bitunshuffle_range), or -- every other time -- word by word from the last to the first, as a tile of several segments has them.
// Every source and every destination lies in a heap block of EXACTLY the sixteen-byte words its span touches: a load or a store one word too far
// would be reported; the destination's bytes beside the segment must keep their pattern.  Exits 0 when everything agreed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_bitunshuffle.h"
#include "brotli_device_abi.h"
#include "san_block.h"

static uint32_t g_seed = 2027u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
static unsigned long long g_items = 0;
static const uint32_t kBlocks[6] = {0u, 8u, 24u, 32u, 40u, 2048u};

// the definition: byte p of the destination from the source's bytes
static uint8_t want_byte(const uint8_t* s, size_t len, uint32_t w, uint32_t B, size_t p) {
  const size_t m = len / w;
  if (p >= m / 8u * 8u * w) return s[p];
  const size_t e = p / w, j = p % w;
  const size_t b0 = (B == 0u || B >= m) ? 0u : e / B * B;
  const size_t c = (B == 0u || B >= m) ? m / 8u * 8u : (m - b0 >= B ? B : (m - b0) / 8u * 8u);
  const size_t i = e - b0;
  if (i >= c) return s[p];
  uint8_t v = 0;
  for (uint32_t k = 0; k < 8u; k++) v |= (uint8_t)(((s[b0 * w + (8u * j + k) * (c / 8u) + i / 8u] >> (i % 8u)) & 1u) << k);
  return v;
}

static int one(uint32_t w, uint32_t B, size_t len, uint32_t ss, uint32_t ds) {
  SanBlock sb(len, ss), db(len, ds);
  sb.fill_random(rnd);
  db.fill_pattern();
  const uint64_t src = sb.addr(), dst = db.addr();
  const uint64_t units = brotli_amd_seg_units(dst, len);
  if (units != db.span / 16u) { std::fprintf(stderr, "units %llu of a span of %zu\n", (unsigned long long)units, db.span); return 1; }
  if (rnd() & 1u) {
    const uint64_t tile = BROTLI_AMD_BITUNSHUFFLE_TILE_BYTES / 16u, slot = 2u * w;
    for (uint64_t t0 = 0; t0 < units; t0 += tile) {
      const uint64_t t1 = std::min(t0 + tile, units);
      for (uint64_t s = t0 / slot; slot * s < t1; s++)
        g_items += brotli_amd_bitunshuffle_range(src, dst, len, w, B, std::max(slot * s, t0), std::min(slot * (s + 1u), t1));
    }
  } else {
    for (uint64_t k = units; k-- > 0;) g_items += brotli_amd_bitunshuffle_range(src, dst, len, w, B, k, k + 1u);
  }
  size_t i = 0;
  uint8_t is = 0, must = 0;
  if (!db.holds([&](size_t p) { return want_byte(sb.at(), len, w, B, p); }, &i, &is, &must)) {
    std::fprintf(stderr, "width %u block %u length %zu skews %u %u: byte %zu is %02x, not %02x\n", w, B, len, ss, ds, i, is, must);
    return 1;
  }
  return 0;
}

int main() {
  unsigned long long segments = 0;
  const size_t tile = BROTLI_AMD_BITUNSHUFFLE_TILE_BYTES;
  for (uint32_t w : {1u, 2u, 4u, 8u}) {
    for (uint32_t Bsel = 0; Bsel < 7u; Bsel++) {
      for (size_t len = 0; len <= 160; len++) {
        const uint32_t B = Bsel < 6u ? kBlocks[Bsel] : (uint32_t)(len / w / 8u * 8u + 16u);
        if (len <= 40) {
          for (uint32_t ss = 0; ss < 16u; ss++)
            for (uint32_t ds = 0; ds < 16u; ds++) { if (int e = one(w, B, len, ss, ds)) return e; segments++; }
        } else {
          for (uint32_t k = 0; k < 4u; k++) {
            if (int e = one(w, B, len, 4u * k + (k & 1u), 4u * k + (k & 1u))) return e;
            if (int e = one(w, B, len, rnd() & 15u, k == 0u ? 0u : rnd() & 15u)) return e;
            segments += 2;
          }
        }
      }
      std::vector<size_t> lens = {1023, 1024, 1025, tile - 1u, tile, tile + 1u, 2u * tile + 8u * w + 1u};
      for (size_t q : {1u, 3u, 4u, 5u, 8u, 33u})
        for (size_t d : {(size_t)0, (size_t)1, (size_t)w, (size_t)(8u * w - 1u)}) lens.push_back(8u * w * q + d);
      for (size_t len : lens) {
        const uint32_t B = Bsel < 6u ? kBlocks[Bsel] : (uint32_t)(len / w / 8u * 8u + 16u);
        for (uint32_t k = 0; k < 6u; k++) {
          // (destination skews 0 and 8 among them: the fast items)
          if (int e = one(w, B, len, k < 2u ? 15u * k : rnd() & 15u, k < 2u ? 15u - 15u * k : k == 2u ? 0u : k == 3u ? 8u : rnd() & 15u)) return e;
          segments++;
        }
      }
    }
  }
  if (g_items == 0) { std::fprintf(stderr, "no fast item was taken\n"); return 1; }
  // a width that is none: nothing is read or written
  uint8_t guard[32];
  for (int i = 0; i < 32; i++) guard[i] = (uint8_t)i;
  (void)brotli_amd_bitunshuffle_range((uint64_t)(uintptr_t)guard, (uint64_t)(uintptr_t)guard + 16u, 16, 3u, 0u, 0, 1);
  brotli_amd_bitunshuffle_unit((uint64_t)(uintptr_t)guard, (uint64_t)(uintptr_t)guard + 16u, 16, 3u, 0u, 0);
  for (int i = 0; i < 32; i++) if (guard[i] != (uint8_t)i) return 1;
  std::printf("%llu segments, %llu fast items\n", segments, g_items);
  return 0;
}
