// bitunpack_san.cpp -- the bit-unpack functions (csrc/brotli_bitunpack.h) under AddressSanitizer and UBSan, as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I rust-brotli-decompressor_amd/csrc tests/tools/bitunpack_san.cpp
// Every valid (width, bits) pair under both bit orders and both extensions: every count 0..40 at seeded pairs of skews (all 16 x 16 pairs at a
// handful of field widths), the counts round multiples of 32 and the tile's edges, against a loop of its own that goes bit by bit.  The work is
// taken as the kernel's lanes take it in a tile inside one segment: tile after tile, slot after slot (brotli_amd_bitunpack_slot), or -- every
// other time -- word by word from the last to the first, as a tile of several segments has them (brotli_amd_bitunpack_word_alone).
// Every source lies in a heap block of EXACTLY the sixteen-byte words that its ceil(m k / 8) bytes touch, every destination in one of exactly
// its bytes' words: a load or a store one word too far would be reported; the destination's bytes beside the segment must keep their pattern.
// Exits 0 when everything agreed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_bitunpack.h"
#include "brotli_device_abi.h"
#include "san_block.h"

static uint32_t g_seed = 2028u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
static unsigned long long g_items = 0;

// the definition: byte p of the destination from the source's bits
static uint8_t want_byte(const uint8_t* s, uint32_t k, uint32_t w, uint32_t flags, size_t p) {
  const size_t i = p / w, j = p % w;
  uint8_t v = 0;
  for (uint32_t t = 0; t < 8u; t++) {
    uint32_t vb = 8u * (uint32_t)j + t;                       // the value's bit
    if (vb >= k) { if (!(flags & 2u)) continue; vb = k - 1u; }   // (the extension: the sign's bit again, or nothing)
    const size_t b = i * k + ((flags & 1u) ? k - 1u - vb : vb);   // the stream's bit
    const uint32_t bit = (flags & 1u) ? (s[b / 8u] >> (7u - b % 8u)) & 1u : (s[b / 8u] >> (b % 8u)) & 1u;
    v |= (uint8_t)(bit << t);
  }
  return v;
}

static int one(uint32_t w, uint32_t k, uint32_t flags, size_t m, uint32_t ss, uint32_t ds) {
  const size_t slen = (m * k + 7u) / 8u, len = m * w;
  SanBlock sb(slen, ss), db(len, ds);
  sb.fill_random(rnd);
  db.fill_pattern();
  const uint64_t src = sb.addr(), dst = db.addr();
  const uint64_t units = brotli_amd_seg_units(dst, len);
  if (units != db.span / 16u) { std::fprintf(stderr, "units %llu of a span of %zu\n", (unsigned long long)units, db.span); return 1; }
  const uint64_t tile = BROTLI_AMD_BITUNPACK_TILE_BYTES / 16u, slot = 2u * w;
  if (rnd() & 1u) {
    for (uint64_t t0 = 0; t0 < units; t0 += tile) {
      const uint64_t t1 = std::min(t0 + tile, units);
      for (uint64_t s = t0 / slot; slot * s < t1; s++) g_items += brotli_amd_bitunpack_slot(src, dst, m, w, k, flags, s, t0, t1);
    }
  } else {
    // (the tiles from the last to the first, and in each the words from the last to the first)
    for (uint64_t t1 = units; t1 > 0;) {
      const uint64_t t0 = (t1 - 1u) / tile * tile;
      for (uint64_t u = t1; u-- > t0;) brotli_amd_bitunpack_word_alone(src, dst, m, w, k, flags, u, t0, t1);
      t1 = t0;
    }
  }
  size_t i = 0;
  uint8_t is = 0, must = 0;
  if (!db.holds([&](size_t p) { return want_byte(sb.at(), k, w, flags, p); }, &i, &is, &must)) {
    std::fprintf(stderr, "width %u bits %u flags %u count %zu skews %u %u: byte %zu is %02x, not %02x\n", w, k, flags, m, ss, ds, i, is, must);
    return 1;
  }
  return 0;
}

int main() {
  unsigned long long segments = 0;
  for (uint32_t w : {1u, 2u, 4u, 8u}) {
    const size_t tile = BROTLI_AMD_BITUNPACK_TILE_BYTES / w;   // elements of a tile
    for (uint32_t k = 1; k <= 8u * w; k++) {
      const bool every = k == 1u || k == 3u || k == 7u || k == 8u || k == 13u || k == 31u || k == 32u || k == 33u || k == 63u || k == 64u;
      for (uint32_t flags = 0; flags < 4u; flags++) {
        for (size_t m = 0; m <= 40; m++) {
          if (every && (m <= 3 || m == 32 || m == 33)) {
            for (uint32_t ss = 0; ss < 16u; ss++)
              for (uint32_t ds = 0; ds < 16u; ds++) { if (int e = one(w, k, flags, m, ss, ds)) return e; segments++; }
          } else {
            if (int e = one(w, k, flags, m, rnd() & 15u, 0u)) return e;
            if (int e = one(w, k, flags, m, rnd() & 15u, rnd() & 15u)) return e;
            segments += 2;
          }
        }
        std::vector<size_t> counts = {63, 64, 65, 95, 96, 97, 257, 1024 + 31};
        if (((k + flags) & 3u) == 0u) { counts.push_back(tile - 1u); counts.push_back(tile); counts.push_back(tile + 1u); }
        if (((k + flags) & 15u) == 0u) counts.push_back(2u * tile + 33u);
        for (size_t m : counts) {
          // (destination skew 0 twice: the fast items by the slots and, where the seed says so, word by word)
          if (int e = one(w, k, flags, m, rnd() & 15u, 0u)) return e;
          if (int e = one(w, k, flags, m, rnd() & 15u, 0u)) return e;
          if (int e = one(w, k, flags, m, rnd() & 15u, 1u + rnd() % 15u)) return e;
          segments += 3;
        }
      }
    }
  }
  if (g_items == 0) { std::fprintf(stderr, "no fast item was taken\n"); return 1; }
  // a shape that is none: nothing is read or written
  uint8_t guard[32];
  for (int i = 0; i < 32; i++) guard[i] = (uint8_t)i;
  const uint64_t g = (uint64_t)(uintptr_t)guard;
  (void)brotli_amd_bitunpack_slot(g, g + 16u, 16, 3u, 3u, 0u, 0, 0, 1);
  (void)brotli_amd_bitunpack_slot(g, g + 16u, 16, 1u, 9u, 0u, 0, 0, 1);
  (void)brotli_amd_bitunpack_slot(g, g + 16u, 16, 1u, 3u, 4u, 0, 0, 1);
  brotli_amd_bitunpack_unit(g, g + 16u, 16, 1u, 0u, 0u, 0);
  brotli_amd_bitunpack_word_alone(g, g + 16u, 16, 2u, 17u, 0u, 0, 0, 1);
  for (int i = 0; i < 32; i++) if (guard[i] != (uint8_t)i) return 1;
  std::printf("%llu segments, %llu fast items\n", segments, g_items);
  return 0;
}
