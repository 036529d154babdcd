// undelta_san.cpp -- the undelta unit and tile functions (csrc/brotli_undelta.h) under AddressSanitizer and UBSan, as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I rust-brotli-decompressor_amd/csrc tests/tools/undelta_san.cpp
// All three phases -- the tiles' summaries, the carries, the running sums -- with tiles of 1, 2, 3 and 5 units and the kernel's own, against an
// elementwise loop of its own.  Single segments: every width; every length 0..160 at every pair of skews for lengths up to 48 and at 32 pairs
// beyond, the lengths 16 w k + d, 1023 .. 1025 and the tile's edges at 8 pairs; in place at element-aligned skews.  Tables of many segments of
// mixed widths, zero-length ones among them.  Every source and every destination lies in a heap block of EXACTLY the sixteen-byte words its span
// touches: a load or a store one word too far would be reported; the destination's bytes beside the segment must keep their pattern.  Exits 0
// when everything agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_device_abi.h"
#include "brotli_undelta.h"
#include "san_block.h"

static uint32_t g_seed = 2027u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

typedef SanBlock Block;

// want[0, len): the transform of s[0, len), element by element
static void expect(const uint8_t* s, size_t len, uint32_t w, uint8_t* want) {
  const size_t m = len / w;
  uint64_t run = 0;
  for (size_t e = 0; e < m; e++) {
    uint64_t x = 0;
    for (uint32_t j = 0; j < w; j++) x |= (uint64_t)s[e * w + j] << (8u * j);
    run += x;
    for (uint32_t j = 0; j < w; j++) want[e * w + j] = (uint8_t)(run >> (8u * j));
  }
  for (size_t p = m * w; p < len; p++) want[p] = s[p];
}

// the three phases over segs with tiles of tile_units, phases 1 and 3 from the last tile to the first or the other way round
static void run(const std::vector<BrotliAmdUnshuffleSeg>& segs, uint64_t tile_units, bool backwards) {
  const uint32_t n = (uint32_t)segs.size();
  std::vector<uint64_t> pre(n + 1u, 0u);
  for (uint32_t i = 0; i < n; i++) pre[i + 1u] = pre[i] + brotli_amd_seg_units((uint64_t)(uintptr_t)segs[i].dst, segs[i].len);
  const uint64_t units = pre[n], ntiles = (units + tile_units - 1u) / tile_units;
  std::vector<BrotliAmdUndeltaTile> tiles(ntiles);
  std::vector<uint64_t> carries(ntiles);
  auto end_of = [&](uint64_t t) { return (t + 1u) * tile_units < units ? (t + 1u) * tile_units : units; };
  for (uint64_t i = 0; i < ntiles; i++) {
    const uint64_t t = backwards ? ntiles - 1u - i : i;
    tiles[t] = brotli_amd_undelta_host_summary(segs.data(), pre.data(), n, t * tile_units, end_of(t));
  }
  BrotliAmdUndeltaPair out = {0u, 0u};
  for (uint64_t t = 0; t < ntiles; t++) {
    carries[t] = brotli_amd_undelta_carry_in(out.sum, tiles[t]);
    out = brotli_amd_undelta_combine(out, brotli_amd_undelta_tile_pair(tiles[t]));
  }
  for (uint64_t i = 0; i < ntiles; i++) {
    const uint64_t t = backwards ? i : ntiles - 1u - i;
    brotli_amd_undelta_host_apply(segs.data(), pre.data(), n, t * tile_units, end_of(t), carries[t]);
  }
}

static int check(const Block& s0, const Block& d, uint32_t w, const char* what) {
  std::vector<uint8_t> want(d.len ? d.len : 1u);
  expect(s0.at(), d.len, w, want.data());
  size_t i = 0;
  uint8_t is = 0, must = 0;
  if (d.holds([&](size_t p) { return want[p]; }, &i, &is, &must)) return 0;
  std::fprintf(stderr, "%s: width %u length %zu skews %u %u: byte %zu is %02x, not %02x\n", what, w, d.len, s0.skew, d.skew, i, is, must);
  return 1;
}

static int one(uint32_t w, size_t len, uint32_t ss, uint32_t ds, uint64_t tile_units) {
  Block s(len, ss), d(len, ds);
  s.fill_random(rnd);
  d.fill_pattern();
  if (brotli_amd_seg_units((uint64_t)(uintptr_t)d.at(), len) != d.span / 16u) { std::fprintf(stderr, "units of a span of %zu\n", d.span); return 1; }
  run({BrotliAmdUnshuffleSeg{s.at(), d.at(), len, w, 0u}}, tile_units, (rnd() & 1u) != 0u);
  return check(s, d, w, "out of place");
}

// in place: the block holds the deltas, then the values; what lies beside the segment in its words keeps its pattern
static int one_in_place(uint32_t w, size_t len, uint32_t ds, uint64_t tile_units) {
  Block d(len, ds), copy(len, ds);
  d.fill_pattern();
  for (size_t i = 0; i < len; i++) d.at()[i] = copy.at()[i] = (uint8_t)rnd();
  run({BrotliAmdUnshuffleSeg{d.at(), d.at(), len, w, 0u}}, tile_units, (rnd() & 1u) != 0u);
  return check(copy, d, w, "in place");
}

// a table of segments of mixed widths, every one in blocks of its own
static int table(uint32_t count, uint64_t tile_units) {
  std::vector<Block*> src, dst;
  std::vector<BrotliAmdUnshuffleSeg> segs;
  for (uint32_t i = 0; i < count; i++) {
    const uint32_t w = 1u << (rnd() & 3u);
    const uint32_t pick = rnd() % 10u;
    const size_t len = pick == 0u ? 0u : pick == 1u ? 700u + rnd() % 50u : rnd() % 70u;
    src.push_back(new Block(len, rnd() & 15u)); dst.push_back(new Block(len, rnd() & 15u));
    src.back()->fill_random(rnd);
    dst.back()->fill_pattern();
    segs.push_back(BrotliAmdUnshuffleSeg{src.back()->at(), dst.back()->at(), len, w, 0u});
  }
  run(segs, tile_units, (rnd() & 1u) != 0u);
  int e = 0;
  for (uint32_t i = 0; i < count && !e; i++) e = check(*src[i], *dst[i], segs[i].width, "table");
  for (Block* b : src) delete b;
  for (Block* b : dst) delete b;
  return e;
}

int main() {
  unsigned long long segments = 0;
  const uint64_t own = BROTLI_AMD_UNDELTA_TILE_BYTES / 16u;
  const uint64_t small[4] = {1u, 2u, 3u, 5u};
  for (uint32_t w : {1u, 2u, 4u, 8u}) {
    for (size_t len = 0; len <= 160; len++) {
      if (len <= 48) {
        for (uint32_t ss = 0; ss < 16u; ss++)
          for (uint32_t ds = 0; ds < 16u; ds++) { if (int e = one(w, len, ss, ds, small[(ss + ds + len) & 3u])) return e; segments++; }
      } else {
        for (uint32_t k = 0; k < 16u; k++) {
          if (int e = one(w, len, k, k, small[k & 3u])) return e;
          if (int e = one(w, len, rnd() & 15u, rnd() & 15u, small[rnd() & 3u])) return e;
          segments += 2;
        }
      }
      for (uint32_t ds = 0; ds < 16u; ds += w) { if (int e = one_in_place(w, len, ds, small[(ds / w + len) & 3u])) return e; segments++; }
    }
    std::vector<size_t> lens = {1023, 1024, 1025, BROTLI_AMD_UNDELTA_TILE_BYTES - 1u, BROTLI_AMD_UNDELTA_TILE_BYTES, BROTLI_AMD_UNDELTA_TILE_BYTES + w + 1u};
    for (size_t k = 1; k <= 5; k++)
      for (int d = -1; d <= (int)w; d++) lens.push_back(16u * w * k + d);
    for (size_t len : lens)
      for (uint32_t k = 0; k < 8u; k++) {
        if (int e = one(w, len, k < 2u ? 15u * k : rnd() & 15u, k < 2u ? 15u - 15u * k : rnd() & 15u, (k & 1u) ? own : small[(k >> 1) & 3u])) return e;
        segments++;
      }
    if (int e = one_in_place(w, BROTLI_AMD_UNDELTA_TILE_BYTES + w + 1u, 8u, own)) return e;
  }
  for (uint32_t round = 0; round < 12u; round++) { if (int e = table(150u, round < 8u ? small[round & 3u] : own)) return e; segments += 150u; }
  // a width that is none: nothing is read or written
  uint8_t guard[32];
  for (int i = 0; i < 32; i++) guard[i] = (uint8_t)i;
  const BrotliAmdU4 v = brotli_amd_undelta_fetch((uint64_t)(uintptr_t)guard, (uint64_t)(uintptr_t)guard + 16u, 16, 3u, 0);
  brotli_amd_undelta_finish((uint64_t)(uintptr_t)guard, (uint64_t)(uintptr_t)guard + 16u, 16, 3u, 0, v, 5u);
  for (int i = 0; i < 32; i++) if (guard[i] != (uint8_t)i) return 1;
  if (v.x | v.y | v.z | v.w | (uint32_t)brotli_amd_undelta_total(v, 3u)) return 1;
  std::printf("%llu segments\n", segments);
  return 0;
}
