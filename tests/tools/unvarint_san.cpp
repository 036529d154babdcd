// unvarint_san.cpp -- the unvarint unit and tile functions (csrc/brotli_unvarint.h) under AddressSanitizer and UBSan, as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I include -I rust-brotli-decompressor_amd/csrc tests/tools/unvarint_san.cpp
// All three phases -- the tiles' counts, the carries, the elements -- with tiles of 1, 2, 3 and 5 units and the kernel's own, against a serial
// decoder of its own.  Single segments: every width, plain and zigzag; every length 0..100 at every pair of skews for lengths up to 40 and at 32
// pairs beyond, 1023 .. 1025 and the tile's edges at 8 pairs; capacities of 0, m - 1, m and m + 5.  The bytes are seeded: half of them end a
// varint, and runs of continuation bytes are put in so that overlong varints occur in short segments too.  Tables of many segments of mixed
// widths, zero-length ones among them.  Every source lies in a heap block of EXACTLY the sixteen-byte words its span touches, every destination
// in one of the words its min(m, cap) elements touch: a load or a store one word too far would be reported; the destination's bytes beside the
// elements must keep their pattern.  Exits 0 when everything agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_device_abi.h"
#include "brotli_unvarint.h"
#include "san_block.h"

static uint32_t g_seed = 2028u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

typedef SanBlock Block;

struct Want { std::vector<uint64_t> elems; BrotliAmdUnvarintResult res; };

// the varints of s[0, len), one byte after the other
static Want expect(const uint8_t* s, size_t len, uint32_t flags) {
  Want w;
  w.res = BrotliAmdUnvarintResult{0u, 0u, 0u};
  uint64_t v = 0;
  uint32_t n = 0;
  for (size_t p = 0; p < len; p++) {
    if (n < 9u) v |= (uint64_t)(s[p] & 0x7Fu) << (7u * n);
    else if (n == 9u) v |= (uint64_t)(s[p] & 1u) << 63;
    n++;
    if (s[p] < 0x80u) {
      if (flags & BROTLI_AMD_UNVARINT_ZIGZAG) v = (v >> 1) ^ ((uint64_t)0 - (v & 1u));
      if (n > 10u) { v = 0; w.res.overlong++; }
      w.elems.push_back(v);
      w.res.count++; w.res.consumed = p + 1u;
      v = 0; n = 0;
    }
  }
  return w;
}

// the three phases over segs with tiles of tile_units, phases 1 and 3 from the last tile to the first or the other way round
static void run(const std::vector<BrotliAmdUnvarintSeg>& segs, uint64_t tile_units, bool backwards, std::vector<BrotliAmdUnvarintResult>* results) {
  const uint32_t n = (uint32_t)segs.size();
  results->assign(n, BrotliAmdUnvarintResult{0u, 0u, 0u});
  std::vector<uint64_t> pre(n + 1u, 0u);
  for (uint32_t i = 0; i < n; i++) pre[i + 1u] = pre[i] + brotli_amd_seg_units((uint64_t)(uintptr_t)segs[i].src, segs[i].len);
  const uint64_t units = pre[n], ntiles = (units + tile_units - 1u) / tile_units;
  std::vector<BrotliAmdUndeltaTile> tiles(ntiles);
  std::vector<uint64_t> carries(ntiles);
  auto end_of = [&](uint64_t t) { return (t + 1u) * tile_units < units ? (t + 1u) * tile_units : units; };
  for (uint64_t i = 0; i < ntiles; i++) {
    const uint64_t t = backwards ? ntiles - 1u - i : i;
    tiles[t] = brotli_amd_unvarint_host_summary(segs.data(), pre.data(), n, t * tile_units, end_of(t));
  }
  BrotliAmdUndeltaPair out = {0u, 0u};
  for (uint64_t t = 0; t < ntiles; t++) {
    carries[t] = brotli_amd_undelta_carry_in(out.sum, tiles[t]);
    out = brotli_amd_undelta_combine(out, brotli_amd_undelta_tile_pair(tiles[t]));
  }
  for (uint64_t i = 0; i < ntiles; i++) {
    const uint64_t t = backwards ? i : ntiles - 1u - i;
    brotli_amd_unvarint_host_emit(segs.data(), pre.data(), n, t * tile_units, end_of(t), carries[t], results->data());
  }
}

// seeded bytes with a run of continuation bytes here and there
static void fill_source(Block& s) {
  s.fill_random(rnd);
  for (size_t i = 0; i + 14u < s.len; i += 20u + rnd() % 60u)
    for (uint32_t j = 0, run = 8u + rnd() % 6u; j < run; j++) s.at()[i + j] |= 0x80u;
}

static int check(const Want& want, const BrotliAmdUnvarintResult& got, const Block& s, const Block& d, uint32_t w, uint64_t cap, const char* what) {
  if (got.count != want.res.count || got.consumed != want.res.consumed || got.overlong != want.res.overlong) {
    std::fprintf(stderr, "%s: width %u length %zu skews %u %u: result %llu %llu %llu, not %llu %llu %llu\n", what, w, s.len, s.skew, d.skew,
                 (unsigned long long)got.count, (unsigned long long)got.consumed, (unsigned long long)got.overlong, (unsigned long long)want.res.count,
                 (unsigned long long)want.res.consumed, (unsigned long long)want.res.overlong);
    return 1;
  }
  (void)cap;
  size_t i = 0;
  uint8_t is = 0, must = 0;
  if (d.holds([&](size_t p) { return (uint8_t)(want.elems[p / w] >> (8u * (p % w))); }, &i, &is, &must)) return 0;
  std::fprintf(stderr, "%s: width %u length %zu skews %u %u: byte %zu is %02x, not %02x\n", what, w, s.len, s.skew, d.skew, i, is, must);
  return 1;
}

// cap_kind: 0: cap 0, 1: m - 1, 2: m, 3: m + 5
static int one(uint32_t w, uint32_t flags, size_t len, uint32_t ss, uint32_t ds, uint64_t tile_units, uint32_t cap_kind) {
  Block s(len, ss);
  fill_source(s);
  const Want want = expect(s.at(), len, flags);
  const uint64_t m = want.res.count;
  const uint64_t cap = cap_kind == 0u ? 0u : cap_kind == 1u ? (m ? m - 1u : 0u) : cap_kind == 2u ? m : m + 5u;
  Block d((size_t)((m < cap ? m : cap) * w), ds);
  d.fill_pattern();
  std::vector<BrotliAmdUnvarintResult> res;
  run({BrotliAmdUnvarintSeg{s.at(), d.at(), len, cap, w, flags}}, tile_units, (rnd() & 1u) != 0u, &res);
  return check(want, res[0], s, d, w, cap, "one segment");
}

// a table of segments of mixed widths, every one in blocks of its own
static int table(uint32_t count, uint64_t tile_units) {
  std::vector<Block*> src, dst;
  std::vector<Want> wants;
  std::vector<BrotliAmdUnvarintSeg> segs;
  for (uint32_t i = 0; i < count; i++) {
    const uint32_t w = 1u << (rnd() & 3u), flags = rnd() & 1u;
    const uint32_t pick = rnd() % 10u;
    const size_t len = pick == 0u ? 0u : pick == 1u ? 700u + rnd() % 50u : rnd() % 70u;
    src.push_back(new Block(len, rnd() & 15u));
    fill_source(*src.back());
    wants.push_back(expect(src.back()->at(), len, flags));
    const uint64_t m = wants.back().res.count, cap = (rnd() & 3u) == 0u ? m / 2u : m + (rnd() & 7u);
    dst.push_back(new Block((size_t)((m < cap ? m : cap) * w), rnd() & 15u));
    dst.back()->fill_pattern();
    segs.push_back(BrotliAmdUnvarintSeg{src.back()->at(), dst.back()->at(), len, cap, w, flags});
  }
  std::vector<BrotliAmdUnvarintResult> res;
  run(segs, tile_units, (rnd() & 1u) != 0u, &res);
  int e = 0;
  for (uint32_t i = 0; i < count && !e; i++) e = check(wants[i], res[i], *src[i], *dst[i], segs[i].width, segs[i].cap, "table");
  for (Block* b : src) delete b;
  for (Block* b : dst) delete b;
  return e;
}

int main() {
  unsigned long long segments = 0;
  const uint64_t own = BROTLI_AMD_UNVARINT_TILE_BYTES / 16u;
  const uint64_t small[4] = {1u, 2u, 3u, 5u};
  for (uint32_t w : {1u, 2u, 4u, 8u}) {
    for (uint32_t flags = 0; flags < 2u; flags++) {
      for (size_t len = 0; len <= 100; len++) {
        if (len <= 40) {
          for (uint32_t ss = 0; ss < 16u; ss++)
            for (uint32_t ds = 0; ds < 16u; ds++) { if (int e = one(w, flags, len, ss, ds, small[(ss + ds + len) & 3u], (ss + ds) & 3u)) return e; segments++; }
        } else {
          for (uint32_t k = 0; k < 16u; k++) {
            if (int e = one(w, flags, len, k, k, small[k & 3u], k & 3u)) return e;
            if (int e = one(w, flags, len, rnd() & 15u, rnd() & 15u, small[rnd() & 3u], rnd() & 3u)) return e;
            segments += 2;
          }
        }
      }
      const size_t lens[] = {1023, 1024, 1025, BROTLI_AMD_UNVARINT_TILE_BYTES - 1u, BROTLI_AMD_UNVARINT_TILE_BYTES, BROTLI_AMD_UNVARINT_TILE_BYTES + 18u,
                             2u * BROTLI_AMD_UNVARINT_TILE_BYTES + 5u};
      for (size_t len : lens)
        for (uint32_t k = 0; k < 8u; k++) {
          if (int e = one(w, flags, len, k < 2u ? 15u * k : rnd() & 15u, k < 2u ? 15u - 15u * k : rnd() & 15u, (k & 1u) ? own : small[(k >> 1) & 3u], k & 3u)) return e;
          segments++;
        }
    }
  }
  for (uint32_t round = 0; round < 12u; round++) { if (int e = table(150u, round < 8u ? small[round & 3u] : own)) return e; segments += 150u; }
  // a width that is none: nothing is written
  uint8_t guard[48];
  for (int i = 0; i < 48; i++) guard[i] = (uint8_t)i;
  uint8_t* in = guard + ((16u - ((uintptr_t)guard & 15u)) & 15u);   // sixteen bytes of it, aligned: all of them ends
  const BrotliAmdUnvarintSeg odd = {in, in + 16, 16u, 100u, 3u, 0u};
  uint32_t ends = 0;
  const BrotliAmdU4 cur = brotli_amd_unvarint_fetch((uint64_t)(uintptr_t)in, 16u, 0u, &ends);
  const BrotliAmdUnvarintPart part = brotli_amd_unvarint_emit(odd, 0u, BrotliAmdU4{0u, 0u, 0u, 0u}, cur, ends, 0u);
  for (int i = 0; i < 48; i++) if (guard[i] != (uint8_t)i) return 1;
  if (ends != 0xFFFFu || part.consumed != 16u || part.overlong != 0u) return 1;
  std::printf("%llu segments\n", segments);
  return 0;
}
