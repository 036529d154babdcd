// seg_walk_san.cpp -- the segment walk's arithmetic (csrc/brotli_seg_walk.h: brotli_amd_seg_chunk_tiles under brotli_amd_seg_walk_model) under
// AddressSanitizer and UBSan, as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I rust-brotli-decompressor_amd/csrc tests/tools/seg_walk_san.cpp
// The tables of tests/test_seg_walk_cpu.py with tiles of 4 and 1024 units and grids of 1, 2, 7 and more blocks than tiles: every unit is
// marked once, in a vector of exactly as many entries as there are units; every part lies inside its tile and inside one chunk of 1024
// segments; a tile's parts are block tile % grid's.  Exits 0 when everything agreed.
#include <cstdio>
#include <vector>

#include "brotli_seg_walk.h"

static int walk(const std::vector<uint64_t>& units, uint32_t tile_units, uint32_t grid, const char* what) {
  const uint32_t n = (uint32_t)units.size();
  std::vector<uint64_t> chunk_end;   // the units in front of the end of every chunk of segments
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    total += units[i];
    if ((i + 1u) % BROTLI_AMD_SEG_CHUNK_SEGS == 0u || i + 1u == n) chunk_end.push_back(total);
  }
  std::vector<uint8_t> seen(total, 0);
  int bad = 0;
  unsigned long long parts = 0;
  brotli_amd_seg_walk_model(units.data(), n, tile_units, grid, [&](uint32_t block, uint64_t tile, uint64_t lo, uint64_t hi) {
    parts++;
    if (!(lo < hi && hi <= total && tile * tile_units <= lo && hi <= (tile + 1u) * tile_units && tile % grid == block)) { bad = 1; return; }
    uint64_t begin = 0;   // the chunk that holds lo holds hi - 1 as well
    for (uint64_t end : chunk_end) {
      if (lo < end) { if (lo < begin || hi > end) bad = 1; break; }
      begin = end;
    }
    for (uint64_t g = lo; g < hi; g++) { if (seen.at(g)) bad = 1; seen.at(g) = 1; }
  });
  for (uint8_t s : seen) if (!s) bad = 1;
  if (bad) std::fprintf(stderr, "%s: tiles of %u units, %u blocks: the parts do not tile the units\n", what, tile_units, grid);
  else std::printf("%s: tiles of %u, %u blocks: %llu parts\n", what, tile_units, grid, parts);
  return bad;
}

// the units of segments of these lengths, one behind the other from address `at`
static std::vector<uint64_t> packed(const std::vector<uint64_t>& lens, uint64_t at) {
  std::vector<uint64_t> units;
  for (uint64_t len : lens) { units.push_back(brotli_amd_seg_units(at, len)); at += len; }
  return units;
}

int main() {
  for (uint32_t tile_units : {4u, 1024u}) {
    const uint64_t tile = 16u * (uint64_t)tile_units;
    std::vector<uint64_t> gap = {tile / 2u + 7u};
    gap.insert(gap.end(), 2500, 0u);
    gap.insert(gap.end(), {tile + 9u, 5u, 0u, 1u});
    gap.insert(gap.end(), 1100, 0u);
    gap.push_back(3u * tile);
    const std::pair<const char*, std::vector<uint64_t>> tables[] = {
        {"a tile across empty segments", packed(gap, 9u)},
        {"1024 segments of one unit", std::vector<uint64_t>(1024, 1u)},
        {"1025 segments of one unit", std::vector<uint64_t>(1025, 1u)},
        {"3000 segments of one unit", std::vector<uint64_t>(3000, 1u)},
        {"one segment of ten tiles and a unit", {10u * tile_units + 1u}},
        {"all segments empty", std::vector<uint64_t>(2100, 0u)},
        {"no segments", {}},
    };
    for (const auto& t : tables) {
      uint64_t total = 0;
      for (uint64_t u : t.second) total += u;
      const uint32_t tiles = (uint32_t)((total + tile_units - 1u) / tile_units);
      for (uint32_t grid : {1u, 2u, 7u, tiles + 3u})
        if (walk(t.second, tile_units, grid, t.first)) return 1;
    }
  }
  return 0;
}
