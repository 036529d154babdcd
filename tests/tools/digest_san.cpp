// digest_san.cpp -- the digest arithmetic (csrc/brotli_crc.h) under AddressSanitizer and UBSan, as a program of its own:
//   g++ -fsanitize=address,undefined -I rust-brotli-decompressor_amd/csrc tests/tools/digest_san.cpp
// Both polynomials; every length 0..300 and a few around 4096 at every skew 0..15 past a 16-byte boundary, cut into pieces of 1, 2, 3, 4, 7 and
// the kernel's number of units, against a bitwise loop of its own.  Every segment lies in a heap block of EXACTLY the sixteen-byte words it
// touches: a load of a word that holds none of its bytes would be reported.  Then the shift: against feeding zero bytes bit by bit, and
// shift(shift(c, a), b) == shift(c, a + b) for counts beyond 4 GiB.  Exits 0 when everything agreed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "brotli_crc.h"
#include "san_block.h"

static constexpr BrotliAmdCrcConsts kConsts[2] = {brotli_amd_crc_make_consts(BROTLI_AMD_CRC32_POLY), brotli_amd_crc_make_consts(BROTLI_AMD_CRC32C_POLY)};

static uint32_t raw_bitwise(uint32_t poly, uint32_t reg, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) {
    reg ^= p[i];
    for (int k = 0; k < 8; k++) reg = (reg >> 1) ^ ((reg & 1u) ? poly : 0u);
  }
  return reg;
}

int main() {
  unsigned long long digests = 0;
  uint32_t seed = 12345u;
  for (uint32_t kind = 1; kind <= 2u; kind++) {
    const uint32_t poly = brotli_amd_crc_poly(kind);
    const BrotliAmdCrcConsts& c = kConsts[kind - 1u];
    std::vector<size_t> lens;
    for (size_t n = 0; n <= 300; n++) lens.push_back(n);
    for (size_t n : {4079, 4080, 4081, 4095, 4096, 4097, 12293}) lens.push_back(n);
    for (size_t n : lens)
      for (uint32_t skew = 0; skew < 16u; skew++) {
        SanBlock block(n, skew);
        block.fill_random([&seed] { seed = seed * 1664525u + 1013904223u; return seed >> 24; });
        const size_t span = block.span;
        const uint64_t at = block.addr();
        const uint32_t want = n ? ~raw_bitwise(poly, 0xFFFFFFFFu, block.at(), n) : 0u;
        const auto load = [](uint64_t W, uint32_t* w) { std::memcpy(w, reinterpret_cast<const void*>((uintptr_t)W), 16); };
        const uint64_t units = brotli_amd_seg_units(at, n);
        if (units != span / 16u) { std::fprintf(stderr, "units %llu of a span of %zu\n", (unsigned long long)units, span); return 1; }
        for (uint32_t run : {1u, 2u, 3u, 4u, 7u, (uint32_t)BROTLI_AMD_CRC_RUN_UNITS}) {
          uint32_t got = 0;
          for (uint64_t u0 = 0; u0 < units; u0 += run) {
            uint64_t behind = 0;
            const uint32_t reg = brotli_amd_crc_piece(&c.t[0][0], load, at, n, u0, std::min<uint64_t>(u0 + run, units), &behind);
            got ^= brotli_amd_crc_piece_term(poly, c.pw, reg, behind);
          }
          digests++;
          if (got != want) { std::fprintf(stderr, "kind %u length %zu skew %u run %u: %08x, not %08x\n", kind, n, skew, run, got, want); return 1; }
        }
      }
    // the shift: n zero bytes behind a raw register, bit by bit
    const std::vector<uint8_t> zeros(5000, 0);
    for (uint32_t reg : {0u, 1u, 0x80000000u, 0xFFFFFFFFu, 0xDEADBEEFu})
      for (size_t n : {0, 1, 2, 3, 4, 15, 16, 17, 255, 256, 1000, 4999})
        if (brotli_amd_crc_shift(poly, c.pw, reg, n) != raw_bitwise(poly, reg, zeros.data(), n)) { std::fprintf(stderr, "kind %u shift by %zu\n", kind, n); return 1; }
    for (uint64_t a : {(uint64_t)0, (uint64_t)5, ((uint64_t)1 << 32) + 5u, (uint64_t)1 << 40, ~(uint64_t)0 >> 1})
      for (uint64_t b : {(uint64_t)0, (uint64_t)77, (uint64_t)1 << 33, ((uint64_t)1 << 62) + 3u})
        if (brotli_amd_crc_shift(poly, c.pw, brotli_amd_crc_shift(poly, c.pw, 0x12345678u, a), b) != brotli_amd_crc_shift(poly, c.pw, 0x12345678u, a + b)) {
          std::fprintf(stderr, "kind %u shifts by %llu and %llu\n", kind, (unsigned long long)a, (unsigned long long)b);
          return 1;
        }
  }
  std::printf("%llu digests\n", digests);
  return 0;
}
