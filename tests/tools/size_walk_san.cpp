// size_walk_san.cpp -- the size walk (csrc/brotli_size_walk.h) under AddressSanitizer and UBSan, as a program of its own:
//   g++ -fsanitize=address,undefined -I include -I rust-brotli-decompressor_amd/csrc tests/tools/size_walk_san.cpp
// Every argument is a file that holds a .br stream.  Every prefix of each, the whole stream included, is copied into a heap block of
// exactly its size and walked from there, with and without the large-window flag: a walk that fetched one byte beyond its input would be
// reported.  Exits 0 when every walk kept the contract a prefix can be held to.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "brotli_size_walk.h"

int main(int argc, char** argv) {
  unsigned long long walks = 0;
  for (int a = 1; a < argc; a++) {
    std::FILE* f = std::fopen(argv[a], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> all;
    uint8_t buf[4096];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) != 0;) all.insert(all.end(), buf, buf + got);
    std::fclose(f);
    for (uint32_t flags = 0; flags < 2; flags++) {
      BrotliAmdSizeHint whole = brotli_amd_size_walk(BrotliAmdWalkBytes{all.data()}, all.size(), flags);
      for (size_t n = 0; n <= all.size(); n++) {
        uint8_t* block = static_cast<uint8_t*>(std::malloc(n));   // (exactly n bytes: n == 0 included)
        if (n) std::memcpy(block, all.data(), n);
        const BrotliAmdSizeHint h = brotli_amd_size_walk(BrotliAmdWalkBytes{block}, n, flags);
        std::free(block);
        walks++;
        // a prefix never says more than the whole stream, never walks beyond its bytes, and a rejection does not depend on what follows
        const bool ok = h.walked_in <= n && h.status <= 2u && h.exact <= 1u && h.bytes <= whole.bytes &&
                        (h.status != BROTLI_AMD_SIZE_REJECTED || whole.status == BROTLI_AMD_SIZE_REJECTED) && (n != 0 || h.status == BROTLI_AMD_SIZE_TRUNCATED);
        if (!ok) {
          std::fprintf(stderr, "%s: prefix %zu flags %u: bytes %llu walked_in %llu exact %u status %u\n", argv[a], n, flags,
                       (unsigned long long)h.bytes, (unsigned long long)h.walked_in, h.exact, h.status);
          return 1;
        }
      }
    }
  }
  std::printf("%llu walks\n", walks);
  return 0;
}
