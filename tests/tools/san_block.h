// san_block.h -- what the *_san.cpp programs of the segment calls share: a segment's bytes at a skew, in a heap block of EXACTLY the sixteen-byte
// words they touch, so that AddressSanitizer reports a load or a store one word too far; a destination's block is patterned in front of the
// work, and behind it every byte beside the segment must still hold the pattern.
#ifndef TESTS_TOOLS_SAN_BLOCK_H_
#define TESTS_TOOLS_SAN_BLOCK_H_
#include <cstdint>
#include <cstdlib>

struct SanBlock {
  uint8_t* base = nullptr; size_t span = 0; uint32_t skew = 0; size_t len = 0;
  SanBlock(size_t len_, uint32_t skew_) : skew(skew_), len(len_) {
    span = len ? (skew + len + 15u) & ~(size_t)15 : 0;   // (no bytes: a block of which no word may be touched)
    base = static_cast<uint8_t*>(span ? std::aligned_alloc(16, span) : std::malloc(1));
    if (!base) std::abort();
  }
  SanBlock(const SanBlock&) = delete;
  ~SanBlock() { std::free(base); }
  uint8_t* at() const { return base + skew; }
  uint64_t addr() const { return (uint64_t)(uintptr_t)at(); }

  static uint8_t pattern(size_t i) { return (uint8_t)(0xA5u ^ i); }
  void fill_pattern() { for (size_t i = 0; i < span; i++) base[i] = pattern(i); }
  template <class Rnd> void fill_random(Rnd rnd) { for (size_t i = 0; i < span; i++) base[i] = (uint8_t)rnd(); }   // the whole block: a source

  // whether every byte of the block is what it must be: want(p) at byte p of the segment, the pattern beside it.  False: byte *i of the block
  // is *is and must be *must.
  template <class Want>
  bool holds(Want want, size_t* i, uint8_t* is, uint8_t* must) const {
    for (size_t k = 0; k < span; k++) {
      const uint8_t x = k >= skew && k < skew + len ? (uint8_t)want(k - skew) : pattern(k);
      if (base[k] != x) { *i = k; *is = base[k]; *must = x; return false; }
    }
    return true;
  }
};

#endif  // TESTS_TOOLS_SAN_BLOCK_H_
