// brotli_size_walk.h -- how large does a .br stream decode?  What its HEADERS say, without decoding a prefix code.
//
// Brotli has no size field, but metadata and stored metablocks carry their own byte lengths and every compressed metablock states its MLEN
// in front of its prefix codes (RFC 7932 section 9.2; reference src/decode.rs:152-187 DecodeWindowBits, 243-372 DecodeMetaBlockLength).  The
// walk steps from bit 0 over the stream header and every metadata and stored metablock, and stops at the first compressed metablock -- whose
// MLEN it still counts --, at an empty last metablock, at the end of the input or at a header the decoder rejects.  A stream of one
// metablock (the rule for small documents) and one whose first compressed metablock is its last are sized exactly.
//
// One function for the host (BrotliAmdDebugSizeWalk, tests/tools/size_walk_san.cpp) and the device (csrc/brotli_size_kernels.hip): it sees
// the stream through a byte-fetch functor, `uint32_t fetch(uint64_t i)` = byte i of the stream, and asks for a byte only where i < n --
// payloads are stepped over by arithmetic, never read.  Every bit is checked to exist before it is looked at, in the decoder's own order:
// status 2 is said for bits the decoder reads as well, so the decoder reports an error wherever the walk does (the walk need not find every
// error: it reads no prefix code).
#ifndef BROTLI_AMD_SIZE_WALK_H_
#define BROTLI_AMD_SIZE_WALK_H_

#include <stdint.h>

#include "brotli/batch.h"   // BrotliAmdSizeHint, BROTLI_AMD_BATCH_LARGE_WINDOW

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BROTLI_AMD_HD __host__ __device__
#else
#define BROTLI_AMD_HD
#endif

#define BROTLI_AMD_SIZE_OK 0u          // BrotliAmdSizeHint.status
#define BROTLI_AMD_SIZE_TRUNCATED 1u   // the input ended inside the walk
#define BROTLI_AMD_SIZE_REJECTED 2u    // a header the decoder rejects

// k bits (k <= 8) at bit position *pos of the n-byte stream; false where the stream ends in front of their last (nothing is fetched then)
template <class Fetch>
BROTLI_AMD_HD inline bool brotli_amd_walk_bits(Fetch& fetch, uint64_t n, uint64_t* pos, uint32_t k, uint32_t* v) {
  if (k == 0u) { *v = 0u; return true; }
  const uint64_t p = *pos;
  if (n < ((p + k + 7u) >> 3)) return false;
  const uint32_t sh = (uint32_t)(p & 7u);
  uint32_t w = fetch(p >> 3);
  if (sh + k > 8u) w |= fetch((p >> 3) + 1u) << 8;
  *v = (w >> sh) & ((1u << k) - 1u);
  *pos = p + k;
  return true;
}

template <class Fetch>
BROTLI_AMD_HD inline BrotliAmdSizeHint brotli_amd_size_walk(Fetch fetch, uint64_t n, uint32_t flags) {
  BrotliAmdSizeHint h;
  h.bytes = 0; h.walked_in = 0; h.exact = 0; h.status = BROTLI_AMD_SIZE_TRUNCATED;
  uint64_t pos = 0;
  uint32_t v = 0;
#define WALK_TAKE(k) do { if (!brotli_amd_walk_bits(fetch, n, &pos, (k), &v)) return h; } while (0)
#define WALK_REJECT() do { h.status = BROTLI_AMD_SIZE_REJECTED; return h; } while (0)
  // WBITS (decode.rs:152-187); the large-window form is 14 bits: 0010001, a zero, six bits of window size (10..30)
  WALK_TAKE(1);
  if (v != 0u) {
    WALK_TAKE(3);
    if (v == 0u) {
      WALK_TAKE(3);
      if (v == 1u) {
        if (!(flags & BROTLI_AMD_BATCH_LARGE_WINDOW)) WALK_REJECT();
        WALK_TAKE(1);
        if (v == 1u) WALK_REJECT();
        WALK_TAKE(6);
        if (v < 10u || v > 30u) WALK_REJECT();
      }
    }
  }
  for (;;) {
    h.walked_in = pos >> 3;   // a walk that ends inside this metablock's header, or at a compressed one, has come this far
    uint32_t is_last, mlen = 0;
    WALK_TAKE(1); is_last = v;
    if (is_last) {
      WALK_TAKE(1);   // ISLASTEMPTY
      if (v) { h.walked_in = (pos + 7u) >> 3; h.exact = 1; h.status = BROTLI_AMD_SIZE_OK; return h; }
    }
    WALK_TAKE(2);   // MNIBBLES
    const bool metadata = v == 3u;
    if (metadata) {
      WALK_TAKE(1);
      if (v) WALK_REJECT();   // reserved bit
      WALK_TAKE(2);
      const uint32_t nbytes = v;   // MSKIPBYTES
      for (uint32_t i = 0; i < nbytes; i++) {
        WALK_TAKE(8);
        if (i + 1u == nbytes && nbytes > 1u && v == 0u) WALK_REJECT();   // exuberant meta nibble
        mlen |= v << (8u * i);
      }
      if (nbytes != 0u) mlen += 1u;
    } else {
      const uint32_t nibbles = v + 4u;
      for (uint32_t i = 0; i < nibbles; i++) {
        WALK_TAKE(4);
        if (i + 1u == nibbles && nibbles > 4u && v == 0u) WALK_REJECT();   // exuberant nibble
        mlen |= v << (4u * i);
      }
      mlen += 1u;
      uint32_t stored = 0;
      if (!is_last) { WALK_TAKE(1); stored = v; }
      if (!stored) {   // the first compressed metablock: its MLEN is known, what follows it is not
        h.bytes += mlen; h.exact = is_last; h.status = BROTLI_AMD_SIZE_OK;
        return h;
      }
    }
    // a metadata or stored metablock: zero padding to the byte boundary, then mlen bytes to step over
    WALK_TAKE((uint32_t)((8u - (pos & 7u)) & 7u));
    if (v != 0u) WALK_REJECT();
    const uint64_t at = pos >> 3;
    if (n - at < (uint64_t)mlen) return h;   // (truncated inside the payload: it is not counted, and walked_in stays in front of the block)
    pos = (at + mlen) << 3;
    if (!metadata) h.bytes += mlen;
    if (is_last) { h.walked_in = pos >> 3; h.exact = 1; h.status = BROTLI_AMD_SIZE_OK; return h; }   // (a last metablock of metadata)
  }
#undef WALK_TAKE
#undef WALK_REJECT
}

// the stream as plain memory
struct BrotliAmdWalkBytes {
  const uint8_t* in;
  BROTLI_AMD_HD uint32_t operator()(uint64_t i) const { return in[i]; }
};

// one stream of a size-walk launch: device address of its bytes (any alignment) and their number
typedef struct BrotliAmdSizeDesc {
  const uint8_t* in;
  uint64_t in_size;
} BrotliAmdSizeDesc;

#endif  // BROTLI_AMD_SIZE_WALK_H_
