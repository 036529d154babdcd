// brotli_unrle.h -- runs of the RLE / bit-packed hybrid back into elements: one run of the walk, one element of a run and the bookkeeping of one
// item, once, for the host and the device.
//
// THE TRANSFORM (include/brotli/batch.h has it in full).  A segment of len bytes, a field width k (0 .. 32), an element width w (1, 2, 4 or 8,
// k <= 8 w), flags and a capacity cap in elements.  From offset 0 (1 with BROTLI_AMD_UNRLE_WIDTH_BYTE, the first byte then being k) it is a
// sequence of RUNS: a header h, a LEB128 varint of 1 .. 5 bytes, and then, for an odd h, (h >> 1) k bytes that hold 8 (h >> 1) fields of k
// bits LSB-first, or, for an even h, ceil(k / 8) bytes of one little-endian value that stands h >> 1 times.  The decode ends at the segment's
// end or at the first STOP; what lies in front of a stop is delivered.  Element i of the concatenated runs goes to dst + i w for
// i < min(count, cap).  Every segment has a result: count, consumed, runs, status and the k that was used.
//
// Where a header lies depends on every header in front of it, so a segment is WALKED, run after run, by one taker -- brotli_amd_unrle_walk,
// which reads the headers and the repeated values and never a packed payload.  The destination is cut into ITEMS of item_elems elements: item j
// holds the elements [j C, (j + 1) C) below min(count, cap).  The walk leaves every item a CHECKPOINT -- the header offset and the first
// element of the run that holds the item's first element --, and an item is then EXPANDED by itself from there: the runs that cover it, every
// element by brotli_amd_unrle_element, stored by unvarint's element store.  Items of one segment write disjoint bytes, in any order.
//
// LOADS.  Single bytes of [src, src + len) (the device's walk: the aligned 16-byte words that hold them, through LDS).  A packed field is read
// by bit-unpack's slow form: the single bytes that hold it.  STORES.  Element i as one store of w bytes where dst + i w is a multiple of w,
// byte by byte elsewhere (the device puts neighbouring elements together into aligned 16-byte stores where a lane has them all).
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUnrleHost; tests/tools/unrle_san.cpp) and the device
// (csrc/brotli_unrle_kernels.hip); only the staging through LDS and the sharing among a wave's lanes are the device's own.  Addresses are integers.
#ifndef BROTLI_AMD_UNRLE_H_
#define BROTLI_AMD_UNRLE_H_

#include "brotli/batch.h"       // BrotliAmdUnrleResult, BROTLI_AMD_UNRLE_*
#include "brotli_bitunpack.h"   // a packed field: brotli_amd_bitunpack_value
#include "brotli_device_abi.h"  // the segment of a launch: BrotliAmdUnrleSeg
#include "brotli_unvarint.h"    // the element store: brotli_amd_unvarint_store

#define BROTLI_AMD_UNRLE_HD BROTLI_AMD_UNSHUFFLE_HD
#define BROTLI_AMD_UNRLE_FLAGS BROTLI_AMD_UNRLE_WIDTH_BYTE   // the flag bits there are
#define BROTLI_AMD_UNRLE_MAX_CAP ((uint64_t)1 << 56)         // (so that cap w cannot overflow)
#define BROTLI_AMD_UNRLE_MAX_BITS 32u
#define BROTLI_AMD_UNRLE_NONE (~(uint64_t)0)                 // the checkpoint of an item beyond count; the payload of a run that has none

// a field width and an element width that go together
BROTLI_AMD_UNRLE_HD bool brotli_amd_unrle_bits_ok(uint32_t k, uint32_t w) { return k <= BROTLI_AMD_UNRLE_MAX_BITS && k <= 8u * w; }

// ---- one run ----
enum { BROTLI_AMD_UNRLE_RLE = 0, BROTLI_AMD_UNRLE_PACKED = 1, BROTLI_AMD_UNRLE_STOP = 2 };

// where a walk stands: the offset of the next header and the elements of the runs in front of it
struct BrotliAmdUnrleWalk { uint64_t off, elems; };

struct BrotliAmdUnrleRun {
  uint32_t kind;      // BROTLI_AMD_UNRLE_RLE, _PACKED or _STOP
  uint32_t status;    // OK; of a STOP its reason; TRUNCATED for a packed run whose payload the segment's end cuts: its whole values count, the walk ends
  uint64_t count;     // its values (a STOP: 0)
  uint64_t payload;   // the offset of its payload
  uint64_t next;      // the offset behind it (a STOP: the header's own)
  uint32_t value;     // of an RLE run: the repeated value, not masked
};

// The run whose header lies at st.off < len.  rd.window(o, avail, &b8) gives the segment's bytes at offsets o .. o + 7, little-endian, and the
// byte at o + 8 -- a header and a repeated value are nine bytes at the most --, avail = len - o; what of them lies at or behind len may be
// anything, and is taken as 0 here.  Nothing else is asked for, and of a packed run nothing behind its header.  Without a loop: the header's
// length is the first of its five bytes with bit 7 clear, and its groups are put together by unvarint's pack.
template <class Reader>
BROTLI_AMD_UNRLE_HD BrotliAmdUnrleRun brotli_amd_unrle_run(const Reader& rd, uint64_t len, uint32_t k, BrotliAmdUnrleWalk st) {
  BrotliAmdUnrleRun r = {BROTLI_AMD_UNRLE_STOP, BROTLI_AMD_UNRLE_TRUNCATED, 0u, st.off, st.off, 0u};
  const uint64_t avail = len - st.off;
  uint32_t b8 = 0;
  uint64_t x = rd.window(st.off, avail, &b8);
  if (avail < 8u) x &= ((uint64_t)1 << (8u * (uint32_t)avail)) - 1u;
  if (avail < 9u) b8 = 0u;
  const uint64_t ends = ~x & 0x8080808080ull;   // (a byte behind len ends the header here: it is found out below)
  if (ends == 0u) { r.status = BROTLI_AMD_UNRLE_BAD_HEADER; return r; }   // five bytes with bit 7 set: all of them are the segment's
  const uint32_t i = ((uint32_t)__builtin_ctzll(ends) >> 3) + 1u;   // the header's bytes
  if (i > avail) return r;   // the header's continuation reaches len
  const uint64_t h = brotli_amd_unvarint_pack7((uint32_t)x, (uint32_t)(x >> 32)) & (((uint64_t)1 << (7u * i)) - 1u);
  const uint64_t n = h >> 1, at = st.off + i, have = avail - i;
  if (n == 0u) { r.status = BROTLI_AMD_UNRLE_ZERO_RUN; return r; }
  if ((h & 1u) != 0u) {
    const uint64_t need = n * k;   // (n < 2^34, k <= 32)
    r.kind = BROTLI_AMD_UNRLE_PACKED; r.payload = at;
    if (need > have) { r.count = have * 8u / k; r.next = len; return r; }   // (k != 0 here; have < 2^39)
    r.status = BROTLI_AMD_UNRLE_OK; r.count = 8u * n; r.next = at + need;
    return r;
  }
  const uint32_t nb = (k + 7u) >> 3;
  if (nb > have) return r;   // the value reaches len
  const uint32_t v = (uint32_t)((x >> (8u * i)) | ((uint64_t)b8 << (64u - 8u * i)));   // bytes i .. i + 3 of the nine
  r.kind = BROTLI_AMD_UNRLE_RLE; r.status = BROTLI_AMD_UNRLE_OK; r.count = n; r.payload = at; r.next = at + nb;
  r.value = nb >= 4u ? v : v & ((1u << (8u * nb)) - 1u);
  return r;
}

// Element i of a run of the segment at address src: `payload` is the run's payload offset for a packed run and BROTLI_AMD_UNRLE_NONE for an
// RLE run, whose value is `value`.
BROTLI_AMD_UNRLE_HD uint64_t brotli_amd_unrle_element(uint64_t src, uint64_t payload, uint32_t value, uint32_t k, uint64_t i) {
  if (payload == BROTLI_AMD_UNRLE_NONE) return value;
  return k ? brotli_amd_bitunpack_value(src + payload, i, k, 0u) : 0u;
}

// ---- the items ----
struct BrotliAmdUnrleCheckpoint {
  uint64_t off;     // the header offset of the run that holds the item's first element (BROTLI_AMD_UNRLE_NONE: the item lies beyond count)
  uint64_t first;   // that run's first element
};

BROTLI_AMD_UNRLE_HD uint64_t brotli_amd_unrle_items(uint64_t cap, uint32_t item_elems) { return (cap + item_elems - 1u) / item_elems; }
// the elements [*e0, *e1) of item j of a segment that delivers min(count, cap) elements (*e0 >= *e1: none)
BROTLI_AMD_UNRLE_HD void brotli_amd_unrle_item_range(uint64_t count, uint64_t cap, uint64_t j, uint32_t item_elems, uint64_t* e0, uint64_t* e1) {
  const uint64_t end = count < cap ? count : cap;
  *e0 = j * item_elems;
  *e1 = *e0 + item_elems < end ? *e0 + item_elems : end;
}
// The items [*j0, *j1) whose first element lies in the run of `count` values from element `first` on, below cap.
BROTLI_AMD_UNRLE_HD void brotli_amd_unrle_run_items(uint64_t first, uint64_t count, uint64_t cap, uint32_t item_elems, uint64_t* j0, uint64_t* j1) {
  const uint64_t end = first + count < cap ? first + count : cap;
  *j0 = (first + item_elems - 1u) / item_elems;
  *j1 = first < end ? (end + item_elems - 1u) / item_elems : *j0;
}

// ---- the walk ----
// A segment's runs one after the other -> its result.  rd.ensure(o) is called in front of a run whose header lies at offset o < len (the
// device stages the bytes around it), and rd.window gives the bytes from o on (brotli_amd_unrle_run).  mark(j0, j1, off, first): the items [j0, j1) have the checkpoint
// (off, first).  Nothing is written but through mark.
template <class Reader, class Mark>
BROTLI_AMD_UNRLE_HD BrotliAmdUnrleResult brotli_amd_unrle_walk(Reader& rd, uint64_t len, uint64_t cap, uint32_t width, uint32_t bits, uint32_t flags,
                                                               uint32_t item_elems, Mark mark) {
  BrotliAmdUnrleResult res = {0u, 0u, 0u, BROTLI_AMD_UNRLE_OK, bits};
  BrotliAmdUnrleWalk st = {0u, 0u};
  if ((flags & BROTLI_AMD_UNRLE_WIDTH_BYTE) != 0u) {
    res.bits = 0u;
    if (len != 0u) { uint32_t b8; rd.ensure(0u); res.bits = (uint32_t)rd.window(0u, len, &b8) & 0xFFu; }
    if (len == 0u || !brotli_amd_unrle_bits_ok(res.bits, width)) { res.status = BROTLI_AMD_UNRLE_BAD_WIDTH; return res; }
    st.off = 1u;
  }
  const uint32_t k = res.bits;
  while (st.off < len) {
    rd.ensure(st.off);
    const BrotliAmdUnrleRun run = brotli_amd_unrle_run(rd, len, k, st);
    if (run.kind != BROTLI_AMD_UNRLE_STOP && run.count != 0u) {
      uint64_t j0, j1;
      brotli_amd_unrle_run_items(st.elems, run.count, cap, item_elems, &j0, &j1);
      if (j0 < j1) mark(j0, j1, st.off, st.elems);
      res.runs++;
    }
    st.off = run.next; st.elems += run.count;
    if (run.status != BROTLI_AMD_UNRLE_OK) { res.status = run.status; break; }
  }
  res.count = st.elems; res.consumed = st.off;
  return res;
}

// the bytes of a segment as they lie in memory (the host's reader, and the one of tests/tools/unrle_san.cpp)
struct BrotliAmdUnrleDirect {
  uint64_t src;
  BROTLI_AMD_UNRLE_HD void ensure(uint64_t) {}
  BROTLI_AMD_UNRLE_HD uint64_t window(uint64_t o, uint64_t avail, uint32_t* b8) const {   // single bytes, none at or behind len
    uint64_t x = 0;
    for (uint32_t j = 0; j < 8u && j < avail; j++) x |= (uint64_t)brotli_amd_unshuffle_ld8(src + o + j) << (8u * j);
    *b8 = avail > 8u ? brotli_amd_unshuffle_ld8(src + o + 8u) : 0u;
    return x;
  }
};

// ---- the walk and an item over host memory (the device replaces the loops over an item's elements by its lanes) ----
// ckpts[0 .. brotli_amd_unrle_items(sg.cap, item_elems)) start as BROTLI_AMD_UNRLE_NONE
inline BrotliAmdUnrleResult brotli_amd_unrle_host_walk(const BrotliAmdUnrleSeg& sg, uint32_t item_elems, BrotliAmdUnrleCheckpoint* ckpts) {
  BrotliAmdUnrleDirect rd = {(uint64_t)(uintptr_t)sg.src};
  return brotli_amd_unrle_walk(rd, sg.len, sg.cap, sg.width, sg.bits, sg.flags, item_elems, [&](uint64_t j0, uint64_t j1, uint64_t off, uint64_t first) {
    for (uint64_t j = j0; j < j1; j++) ckpts[j] = BrotliAmdUnrleCheckpoint{off, first};
  });
}
// Item j of a segment of len bytes at src with capacity cap, count and k being its walk's and cp the item's checkpoint: each(e, v) for every
// element e of the item, v being the value of its run (brotli_amd_undict.h takes v as an index)
template <class Each>
inline void brotli_amd_unrle_host_item_each(uint64_t src, uint64_t len, uint64_t cap, uint64_t count, uint32_t k, BrotliAmdUnrleCheckpoint cp, uint64_t j,
                                            uint32_t item_elems, Each each) {
  uint64_t e0, e1;
  brotli_amd_unrle_item_range(count, cap, j, item_elems, &e0, &e1);
  if (cp.off == BROTLI_AMD_UNRLE_NONE || e0 >= e1) return;
  BrotliAmdUnrleDirect rd = {src};
  BrotliAmdUnrleWalk st = {cp.off, cp.first};
  for (uint64_t e = e0; e < e1;) {
    const BrotliAmdUnrleRun run = brotli_amd_unrle_run(rd, len, k, st);
    if (run.kind == BROTLI_AMD_UNRLE_STOP) return;   // (not below count)
    const uint64_t run_end = st.elems + run.count, payload = run.kind == BROTLI_AMD_UNRLE_RLE ? BROTLI_AMD_UNRLE_NONE : run.payload;
    for (; e < run_end && e < e1; e++) each(e, brotli_amd_unrle_element(src, payload, run.value, k, e - st.elems));
    st.off = run.next; st.elems = run_end;
    if (run.status != BROTLI_AMD_UNRLE_OK) return;
  }
}
// item j of the segment, res being the walk's result and cp the item's checkpoint
inline void brotli_amd_unrle_host_item(const BrotliAmdUnrleSeg& sg, const BrotliAmdUnrleResult& res, BrotliAmdUnrleCheckpoint cp, uint64_t j, uint32_t item_elems) {
  const uint64_t dst = (uint64_t)(uintptr_t)sg.dst;
  brotli_amd_unrle_host_item_each((uint64_t)(uintptr_t)sg.src, sg.len, sg.cap, res.count, res.bits, cp, j, item_elems,
                                  [&](uint64_t e, uint64_t v) { brotli_amd_unvarint_store(dst + e * sg.width, sg.width, v); });
}

#endif  // BROTLI_AMD_UNRLE_H_
