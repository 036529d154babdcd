// brotli_undbp.h -- blocks of Parquet's DELTA_BINARY_PACKED back into elements: a varint, the stream header, one block of the walk, one group of
// 32 fields and the bookkeeping of one item, once, for the host and the device.
//
// THE TRANSFORM (include/brotli/batch.h has it in full).  A segment of len bytes, an element width w (1, 2, 4 or 8) and a capacity cap in
// elements.  From offset 0 it is a HEADER of four LEB128 varints -- B values a block, M miniblocks a block, N values in all, the first value
// (zigzag) -- and then ceil((N - 1) / B) BLOCKS: min_delta (a zigzag varint), M width bytes, and the payloads of the needed miniblocks, miniblock
// j being V = B / M fields of width[j] bits, LSB-first.  v_0 = first, v_i = v_(i-1) + min_delta + field, wrapping at 64 bits; element i is the
// low 8 w bits of v_i at dst + i w for i < min(count, cap).  The decode ends at the first STOP; what lies in front of it is delivered.
//
// Where a block lies depends on every block header in front of it, so a segment is WALKED, block after block, by one taker --
// brotli_amd_undbp_walk, which reads the headers and the width bytes and never a payload.  The DELTAS (delta d makes element d + 1) are cut into
// ITEMS of item_deltas deltas, a multiple of 32: item j holds the deltas [j C, (j + 1) C) below min(count, cap) - 1, and item 0 element 0 as
// well.  The walk leaves every item a CHECKPOINT -- the offset and first delta of the block that holds the item's first delta.  From there an
// item finds its GROUPS by itself (brotli_amd_undbp_item_blocks): a group is 32 fields of one width k, 4 k bytes from a byte boundary on,
// because V is a multiple of 32.  The values are a running sum across all blocks, so an item is taken twice: once for the SUM of its deltas,
// left as an undelta tile record (csrc/brotli_undelta.h; the first item of a segment is a head and carries `first`), and, behind undelta's
// carry launch over those records, once more to STORE its elements on top of its carry-in.  Items of one segment write disjoint bytes.
//
// LOADS.  Single bytes of [src, src + len) (the device's walk: the aligned 16-byte words that hold them, through LDS).  A field is read by
// bit-unpack's slow form: the single bytes that hold it.  STORES.  Element i as one store of w bytes where dst + i w is a multiple of w, byte by
// byte elsewhere (the device puts a lane's neighbouring elements together into aligned 16-byte stores).
//
// One set of functions for the host (csrc/brotli_filters.cpp: BrotliAmdDebugUndbpHost; tests/tools/undbp_san.cpp) and the device
// (csrc/brotli_undbp_kernels.hip); only the staging through LDS and the sharing among a wave's lanes are the device's own.  Addresses are integers.
#ifndef BROTLI_AMD_UNDBP_H_
#define BROTLI_AMD_UNDBP_H_

#include "brotli/batch.h"       // BrotliAmdUndbpResult, BROTLI_AMD_UNDBP_*
#include "brotli_bitunpack.h"   // a field: brotli_amd_bitunpack_value
#include "brotli_device_abi.h"  // the segment of a launch: BrotliAmdUndbpSeg
#include "brotli_undelta.h"     // an item's sum: BrotliAmdUndeltaTile
#include "brotli_unrle.h"       // the items that begin in a stretch: brotli_amd_unrle_run_items; the host's reader: BrotliAmdUnrleDirect
#include "brotli_unvarint.h"    // the varint's groups: brotli_amd_unvarint_pack7; unzigzag; the element store: brotli_amd_unvarint_store

#define BROTLI_AMD_UNDBP_HD BROTLI_AMD_UNSHUFFLE_HD
#define BROTLI_AMD_UNDBP_MAX_CAP ((uint64_t)1 << 56)   // (so that cap w cannot overflow)
#define BROTLI_AMD_UNDBP_MAX_BLOCK 65536u              // values a block, at the most
#define BROTLI_AMD_UNDBP_MAX_BITS 64u
#define BROTLI_AMD_UNDBP_GROUP 32u                     // fields of a group
#define BROTLI_AMD_UNDBP_NONE (~(uint64_t)0)           // the checkpoint of an item beyond count

// ---- a varint ----
// The eight bytes at the offsets off .. off + 7 < len, little-endian; what lies at or behind len reads as 0.  rd.ensure(o) is called in front of
// rd.window(o, ..) (the device stages the bytes around o), as in csrc/brotli_unrle.h.
template <class Reader>
BROTLI_AMD_UNDBP_HD uint64_t brotli_amd_undbp_bytes8(Reader& rd, uint64_t len, uint64_t off) {
  const uint64_t avail = len - off;
  uint32_t b8 = 0;
  rd.ensure(off);
  const uint64_t x = rd.window(off, avail, &b8);
  return avail < 8u ? x & (((uint64_t)1 << (8u * (uint32_t)avail)) - 1u) : x;
}

struct BrotliAmdUndbpVarint {
  uint64_t value;    // by unvarint's rule: the groups of 7 bits, low group first; of ten bytes the lowest 64 bits
  uint32_t bytes;    // 1 .. 10
  uint32_t status;   // OK; TRUNCATED: it reaches len; BAD_HEADER: ten bytes with bit 7 set
};
// The varint at offset off <= len.  Without a loop: its length is the first byte with bit 7 clear.
template <class Reader>
BROTLI_AMD_UNDBP_HD BrotliAmdUndbpVarint brotli_amd_undbp_varint(Reader& rd, uint64_t len, uint64_t off) {
  BrotliAmdUndbpVarint r = {0u, 0u, BROTLI_AMD_UNDBP_TRUNCATED};
  if (off >= len) return r;
  const uint64_t avail = len - off;
  const uint64_t x = brotli_amd_undbp_bytes8(rd, len, off);
  const uint64_t ends = ~x & 0x8080808080808080ull;   // (a byte behind len ends the varint here: it is found out below)
  const uint64_t low = brotli_amd_unvarint_pack7((uint32_t)x, (uint32_t)(x >> 32));
  if (ends != 0u) {
    const uint32_t i = ((uint32_t)__builtin_ctzll(ends) >> 3) + 1u;
    if (i > avail) return r;
    r.value = i < 8u ? low & (((uint64_t)1 << (7u * i)) - 1u) : low;
    r.bytes = i; r.status = BROTLI_AMD_UNDBP_OK;
    return r;
  }
  // eight bytes with bit 7 set, all of them the segment's: the ninth and the tenth
  if (avail < 9u) return r;
  const uint64_t y = brotli_amd_undbp_bytes8(rd, len, off + 8u);
  const uint64_t b8 = y & 0xFFu, b9 = (y >> 8) & 0xFFu;
  if ((b8 & 0x80u) == 0u) { r.value = low | (b8 << 56); r.bytes = 9u; r.status = BROTLI_AMD_UNDBP_OK; return r; }
  if (avail < 10u) return r;
  if ((b9 & 0x80u) != 0u) { r.status = BROTLI_AMD_UNDBP_BAD_HEADER; return r; }
  r.value = low | ((b8 & 0x7Fu) << 56) | (b9 << 63); r.bytes = 10u; r.status = BROTLI_AMD_UNDBP_OK;
  return r;
}

// ---- the stream header ----
struct BrotliAmdUndbpHeader {
  uint32_t status;   // OK, TRUNCATED or BAD_HEADER: the four varints in their order first, then what they say
  uint32_t block;    // B, M and V = B / M (0 where the varints were not all read; V 0 where M does not divide B)
  uint32_t mini;
  uint32_t per;
  uint64_t total;    // N
  uint64_t first;    // value 0
  uint64_t end;      // the offset behind the header
};
template <class Reader>
BROTLI_AMD_UNDBP_HD BrotliAmdUndbpHeader brotli_amd_undbp_header(Reader& rd, uint64_t len) {
  BrotliAmdUndbpHeader h = {BROTLI_AMD_UNDBP_OK, 0u, 0u, 0u, 0u, 0u, 0u};
  uint64_t v[4], off = 0;
  for (uint32_t i = 0; i < 4u; i++) {
    const BrotliAmdUndbpVarint x = brotli_amd_undbp_varint(rd, len, off);
    if (x.status != BROTLI_AMD_UNDBP_OK) { h.status = x.status; return h; }
    v[i] = x.value; off += x.bytes;
  }
  h.end = off; h.total = v[2]; h.first = brotli_amd_unvarint_unzigzag(v[3]);
  h.block = v[0] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v[0];   // (what does not fit is refused below, and reported as the largest there is)
  h.mini = v[1] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v[1];
  if (v[0] == 0u || v[0] % 128u != 0u || v[0] > BROTLI_AMD_UNDBP_MAX_BLOCK || v[1] == 0u || v[0] % v[1] != 0u || (v[0] / v[1]) % BROTLI_AMD_UNDBP_GROUP != 0u) {
    h.status = BROTLI_AMD_UNDBP_BAD_HEADER;
    return h;
  }
  h.per = h.block / h.mini;
  return h;
}

// ---- one block ----
struct BrotliAmdUndbpBlock {
  uint32_t status;      // OK; BAD_HEADER, BAD_WIDTH, TRUNCATED: the walk ends
  uint64_t values;      // the deltas it gives (a stop in its header: 0)
  uint64_t next;        // the offset behind its last needed miniblock (a stop in its header: its own; a payload that reaches len: len)
};
// The block at offset off <= len of which `remaining` != 0 deltas are still needed, per = V and mini = M.  It reads the block's min_delta and
// its width bytes, eight at a time, and no payload.  A needed width above 64 stops the block whatever lies in front of it: the width bytes
// come first in the stream.
template <class Reader>
BROTLI_AMD_UNDBP_HD BrotliAmdUndbpBlock brotli_amd_undbp_block(Reader& rd, uint64_t len, uint32_t per, uint32_t mini, uint64_t off, uint64_t remaining) {
  BrotliAmdUndbpBlock r = {BROTLI_AMD_UNDBP_TRUNCATED, 0u, off};
  const BrotliAmdUndbpVarint md = brotli_amd_undbp_varint(rd, len, off);
  if (md.status != BROTLI_AMD_UNDBP_OK) { r.status = md.status; return r; }
  const uint64_t wat = off + md.bytes;
  if (mini > len - wat) return r;   // the width bytes reach len
  const uint64_t whole = remaining / per, need64 = whole + (remaining % per != 0u ? 1u : 0u);
  const uint32_t need = need64 < mini ? (uint32_t)need64 : mini;
  uint64_t pos = wat + mini, vals = 0;
  bool cut = false;
  for (uint32_t j = 0; j < need; j += 8u) {
    const uint64_t x = brotli_amd_undbp_bytes8(rd, len, wat + j);
    for (uint32_t t = 0; t < 8u && j + t < need; t++) {
      const uint32_t k = (uint32_t)(x >> (8u * t)) & 0xFFu;
      if (k > BROTLI_AMD_UNDBP_MAX_BITS) { r.status = BROTLI_AMD_UNDBP_BAD_WIDTH; r.values = 0u; r.next = off; return r; }
      if (cut) continue;
      const uint64_t left = remaining - vals, bytes = (uint64_t)(per / 8u) * k, have = len - pos;
      if (bytes > have) {   // (k != 0 here) the whole fields of the bytes that are there
        const uint64_t part = have * 8u / k;
        vals += part < left ? part : left;
        pos = len; cut = true;
      } else {
        vals += per < left ? per : left;
        pos += bytes;
      }
    }
  }
  r.status = cut ? BROTLI_AMD_UNDBP_TRUNCATED : BROTLI_AMD_UNDBP_OK; r.values = vals; r.next = pos;
  return r;
}

// ---- the items ----
typedef BrotliAmdUnrleCheckpoint BrotliAmdUndbpCheckpoint;   // off: the offset of the block that holds the item's first delta; first: that block's first delta

// the items of a segment of capacity cap: its deltas below cap - 1 in items of item_deltas, and one item at the least where there is an element
BROTLI_AMD_UNDBP_HD uint64_t brotli_amd_undbp_items(uint64_t cap, uint32_t item_deltas) {
  if (cap == 0u) return 0u;
  const uint64_t items = (cap - 1u + item_deltas - 1u) / item_deltas;
  return items != 0u ? items : 1u;
}
BROTLI_AMD_UNDBP_HD bool brotli_amd_undbp_item_ok(uint32_t item_deltas) { return item_deltas != 0u && item_deltas % BROTLI_AMD_UNDBP_GROUP == 0u; }

// ---- the walk ----
// A segment's header and its blocks one after the other -> its result, and *first (value 0; 0 where there is none).  mark(j0, j1, off, first):
// the items [j0, j1) have the checkpoint (off, first).  Nothing is written but through mark.
template <class Reader, class Mark>
BROTLI_AMD_UNDBP_HD BrotliAmdUndbpResult brotli_amd_undbp_walk(Reader& rd, uint64_t len, uint64_t cap, uint32_t item_deltas, uint64_t* first, Mark mark) {
  BrotliAmdUndbpResult res = {0u, 0u, 0u, 0u, BROTLI_AMD_UNDBP_OK, 0u, 0u};
  *first = 0u;
  const BrotliAmdUndbpHeader h = brotli_amd_undbp_header(rd, len);
  res.status = h.status; res.declared = h.total; res.block_values = h.block; res.miniblocks = h.mini;
  if (h.status != BROTLI_AMD_UNDBP_OK) return res;
  res.consumed = h.end;
  if (h.total == 0u) return res;
  *first = h.first;
  const uint64_t capd = cap != 0u ? cap - 1u : 0u, total = h.total - 1u;   // the deltas there is room for; the deltas there are
  if (cap != 0u) mark(0u, 1u, h.end, 0u);   // (item 0 holds element 0, whatever becomes of the first block)
  uint64_t off = h.end, done = 0;
  while (done < total) {
    const BrotliAmdUndbpBlock blk = brotli_amd_undbp_block(rd, len, h.per, h.mini, off, total - done);
    if (blk.values != 0u) {
      uint64_t j0, j1;
      brotli_amd_unrle_run_items(done, blk.values, capd, item_deltas, &j0, &j1);
      if (j0 < j1) mark(j0, j1, off, done);
      res.blocks++;
    }
    done += blk.values; off = blk.next;
    if (blk.status != BROTLI_AMD_UNDBP_OK) { res.status = blk.status; break; }
  }
  res.count = 1u + done; res.consumed = off;
  return res;
}

// ---- an item ----
// the deltas [*a, *b) of item j of a segment whose walk gave `count` values (none: *a >= *b)
BROTLI_AMD_UNDBP_HD void brotli_amd_undbp_item_range(uint64_t count, uint64_t cap, uint64_t j, uint32_t item_deltas, uint64_t* a, uint64_t* b) {
  const uint64_t end = count < cap ? count : cap, dn = end != 0u ? end - 1u : 0u;
  *a = j * item_deltas;
  *b = *a + item_deltas < dn ? *a + item_deltas : dn;
}
// The miniblocks that cover the deltas [a, b), a a multiple of 32, from the checkpoint cp on: the few block headers are read again, every lane
// the same, and emit(lo, hi, pos, k, min_delta, m0) says that the deltas [lo, hi) are fields of k bits of the miniblock whose first delta is m0
// and whose payload lies at offset pos; lo - m0 is a multiple of 32.  The walk has been over all of it: below count no stop is met.
template <class Reader, class Emit>
BROTLI_AMD_UNDBP_HD void brotli_amd_undbp_item_blocks(Reader& rd, uint64_t len, uint32_t per, uint32_t mini, BrotliAmdUndbpCheckpoint cp, uint64_t a, uint64_t b,
                                                      Emit emit) {
  uint64_t off = cp.off, m0 = cp.first;
  while (m0 < b) {
    const BrotliAmdUndbpVarint md = brotli_amd_undbp_varint(rd, len, off);
    if (md.status != BROTLI_AMD_UNDBP_OK || mini > len - (off + md.bytes)) return;   // (not below count)
    const uint64_t wat = off + md.bytes, min_delta = brotli_amd_unvarint_unzigzag(md.value);
    uint64_t pos = wat + mini;
    for (uint32_t j = 0; j < mini && m0 < b; j += 8u) {
      const uint64_t x = brotli_amd_undbp_bytes8(rd, len, wat + j);
      for (uint32_t t = 0; t < 8u && j + t < mini && m0 < b; t++) {
        const uint32_t k = (uint32_t)(x >> (8u * t)) & 0xFFu;
        if (k > BROTLI_AMD_UNDBP_MAX_BITS) return;   // (not below count)
        if (m0 + per > a) emit(m0 > a ? m0 : a, m0 + per < b ? m0 + per : b, pos, k, min_delta, m0);
        pos += (uint64_t)(per / 8u) * k; m0 += per;
      }
    }
    off = pos;
  }
}

// ---- a group: up to 32 fields of k bits from the address `at` on, under one min_delta ----
BROTLI_AMD_UNDBP_HD uint64_t brotli_amd_undbp_field(uint64_t at, uint32_t k, uint32_t t) { return k != 0u ? brotli_amd_bitunpack_value(at, t, k, 0u) : 0u; }
// the sum of its first nf deltas
BROTLI_AMD_UNDBP_HD uint64_t brotli_amd_undbp_group_sum(uint64_t at, uint32_t k, uint64_t min_delta, uint32_t nf) {
  uint64_t s = min_delta * nf;
  if (k != 0u) for (uint32_t t = 0; t < nf; t++) s += brotli_amd_bitunpack_value(at, t, k, 0u);
  return s;
}
// what an item leaves for the carry launch: its sum; the first item of a segment is a head and carries `first`
BROTLI_AMD_UNDBP_HD BrotliAmdUndeltaTile brotli_amd_undbp_tile(uint64_t j, uint64_t first, uint64_t sum) {
  return j == 0u ? BrotliAmdUndeltaTile{first + sum, 0u, 0u} : BrotliAmdUndeltaTile{sum, 1u, 1u};
}

// ---- the walk and an item over host memory (the device replaces the loops over an item's groups by its lanes) ----
// ckpts[0 .. brotli_amd_undbp_items(sg.cap, item_deltas)) start as BROTLI_AMD_UNDBP_NONE
inline BrotliAmdUndbpResult brotli_amd_undbp_host_walk(const BrotliAmdUndbpSeg& sg, uint32_t item_deltas, BrotliAmdUndbpCheckpoint* ckpts, uint64_t* first) {
  BrotliAmdUnrleDirect rd = {(uint64_t)(uintptr_t)sg.src};
  return brotli_amd_undbp_walk(rd, sg.len, sg.cap, item_deltas, first, [&](uint64_t j0, uint64_t j1, uint64_t off, uint64_t d0) {
    for (uint64_t j = j0; j < j1; j++) ckpts[j] = BrotliAmdUndbpCheckpoint{off, d0};
  });
}
// item j's record, res being the walk's result, cp the item's checkpoint and `first` value 0
inline BrotliAmdUndeltaTile brotli_amd_undbp_host_sum(const BrotliAmdUndbpSeg& sg, const BrotliAmdUndbpResult& res, BrotliAmdUndbpCheckpoint cp, uint64_t first, uint64_t j,
                                                      uint32_t item_deltas) {
  uint64_t a, b, sum = 0;
  brotli_amd_undbp_item_range(res.count, sg.cap, j, item_deltas, &a, &b);
  if (cp.off != BROTLI_AMD_UNDBP_NONE && a < b) {
    const uint64_t src = (uint64_t)(uintptr_t)sg.src;
    BrotliAmdUnrleDirect rd = {src};
    brotli_amd_undbp_item_blocks(rd, sg.len, res.block_values / res.miniblocks, res.miniblocks, cp, a, b, [&](uint64_t lo, uint64_t hi, uint64_t pos, uint32_t k, uint64_t md, uint64_t m0) {
      for (uint64_t g = lo; g < hi; g += BROTLI_AMD_UNDBP_GROUP)
        sum += brotli_amd_undbp_group_sum(src + pos + (g - m0) / 8u * k, k, md, (uint32_t)(hi - g < BROTLI_AMD_UNDBP_GROUP ? hi - g : BROTLI_AMD_UNDBP_GROUP));
    });
  }
  return brotli_amd_undbp_tile(j, first, sum);
}
// item j's elements on top of its carry-in
inline void brotli_amd_undbp_host_store(const BrotliAmdUndbpSeg& sg, const BrotliAmdUndbpResult& res, BrotliAmdUndbpCheckpoint cp, uint64_t first, uint64_t j,
                                        uint32_t item_deltas, uint64_t carry_in) {
  uint64_t a, b;
  brotli_amd_undbp_item_range(res.count, sg.cap, j, item_deltas, &a, &b);
  if (cp.off == BROTLI_AMD_UNDBP_NONE) return;
  const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst;
  uint64_t v = carry_in;
  if (j == 0u) {
    if (res.count == 0u || sg.cap == 0u) return;
    v += first;
    brotli_amd_unvarint_store(dst, sg.width, v);
  }
  if (a >= b) return;
  BrotliAmdUnrleDirect rd = {src};
  brotli_amd_undbp_item_blocks(rd, sg.len, res.block_values / res.miniblocks, res.miniblocks, cp, a, b, [&](uint64_t lo, uint64_t hi, uint64_t pos, uint32_t k, uint64_t md, uint64_t m0) {
    for (uint64_t d = lo; d < hi; d++) {
      v += md + brotli_amd_undbp_field(src + pos, k, (uint32_t)(d - m0));
      brotli_amd_unvarint_store(dst + (d + 1u) * sg.width, sg.width, v);
    }
  });
}

#endif  // BROTLI_AMD_UNDBP_H_
