// brotli_undba_kernels.hip -- nine launches in stream order that turn the DELTA_BYTE_ARRAY bodies of n independent segments, of any alignment
// and length, into Arrow string columns -- offsets and bytes --, and give every segment its result (gfx950, wave64).  The transform, the test
// of an element, the carry-in behind the first bad element and where a byte comes from in each phase are csrc/brotli_undba.h; the grammar, a
// block, a group and the bookkeeping of an item are undbp's (csrc/brotli_undbp.h, csrc/brotli_undbp_groups.h); the offsets' stores are
// undlba's.  No block ever waits for another block's result -- no flags, no spins, no atomics on offsets or data.
//   1. brotli_amd_undba_walk_kernel     undbp's walk as it is, ONE WAVE A SEGMENT, over P and then over S from P's consumed: the segment's
//                                       result, both first values, both streams' checkpoints, the segment's entry of the items' prefix array,
//                                       and both streams as undbp segments and undbp results for the items -- derived here, on the device.
//   2. brotli_amd_undba_sum_kernel      ONE WAVE AN ITEM, undbp's item function and group sum for both streams: two undelta tile records.
//   3. brotli_amd_undelta_carry_kernel  undelta's carry launch itself (csrc/brotli_undelta_kernels.hip) over the 2 x items records at once:
//                                       every segment's first item is a head in both halves.
//   4. brotli_amd_undba_lengths_kernel  the lanes redo their 32 elements on top of the carry-ins and test each against the one in front of it.
//                                       The item's sums of L and of s up to its first bad element are two more tile records; that element
//                                       goes to the segment's result with one atomicMin.
//   5. brotli_amd_undelta_carry_kernel  the carry launch again, over those.
//   6. brotli_amd_undba_expand_kernel   the offsets, as undlba's expand kernel stores them.  The item of first_bad writes bad_kind, the item
//                                       of the last delivered element bytes, suffix_bytes and data_status.
//   7. brotli_amd_undba_a_kernel        PHASE A, one wave an item, TWO WAVES A BLOCK: the item's p and s go to LDS (8 bytes an element); the
//                                       wave then takes the elements one after the other, 64 at a time scanned for their places, a lane a
//                                       byte: suffix bytes from the source, the bytes [r_e, p_e) from the running string in LDS
//                                       (BROTLI_AMD_UNDBA_LDS_STRING bytes; beyond: brotli_amd_undba_back_byte, from the source again).  No
//                                       byte this kernel stores is loaded by it.
//   8. brotli_amd_undba_b_kernel        PHASE B, one wave a segment and a block, the segment's items one after the other: the carried string
//                                       in LDS (BROTLI_AMD_UNDBA_LDS_CARRY bytes; beyond: brotli_amd_undba_far_byte, from what launch 7 stored).
//   9. brotli_amd_undba_c_kernel        PHASE C, one wave an item: 64 elements' bytes [0, r_e) at a time, spread evenly over the lanes by a
//                                       search in their running sum; the source is what launches 7 and 8 stored.
// A measuring call has no destinations: every store but those of the result is predicated off (keep is 0).  A call that only counts has no
// items and is the first launch alone.
// THE SCRATCH behind the table: the n results; 2n undbp results, 2n undbp segments and 2n first values (P's, then S's); the items' prefix
// array; and for every item two checkpoints, four tile records, four carries (all P's or L's first, then S's or s's) and its last element.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_run_items.h"      // the scratch's padding, the carry launch
#include "brotli_seg_walk.h"
#include "brotli_undba.h"
#include "brotli_undbp_groups.h"   // an item's groups, a group a lane
#include "brotli_wave_stage.h"

namespace {

constexpr uint32_t kThreads = brotli_amd_wave::kSegThreads, kWaves = brotli_amd_wave::kSegWaves;
constexpr uint32_t kChunk = brotli_amd_wave::kStageChunk, kItem = BROTLI_AMD_UNDBP_ITEM_DELTAS, kGroup = BROTLI_AMD_UNDBP_GROUP;
constexpr uint32_t kDataWaves = 2, kDataThreads = 64u * kDataWaves;   // launches 7 and 9
constexpr uint32_t kString = BROTLI_AMD_UNDBA_LDS_STRING, kCarry = BROTLI_AMD_UNDBA_LDS_CARRY;

static_assert(kItem == 64u * kGroup, "a group a lane");
static_assert(kDataWaves * (2u * (kItem + 1u) * 4u + 2u * kChunk + kString + 64u * 16u) <= 65536u && kCarry <= 65536u, "LDS of a block");

using brotli_amd_wave::dbp_item_groups;
using brotli_amd_wave::lds_sync;
using brotli_amd_wave::pad16;
using brotli_amd_wave::same;
using brotli_amd_wave::Stage;
using brotli_amd_wave::Word16;

typedef BrotliAmdUndbaSeg Seg;
typedef BrotliAmdUndbaResult Result;
typedef BrotliAmdUndbpSeg DbpSeg;
typedef BrotliAmdUndbpResult DbpResult;
typedef BrotliAmdUndbpCheckpoint Checkpoint;
typedef BrotliAmdUndeltaTile Tile;
typedef BrotliAmdUndbaLast Last;
typedef brotli_amd_wave::DbpGroup Group;

// what every launch behind the walk reads (P's or L's half first, S's or s's `n` or `items` entries behind it)
struct Walked {
  const DbpSeg* segs;
  const DbpResult* res;
  const uint64_t* firsts;
  const uint64_t* pre;
  const Checkpoint* ckpts;
  const uint64_t* carries;
  uint32_t n;
  uint64_t items;
};

// ---- launch 1 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undba_walk_kernel(const Seg* __restrict__ segs, uint32_t n, uint64_t items, Result* __restrict__ results,
                                                                         DbpSeg* __restrict__ dbp_segs, DbpResult* __restrict__ dbp_res, uint64_t* __restrict__ firsts,
                                                                         uint64_t* __restrict__ pre, Checkpoint* __restrict__ ckpts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + wave; i < n; i += (uint64_t)gridDim.x * kWaves) {
    const Seg sg = segs[i];
    uint64_t first_p = 0, first_s = 0;
    Checkpoint* mine = ckpts + sg.first_item;
    Stage rd_p(stage[wave], (uint64_t)(uintptr_t)sg.src, sg.len, lane);
    const DbpResult p = brotli_amd_undbp_walk(rd_p, sg.len, sg.cap, kItem, &first_p, [&](uint64_t j0, uint64_t j1, uint64_t off, uint64_t first) {
      for (uint64_t j = j0 + lane; j < j1; j += 64u) mine[j] = Checkpoint{off, first};
    });
    const DbpSeg seg_s = brotli_amd_undba_seg_s(sg, p.consumed);   // S begins where P's walk stopped
    mine += items;
    lds_sync();   // (the stage is taken again)
    Stage rd_s(stage[wave], (uint64_t)(uintptr_t)seg_s.src, seg_s.len, lane);
    const DbpResult s = brotli_amd_undbp_walk(rd_s, seg_s.len, sg.cap, kItem, &first_s, [&](uint64_t j0, uint64_t j1, uint64_t off, uint64_t first) {
      for (uint64_t j = j0 + lane; j < j1; j += 64u) mine[j] = Checkpoint{off, first};
    });
    if (lane == 0u) {
      results[i] = brotli_amd_undba_result(p, s, sg.len);   // (what the items add to)
      dbp_segs[i] = brotli_amd_undba_seg_p(sg); dbp_segs[n + i] = seg_s;
      dbp_res[i] = p; dbp_res[n + i] = s;
      firsts[i] = first_p; firsts[n + i] = first_s;
      pre[i] = sg.first_item;
      if (i + 1u == n) pre[n] = items;
    }
  }
}

// ---- launch 2 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undba_sum_kernel(Walked w, Tile* __restrict__ tiles) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < w.items; g += (uint64_t)gridDim.x * kWaves) {
#pragma unroll 1
    for (uint32_t half = 0; half < 2u; half++) {
      uint32_t i; uint64_t j, a; Group grp;
      uint64_t sum = 0;
      if (dbp_item_groups<kItem>(stage[wave], w.segs + half * w.n, w.n, w.res + half * w.n, w.pre, w.ckpts + half * w.items, g, lane, &i, &j, &a, &grp)) {
        sum = brotli_amd_undbp_group_sum(grp.at, grp.k, grp.min_delta, grp.nf);
#pragma unroll
        for (uint32_t off = 32; off != 0u; off >>= 1) sum += (uint64_t)__shfl_down((unsigned long long)sum, off, 64);
      }
      if (lane == 0u) tiles[half * w.items + g] = brotli_amd_undbp_tile(j, j == 0u ? w.firsts[half * w.n + i] : 0u, sum);
      lds_sync();   // (the stage is taken again)
    }
  }
}

// ---- an item's elements, a lane 32 of them (and element 0 in front of them for the first lane of a first item) ----
// The value in front of this lane's group: the item's carry-in, `first` in a segment's first item, the groups of the lanes below.
__device__ __forceinline__ uint64_t value_in_front(const Group& grp, uint64_t carry, uint64_t first, uint32_t lane) {
  const uint64_t sum = brotli_amd_undbp_group_sum(grp.at, grp.k, grp.min_delta, grp.nf);
  uint64_t inc = sum;
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint64_t q = (uint64_t)__shfl_up((unsigned long long)inc, off, 64);
    if (lane >= off) inc += q;
  }
  return carry + first + (inc - sum);
}
struct LaneElems {
  uint32_t i;        // the item's segment,
  uint64_t j;        // its place in it,
  uint64_t m;        // and the segment's delivered elements
  uint64_t lo, hi;   // the item's elements
  Group gp, gs;
  uint64_t vp, vs;   // the two values in front of this lane's first delta (element 0's in the first lane of a first item)
  uint64_t e0;       // the element behind this lane's first delta
  uint32_t nf;       // this lane's deltas that are elements of both streams
  bool lead0;        // this lane has element 0 in front of them

  __device__ __forceinline__ LaneElems(uint8_t* stage, const Walked& w, uint64_t g, uint32_t lane) {
    uint64_t a = 0, a_s = 0, j_s;
    uint32_t i_s;
    const bool dp = dbp_item_groups<kItem>(stage, w.segs, w.n, w.res, w.pre, w.ckpts, g, lane, &i, &j, &a, &gp);
    lds_sync();   // (the stage is taken again)
    const bool ds = dbp_item_groups<kItem>(stage, w.segs + w.n, w.n, w.res + w.n, w.pre, w.ckpts + w.items, g, lane, &i_s, &j_s, &a_s, &gs);
    m = brotli_amd_undba_m(w.res[i].count, w.res[w.n + i].count, w.segs[i].cap);
    brotli_amd_undba_item_elems(m, j, kItem, &lo, &hi);
    // (every lane takes part in the two scans, whatever it has)
    vp = value_in_front(gp, w.carries[g], j == 0u ? w.firsts[i] : 0u, lane);
    vs = value_in_front(gs, w.carries[w.items + g], j == 0u ? w.firsts[w.n + i] : 0u, lane);
    e0 = j * kItem + (uint64_t)kGroup * lane + 1u;
    nf = dp && ds && lo < hi ? (gp.nf < gs.nf ? gp.nf : gs.nf) : 0u;
    lead0 = j == 0u && lane == 0u && m != 0u;
  }
  // this lane's first element (where it has one)
  __device__ __forceinline__ uint64_t first_elem() const { return lead0 ? 0u : e0; }
  // each(e, p, s, d_prev) for this lane's elements, one after the other
  template <class Each>
  __device__ __forceinline__ void each(Each f) const {
    uint64_t p = vp, s = vs;
    if (lead0) f((uint64_t)0, (int32_t)(uint32_t)p, (int32_t)(uint32_t)s, (int64_t)0);
    for (uint32_t t = 0; t < nf; t++) {
      const int64_t d_prev = brotli_amd_undba_d(p, s);
      p += gp.min_delta + brotli_amd_undbp_field(gp.at, gp.k, t);
      s += gs.min_delta + brotli_amd_undbp_field(gs.at, gs.k, t);
      f(e0 + t, (int32_t)(uint32_t)p, (int32_t)(uint32_t)s, d_prev);
    }
  }
};
// what item g has in front of it of L and of s, by its second carries and first_bad (brotli_amd_undba_sum_in)
__device__ __forceinline__ void sums_in(const Walked& w, const Tile* __restrict__ tiles2, const uint64_t* __restrict__ carries2, uint64_t g, uint32_t i, uint64_t lo, uint64_t first_bad,
                                        uint64_t* bytes_in, uint64_t* suffix_in) {
  uint64_t gb = g;
  if (lo > first_bad) gb = w.pre[i] + brotli_amd_undba_item_of(first_bad, kItem);
  *bytes_in = brotli_amd_undba_sum_in(first_bad, lo, carries2[g], carries2[gb], tiles2[gb].sum);
  *suffix_in = brotli_amd_undba_sum_in(first_bad, lo, carries2[w.items + g], carries2[w.items + gb], tiles2[w.items + gb].sum);
}

// ---- launch 4 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undba_lengths_kernel(Walked w, Result* results, Tile* __restrict__ tiles2) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < w.items; g += (uint64_t)gridDim.x * kWaves) {
    const LaneElems le(stage[wave], w, g, lane);
    uint64_t sum_l = 0, sum_s = 0, bad_at = BROTLI_AMD_UNDBA_NONE;   // this lane's sums up to its first bad element
    le.each([&](uint64_t e, int32_t p, int32_t s, int64_t d_prev) {
      if (bad_at != BROTLI_AMD_UNDBA_NONE) return;
      if (brotli_amd_undba_bad_kind(p, s, d_prev) != BROTLI_AMD_UNDBA_BAD_NONE) { bad_at = e; return; }
      sum_l += (uint64_t)((int64_t)p + s); sum_s += (uint64_t)s;
    });
    uint64_t item_bad = bad_at;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t other = __shfl_xor((unsigned long long)item_bad, off);
      item_bad = other < item_bad ? other : item_bad;
    }
    if (le.first_elem() > item_bad) { sum_l = 0u; sum_s = 0u; }   // (a lane behind the item's first bad element)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sum_l += __shfl_xor((unsigned long long)sum_l, off);
      sum_s += __shfl_xor((unsigned long long)sum_s, off);
    }
    if (lane == 0u) {
      tiles2[g] = brotli_amd_undbp_tile(le.j, 0u, sum_l);
      tiles2[w.items + g] = brotli_amd_undbp_tile(le.j, 0u, sum_s);
      if (item_bad != BROTLI_AMD_UNDBA_NONE) atomicMin(reinterpret_cast<unsigned long long*>(&results[le.i].first_bad), (unsigned long long)item_bad);
    }
    lds_sync();
  }
}

// ---- launch 6 ----
__global__ __launch_bounds__(kThreads) void brotli_amd_undba_expand_kernel(Walked w, const Seg* __restrict__ segs, Result* results, const Tile* __restrict__ tiles2,
                                                                           const uint64_t* __restrict__ carries2) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][2u * kChunk];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < w.items; g += (uint64_t)gridDim.x * kWaves) {
    const LaneElems le(stage[wave], w, g, lane);
    const Seg sg = segs[le.i];
    const uint64_t first_bad = results[le.i].first_bad;
    if (le.j == 0u && lane == 0u) brotli_amd_undlba_first_offset(sg);
    uint64_t total, total_s;   // the bytes up to and with this item's elements
    sums_in(w, tiles2, carries2, g, le.i, le.lo, first_bad, &total, &total_s);
    // this lane's bytes, and with those of the lanes below and the carry-in its first offset
    uint64_t mine = 0, mine_s = 0;
    le.each([&](uint64_t e, int32_t p, int32_t s, int64_t d_prev) {
      if (e < first_bad) { mine += (uint64_t)((int64_t)p + s); mine_s += (uint64_t)s; }
      else if (e == first_bad) results[le.i].bad_kind = brotli_amd_undba_bad_kind(p, s, d_prev);
    });
    uint64_t inc = mine;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
      const uint64_t q = (uint64_t)__shfl_up((unsigned long long)inc, off, 64);
      if (lane >= off) inc += q;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine_s += __shfl_xor((unsigned long long)mine_s, off);
    uint64_t run = total + (inc - mine);
    total += (uint64_t)__shfl((unsigned long long)inc, 63, 64);
    total_s += mine_s;
    if (sg.offsets != nullptr) {   // (the same in every lane)
      // this lane's elements [e, e1); the end of element e is entry e from `ends` on: a lane's entries are neighbours, and go out as aligned
      // 16-byte words wherever it has a whole one
      const uint32_t width = brotli_amd_undlba_offset_width(sg.flags), per_word = 16u / width;
      const uint64_t ends = brotli_amd_undlba_ends_at(sg), e1 = le.e0 + le.nf;
      Word16 word;
      uint32_t in_word = 0;
      le.each([&](uint64_t at_e, int32_t p, int32_t s, int64_t) {
        if (at_e < first_bad) run += (uint64_t)((int64_t)p + s);
        const uint64_t at = ends + at_e * width;
        if (in_word == 0u && ((at & 15u) != 0u || at_e + per_word > e1)) { brotli_amd_unvarint_store(at, width, sg.offset_base + run); return; }
        word.put(in_word * width, width, sg.offset_base + run);
        if (++in_word == per_word) {
          brotli_amd_unshuffle_st128(at - (uint64_t)(per_word - 1u) * width, word.word());
          word = Word16(); in_word = 0u;
        }
      });
    }
    uint64_t a, b;
    brotli_amd_undbp_item_range(le.m, le.m, le.j, kItem, &a, &b);
    if (lane == 0u && brotli_amd_undlba_last_item(le.m, le.m, le.j, a, b)) brotli_amd_undba_finish(&results[le.i], total, total_s);
    lds_sync();
  }
}

// ---- launches 7 and 9: the item's p and s in LDS, 0 and 0 from first_bad on ----
struct ItemLens {
  uint32_t* p;
  uint32_t* s;
  __device__ __forceinline__ void fill(const LaneElems& le, uint64_t first_bad) {
    le.each([&](uint64_t e, int32_t pe, int32_t se, int64_t) {
      if (e >= le.hi) return;
      const bool good = e < first_bad;
      p[e - le.lo] = good ? (uint32_t)pe : 0u;
      s[e - le.lo] = good ? (uint32_t)se : 0u;
    });
    lds_sync();
  }
};
// an inclusive scan over the wave
__device__ __forceinline__ uint64_t scan_add(uint64_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint64_t q = (uint64_t)__shfl_up((unsigned long long)v, off, 64);
    if (lane >= off) v += q;
  }
  return v;
}
__device__ __forceinline__ uint32_t scan_min(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint32_t q = __shfl_up(v, off, 64);
    if (lane >= off) v = q < v ? q : v;
  }
  return v;
}

// ---- launch 7: PHASE A ----
__global__ __launch_bounds__(kDataThreads) void brotli_amd_undba_a_kernel(Walked w, const Seg* __restrict__ segs, const Result* __restrict__ results, const Tile* __restrict__ tiles2,
                                                                          const uint64_t* __restrict__ carries2, Last* __restrict__ lasts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kDataWaves][2u * kChunk];
  __shared__ uint32_t lens_p[kDataWaves][kItem + 1u], lens_s[kDataWaves][kItem + 1u];
  __shared__ __attribute__((aligned(16))) uint8_t strings[kDataWaves][kString];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  ItemLens lens = {lens_p[wave], lens_s[wave]};
  uint8_t* cur = strings[wave];
  for (uint64_t g = (uint64_t)blockIdx.x * kDataWaves + wave; g < w.items; g += (uint64_t)gridDim.x * kDataWaves) {
    const uint32_t i = brotli_amd_seg_find(w.pre, w.n, g);
    const Seg sg = segs[i];
    const Result res = results[i];
    const uint64_t keep = brotli_amd_undba_keep(sg, res.bytes);
    if (keep == 0u) continue;   // (nothing is stored: a measuring call, a capacity of no bytes; the same in every lane)
    const LaneElems le(stage[wave], w, g, lane);
    uint64_t bytes_in, suffix_in;
    sums_in(w, tiles2, carries2, g, i, le.lo, res.first_bad, &bytes_in, &suffix_in);
    lens.fill(le, res.first_bad);
    const uint32_t ne = (uint32_t)(le.hi - le.lo);
    const uint64_t data = (uint64_t)(uintptr_t)sg.data, suffixes = (uint64_t)(uintptr_t)sg.src + res.consumed_p + res.consumed_s, avail = res.data_avail;
    Last last = {bytes_in, 0u, 0u};
    uint32_t r_in = ~0u;
    for (uint32_t x0 = 0; x0 < ne; x0 += 64u) {
      // 64 elements' places: a lane an element
      const uint32_t x = x0 + lane, pe = x < ne ? lens.p[x] : 0u, se = x < ne ? lens.s[x] : 0u;
      const uint64_t len = (uint64_t)pe + se, ends = scan_add(len, lane), suffix_ends = scan_add(se, lane);
      const uint64_t at = bytes_in + (ends - len), q = suffix_in + (suffix_ends - se);
      uint32_t r = scan_min(x < ne ? pe : ~0u, lane);
      r = r < r_in ? r : r_in;
      const uint32_t nb = ne - x0 < 64u ? ne - x0 : 64u;
      // ... and the elements one after the other, a lane a byte
      for (uint32_t t = 0; t < nb; t++) {
        const uint32_t p_t = same(__shfl(pe, t, 64)), len_t = same(__shfl((uint32_t)len, t, 64)), r_t = same(__shfl(r, t, 64));
        const uint64_t at_t = (uint64_t)__shfl((unsigned long long)at, t, 64), q_t = (uint64_t)__shfl((unsigned long long)q, t, 64);
        // (only what is stored: the work follows min(bytes, data_cap), never a declared length; nothing behind `keep` is read again)
        const uint64_t end_t = brotli_amd_undba_stored(at_t, len_t, keep);
        for (uint64_t k64 = (uint64_t)r_t + lane; k64 < end_t; k64 += 64u) {
          const uint32_t k = (uint32_t)k64;
          const uint32_t byte = brotli_amd_undba_a_byte(lens.p, lens.s, cur, kString, x0 + t, q_t, k, suffixes, avail);
          brotli_amd_undba_put(data, keep, at_t + k, byte);
          if (k >= p_t && k < kString) cur[k] = (uint8_t)byte;
        }
        lds_sync();   // (the next element reads what this one put into the string)
        if (t + 1u == nb) last = Last{at_t, len_t, r_t};
      }
      bytes_in += (uint64_t)__shfl((unsigned long long)ends, 63, 64);
      suffix_in += (uint64_t)__shfl((unsigned long long)suffix_ends, 63, 64);
      r_in = __shfl(r, 63, 64);
    }
    if (lane == 0u) lasts[g] = last;
    lds_sync();   // (the next item's p and s)
  }
}

// ---- launch 8: PHASE B ----
__global__ __launch_bounds__(64) void brotli_amd_undba_b_kernel(Walked w, const Seg* __restrict__ segs, const Result* __restrict__ results, const Last* __restrict__ lasts) {
  __shared__ __attribute__((aligned(16))) uint8_t cur[kCarry];
  const uint32_t lane = threadIdx.x;
  for (uint64_t i = blockIdx.x; i < w.n; i += gridDim.x) {
    const Seg sg = segs[i];
    const uint64_t keep = brotli_amd_undba_keep(sg, results[i].bytes), data = (uint64_t)(uintptr_t)sg.data;
    if (keep == 0u) continue;
    const Last* mine = lasts + w.pre[i];
    const uint64_t items = w.pre[i + 1u] - w.pre[i];
    for (uint64_t j = 0; j < items; j++) {
      const Last me = mine[j];
      const uint32_t r = j != 0u ? me.r : 0u;
      const uint32_t stored = (uint32_t)brotli_amd_undba_stored(me.at, r, keep);   // (only what is stored)
      for (uint32_t k = lane; k < stored; k += 64u)
        brotli_amd_undba_put(data, keep, me.at + k, k < kCarry ? cur[k] : brotli_amd_undba_far_byte(mine, j, k, data, keep));
      lds_sync();
      // what launch 7 stored of this element goes behind what was carried into it
      const uint32_t end = me.len < kCarry ? me.len : kCarry;
      for (uint32_t k = r + lane; k < end; k += 64u) cur[k] = me.at + k < keep ? (uint8_t)brotli_amd_unshuffle_ld8(data + me.at + k) : 0u;   // (end <= kCarry)
      lds_sync();
    }
  }
}

// ---- launch 9: PHASE C ----
__global__ __launch_bounds__(kDataThreads) void brotli_amd_undba_c_kernel(Walked w, const Seg* __restrict__ segs, const Result* __restrict__ results, const Tile* __restrict__ tiles2,
                                                                          const uint64_t* __restrict__ carries2, const Last* __restrict__ lasts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kDataWaves][2u * kChunk];
  __shared__ uint32_t lens_p[kDataWaves][kItem + 1u], lens_s[kDataWaves][kItem + 1u];
  __shared__ uint64_t run_ends[kDataWaves][64], places[kDataWaves][64];
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  ItemLens lens = {lens_p[wave], lens_s[wave]};
  for (uint64_t g = (uint64_t)blockIdx.x * kDataWaves + wave; g < w.items; g += (uint64_t)gridDim.x * kDataWaves) {
    const uint32_t i = brotli_amd_seg_find(w.pre, w.n, g);
    if (g == w.pre[i]) continue;   // (a segment's first item has nothing in front of it)
    const Seg sg = segs[i];
    const Result res = results[i];
    const uint64_t keep = brotli_amd_undba_keep(sg, res.bytes);
    if (keep == 0u) continue;
    const LaneElems le(stage[wave], w, g, lane);
    uint64_t bytes_in, suffix_in;
    sums_in(w, tiles2, carries2, g, i, le.lo, res.first_bad, &bytes_in, &suffix_in);
    lens.fill(le, res.first_bad);
    const uint32_t ne = (uint32_t)(le.hi - le.lo);
    const uint64_t data = (uint64_t)(uintptr_t)sg.data, from = data + lasts[g - 1u].at;
    uint32_t r_in = ~0u;
    for (uint32_t x0 = 0; x0 + 1u < ne; x0 += 64u) {
      const uint32_t x = x0 + lane, pe = x < ne ? lens.p[x] : 0u, se = x < ne ? lens.s[x] : 0u;
      const uint64_t len = (uint64_t)pe + se, ends = scan_add(len, lane);
      uint32_t r = scan_min(x < ne ? pe : ~0u, lane);
      r = r < r_in ? r : r_in;
      const uint64_t place = bytes_in + (ends - len);
      const uint64_t todo = x + 1u < ne ? brotli_amd_undba_stored(place, r, keep) : 0u, todo_ends = scan_add(todo, lane);   // (the item's last element is launch 8's)
      run_ends[wave][lane] = todo_ends;
      places[wave][lane] = place;
      lds_sync();
      const uint64_t all = run_ends[wave][63];
      for (uint64_t t = lane; t < all; t += 64u) {
        uint32_t el = 0;   // the first element whose bytes end behind t
#pragma unroll
        for (uint32_t step = 32; step != 0u; step >>= 1)
          if (run_ends[wave][el + step - 1u] <= t) el += step;
        const uint64_t k = t - (el != 0u ? run_ends[wave][el - 1u] : 0u), at = places[wave][el] + k;
        if (at < keep) brotli_amd_undba_put(data, keep, at, brotli_amd_unshuffle_ld8(from + k));
      }
      bytes_in += (uint64_t)__shfl((unsigned long long)ends, 63, 64);
      r_in = __shfl(r, 63, 64);
      lds_sync();
    }
    lds_sync();
  }
}

// the scratch, carved
struct Scratch {
  Result* results;
  DbpResult* dbp_res;
  DbpSeg* dbp_segs;
  uint64_t* firsts;
  uint64_t* pre;
  Checkpoint* ckpts;
  Tile* tiles;
  uint64_t* carries;
  Tile* tiles2;
  uint64_t* carries2;
  Last* lasts;
  static uint64_t bytes(uint64_t items, uint32_t n) {
    return pad16((uint64_t)n * sizeof(Result)) + pad16(2u * (uint64_t)n * sizeof(DbpResult)) + pad16(2u * (uint64_t)n * sizeof(DbpSeg)) + pad16(2u * (uint64_t)n * sizeof(uint64_t)) +
           brotli_amd_wave::pre_bytes(n) + items * (2u * sizeof(Checkpoint) + 4u * sizeof(Tile) + 4u * sizeof(uint64_t) + sizeof(Last));
  }
  Scratch(void* d_scratch, uint64_t items, uint32_t n) {
    uint8_t* at = static_cast<uint8_t*>(d_scratch);
    results = reinterpret_cast<Result*>(at); at += pad16((uint64_t)n * sizeof(Result));
    dbp_res = reinterpret_cast<DbpResult*>(at); at += pad16(2u * (uint64_t)n * sizeof(DbpResult));
    dbp_segs = reinterpret_cast<DbpSeg*>(at); at += pad16(2u * (uint64_t)n * sizeof(DbpSeg));
    firsts = reinterpret_cast<uint64_t*>(at); at += pad16(2u * (uint64_t)n * sizeof(uint64_t));
    pre = reinterpret_cast<uint64_t*>(at); at += brotli_amd_wave::pre_bytes(n);
    ckpts = reinterpret_cast<Checkpoint*>(at); at += 2u * items * sizeof(Checkpoint);
    tiles = reinterpret_cast<Tile*>(at); at += 2u * items * sizeof(Tile);
    tiles2 = reinterpret_cast<Tile*>(at); at += 2u * items * sizeof(Tile);
    lasts = reinterpret_cast<Last*>(at); at += items * sizeof(Last);
    carries = reinterpret_cast<uint64_t*>(at); at += 2u * items * sizeof(uint64_t);
    carries2 = reinterpret_cast<uint64_t*>(at);
  }
};

}  // namespace

// the scratch of a launch over `units` units of n segments -- a unit a segment and a unit an item
extern "C" uint64_t brotli_amd_undba_scratch_bytes(uint64_t units, uint32_t n) { return pad16(Scratch::bytes(units - n, n)); }
extern "C" uint32_t brotli_amd_undba_lds_string(void) { return kString; }
extern "C" uint32_t brotli_amd_undba_lds_carry(void) { return kCarry; }

// d_table: the n segments; units: n + the items of all segments (the host has the table); d_scratch: brotli_amd_undba_scratch_bytes of device
// memory, 16-byte aligned; ev[0..9], where not NULL, are recorded in front of, between and behind the nine launches.  A call without items is
// the walk alone.
extern "C" hipError_t brotli_amd_launch_undba(const void* d_table, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  if (n == 0u) return hipSuccess;
  const Seg* d_segs = static_cast<const Seg*>(d_table);
  const uint64_t items = units - n;
  const Scratch s(d_scratch, items, n);
  hipError_t e = hipSuccess;
  uint32_t grid = 0, data_grid = 0, seg_grid = 0;
  if (items != 0u && (e = hipMemsetAsync(s.ckpts, 0xFF, (size_t)(2u * items) * sizeof(Checkpoint), stream)) != hipSuccess) return e;
  if ((e = brotli_amd_wave::wave_grid(n, kWaves, &grid)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(brotli_amd_undba_walk_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n, items, s.results, s.dbp_segs, s.dbp_res, s.firsts, s.pre, s.ckpts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
  const Walked w = {s.dbp_segs, s.dbp_res, s.firsts, s.pre, s.ckpts, s.carries, n, items};
  const Result* results = s.results;
  const Tile* tiles2 = s.tiles2;
  const uint64_t* carries2 = s.carries2;
  const Last* lasts = s.lasts;
  if (items != 0u) {
    if ((e = brotli_amd_wave::wave_grid(items, kWaves, &grid)) != hipSuccess) return e;
    if ((e = brotli_amd_wave::wave_grid(items, kDataWaves, &data_grid)) != hipSuccess) return e;
    if ((e = brotli_amd_wave::wave_grid(n, 1u, &seg_grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(brotli_amd_undba_sum_kernel, dim3(grid), dim3(kThreads), 0, stream, w, s.tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
  if (items != 0u && (e = brotli_amd_launch_tile_carries(s.tiles, s.carries, 2u * items, stream)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[3], stream)) != hipSuccess) return e;
  if (items != 0u) {
    hipLaunchKernelGGL(brotli_amd_undba_lengths_kernel, dim3(grid), dim3(kThreads), 0, stream, w, s.results, s.tiles2);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[4], stream)) != hipSuccess) return e;
  if (items != 0u && (e = brotli_amd_launch_tile_carries(s.tiles2, s.carries2, 2u * items, stream)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[5], stream)) != hipSuccess) return e;
  if (items != 0u) {
    hipLaunchKernelGGL(brotli_amd_undba_expand_kernel, dim3(grid), dim3(kThreads), 0, stream, w, d_segs, s.results, tiles2, carries2);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[6], stream)) != hipSuccess) return e;
  if (items != 0u) {
    hipLaunchKernelGGL(brotli_amd_undba_a_kernel, dim3(data_grid), dim3(kDataThreads), 0, stream, w, d_segs, results, tiles2, carries2, s.lasts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[7], stream)) != hipSuccess) return e;
  if (items != 0u) {
    hipLaunchKernelGGL(brotli_amd_undba_b_kernel, dim3(seg_grid), dim3(64), 0, stream, w, d_segs, results, lasts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[8], stream)) != hipSuccess) return e;
  if (items != 0u) {
    hipLaunchKernelGGL(brotli_amd_undba_c_kernel, dim3(data_grid), dim3(kDataThreads), 0, stream, w, d_segs, results, tiles2, carries2, lasts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[9], stream)) != hipSuccess) return e;
  return hipSuccess;
}
