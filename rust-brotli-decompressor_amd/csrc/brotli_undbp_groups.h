// brotli_undbp_groups.h -- an item of a DELTA_BINARY_PACKED stream as one wave takes it (device only; gfx950, wave64): from the item's
// checkpoint the wave reads the few block headers that cover the item again and gives each lane ONE GROUP of 32 fields.  Shared by the kernels
// whose items are undbp's: csrc/brotli_undbp_kernels.hip and csrc/brotli_undlba_kernels.hip.
#ifndef BROTLI_AMD_UNDBP_GROUPS_H_
#define BROTLI_AMD_UNDBP_GROUPS_H_

#include <hip/hip_runtime.h>

#include "brotli_seg_walk.h"
#include "brotli_undbp.h"
#include "brotli_wave_stage.h"

namespace brotli_amd_wave {

// a lane's group: nf (0 .. 32) fields of k bits from the address `at` on, under min_delta
struct DbpGroup { uint64_t at, min_delta; uint32_t k, nf; };

// item g of the flat list: its segment i and its place j in it; the groups of its deltas [a, b), this lane's being *mine.  False: the item has
// no deltas.  Seg has src, len and cap, Result undbp's count, block_values and miniblocks.
template <uint32_t kItem, class Seg, class Result>
__device__ __forceinline__ bool dbp_item_groups(uint8_t* lds, const Seg* __restrict__ segs, uint32_t n, const Result* __restrict__ results, const uint64_t* __restrict__ pre,
                                                const BrotliAmdUndbpCheckpoint* __restrict__ ckpts, uint64_t g, uint32_t lane, uint32_t* i_out, uint64_t* j_out, uint64_t* a_out,
                                                DbpGroup* mine) {
  constexpr uint32_t kGroup = BROTLI_AMD_UNDBP_GROUP;
  const uint32_t i = brotli_amd_seg_find(pre, n, g);
  const uint64_t j = g - pre[i];
  *i_out = i; *j_out = j;
  *mine = DbpGroup{0u, 0u, 0u, 0u};
  const BrotliAmdUndbpCheckpoint cp = ckpts[g];
  if (cp.off == BROTLI_AMD_UNDBP_NONE) return false;   // (beyond count; the same in every lane)
  const Seg sg = segs[i];
  const Result res = results[i];
  uint64_t a, b;
  brotli_amd_undbp_item_range(res.count, sg.cap, j, kItem, &a, &b);
  *a_out = a;
  if (a >= b) return false;
  const uint64_t src = (uint64_t)(uintptr_t)sg.src, gl = a + (uint64_t)kGroup * lane;   // this lane's first delta
  Stage rd(lds, src, sg.len, lane);
  DbpGroup got = {0u, 0u, 0u, 0u};
  brotli_amd_undbp_item_blocks(rd, sg.len, res.block_values / res.miniblocks, res.miniblocks, cp, a, b, [&](uint64_t lo, uint64_t hi, uint64_t pos, uint32_t k, uint64_t md, uint64_t m0) {
    if (gl >= lo && gl < hi) got = DbpGroup{src + pos + (gl - m0) / 8u * k, md, k, (uint32_t)(hi - gl < kGroup ? hi - gl : kGroup)};
  });
  *mine = got;
  return true;
}

}  // namespace brotli_amd_wave

#endif  // BROTLI_AMD_UNDBP_GROUPS_H_
