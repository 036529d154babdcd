// brotli_launch_plan.h -- the shape of every decode launch: grid, waves per block, table arena, gangs and pools, whether the device is asked
// first what kind the streams are, and what a later pass over the streams that came back looks like.  Pure functions of their arguments: no
// HIP call, no getenv, nothing of the batch object -- the host (csrc/brotli_batch.cpp: submit(), retry_with_larger_arenas()) applies what
// they say, and BrotliAmdDebugPlanLaunch / BrotliAmdDebugPlanLaterPass / BrotliAmdDebugPlanGangs hand them to tests on machines without a GPU
// (tests/test_launch_plan_cpu.py holds plans recorded from real launches).
#ifndef BROTLI_AMD_LAUNCH_PLAN_H_
#define BROTLI_AMD_LAUNCH_PLAN_H_
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "brotli_device_abi.h"

// What BrotliAmdBatchCreate learned of the device and of the object's configuration (plain words: ctypes fills it in tests).
struct BrotliAmdPlanDevice {
  uint32_t cus;             // compute units
  uint32_t lds_per_cu;      // bytes of LDS a CU has
  uint32_t block_max;       // largest LDS a block may ask for (at most 64 KiB)
  uint32_t lds_fixed;       // a block's fixed carve
  uint32_t lds_helper4, lds_helper8, lds_helper16;   // what the helper waves of a block of 4 / 8 / 16 waves add
  uint32_t lds_arena;       // the configured table arena (a four-wave block's)
  uint32_t max_arena;       // the arena of the last pass: the largest block the device allows
  uint32_t grid_max;        // blocks of the configured arena the device holds (or the caller's grid_blocks)
  uint32_t retry_grid_max;  // blocks of the largest arena it holds
  uint32_t auto_arena;      // 1: no lds_arena_bytes given, the arena follows the batch
  uint32_t engine_ok;       // 1: the device's LDS holds a sixteen-wave block with a command engine, and none has been refused since
};

// The environment's knobs, as numbers (csrc/brotli_batch.cpp: launch_knobs() reads them, and says when).
struct BrotliAmdPlanKnobs {
  // read once per process
  uint32_t max_blocks_per_cu;   // BROTLI_AMD_MAX_BLOCKS_PER_CU (14): one-wave blocks per CU at most -- a CU's registers hold sixteen waves of the kernel
  uint32_t min_small_arena;     // BROTLI_AMD_MIN_SMALL_ARENA (3584): the smallest table arena worth a first pass (16 blocks per CU: 4016 bytes)
  uint32_t no_scan;             // BROTLI_AMD_NO_SCAN: no command engine (BrotliAmdBatchCreate: engine_ok)
  uint32_t no_engine_queue;     // BROTLI_AMD_NO_ENGINE_QUEUE: no sixteen-wave blocks for more streams than CUs
  uint32_t engine_queue_max;    // BROTLI_AMD_ENGINE_QUEUE_MAX (4): streams per CU up to which such blocks take them one after the other
  uint32_t no_record_blocks;    // BROTLI_AMD_NO_RECORD_BLOCKS: no four-wave blocks for large batches of text
  uint32_t no_order;            // BROTLI_AMD_NO_ORDER: the blocks take the streams as they come
  // read on every call (tests flip them inside one process)
  int32_t gang;                 // BROTLI_AMD_GANG (-1 unset; 0, 1: nothing at all; 2, 4, 8, 16: gangs of at most that many, no pool)
  int32_t pool;                 // BROTLI_AMD_POOL (-1 unset; 0: no pool; 2: a pool whatever the sizes where there would be no gangs)
  uint32_t gang_no_helpers;     // BROTLI_AMD_GANG_NO_HELPERS: a gang's helper blocks leave at once (launch(): queue word 6)
  uint32_t debug_probe;         // BROTLI_AMD_DEBUG_PROBE: submit() prints the probe's kinds
};

// What a launch is to look like.  Where want_probe is set the plan is the PROBE launch's (grid, waves, arena), and the planner is asked again
// with the kinds the probe found.
struct BrotliAmdLaunchPlan {
  uint32_t grid, waves, arena;
  uint32_t cur_per_cu;     // blocks per CU this first pass was shaped for (0: the configured arena or larger)
  uint32_t gang;           // the queue's gang word: 0, 2 / 4 / 8 / 16, or 0x108 for a pool
  uint32_t ordered;        // the blocks take the streams longest first
  uint32_t want_probe;     // ask the device first what kind the streams are
  uint32_t engine_queue;   // streams of kind 7 get BROTLI_AMD_FLAG_ENGINE_ONLY, all others BROTLI_AMD_FLAG_DEFER
  uint32_t no_spill;       // streams without BROTLI_AMD_BATCH_SPILL_IN_PLACE get BROTLI_AMD_FLAG_NO_SPILL: a larger arena exists
};

// A later pass over what came back (BROTLI_AMD_RESULT_RETRY_ARENA): its level (blocks per CU), and whether it is the last, which may spill.
struct BrotliAmdLaterPass {
  uint32_t level, arena, grid_max, waves, last;
};

namespace brotli_amd_plan {

constexpr size_t kGang16MinBytes = (size_t)2 << 20;   // compressed bytes of a batch's largest stream from which a gang is sixteen blocks (plan_gangs)
constexpr uint32_t kGangPool = BROTLI_AMD_GANG_POOL_FLAG | 8u;   // plan_gangs' word for a pool launch (queue[2])
constexpr uint64_t kProbeMinMeanBytes = 8192;     // mean compressed size of a batch from which the device is asked what kind its streams are
constexpr uint32_t kEngineQueueMaxPerCu = 4;      // streams per CU up to which blocks of sixteen waves, one a CU, take a batch's streams one after the other -- where the
                                                  // DEVICE says they are a command engine's kind (probe_streams); beyond, streams in flight beat the engine (2048 x 1 MiB of the
                                                  // metric's make-up: 220 GB/s eight to a CU in one-wave blocks, 151 through engine blocks)
constexpr uint32_t kScanArena = 40960;  // table arena of a sixteen-wave block (with the engine's rings: about 108 KiB of LDS)

// Table arena of one-wave blocks packed per_cu to a CU (0: too small to be worth a pass).
inline uint32_t small_arena(const BrotliAmdPlanDevice& d, const BrotliAmdPlanKnobs& k, uint32_t per_cu) {
  const uint32_t per_block = (d.lds_per_cu / per_cu) & ~255u;
  return per_block > d.lds_fixed + k.min_small_arena ? (per_block - d.lds_fixed) & ~15u : 0u;
}

// Many streams in flight: one-wave blocks, several a CU, with a small arena -- how many a CU for n streams (0: not worth it, four-wave blocks
// with the configured arena instead) and their arena.  What does not fit such an arena comes back in a later pass.
inline uint32_t many_blocks_per_cu(const BrotliAmdPlanDevice& d, const BrotliAmdPlanKnobs& k, uint32_t per_cu_cap, uint32_t n, uint32_t* arena) {
  const uint32_t per_cu = (uint32_t)std::min<size_t>(per_cu_cap, ((size_t)n + d.cus - 1) / d.cus);  // blocks per CU wanted
  const uint32_t a = per_cu > 4u ? small_arena(d, k, per_cu) : 0u;
  if (a == 0u || a >= d.lds_arena) return 0u;
  *arena = a;
  return per_cu;
}

// Several blocks on a stream (csrc/brotli_path_engine.h, path_engine<false, true>): what a launch of sixteen-wave blocks, one a stream, gets on top.
// Returns 0 (nothing), 2 / 4 / 8 / 16 (GANGS: that many blocks a stream, dealt at the launch -- its owner and one, three or seven helper blocks that take
// the path engine's regions in turns with it; eight streams' gangs side by side, a gang's members eight block numbers apart: one XCD; streams beyond a
// multiple of eight leave their gangs' blocks without work) or 0x108 (a POOL: as many blocks as CUs; a block without a stream of its own -- at once where
// there are fewer streams than CUs, else when its stream is done -- joins the largest stream still being decoded), and the launch's blocks in *grid.
//   * Not for batches of small streams: a gang has something to divide from a dozen regions on -- 64 KiB of compressed data --, and costs a launch ten
//     microseconds (its blocks' start, the control blocks' zeroing, the helpers' last look at the word that lets them go).
//   * Gangs of eight up to an eighth of the CUs' streams, of four up to a quarter, of two up to half; of SIXTEEN up to a sixteenth where a stream is long
//     (kGang16MinBytes compressed: eight blocks on one long stream are busy building and consuming, not waiting -- one 64 MiB stream 26.6 -> 24.3 ms,
//     one of 1 GiB 387 -> 356 ms; streams of the metric's 4 MiB gain nothing: their invocations are a dozen regions).
//   * A pool where the sizes differ -- the largest more than twice the median, and a long pole worth it: 256 KiB compressed, a millisecond and more
//     alone -- and the gangs would be of four or two blocks or none: the long one gets seven helpers (one 64 MiB stream among 39 / 99 / 199 of 1 MiB:
//     43.5 / 76.7 / 127.6 -> 29 ms).  Not where the streams are of a size: they end within a few per cent of each other, and the control blocks'
//     zeroing and the owners' looks at them cost what the last invocations' help brings (a pool forced on 192 x 4 MiB: +1 %, on 250 x 4 MiB: -4 %).
// gang_env, pool_env: BrotliAmdPlanKnobs' gang and pool.
inline uint32_t plan_gangs(uint32_t n, uint32_t cus, const size_t* in_sizes, int gang_env, int pool_env, uint32_t* grid) {
  if (n == 0u || n > cus || gang_env == 0 || gang_env == 1) return 0u;
  size_t largest_in = 0;
  for (uint32_t i = 0; i < n; i++) largest_in = std::max<size_t>(largest_in, in_sizes[i]);
  if (largest_in < 65536u) return 0u;
  uint32_t gang = 0u;
  const uint32_t groups = (n + 7u) / 8u;
  uint32_t m = groups * 64u <= cus ? 8u : groups * 32u <= cus ? 4u : groups * 16u <= cus ? 2u : 0u;
  // (round 6) sixteen blocks a stream where the device has them and a stream is long enough to keep them busy -- 2 MiB compressed, a few hundred regions:
  // eight blocks on one long stream are BUSY (96 % of the launch building their windows' tables and taking their regions through), not waiting for one another
  if (m == 8u && groups * 128u <= cus && largest_in >= kGang16MinBytes) m = 16u;
  if (gang_env > 1 && m > (uint32_t)gang_env) m = gang_env >= 16 ? 16u : gang_env >= 8 ? 8u : gang_env >= 4 ? 4u : 2u;
  if (gang_env == 16 && groups * 128u <= cus) m = 16u;   // (experiments: sixteen whatever the sizes)
  if (m > 1u) { gang = m; *grid = groups * 8u * m; }
  if (m < 8u && pool_env != 0 && gang_env < 0) {
    std::vector<size_t> sz(in_sizes, in_sizes + n);
    std::nth_element(sz.begin(), sz.begin() + n / 2, sz.end());
    if ((largest_in > 2u * sz[n / 2] && largest_in >= (256u << 10)) || (pool_env == 2 && m == 0u)) { gang = kGangPool; *grid = cus; }
  }
  return gang;
}

// The first launch of a batch of n streams (n != 0).  per_cu_cap: the object's present limit of blocks per CU; size_at(i): stream i's
// compressed bytes; kinds: the probe's answer for every stream (probe_streams), or nullptr where the device has not been asked.
template <class SizeAt>
BrotliAmdLaunchPlan plan_launch(const BrotliAmdPlanDevice& d, const BrotliAmdPlanKnobs& k, uint32_t per_cu_cap, uint32_t n, SizeAt&& size_at,
                                const uint8_t* kinds) {
  BrotliAmdLaunchPlan p = {};
  // The arena: the configured one, or a smaller one when the batch has more streams than the device can hold blocks of the configured size
  // (more waves in flight; what does not fit goes to a later pass).
  p.arena = d.lds_arena;
  uint32_t grid_max = d.grid_max;
  if (d.auto_arena && n > d.grid_max && d.max_arena > d.lds_arena) {
    uint32_t arena = 0;
    const uint32_t per_cu = many_blocks_per_cu(d, k, per_cu_cap, n, &arena);
    if (per_cu != 0u) { p.arena = arena; grid_max = d.cus * per_cu; p.cur_per_cu = per_cu; }
  }
  p.grid = std::min(n, grid_max);
  // Waves per block: one decoding wave plus helpers for long literal runs.  A CU's registers hold sixteen waves of this
  // kernel: eight-wave blocks where at most two blocks per CU are wanted, four-wave blocks up to four, one-wave blocks
  // beyond (streams in flight are worth more than helpers there).
  p.waves = p.grid > 4u * d.cus ? 1u : 4u;
  if (p.grid <= 2u * d.cus) {
    const uint32_t room = std::min(d.block_max, d.lds_per_cu / 2u);
    if (d.auto_arena && room > d.lds_fixed + d.lds_helper8 + d.lds_arena) { p.arena = (room - d.lds_fixed - d.lds_helper8) & ~15u; p.waves = 8; }
    else if (d.lds_fixed + d.lds_helper8 + p.arena <= room) p.waves = 8;
  }
  // Up to three large streams per CU: sixteen-wave blocks, one per CU, take them one after the other (the command engine
  // decodes a stream 3.5x faster than one wave does; measured on 384 / 512 x 4 MiB of the metric's data: 61 / 81 GB/s
  // against 33 / 44 with two eight-wave blocks per CU, while 1024 streams are faster four to a CU).  Metablocks the
  // engine cannot take go back and continue in a launch of small blocks (BROTLI_AMD_FLAG_ENGINE_ONLY).
  // (whether a block of sixteen waves fits is settled first: only then is the grid cut down to one block per CU)
  uint32_t arena16 = 0;
  bool can16 = false;
  if (d.engine_ok) {
    const size_t room = d.lds_per_cu > (size_t)d.lds_fixed + d.lds_helper16 ? (size_t)d.lds_per_cu - d.lds_fixed - d.lds_helper16 : 0;
    arena16 = d.auto_arena ? (uint32_t)std::min<size_t>(kScanArena, room & ~(size_t)15) : p.arena;
    can16 = arena16 <= room && (!d.auto_arena || arena16 >= 16384u);
  }
  // (round 6) ... and beyond that many: one-wave blocks, fourteen a CU -- unless the streams are the RECORD LOOP's: context-modelled ones and text (the probe's
  // kinds 5 and 15), which four-wave blocks, four a CU, taking the streams off the queue one after the other, decode half as fast again as fourteen
  // one-wave blocks a CU do (4096 x alice29: 13.2 -> 19+ GB/s; 4096 x lcet10 at -q 5: 16.6 -> 24+): the same probe says which
  const bool few = n <= k.engine_queue_max * d.cus;
  bool engine_queue = false, record_blocks = false;
  if (d.auto_arena && p.grid > d.cus && (few ? can16 && !k.no_engine_queue : !k.no_record_blocks)) {
    // more streams than CUs, few enough for engine blocks to pay where the streams are the engines' kind: the device says which are.
    // Not for batches of small streams (a mean of less than 8 KiB compressed: an engine has nothing to spread out, and the probe -- a
    // launch and a wait on the caller's stream -- would cost such a batch more than its decode).
    uint64_t in_total = 0;
    for (uint32_t i = 0; i < n; i++) in_total += size_at(i);
    if (in_total >= (uint64_t)n * kProbeMinMeanBytes) {
      if (kinds == nullptr) { p.want_probe = 1; return p; }   // (the probe's launch: the shape so far)
      uint64_t in_engine = 0, in_rec = 0;
      for (uint32_t i = 0; i < n; i++) {
        if (kinds[i] == 7u) in_engine += size_at(i);   // (15: the engines' kind but for its short commands -- text)
        else if (kinds[i] == 5u || kinds[i] == 15u) in_rec += size_at(i);
      }
      if (few) { if (in_engine * 2u >= in_total && in_engine != 0u) { engine_queue = true; p.grid = d.cus; p.cur_per_cu = 0; } }
      else record_blocks = in_rec * 2u >= in_total && in_rec != 0u;
    }
  }
  if (record_blocks) { p.arena = d.lds_arena; p.cur_per_cu = 0; p.grid = std::min(n, d.grid_max); p.waves = 4u; }
  if (can16 && p.grid <= d.cus) { p.arena = arena16; p.waves = 16; }
  // Fewer streams than half the CUs: GANGS of blocks, a CU each, on one stream -- its owner and one, three or seven helper blocks that take
  // the path engine's regions in turns with it (csrc/brotli_path_engine.h, path_engine<false, true>).  Eight streams' gangs are launched side by side,
  // a gang's members eight block numbers apart (one XCD); streams beyond a multiple of eight leave their gangs' blocks without work.
  if (p.waves == 16u && d.auto_arena && p.arena <= 49152u && n <= d.cus) {
    std::vector<size_t> sz(n);
    for (uint32_t i = 0; i < n; i++) sz[i] = size_at(i);
    p.gang = plan_gangs(n, d.cus, sz.data(), k.gang, k.pool, &p.grid);
  }
  // (the engines' streams to the engine blocks; the others wait for the launch of small blocks behind it)
  p.engine_queue = engine_queue && p.waves == 16u;
  // where a larger arena exists, tables that do not fit this one are a reason to come back, not to spill
  p.no_spill = p.arena < d.max_arena;
  // more streams than blocks: the blocks take them longest first (compressed size as the measure), so that no block starts
  // a long stream when the others are done
  p.ordered = n > p.grid && !k.no_order;
  return p;
}

// The pass after one of `level` blocks per CU (0: the first pass had the configured arena already) whose arena was cur_arena, for m streams that
// came back: a first pass packed more than eight blocks to a CU is followed by one with eight, then by the configured arena, then by the largest
// block the device allows, where spilling to global memory is allowed.  deferred: the streams were sent back unread by an engine launch
// (BROTLI_AMD_FLAG_DEFER) and get the launch of small blocks they were promised -- the shape plan_launch gives m streams without engine blocks.
inline BrotliAmdLaterPass plan_later_pass(const BrotliAmdPlanDevice& d, const BrotliAmdPlanKnobs& k, uint32_t per_cu_cap, uint32_t level,
                                          uint32_t cur_arena, uint32_t m, bool deferred) {
  if (deferred) {
    uint32_t arena = 0;
    const uint32_t per_cu = many_blocks_per_cu(d, k, per_cu_cap, m, &arena);
    if (per_cu != 0u) return BrotliAmdLaterPass{per_cu, arena, d.cus * per_cu, 1u, 0u};
    return BrotliAmdLaterPass{4u, d.lds_arena, d.grid_max, 4u, 0u};
  }
  if (level > 8u && small_arena(d, k, 8) > cur_arena) return BrotliAmdLaterPass{8u, small_arena(d, k, 8), d.cus * 8u, 1u, 0u};
  if (level > 4u && d.lds_arena > cur_arena) return BrotliAmdLaterPass{4u, d.lds_arena, d.grid_max, 4u, 0u};
  return BrotliAmdLaterPass{2u, d.max_arena, d.retry_grid_max, 4u, 1u};
}

}  // namespace brotli_amd_plan
#endif  // BROTLI_AMD_LAUNCH_PLAN_H_
