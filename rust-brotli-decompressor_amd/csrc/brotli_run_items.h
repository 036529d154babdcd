// brotli_run_items.h -- what the kernels of the filters that WALK a segment and then take its ITEMS have in common (gfx950, wave64): unrle,
// undbp, undict and unnull (csrc/brotli_<name>_kernels.hip).  Every one of them is a serial walk, one wave a segment, that leaves a checkpoint
// an item, and then one wave an item, in two launches (unrle, undict) or in four with undelta's carry launch between two of them (undbp,
// unnull).  Here, once:
//   RunBatch, RunCursor   the runs that cover an item, up to 64 at a time in LDS, and a lane's way through them (unrle's grammar: unrle,
//                         undict, unnull)
//   walk_segments         the walk kernels' frame: the waves over the table, the lanes over the checkpoints of a stretch, the prefix array
//   ItemScratch           the scratch behind the table, carved
//   launch_walk_expand, launch_walk_count_carry_expand   the two launcher bodies
// What a filter's kernels keep is the filter's: which walk, which column beside the results, what a lane does with its elements.
#ifndef BROTLI_AMD_RUN_ITEMS_H_
#define BROTLI_AMD_RUN_ITEMS_H_

#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_unrle.h"        // a run, where a walk stands, brotli_amd_unvarint_store
#include "brotli_wave_stage.h"   // Stage, Word16, lds_sync, same, wave_grid

// (csrc/brotli_undelta_kernels.hip)
extern "C" hipError_t brotli_amd_launch_tile_carries(const BrotliAmdUndeltaTile* tiles, uint64_t* carries, uint64_t ntiles, hipStream_t stream);

namespace brotli_amd_wave {

constexpr uint32_t kSegThreads = BROTLI_AMD_SEG_THREADS, kSegWaves = kSegThreads / 64u;
constexpr uint32_t kRunBatch = 64;   // runs collected at a time

// ---- the runs that cover an item ----
// A batch of runs in the wave's three LDS arrays: first[r] is the first element of run r and first[nr] the batch's end (kRunBatch + 1
// entries); payload[r] is the run's payload offset, BROTLI_AMD_UNRLE_NONE for an RLE run, whose value is value[r].
struct RunBatch {
  uint64_t* first;
  uint64_t* payload;
  uint32_t* value;
  uint64_t lo;   // the batch's first element (its end: st.elems behind collect)
  uint32_t nr;   // its runs

  __device__ __forceinline__ RunBatch(uint64_t* first_, uint64_t* payload_, uint32_t* value_) : first(first_), payload(payload_), value(value_), lo(0u), nr(0u) {}

  // The next runs from st on, up to kRunBatch of them and up to element e1, fields of k bits in a segment of len bytes behind rd: every lane
  // walks, lane 0 keeps.  st goes behind them; `more` goes false where the runs end (a stop is not below count).
  __device__ __forceinline__ void collect(Stage& rd, uint64_t len, uint32_t k, BrotliAmdUnrleWalk& st, bool& more, uint64_t e1, uint32_t lane) {
    lo = st.elems;
    uint32_t got = 0;
    lds_sync();   // (the batch before is done with)
    while (more && got < kRunBatch && st.elems < e1) {
      rd.ensure(st.off);
      const BrotliAmdUnrleRun run = brotli_amd_unrle_run(rd, len, k, st);
      if (run.kind == BROTLI_AMD_UNRLE_STOP) { more = false; break; }
      if (lane == 0u) {
        first[got] = st.elems;
        payload[got] = run.kind == BROTLI_AMD_UNRLE_RLE ? BROTLI_AMD_UNRLE_NONE : run.payload;
        value[got] = run.value;
      }
      got++;
      st.off = run.next; st.elems += run.count;
      more = run.status == BROTLI_AMD_UNRLE_OK;
    }
    if (lane == 0u) first[got] = st.elems;
    lds_sync();
    nr = got;
  }
  // the run that holds element a of the batch
  __device__ __forceinline__ uint32_t find(uint64_t a) const {
    uint32_t r = 0, hi = nr;
    while (hi - r > 1u) { const uint32_t m = (r + hi) >> 1; if (first[m] <= a) r = m; else hi = m; }
    return r;
  }
};

// A lane's way through a batch, forward only, from the run that holds element a: run r is the elements [first, end); with kValues its payload
// and value are kept beside them.
template <bool kValues>
struct RunCursor {
  const RunBatch& batch;
  uint32_t r;
  uint64_t first, end, payload;
  uint32_t value;

  __device__ __forceinline__ RunCursor(const RunBatch& b, uint64_t a)
      : batch(b), r(b.find(a)), first(b.first[r]), end(b.first[r + 1u]), payload(kValues ? b.payload[r] : 0u), value(kValues ? b.value[r] : 0u) {}
  // to the run that holds element e, not in front of where it stands -> whether it moved
  __device__ __forceinline__ bool seek(uint64_t e) {
    bool moved = false;
    while (e >= end) {
      r++; first = end; end = batch.first[r + 1u];
      if (kValues) { payload = batch.payload[r]; value = batch.value[r]; }
      moved = true;
    }
    return moved;
  }
};

// ---- the walk kernels' frame ----
// One wave a segment, the waves striding over the table.  walk(sg, rd, mark) walks segment sg -- rd: this wave's stage over its len bytes at
// src -- and calls mark(j0, j1, off, first) for the items [j0, j1) whose checkpoint is (off, first): the lanes stride over them.  What it
// returns goes to keep(i, sg, ...) in lane 0, which writes the segment's result; the segment's entry of the items' prefix array, and the
// array's end behind the last segment, are written here.
template <class Checkpoint, class Seg, class Walk, class Keep>
__device__ __forceinline__ void walk_segments(uint8_t (*stage)[2u * kStageChunk], const Seg* segs, uint32_t n, uint64_t items, uint64_t* pre, Checkpoint* ckpts, Walk walk,
                                              Keep keep) {
  const uint32_t lane = threadIdx.x & 63u, wave = same(threadIdx.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * kSegWaves + wave; i < n; i += (uint64_t)gridDim.x * kSegWaves) {
    const Seg sg = segs[i];
    Stage rd(stage[wave], (uint64_t)(uintptr_t)sg.src, sg.len, lane);
    Checkpoint* mine = ckpts + sg.first_item;
    const auto got = walk(sg, rd, [&](uint64_t j0, uint64_t j1, uint64_t off, uint64_t first) {
      for (uint64_t j = j0 + lane; j < j1; j += 64u) mine[j] = Checkpoint{off, first};
    });
    if (lane == 0u) {
      keep(i, sg, got);
      pre[i] = sg.first_item;
      if (i + 1u == n) pre[n] = items;
    }
  }
}

// ---- the scratch behind the table, and the launchers ----
constexpr uint64_t pad16(uint64_t bytes) { return (bytes + 15u) & ~(uint64_t)15; }
constexpr uint64_t pre_bytes(uint32_t n) { return pad16(((uint64_t)n + 1u) * sizeof(uint64_t)); }

// The scratch of a launch over n segments and `items` items, in this order, every per-segment part padded to 16 bytes: the n results, with
// kColumn one uint64_t a segment, the items' prefix array (n + 1 entries), a checkpoint an item, and with kCarried a tile record and a carry an
// item.
template <class Result, class Checkpoint, bool kColumn, bool kCarried>
struct ItemScratch {
  Result* results;
  uint64_t* column;
  uint64_t* pre;
  Checkpoint* ckpts;
  BrotliAmdUndeltaTile* tiles;
  uint64_t* carries;

  static_assert(kColumn || sizeof(Result) % 16u == 0u, "the results' padding is none where the prefix array follows them");

  static uint64_t bytes(uint64_t items, uint32_t n) {
    return pad16((uint64_t)n * sizeof(Result)) + (kColumn ? pad16((uint64_t)n * sizeof(uint64_t)) : 0u) + pre_bytes(n) +
           items * (sizeof(Checkpoint) + (kCarried ? sizeof(BrotliAmdUndeltaTile) + sizeof(uint64_t) : 0u));
  }
  ItemScratch(void* d_scratch, uint64_t items, uint32_t n) {
    uint8_t* at = static_cast<uint8_t*>(d_scratch);
    results = reinterpret_cast<Result*>(at); at += pad16((uint64_t)n * sizeof(Result));
    column = kColumn ? reinterpret_cast<uint64_t*>(at) : nullptr; at += kColumn ? pad16((uint64_t)n * sizeof(uint64_t)) : 0u;
    pre = reinterpret_cast<uint64_t*>(at); at += pre_bytes(n);
    ckpts = reinterpret_cast<Checkpoint*>(at); at += items * sizeof(Checkpoint);
    tiles = kCarried ? reinterpret_cast<BrotliAmdUndeltaTile*>(at) : nullptr; at += kCarried ? items * sizeof(BrotliAmdUndeltaTile) : 0u;
    carries = kCarried ? reinterpret_cast<uint64_t*>(at) : nullptr;
  }
};

// The walk's launch of both shapes: the checkpoints set to NONE (all bits), ev[0], the walk over the n segments, ev[1].
template <class Seg, class Checkpoint, class Walk, class... Columns>
inline hipError_t launch_walk(Walk walk, const Seg* d_segs, uint32_t n, uint64_t items, Checkpoint* ckpts, hipStream_t stream, const hipEvent_t* ev, Columns... columns) {
  hipError_t e = hipSuccess;
  uint32_t grid = 0;
  if (items != 0u && (e = hipMemsetAsync(ckpts, 0xFF, (size_t)items * sizeof(Checkpoint), stream)) != hipSuccess) return e;
  if ((e = wave_grid(n, kSegWaves, &grid)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(walk, dim3(grid), dim3(kSegThreads), 0, stream, d_segs, n, items, columns..., ckpts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
  return hipSuccess;
}

// Two launches in stream order over a table of n segments and units - n items: walk(segs, n, items, results, pre, ckpts), then, where there
// are items, expand with the same arguments.  ev[0..2], where not NULL, are recorded in front of, between and behind them.
template <class Seg, class Result, class Checkpoint, class Walk, class Expand>
inline hipError_t launch_walk_expand(Walk walk, Expand expand, const void* d_table, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  if (n == 0u) return hipSuccess;
  const Seg* d_segs = static_cast<const Seg*>(d_table);
  const uint64_t items = units - n;
  const ItemScratch<Result, Checkpoint, false, false> s(d_scratch, items, n);
  hipError_t e = launch_walk(walk, d_segs, n, items, s.ckpts, stream, ev, s.results, s.pre);
  if (e != hipSuccess) return e;
  if (items != 0u) {
    uint32_t grid = 0;
    if ((e = wave_grid(items, kSegWaves, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(expand, dim3(grid), dim3(kSegThreads), 0, stream, d_segs, n, items, s.results, s.pre, s.ckpts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
  return hipSuccess;
}

// Four launches in stream order: walk(segs, n, items, results, column, pre, ckpts), then, where there are items, count(.., ckpts, tiles),
// undelta's carry launch over the tile records, and expand(.., ckpts, carries).  ev[0..4], where not NULL, are recorded in front of, between
// and behind them.
template <class Seg, class Result, class Checkpoint, class Walk, class Count, class Expand>
inline hipError_t launch_walk_count_carry_expand(Walk walk, Count count, Expand expand, const void* d_table, uint32_t n, uint64_t units, void* d_scratch,
                                                 hipStream_t stream, const hipEvent_t* ev) {
  if (n == 0u) return hipSuccess;
  const Seg* d_segs = static_cast<const Seg*>(d_table);
  const uint64_t items = units - n;
  const ItemScratch<Result, Checkpoint, true, true> s(d_scratch, items, n);
  hipError_t e = launch_walk(walk, d_segs, n, items, s.ckpts, stream, ev, s.results, s.column, s.pre);
  if (e != hipSuccess) return e;
  uint32_t grid = 0;
  if (items != 0u) {
    if ((e = wave_grid(items, kSegWaves, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(count, dim3(grid), dim3(kSegThreads), 0, stream, d_segs, n, items, s.results, s.column, s.pre, s.ckpts, s.tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
  if (items != 0u && (e = brotli_amd_launch_tile_carries(s.tiles, s.carries, items, stream)) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[3], stream)) != hipSuccess) return e;
  if (items != 0u) {
    hipLaunchKernelGGL(expand, dim3(grid), dim3(kSegThreads), 0, stream, d_segs, n, items, s.results, s.column, s.pre, s.ckpts, s.carries);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[4], stream)) != hipSuccess) return e;
  return hipSuccess;
}

}  // namespace brotli_amd_wave

#endif  // BROTLI_AMD_RUN_ITEMS_H_
