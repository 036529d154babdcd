// brotli_seg_call.cpp -- what the calls over a table of segments share on the host (brotli_digest.cpp, brotli_filters.cpp):
// the last decode call's outputs as segments (the call itself is run_seg_call in brotli_host.h), and the segment walk of csrc/brotli_seg_walk.h on the host, for tests without a device.
#include "brotli_host.h"
#include "brotli_seg_walk.h"

namespace brotli_amd_host {

// The delivered bytes of every stream of the last decode call (brotli_host.h)
bool delivered_outputs(BrotliAmdBatch* b, std::vector<DeliveredBytes>* outs) {
  outs->clear();
  if (b->packed_valid) {   // a packed call: its buffer and offsets
    for (size_t i = 0; i + 1 < b->packed_offsets.size(); i++)
      outs->push_back(DeliveredBytes{b->packed_out + b->packed_offsets[i], b->packed_offsets[i + 1] - b->packed_offsets[i]});
    return true;
  }
  if (b->outputs == BrotliAmdBatch::Outputs::NoCall) { g_last_error = "no decode call on this batch object yet"; return false; }
  if (b->outputs == BrotliAmdBatch::Outputs::Failed) { g_last_error = "the last decode call on this batch object failed: it has no outputs"; return false; }
  if (b->outputs == BrotliAmdBatch::Outputs::InFlight) { g_last_error = "the last launch has not been waited for (BrotliAmdBatchWait)"; return false; }
  // the streams' own buffers (the staging arena's slots after a host call), as far as each was delivered
  if (b->outputs == BrotliAmdBatch::Outputs::Waited)
    for (uint32_t i = 0; i < b->n; i++)
      outs->push_back(DeliveredBytes{b->h_descs[i].out, std::min<uint64_t>(b->h_status[i].decoded_size, b->h_descs[i].out_cap)});
  return true;
}

}  // namespace brotli_amd_host

// Test hook (no device needed; not in batch.h): the parts that the blocks of a grid of `grid` take of n segments of units[i] units with tiles of
// tile_units, in the order block by block -- parts[4 k ..] = (block, tile, lo, hi) of the first `cap` of them.  -> the number of parts.
extern "C" __attribute__((visibility("default"))) uint64_t BrotliAmdDebugSegWalkParts(uint32_t n, const uint64_t* units, uint32_t tile_units, uint32_t grid,
                                                                                       uint64_t* parts, uint64_t cap) {
  uint64_t count = 0;
  if ((n && !units) || tile_units == 0u || (cap && !parts)) return 0;
  brotli_amd_seg_walk_model(units, n, tile_units, grid, [&](uint32_t block, uint64_t tile, uint64_t lo, uint64_t hi) {
    if (count < cap) { parts[4u * count] = block; parts[4u * count + 1u] = tile; parts[4u * count + 2u] = lo; parts[4u * count + 3u] = hi; }
    count++;
  });
  return count;
}
