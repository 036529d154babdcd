// brotli_undelta.cpp -- undelta on the device (include/brotli/batch.h): the deltas of n segments of device memory back into values, a wrapping
// running sum per segment, in three launches (BrotliAmdBatchUndeltaSegments), those of the delivered bytes of every stream of the last decode call
// (BrotliAmdBatchUndeltaOutputs), and the three phases of csrc/brotli_undelta.h on the host, tile by tile, for tests without a device.
#include "brotli_undelta.h"
#include "brotli_host.h"

#include <numeric>

// (csrc/brotli_undelta_kernels.hip: units: the segments' units together; ev: four events around and between the three launches)
extern "C" hipError_t brotli_amd_launch_undelta(const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream,
                                                const hipEvent_t* ev);
extern "C" uint64_t brotli_amd_undelta_scratch_bytes(uint64_t units);
extern "C" uint32_t brotli_amd_undelta_tile_bytes(void);
extern "C" uint32_t brotli_amd_undelta_carry_span(void);

using namespace brotli_amd_host;

namespace {

bool known_width(uint32_t width) {
  if (brotli_amd_unshuffle_width_ok(width)) return true;
  g_last_error = "undelta width is not 1, 2, 4 or 8";
  return false;
}

// in place is allowed at an address that is a multiple of the width only: there a unit reads exactly the bytes it writes
bool placed_ok(uint64_t src, uint64_t dst, uint32_t width) {
  if (src != dst || dst % width == 0u) return true;
  g_last_error = "undelta in place at an address that is not a multiple of the width";
  return false;
}

bool seg_ok(const void* src, const void* dst, uint32_t width) { return known_width(width) && placed_ok((uint64_t)(uintptr_t)src, (uint64_t)(uintptr_t)dst, width); }

void no_times(BrotliAmdBatch* b) { b->undelta_ms = 0.0f; for (float& ms : b->undelta_phase_ms) ms = 0.0f; }

// segs on `stream`, waited for (the widths and the placement were checked)
int undelta_device(BrotliAmdBatch* b, const std::vector<BrotliAmdUnshuffleSeg>& segs, hipStream_t stream) {
  if (segs.empty()) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const uint32_t n = (uint32_t)segs.size();
  const uint64_t units = width_segments_units(segs);
  if (units == 0u) return 0;   // (segments without bytes: nothing to launch)
  // behind the table: the tiles' summaries and carries -- it grows with the launch
  return run_seg_call(&b->undelta, {"hipMalloc(undelta segments and tiles)", "hipMemcpyAsync(undelta segments)", "hipStreamSynchronize(undelta)"}, segs.data(),
                      sizeof(BrotliAmdUnshuffleSeg) * n, brotli_amd_undelta_scratch_bytes(units), 4u, stream, [&](uint8_t* d_segs, uint8_t* d_scratch, const hipEvent_t* ev) {
    return hip_ok(brotli_amd_launch_undelta(reinterpret_cast<BrotliAmdUnshuffleSeg*>(d_segs), n, units, d_scratch, stream, ev), "brotli_amd_undelta kernels launch");
  }, &b->undelta_ms, b->undelta_phase_ms);
}

}  // namespace

extern "C" int BrotliAmdBatchUndeltaSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, void* const* d_dst, const size_t* lens,
                                             const uint8_t* widths, void* hip_stream) {
  if (!b || (n && (!d_src || !d_dst || !lens || !widths))) { g_last_error = "invalid undelta arguments"; return -1; }
  no_times(b);
  std::vector<BrotliAmdUnshuffleSeg> segs;
  if (!width_segments(n, d_src, d_dst, lens, widths, seg_ok, &segs)) return -1;
  return undelta_device(b, segs, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchUndeltaOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint8_t* widths) {
  if (!b || !d_dst || !widths) { g_last_error = "invalid undelta arguments"; return -1; }
  no_times(b);
  std::vector<BrotliAmdUnshuffleSeg> segs;
  if (!width_segments_of_outputs(b, d_dst, widths, seg_ok, &segs)) return -1;
  return undelta_device(b, segs, b->last_stream);
}

extern "C" float BrotliAmdBatchLastUndeltaMs(BrotliAmdBatch* b) { return b ? b->undelta_ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndeltaPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return b && phase >= 1u && phase <= 3u ? b->undelta_phase_ms[phase - 1u] : 0.0f; }
extern "C" uint32_t BrotliAmdDebugUndeltaTile(void) { return brotli_amd_undelta_tile_bytes(); }
extern "C" uint32_t BrotliAmdDebugUndeltaCarrySpan(void) { return brotli_amd_undelta_carry_span(); }

// The three phases on the host over n segments given as offsets into one source and one destination buffer, which are placed at their skews past
// a 16-byte boundary in rooms of this function's own, among bytes that are not theirs (whole foreign words in front and behind as well).  In
// place: one room, filled from src, with the segments at their DESTINATION offsets.
extern "C" int BrotliAmdDebugUndeltaHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                         const uint64_t* dst_offs, const uint64_t* lens, const uint8_t* widths, uint32_t src_skew, uint32_t dst_skew,
                                         uint32_t tile_units, uint32_t order_seed, int in_place) {
  if ((n && (!src_offs || !dst_offs || !lens || !widths)) || (src_size && !src) || (dst_size && !dst) || src_skew > 15u || dst_skew > 15u ||
      (in_place && src_size != dst_size)) {
    g_last_error = "invalid undelta arguments";
    return -1;
  }
  for (uint32_t i = 0; i < n; i++) {
    if (!known_width(widths[i])) return -1;
    if (lens[i] > dst_size || dst_offs[i] > dst_size - lens[i] || lens[i] > src_size || (!in_place && src_offs[i] > src_size - lens[i])) {
      g_last_error = "invalid undelta arguments: a segment outside its buffer";
      return -1;
    }
  }
  if (tile_units == 0u) tile_units = brotli_amd_undelta_tile_bytes() / 16u;
  std::vector<uint8_t> sroom(in_place ? 0u : src_size + 64u, 0xA5), droom(dst_size + 64u, 0x5A);
  const uint64_t d_at = (((uint64_t)(uintptr_t)droom.data() + 15u) & ~(uint64_t)15) + 16u + dst_skew;
  const uint64_t s_at = in_place ? d_at : (((uint64_t)(uintptr_t)sroom.data() + 15u) & ~(uint64_t)15) + 16u + src_skew;
  if (src_size) std::memcpy(reinterpret_cast<void*>((uintptr_t)s_at), src, src_size);
  std::vector<BrotliAmdUnshuffleSeg> segs(n);
  std::vector<uint64_t> pre(n + 1u, 0u);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t s = s_at + (in_place ? dst_offs[i] : src_offs[i]), d = d_at + dst_offs[i];
    if (!placed_ok(s, d, widths[i])) return -1;
    segs[i] = BrotliAmdUnshuffleSeg{reinterpret_cast<const uint8_t*>((uintptr_t)s), reinterpret_cast<uint8_t*>((uintptr_t)d), lens[i], widths[i], 0u};
    pre[i + 1u] = pre[i] + brotli_amd_seg_units(d, lens[i]);
  }
  const std::vector<uint8_t> before = droom;
  const uint64_t units = pre[n], ntiles = (units + tile_units - 1u) / tile_units;
  // phases 1 and 3 take the tiles in an order shuffled by the seed: the result may not depend on it
  std::vector<uint64_t> order(ntiles);
  std::iota(order.begin(), order.end(), (uint64_t)0);
  uint32_t rnd = order_seed * 2654435761u + 1u;
  auto shuffle = [&]() {
    if (order_seed == 0u) return;
    for (uint64_t i = ntiles; i > 1u; i--) { rnd = rnd * 1664525u + 1013904223u; std::swap(order[i - 1u], order[(rnd >> 8) % i]); }
  };
  auto tile_end = [&](uint64_t t) { return std::min<uint64_t>((t + 1u) * tile_units, units); };
  std::vector<BrotliAmdUndeltaTile> tiles(ntiles);
  std::vector<uint64_t> carries(ntiles);
  shuffle();
  for (uint64_t t : order) tiles[t] = brotli_amd_undelta_host_summary(segs.data(), pre.data(), n, t * tile_units, tile_end(t));
  BrotliAmdUndeltaPair out = {0u, 0u};
  for (uint64_t t = 0; t < ntiles; t++) {
    carries[t] = brotli_amd_undelta_carry_in(out.sum, tiles[t]);
    out = brotli_amd_undelta_combine(out, brotli_amd_undelta_tile_pair(tiles[t]));
  }
  shuffle();
  for (uint64_t t : order) brotli_amd_undelta_host_apply(segs.data(), pre.data(), n, t * tile_units, tile_end(t), carries[t]);
  // no byte outside every segment's destination may have changed
  std::vector<uint8_t> inside(droom.size(), 0);
  const size_t off = (size_t)(d_at - (uint64_t)(uintptr_t)droom.data());
  for (uint32_t i = 0; i < n; i++) std::fill(inside.begin() + off + dst_offs[i], inside.begin() + off + dst_offs[i] + lens[i], 1);
  for (size_t i = 0; i < droom.size(); i++)
    if (!inside[i] && droom[i] != before[i]) { g_last_error = "undelta wrote outside its destination"; return -2; }
  for (uint32_t i = 0; i < n; i++)
    if (lens[i]) std::memcpy(dst + dst_offs[i], reinterpret_cast<const void*>((uintptr_t)(d_at + dst_offs[i])), lens[i]);
  return 0;
}
