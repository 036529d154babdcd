// brotli_unshuffle.cpp -- unshuffle on the device (include/brotli/batch.h): the byte planes of n segments of device memory back into elements in
// one launch (BrotliAmdBatchUnshuffleSegments), those of the delivered bytes of every stream of the last decode call
// (BrotliAmdBatchUnshuffleOutputs), and the unit function of csrc/brotli_unshuffle.h on the host, unit by unit, for tests without a device.
#include "brotli_unshuffle.h"
#include "brotli_host.h"

// (csrc/brotli_unshuffle_kernels.hip: units: the segments' units together)
extern "C" hipError_t brotli_amd_launch_unshuffle(const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, hipStream_t stream);
extern "C" uint32_t brotli_amd_unshuffle_tile_bytes(void);

using namespace brotli_amd_host;

namespace {

bool known_width(uint32_t width) {
  if (brotli_amd_unshuffle_width_ok(width)) return true;
  g_last_error = "unshuffle width is not 1, 2, 4 or 8";
  return false;
}
bool seg_ok(const void*, const void*, uint32_t width) { return known_width(width); }

// segs on `stream`, waited for (the widths were checked)
int unshuffle_device(BrotliAmdBatch* b, const std::vector<BrotliAmdUnshuffleSeg>& segs, hipStream_t stream) {
  if (segs.empty()) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const uint32_t n = (uint32_t)segs.size();
  const uint64_t units = width_segments_units(segs);
  if (units == 0u) return 0;   // (segments without bytes: nothing to launch)
  return run_seg_call(&b->unshuffle, {"hipMalloc(unshuffle segments)", "hipMemcpyAsync(unshuffle segments)", "hipStreamSynchronize(unshuffle)"}, segs.data(),
                      sizeof(BrotliAmdUnshuffleSeg) * n, 0u, 2u, stream, [&](uint8_t* d_segs, uint8_t*, const hipEvent_t* ev) {
    return hip_ok(hipEventRecord(ev[0], stream), "hipEventRecord") &&
           hip_ok(brotli_amd_launch_unshuffle(reinterpret_cast<BrotliAmdUnshuffleSeg*>(d_segs), n, units, stream), "brotli_amd_unshuffle_kernel launch") &&
           hip_ok(hipEventRecord(ev[1], stream), "hipEventRecord");
  }, &b->unshuffle_ms);
}

}  // namespace

extern "C" int BrotliAmdBatchUnshuffleSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, void* const* d_dst, const size_t* lens,
                                               const uint8_t* widths, void* hip_stream) {
  if (!b || (n && (!d_src || !d_dst || !lens || !widths))) { g_last_error = "invalid unshuffle arguments"; return -1; }
  b->unshuffle_ms = 0.0f;
  std::vector<BrotliAmdUnshuffleSeg> segs;
  if (!width_segments(n, d_src, d_dst, lens, widths, seg_ok, &segs)) return -1;
  return unshuffle_device(b, segs, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchUnshuffleOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint8_t* widths) {
  if (!b || !d_dst || !widths) { g_last_error = "invalid unshuffle arguments"; return -1; }
  b->unshuffle_ms = 0.0f;
  std::vector<BrotliAmdUnshuffleSeg> segs;
  if (!width_segments_of_outputs(b, d_dst, widths, seg_ok, &segs)) return -1;
  return unshuffle_device(b, segs, b->last_stream);
}

extern "C" float BrotliAmdBatchLastUnshuffleMs(BrotliAmdBatch* b) { return b ? b->unshuffle_ms : 0.0f; }
extern "C" uint32_t BrotliAmdDebugUnshuffleTile(void) { return brotli_amd_unshuffle_tile_bytes(); }

// The device's unit function on the host over every unit of the segment: source and destination placed at their skews past a 16-byte boundary,
// among bytes that are not theirs (whole foreign words in front and behind as well).
extern "C" int BrotliAmdDebugUnshuffleHost(uint32_t width, const uint8_t* src, size_t len, uint8_t* dst, uint32_t src_skew, uint32_t dst_skew) {
  if (!known_width(width)) return -1;
  if ((len && (!src || !dst)) || src_skew > 15u || dst_skew > 15u) { g_last_error = "invalid unshuffle arguments"; return -1; }
  std::vector<uint8_t> sroom(len + 64u, 0xA5), droom(len + 64u, 0x5A);
  const uint64_t s_at = (((uint64_t)(uintptr_t)sroom.data() + 15u) & ~(uint64_t)15) + 16u + src_skew;
  const uint64_t d_at = (((uint64_t)(uintptr_t)droom.data() + 15u) & ~(uint64_t)15) + 16u + dst_skew;
  if (len) std::memcpy(reinterpret_cast<void*>((uintptr_t)s_at), src, len);
  const std::vector<uint8_t> before = droom;
  const uint64_t units = brotli_amd_seg_units(d_at, len);
  // (two units a step, as a lane takes them in a tile inside one segment; odd `len`s of units end in a single one)
  for (uint64_t k = 0; k < units; k += 2u) brotli_amd_unshuffle_two_units(s_at, d_at, len, width, k, units);
  // no byte beside the destination may have changed
  const size_t off = (size_t)(d_at - (uint64_t)(uintptr_t)droom.data());
  for (size_t i = 0; i < droom.size(); i++)
    if ((i < off || i >= off + len) && droom[i] != before[i]) { g_last_error = "unshuffle wrote outside its destination"; return -2; }
  if (len) std::memcpy(dst, reinterpret_cast<const void*>((uintptr_t)d_at), len);
  return 0;
}
