// brotli_bitunshuffle.cpp -- bit-unshuffle on the device (include/brotli/batch.h): the bit planes of n segments of device memory back into elements
// in one launch (BrotliAmdBatchBitUnshuffleSegments), those of the delivered bytes of every stream of the last decode call
// (BrotliAmdBatchBitUnshuffleOutputs), and the functions of csrc/brotli_bitunshuffle.h on the host, tile by tile and slot by slot as the kernel's
// lanes take them, for tests without a device.
#include "brotli_bitunshuffle.h"
#include "brotli_host.h"

// (csrc/brotli_bitunshuffle_kernels.hip: units: the segments' units together)
extern "C" hipError_t brotli_amd_launch_bitunshuffle(const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, hipStream_t stream);
extern "C" uint32_t brotli_amd_bitunshuffle_tile_bytes(void);

using namespace brotli_amd_host;

namespace {

bool known_width(uint32_t width) {
  if (brotli_amd_unshuffle_width_ok(width)) return true;
  g_last_error = "bit-unshuffle width is not 1, 2, 4 or 8";
  return false;
}
bool known_block(uint32_t block) {
  if (brotli_amd_bitunshuffle_block_ok(block)) return true;
  g_last_error = "bit-unshuffle block_elems is neither 0 nor a multiple of 8";
  return false;
}

// segs on `stream`, waited for (the widths and blocks were checked)
int bitunshuffle_device(BrotliAmdBatch* b, const std::vector<BrotliAmdUnshuffleSeg>& segs, hipStream_t stream) {
  if (segs.empty()) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const uint32_t n = (uint32_t)segs.size();
  const uint64_t units = width_segments_units(segs);
  if (units == 0u) return 0;   // (segments without bytes: nothing to launch)
  return run_seg_call(&b->bitunshuffle, {"hipMalloc(bit-unshuffle segments)", "hipMemcpyAsync(bit-unshuffle segments)", "hipStreamSynchronize(bit-unshuffle)"},
                      segs.data(), sizeof(BrotliAmdUnshuffleSeg) * n, 0u, 2u, stream, [&](uint8_t* d_segs, uint8_t*, const hipEvent_t* ev) {
    return hip_ok(hipEventRecord(ev[0], stream), "hipEventRecord") &&
           hip_ok(brotli_amd_launch_bitunshuffle(reinterpret_cast<BrotliAmdUnshuffleSeg*>(d_segs), n, units, stream), "brotli_amd_bitunshuffle_kernel launch") &&
           hip_ok(hipEventRecord(ev[1], stream), "hipEventRecord");
  }, &b->bitunshuffle_ms);
}

}  // namespace

extern "C" int BrotliAmdBatchBitUnshuffleSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, void* const* d_dst, const size_t* lens,
                                                  const uint8_t* widths, const uint32_t* block_elems, void* hip_stream) {
  if (!b || (n && (!d_src || !d_dst || !lens || !widths))) { g_last_error = "invalid bit-unshuffle arguments"; return -1; }
  b->bitunshuffle_ms = 0.0f;
  std::vector<BrotliAmdUnshuffleSeg> segs;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t block = block_elems ? block_elems[i] : 0u;
    if (!known_width(widths[i]) || !known_block(block)) return -1;
    segs.push_back(BrotliAmdUnshuffleSeg{static_cast<const uint8_t*>(d_src[i]), static_cast<uint8_t*>(d_dst[i]), lens[i], widths[i], block});
  }
  return bitunshuffle_device(b, segs, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchBitUnshuffleOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint8_t* widths, const uint32_t* block_elems) {
  if (!b || !d_dst || !widths) { g_last_error = "invalid bit-unshuffle arguments"; return -1; }
  b->bitunshuffle_ms = 0.0f;
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  std::vector<BrotliAmdUnshuffleSeg> segs;
  for (size_t i = 0; i < outs.size(); i++) {
    if (d_dst[i] == nullptr) continue;   // (a stream the caller does not want: its width and block are not looked at)
    const uint32_t block = block_elems ? block_elems[i] : 0u;
    if (!known_width(widths[i]) || !known_block(block)) return -1;
    segs.push_back(BrotliAmdUnshuffleSeg{outs[i].ptr, static_cast<uint8_t*>(d_dst[i]), outs[i].len, widths[i], block});
  }
  return bitunshuffle_device(b, segs, b->last_stream);
}

extern "C" float BrotliAmdBatchLastBitUnshuffleMs(BrotliAmdBatch* b) { return b ? b->bitunshuffle_ms : 0.0f; }
extern "C" uint32_t BrotliAmdDebugBitUnshuffleTile(void) { return brotli_amd_bitunshuffle_tile_bytes(); }

// The device's functions on the host over every unit of the segment: source and destination placed at their skews past a 16-byte boundary, among
// bytes that are not theirs (whole foreign words in front and behind as well).  The work is taken as the kernel takes a tile inside one segment:
// tile after tile of the segment's units, in each the slots in the lanes' order.
extern "C" int BrotliAmdDebugBitUnshuffleHost(uint32_t width, uint32_t block_elems, const uint8_t* src, size_t len, uint8_t* dst, uint32_t src_skew,
                                              uint32_t dst_skew, uint64_t* fast_items) {
  if (!known_width(width) || !known_block(block_elems)) return -1;
  if ((len && (!src || !dst)) || src_skew > 15u || dst_skew > 15u) { g_last_error = "invalid bit-unshuffle arguments"; return -1; }
  std::vector<uint8_t> sroom(len + 64u, 0xA5), droom(len + 64u, 0x5A);
  const uint64_t s_at = (((uint64_t)(uintptr_t)sroom.data() + 15u) & ~(uint64_t)15) + 16u + src_skew;
  const uint64_t d_at = (((uint64_t)(uintptr_t)droom.data() + 15u) & ~(uint64_t)15) + 16u + dst_skew;
  if (len) std::memcpy(reinterpret_cast<void*>((uintptr_t)s_at), src, len);
  const std::vector<uint8_t> before = droom;
  const uint64_t units = brotli_amd_seg_units(d_at, len), tile = brotli_amd_bitunshuffle_tile_bytes() / 16u, slot = 2u * width;
  uint64_t items = 0;
  for (uint64_t t0 = 0; t0 < units; t0 += tile) {
    const uint64_t t1 = std::min(t0 + tile, units);
    for (uint64_t s = t0 / slot; slot * s < t1; s++) {
      const uint64_t ka = std::max(slot * s, t0), kb = std::min(slot * (s + 1u), t1);
      items += brotli_amd_bitunshuffle_range(s_at, d_at, len, width, block_elems, ka, kb);
    }
  }
  if (fast_items) *fast_items = items;
  // no byte beside the destination may have changed
  const size_t off = (size_t)(d_at - (uint64_t)(uintptr_t)droom.data());
  for (size_t i = 0; i < droom.size(); i++)
    if ((i < off || i >= off + len) && droom[i] != before[i]) { g_last_error = "bit-unshuffle wrote outside its destination"; return -2; }
  if (len) std::memcpy(dst, reinterpret_cast<const void*>((uintptr_t)d_at), len);
  return 0;
}
