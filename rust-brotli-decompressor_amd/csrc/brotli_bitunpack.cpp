// brotli_bitunpack.cpp -- bit-unpack on the device (include/brotli/batch.h): the k-bit fields of n segments of device memory back into elements in
// one launch (BrotliAmdBatchBitUnpackSegments), those of the delivered bytes of every stream of the last decode call
// (BrotliAmdBatchBitUnpackOutputs), and the functions of csrc/brotli_bitunpack.h on the host, tile by tile and slot by slot as the kernel's lanes
// take them, for tests without a device.
#include "brotli_bitunpack.h"
#include "brotli_host.h"

// (csrc/brotli_bitunpack_kernels.hip: units: the segments' units together)
extern "C" hipError_t brotli_amd_launch_bitunpack(const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, hipStream_t stream);
extern "C" uint32_t brotli_amd_bitunpack_tile_bytes(void);

using namespace brotli_amd_host;

namespace {

// k bits into w bytes by these flags; `who` names the segment or stream in the text
bool known_shape(uint32_t bits, uint32_t width, uint32_t flags, const char* who, size_t i) {
  const char* what = nullptr;
  if (!brotli_amd_unshuffle_width_ok(width)) what = "width is not 1, 2, 4 or 8";
  else if (bits == 0u) what = "field of 0 bits";
  else if (bits > 8u * width) what = "field is wider than the element";
  else if ((flags & ~BROTLI_AMD_BITUNPACK_FLAGS) != 0u) what = "unknown flag bits";
  if (!what) return true;
  g_last_error = std::string("bit-unpack ") + who + " " + std::to_string(i) + ": " + what + " (bits " + std::to_string(bits) + ", width " + std::to_string(width) +
                 ", flags " + std::to_string(flags) + ")";
  return false;
}
// `count` fields of `bits` bits lie in src_len bytes
bool known_count(uint64_t count, uint32_t bits, uint64_t src_len, const char* who, size_t i) {
  if (count > BROTLI_AMD_BITUNPACK_MAX_COUNT) {
    g_last_error = std::string("bit-unpack ") + who + " " + std::to_string(i) + ": a count of " + std::to_string(count) + " elements is above 2^56";
    return false;
  }
  if (brotli_amd_bitunpack_src_bytes(count, bits) > src_len) {
    g_last_error = std::string("bit-unpack ") + who + " " + std::to_string(i) + ": " + std::to_string(count) + " fields of " + std::to_string(bits) + " bits need " +
                   std::to_string(brotli_amd_bitunpack_src_bytes(count, bits)) + " source bytes, and there are " + std::to_string(src_len);
    return false;
  }
  return true;
}

BrotliAmdUnshuffleSeg segment(const void* src, void* dst, uint64_t count, uint32_t bits, uint32_t width, uint32_t flags) {
  return BrotliAmdUnshuffleSeg{static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), count * width, width, brotli_amd_bitunpack_param(bits, flags)};
}

// segs on `stream`, waited for (the shapes and counts were checked)
int bitunpack_device(BrotliAmdBatch* b, const std::vector<BrotliAmdUnshuffleSeg>& segs, hipStream_t stream) {
  if (segs.empty()) return 0;
  const uint64_t units = width_segments_units(segs);
  if (units == 0u) return 0;   // (segments without elements: nothing to launch)
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const uint32_t n = (uint32_t)segs.size();
  return run_seg_call(&b->bitunpack, {"hipMalloc(bit-unpack segments)", "hipMemcpyAsync(bit-unpack segments)", "hipStreamSynchronize(bit-unpack)"}, segs.data(),
                      sizeof(BrotliAmdUnshuffleSeg) * n, 0u, 2u, stream, [&](uint8_t* d_segs, uint8_t*, const hipEvent_t* ev) {
    return hip_ok(hipEventRecord(ev[0], stream), "hipEventRecord") &&
           hip_ok(brotli_amd_launch_bitunpack(reinterpret_cast<BrotliAmdUnshuffleSeg*>(d_segs), n, units, stream), "brotli_amd_bitunpack_kernel launch") &&
           hip_ok(hipEventRecord(ev[1], stream), "hipEventRecord");
  }, &b->bitunpack_ms);
}

}  // namespace

extern "C" int BrotliAmdBatchBitUnpackSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                               const uint64_t* counts, const uint8_t* bits, const uint8_t* widths, const uint8_t* flags, void* hip_stream) {
  if (!b || (n && (!d_src || !src_lens || !d_dst || !counts || !bits || !widths))) { g_last_error = "invalid bit-unpack arguments"; return -1; }
  b->bitunpack_ms = 0.0f;
  std::vector<BrotliAmdUnshuffleSeg> segs;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t f = flags ? flags[i] : 0u;
    if (!known_shape(bits[i], widths[i], f, "segment", i) || !known_count(counts[i], bits[i], src_lens[i], "segment", i)) return -1;
    segs.push_back(segment(d_src[i], d_dst[i], counts[i], bits[i], widths[i], f));
  }
  return bitunpack_device(b, segs, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchBitUnpackOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint64_t* counts, const uint8_t* bits, const uint8_t* widths,
                                              const uint8_t* flags) {
  if (!b || !d_dst || !bits || !widths) { g_last_error = "invalid bit-unpack arguments"; return -1; }
  b->bitunpack_ms = 0.0f;
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  std::vector<BrotliAmdUnshuffleSeg> segs;
  for (size_t i = 0; i < outs.size(); i++) {
    if (d_dst[i] == nullptr) continue;   // (a stream the caller does not want: none of its parameters are looked at)
    const uint32_t f = flags ? flags[i] : 0u;
    if (!known_shape(bits[i], widths[i], f, "stream", i)) return -1;
    // without a count: the whole fields that the delivered bytes hold (8 len cannot overflow: len is a size of memory)
    const uint64_t count = counts ? counts[i] : outs[i].len * 8u / bits[i];
    if (!known_count(count, bits[i], outs[i].len, "stream", i)) return -1;
    segs.push_back(segment(outs[i].ptr, d_dst[i], count, bits[i], widths[i], f));
  }
  return bitunpack_device(b, segs, b->last_stream);
}

extern "C" float BrotliAmdBatchLastBitUnpackMs(BrotliAmdBatch* b) { return b ? b->bitunpack_ms : 0.0f; }
extern "C" uint32_t BrotliAmdDebugBitUnpackTile(void) { return brotli_amd_bitunpack_tile_bytes(); }

// The device's functions on the host over every unit of the segment: source and destination placed at their skews past a 16-byte boundary, among
// bytes that are not theirs (whole foreign words in front and behind as well).  The work is taken as the kernel takes a tile inside one segment:
// tile after tile of the segment's units, in each the slots in the lanes' order.
extern "C" int BrotliAmdDebugBitUnpackHost(uint32_t bits, uint32_t width, uint32_t flags, const uint8_t* src, size_t src_len, uint64_t count, uint8_t* dst,
                                           uint32_t src_skew, uint32_t dst_skew, uint64_t* fast_items) {
  if (!known_shape(bits, width, flags, "segment", 0) || !known_count(count, bits, src_len, "segment", 0)) return -1;
  if ((src_len && !src) || (count && !dst) || src_skew > 15u || dst_skew > 15u) { g_last_error = "invalid bit-unpack arguments"; return -1; }
  const uint64_t len = count * width;
  if (len > ((uint64_t)1 << 40)) { g_last_error = "bit-unpack on the host: more than 2^40 destination bytes"; return -1; }
  std::vector<uint8_t> sroom(src_len + 64u, 0xA5), droom(len + 64u, 0x5A);
  const uint64_t s_at = (((uint64_t)(uintptr_t)sroom.data() + 15u) & ~(uint64_t)15) + 16u + src_skew;
  const uint64_t d_at = (((uint64_t)(uintptr_t)droom.data() + 15u) & ~(uint64_t)15) + 16u + dst_skew;
  if (src_len) std::memcpy(reinterpret_cast<void*>((uintptr_t)s_at), src, src_len);
  const std::vector<uint8_t> before = droom;
  const uint64_t units = brotli_amd_seg_units(d_at, len), tile = brotli_amd_bitunpack_tile_bytes() / 16u, slot = 2u * width;
  uint64_t items = 0;
  for (uint64_t t0 = 0; t0 < units; t0 += tile) {
    const uint64_t t1 = std::min(t0 + tile, units);
    for (uint64_t s = t0 / slot; slot * s < t1; s++) items += brotli_amd_bitunpack_slot(s_at, d_at, count, width, bits, flags, s, t0, t1);
  }
  if (fast_items) *fast_items = items;
  // no byte beside the destination may have changed
  const size_t off = (size_t)(d_at - (uint64_t)(uintptr_t)droom.data());
  for (size_t i = 0; i < droom.size(); i++)
    if ((i < off || i >= off + len) && droom[i] != before[i]) { g_last_error = "bit-unpack wrote outside its destination"; return -2; }
  if (len) std::memcpy(dst, reinterpret_cast<const void*>((uintptr_t)d_at), len);
  return 0;
}
