// brotli_digest.cpp -- digests on the device (include/brotli/batch.h): the CRC-32 or CRC-32C of n segments of device memory in one launch
// (BrotliAmdBatchDigestSegments), of the delivered bytes of every stream of the last decode call (BrotliAmdBatchDigestOutputs), and the
// arithmetic of csrc/brotli_crc.h on the host, cut the way the kernel cuts, for tests without a device.
#include "brotli_crc.h"
#include "brotli_host.h"

// (csrc/brotli_crc_kernels.hip: the digests of n segments into n words that were zeroed on the stream; units: the segments' units together)
extern "C" hipError_t brotli_amd_launch_crc(const BrotliAmdCrcSeg* d_segs, uint32_t n, uint32_t kind, uint64_t units, uint32_t* d_out, hipStream_t stream);
extern "C" uint32_t brotli_amd_crc_tile_bytes(void);

using namespace brotli_amd_host;

namespace {

constexpr BrotliAmdCrcConsts kConsts[2] = {brotli_amd_crc_make_consts(BROTLI_AMD_CRC32_POLY), brotli_amd_crc_make_consts(BROTLI_AMD_CRC32C_POLY)};

bool known_kind(uint32_t kind) {
  if (brotli_amd_crc_poly(kind) != 0u) return true;
  g_last_error = "unknown digest kind";
  return false;
}

// the digests of segs[0..n) on `stream`, waited for: digests[0..n) on the host (the object's device is current)
int digest_device(BrotliAmdBatch* b, uint32_t kind, const std::vector<BrotliAmdCrcSeg>& segs, uint32_t* digests, hipStream_t stream) {
  const size_t n = segs.size(), table_bytes = sizeof(BrotliAmdCrcSeg) * n, out_bytes = sizeof(uint32_t) * n;
  b->digest_ms = 0.0f;
  if (!b->d_digest.reserve(table_bytes + out_bytes, "hipMalloc(digests)")) return -1;
  if (!b->ev_digest0 && !(hip_ok(hipEventCreate(&b->ev_digest0), "hipEventCreate") && hip_ok(hipEventCreate(&b->ev_digest1), "hipEventCreate"))) return -1;
  BrotliAmdCrcSeg* d_segs = reinterpret_cast<BrotliAmdCrcSeg*>(b->d_digest.get());
  uint32_t* d_out = reinterpret_cast<uint32_t*>(b->d_digest + table_bytes);
  uint64_t units = 0;
  for (const BrotliAmdCrcSeg& s : segs) units += brotli_amd_crc_seg_units((uint64_t)(uintptr_t)s.ptr, s.len);
  bool ok = hip_ok(hipMemcpyAsync(d_segs, segs.data(), table_bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(digest segments)");
  ok = ok && hip_ok(hipMemsetAsync(d_out, 0, out_bytes, stream), "hipMemsetAsync(digests)");
  ok = ok && hip_ok(hipEventRecord(b->ev_digest0, stream), "hipEventRecord");
  ok = ok && hip_ok(brotli_amd_launch_crc(d_segs, (uint32_t)n, kind, units, d_out, stream), "brotli_amd_crc_kernel launch");
  ok = ok && hip_ok(hipEventRecord(b->ev_digest1, stream), "hipEventRecord");
  ok = ok && hip_ok(hipMemcpyAsync(digests, d_out, out_bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(digests)");
  // (waited for in any case: the copies read and write the caller's and this function's pageable memory)
  if (!hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize(digests)") || !ok) return -1;
  (void)hipEventElapsedTime(&b->digest_ms, b->ev_digest0, b->ev_digest1);
  return 0;
}

}  // namespace

// The delivered bytes of every stream of the last decode call (brotli_host.h)
bool brotli_amd_host::delivered_outputs(BrotliAmdBatch* b, std::vector<DeliveredBytes>* outs) {
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

extern "C" int BrotliAmdBatchDigestSegments(BrotliAmdBatch* b, uint32_t kind, uint32_t n, const void* const* d_ptrs, const size_t* lens,
                                            uint32_t* digests, void* hip_stream) {
  if (!known_kind(kind)) return -1;
  if (!b || (n && (!d_ptrs || !lens || !digests))) { g_last_error = "invalid digest arguments"; return -1; }
  b->digest_ms = 0.0f;
  if (n == 0) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  std::vector<BrotliAmdCrcSeg> segs(n);
  for (uint32_t i = 0; i < n; i++) segs[i] = BrotliAmdCrcSeg{static_cast<const uint8_t*>(d_ptrs[i]), lens[i]};
  return digest_device(b, kind, segs, digests, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchDigestOutputs(BrotliAmdBatch* b, uint32_t kind, uint32_t* digests) {
  if (!known_kind(kind)) return -1;
  if (!b || !digests) { g_last_error = "invalid digest arguments"; return -1; }
  b->digest_ms = 0.0f;
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  std::vector<BrotliAmdCrcSeg> segs;
  for (const DeliveredBytes& o : outs) segs.push_back(BrotliAmdCrcSeg{o.ptr, o.len});
  if (segs.empty()) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  return digest_device(b, kind, segs, digests, b->last_stream);
}

extern "C" float BrotliAmdBatchLastDigestMs(BrotliAmdBatch* b) { return b ? b->digest_ms : 0.0f; }
extern "C" uint32_t BrotliAmdDebugDigestTile(void) { return brotli_amd_crc_tile_bytes(); }

extern "C" uint32_t BrotliAmdDebugDigestShift(uint32_t kind, uint32_t crc, uint64_t nbytes) {
  if (!known_kind(kind)) return 0;
  return brotli_amd_crc_shift(brotli_amd_crc_poly(kind), kConsts[kind - 1u].pw, crc, nbytes);
}

// The kernel's cut on the host: the bytes at `skew` past a 16-byte boundary, among bytes that are not theirs; units; a piece for every run of
// run_units units; the pieces' terms XORed.
extern "C" uint32_t BrotliAmdDebugDigestHost(uint32_t kind, const uint8_t* data, size_t n, uint32_t skew, uint32_t run_units) {
  if (!known_kind(kind)) return 0;
  if ((n && !data) || skew > 15u) { g_last_error = "invalid digest arguments"; return 0; }
  if (run_units == 0u) run_units = BROTLI_AMD_CRC_RUN_UNITS;
  std::vector<uint8_t> room(n + 64u, 0xA5);
  const uint64_t at = (((uint64_t)(uintptr_t)room.data() + 15u) & ~(uint64_t)15) + 16u + skew;   // (a whole foreign word in front as well)
  if (n) std::memcpy(reinterpret_cast<void*>((uintptr_t)at), data, n);
  const uint32_t poly = brotli_amd_crc_poly(kind);
  const BrotliAmdCrcConsts& c = kConsts[kind - 1u];
  const auto load = [](uint64_t W, uint32_t* w) { std::memcpy(w, reinterpret_cast<const void*>((uintptr_t)W), 16); };
  const uint64_t units = brotli_amd_crc_seg_units(at, n);
  uint32_t digest = 0;
  for (uint64_t u0 = 0; u0 < units; u0 += run_units) {
    uint64_t behind = 0;
    const uint32_t reg = brotli_amd_crc_piece(&c.t[0][0], load, at, n, u0, std::min<uint64_t>(u0 + run_units, units), &behind);
    digest ^= brotli_amd_crc_piece_term(poly, c.pw, reg, behind);
  }
  return digest;
}
