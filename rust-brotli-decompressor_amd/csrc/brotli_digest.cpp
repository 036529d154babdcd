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
  const uint32_t n = (uint32_t)segs.size();
  const size_t out_bytes = sizeof(uint32_t) * n;
  uint64_t units = 0;
  for (const BrotliAmdCrcSeg& s : segs) units += brotli_amd_seg_units((uint64_t)(uintptr_t)s.ptr, s.len);
  // behind the table: the n digests, zeroed in front of the launch and brought back behind it
  return run_seg_call(&b->digest, {"hipMalloc(digests)", "hipMemcpyAsync(digest segments)", "hipStreamSynchronize(digests)"}, segs.data(),
                      sizeof(BrotliAmdCrcSeg) * n, out_bytes, 2u, stream, [&](uint8_t* d_segs, uint8_t* d_out, const hipEvent_t* ev) {
    return hip_ok(hipMemsetAsync(d_out, 0, out_bytes, stream), "hipMemsetAsync(digests)") && hip_ok(hipEventRecord(ev[0], stream), "hipEventRecord") &&
           hip_ok(brotli_amd_launch_crc(reinterpret_cast<BrotliAmdCrcSeg*>(d_segs), n, kind, units, reinterpret_cast<uint32_t*>(d_out), stream), "brotli_amd_crc_kernel launch") &&
           hip_ok(hipEventRecord(ev[1], stream), "hipEventRecord") &&
           hip_ok(hipMemcpyAsync(digests, d_out, out_bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(digests)");
  }, &b->digest_ms);
}

}  // namespace

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
  SkewedRoom room(n, skew, 0xA5);
  room.put(data, n);
  const uint64_t at = room.at();
  const uint32_t poly = brotli_amd_crc_poly(kind);
  const BrotliAmdCrcConsts& c = kConsts[kind - 1u];
  const auto load = [](uint64_t W, uint32_t* w) { std::memcpy(w, reinterpret_cast<const void*>((uintptr_t)W), 16); };
  const uint64_t units = brotli_amd_seg_units(at, n);
  uint32_t digest = 0;
  for (uint64_t u0 = 0; u0 < units; u0 += run_units) {
    uint64_t behind = 0;
    const uint32_t reg = brotli_amd_crc_piece(&c.t[0][0], load, at, n, u0, std::min<uint64_t>(u0 + run_units, units), &behind);
    digest ^= brotli_amd_crc_piece_term(poly, c.pw, reg, behind);
  }
  return digest;
}
