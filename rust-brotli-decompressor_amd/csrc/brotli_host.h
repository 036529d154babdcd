// brotli_host.h -- what the parts of the host side of libbrotli_decompressor.so share (nothing of it is exported):
//   brotli_batch.cpp    the batch object: launch shapes applied (brotli_launch_plan.h), the probe, the later passes, the settle pass
//   brotli_staging.cpp  host buffers through staging arenas, size hints, the packed decode
//   brotli_capi.cpp     the reference's C ABI (include/brotli/decode.h): error strings, one-shot, Prealloc, the streaming state
//   brotli_stream_set.cpp  many streaming states in one launch, the ragged copy's debug hook
//   brotli_seg_call.cpp  what the calls below share: the last decode call's outputs as segments, the segment walk's host model
//   brotli_digest.cpp   CRC-32 / CRC-32C of segments of device memory and of the last decode call's outputs
//   brotli_filters.cpp  the element filters of segments of device memory and of the last decode call's outputs: one descriptor a filter and one call;
//                       the plain path (unshuffle, undelta, bit-unshuffle, bit-unpack), the counted path with a result per segment (unvarint,
//                       unrle, undbp, undict), unnull's, undict-bytes', undlba's and undba's paths of their own beside it, the host hooks
#ifndef BROTLI_AMD_HOST_H_
#define BROTLI_AMD_HOST_H_
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "brotli/batch.h"
#include "brotli/decode.h"
#include "brotli_device_abi.h"
#include "brotli_launch_plan.h"

// (csrc/brotli_copy_kernels.hip: n segments of any alignment and length in one launch; max_bytes: what their lengths add up to at most, 0 unknown)
extern "C" hipError_t brotli_amd_launch_ragged_copy(const BrotliAmdCopySeg* d_segs, uint32_t n, hipStream_t stream);
extern "C" hipError_t brotli_amd_launch_ragged_copy_sized(const BrotliAmdCopySeg* d_segs, uint32_t n, uint64_t max_bytes, hipStream_t stream);

namespace brotli_amd_host {

extern thread_local std::string g_last_error;
bool hip_ok(hipError_t e, const char* what);   // false: g_last_error says what failed

// Every entry point leaves the caller's current HIP device as it found it.
struct DeviceGuard {
  int saved = -1;
  DeviceGuard() { if (hipGetDevice(&saved) != hipSuccess) saved = -1; }
  ~DeviceGuard() { if (saved >= 0) (void)hipSetDevice(saved); }
};
bool current_device(int* dev);

// ---- owned memory ----
// Every allocation of the host side but the per-device dictionary: device memory (Mem::Device) or pinned host memory (Mem::Pinned) of T,
// move-only, freed by release() or the destructor -- with the owner's device current (the owners see to that: BrotliAmdBatchDestroy and the
// like).  capacity() is what the owner asked for; `slack` bytes more are allocated behind it: the kernel's reader fetches whole 256-byte
// pieces, and the slack is what keeps it inside the allocation.
enum class Mem { Device, Pinned };
extern std::atomic<size_t> g_live_bytes[2];   // allocated and not yet freed, slack included, by kind (brotli_amd_debug_live_bytes)

template <class T, Mem K>
class Buffer {
 public:
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept { swap(o); }
  Buffer& operator=(Buffer&& o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
  ~Buffer() { release(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }   // bytes

  // At least `bytes` (contents not kept: a larger buffer replaces a smaller one).  what == nullptr: a failure is no error -- the sticky HIP
  // error is cleared and the caller goes on without the buffer.
  bool reserve(size_t bytes, const char* what, size_t slack = 0) {
    if (bytes <= cap_ && (p_ || bytes + slack == 0)) return true;
    release();
    return allocate(bytes, what, slack);
  }
  // Device memory only.  A buffer of at least `bytes` that starts with bytes [from, from + keep) of the present one (a synchronous copy; the old
  // buffer goes after it).  Nothing happens where from == 0 and the present one is large enough; `grown` is the capacity asked for otherwise.
  bool rebase(size_t from, size_t keep, size_t bytes, size_t grown, const char* what, size_t slack) {
    static_assert(K == Mem::Device, "rebase: device memory");
    if (from == 0 && bytes <= cap_ && p_) return true;
    Buffer next;
    if (!next.allocate(grown, what, slack)) return false;
    if (p_ && keep && !hip_ok(hipMemcpy(next.p_, reinterpret_cast<uint8_t*>(p_) + from, keep, hipMemcpyDeviceToDevice), "hipMemcpy(rebase)")) return false;
    swap(next);
    return true;
  }
  void release() {
    if (p_) {
      (void)(K == Mem::Device ? hipFree(p_) : hipHostFree(p_));
      g_live_bytes[(int)K] -= alloc_;
    }
    p_ = nullptr; cap_ = alloc_ = 0;
  }

 private:
  bool allocate(size_t bytes, const char* what, size_t slack) {
    void* p = nullptr;
    const hipError_t e = K == Mem::Device ? hipMalloc(&p, bytes + slack) : hipHostMalloc(&p, bytes + slack, hipHostMallocDefault);
    if (what ? !hip_ok(e, what) : e != hipSuccess) { if (!what) (void)hipGetLastError(); return false; }
    p_ = static_cast<T*>(p); cap_ = bytes; alloc_ = p ? bytes + slack : 0;
    g_live_bytes[(int)K] += alloc_;
    return true;
  }
  void swap(Buffer& o) { std::swap(p_, o.p_); std::swap(cap_, o.cap_); std::swap(alloc_, o.alloc_); }
  T* p_ = nullptr;
  size_t cap_ = 0, alloc_ = 0;
};
template <class T = uint8_t> using DevBuf = Buffer<T, Mem::Device>;
template <class T = uint8_t> using PinBuf = Buffer<T, Mem::Pinned>;

// What a call over a table of segments (run_seg_call) keeps with its batch object
constexpr uint32_t kMaxSegEvents = 10;
struct SegCall {
  DevBuf<> d;                         // the segment table of one call and what the call wants behind it
  hipEvent_t ev[kMaxSegEvents] = {};   // around and between its launches (made at the first call, as many as it needs)
};

enum Filter : uint32_t { kUnshuffle, kUndelta, kBitUnshuffle, kBitUnpack, kUnvarint, kUnrle, kUndbp, kUndict, kUnnull, kUndictBytes, kUndlba, kUndba, kFilters };   // the element filters (brotli_filters.cpp)

constexpr size_t kReaderSlack = 256;   // behind every buffer the kernel reads a stream's bytes from, or writes them to, up to the buffer's end

}  // namespace brotli_amd_host

// ================================================ batch ================================================
struct BrotliAmdBatch {
  int device = 0;
  uint32_t max_streams = 0;
  BrotliAmdPlanDevice dev = {};   // what the device and the configuration are (brotli_launch_plan.h); engine_ok is dropped when the device refuses a block
  uint32_t per_cu_cap = 0;  // blocks per CU a first pass may ask for (lowered when most of a batch had to come back)
  // the launch at hand (submit(): the plan applied)
  uint32_t n = 0, grid = 0, waves = 4;
  uint32_t cur_arena = 0;   // its table arena: the configured one, a smaller one for many streams in flight, a larger one for few
  uint32_t cur_per_cu = 0;  // blocks per CU its first pass was shaped for
  uint32_t gang = 0, last_gang = 0;   // several CUs on one stream: the blocks of a gang in this launch (0: none)
  bool ordered = false;
  brotli_amd_host::DevBuf<BrotliAmdStreamDesc> d_descs;
  brotli_amd_host::DevBuf<BrotliAmdStreamStatus> d_status;
  brotli_amd_host::DevBuf<uint32_t> d_queue;
  brotli_amd_host::DevBuf<> d_scratch;   // the blocks' table scratch
  brotli_amd_host::DevBuf<> d_gang;      // the gangs' control blocks (brotli_device_abi.h)
  brotli_amd_host::PinBuf<BrotliAmdStreamDesc> h_descs;
  brotli_amd_host::PinBuf<BrotliAmdStreamStatus> h_status;
  brotli_amd_host::PinBuf<uint32_t> h_order;   // queue header + the order in which blocks take the streams
  const uint8_t* d_dict = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;  // around the first launch; around a launch of a later pass
  float retry_ms = 0.0f;  // kernel time of the later passes of the last job
  hipStream_t last_stream = nullptr;
  bool launched = false;
  // streams that ran out of output get the reference's verdict (settle_output_limits): set by the batch entry points and decode_descs
  bool exact_limit = false;
  // later passes for streams whose tables did not fit the LDS arena of the first (BROTLI_AMD_FLAG_NO_SPILL), and the settle pass
  uint32_t last_retry_count = 0, last_settle_count = 0;
  brotli_amd_host::DevBuf<BrotliAmdStreamDesc> d_retry_descs;
  brotli_amd_host::DevBuf<BrotliAmdStreamStatus> d_retry_status;
  brotli_amd_host::PinBuf<BrotliAmdStreamDesc> h_retry_descs;
  brotli_amd_host::PinBuf<BrotliAmdStreamStatus> h_retry_status;
  brotli_amd_host::DevBuf<> d_settle;
  // the probe's answers for the batch it was asked about (probe_streams): the same descriptors again are not probed again
  std::vector<uint8_t> probe_kind; uint64_t probe_key = 0; float last_probe_ms = 0.0f;
  // staging of the host entry points (brotli_staging.cpp): inputs, outputs, each distinct custom dictionary once -- and its pinned host side: the
  // caller's buffers are pageable as a rule, a copy engine wants pinned memory
  brotli_amd_host::DevBuf<> d_stage_in, d_stage_out, d_stage_dict;
  brotli_amd_host::PinBuf<> h_pin_in, h_pin_out;
  hipStream_t copy_stream = nullptr;
  // the size walk's descriptors and hints on the device (BrotliAmdBatchSizeHints), and the segment table of the packed decode's ragged copies
  brotli_amd_host::DevBuf<> d_size, d_pack_segs;
  // packed decode (BrotliAmdBatchDecodeDevicePacked): the slots of its first launch and the tight buffer a gather fills are kept with the object;
  // packed_out names the one that holds the last call's output (nullptr: there is none)
  brotli_amd_host::DevBuf<> d_pack_slots, d_pack_tight;
  const uint8_t* packed_out = nullptr;
  bool packed_valid = false;   // the last decode call on the object was a packed call that succeeded
  std::vector<uint64_t> packed_offsets;
  uint32_t last_packed_launches = 0, last_packed_copies = 0;
  float packed_ms = 0.0f;   // decode kernel time of all its launches together
  // digests (brotli_digest.cpp).  What BrotliAmdBatchDigestOutputs finds where the last decode call was not a packed one: no decode call yet; a call
  // that has begun and launched nothing -- where it stays so, it failed --; a call of no streams; a launch nobody has waited for; h_descs and
  // h_status of the launch waited for
  enum class Outputs : uint8_t { NoCall, Failed, None, InFlight, Waited } outputs = Outputs::NoCall;
  brotli_amd_host::SegCall digest;   // behind the table: the digests of one launch
  float digest_ms = 0.0f;
  // the element filters (brotli_filters.cpp), by brotli_amd_host::Filter: each one's call, the kernel time of its last call and, of a filter of
  // several launches, that of each launch (phase_ms[i]: from event i to event i + 1).  What lies behind each table is its launcher's to say.
  struct FilterCall { brotli_amd_host::SegCall call; float ms = 0.0f; float phase_ms[brotli_amd_host::kMaxSegEvents - 1u] = {}; } filter[brotli_amd_host::kFilters];
};

namespace brotli_amd_host {

// Output room for compressed bytes nobody has seen decoded: six times their number, 64 KiB at least -- the streaming decoder's device buffer
// (stream_ensure_out) and the packed decode's first capacity for what the size walk did not reach (packed_decode)
constexpr size_t kGuessOutFactor = 6, kGuessOutFloor = (size_t)1 << 16;
// A custom dictionary as the kernel is told of it: no window reaches further back than (1 << 30) - 16 bytes (decode.rs:1831-1839), so
// of a longer one the tail is named -- the same bytes at the same distances.
constexpr size_t kMaxCustomDict = ((size_t)1 << 30) - 16;
// what a caller's flags may say to the kernel
constexpr uint32_t kCallerFlagMask = BROTLI_AMD_FLAG_LARGE_WINDOW | BROTLI_AMD_FLAG_NO_CANNY | BROTLI_AMD_BATCH_SPILL_IN_PLACE;

// One stream as the kernel is told of it (flags: masked; dict: the tail rule applied; nullptr or size 0: none).
inline BrotliAmdStreamDesc make_desc(const void* in, size_t in_size, void* out, size_t out_cap, uint32_t flags, const void* dict = nullptr, size_t dict_size = 0) {
  BrotliAmdStreamDesc d;
  std::memset(&d, 0, sizeof d);
  d.in = static_cast<const uint8_t*>(in); d.in_size = in_size;
  d.out = static_cast<uint8_t*>(out); d.out_cap = out_cap;
  d.flags = flags & kCallerFlagMask;
  if (dict != nullptr && dict_size != 0) {
    const size_t tail = std::min(dict_size, kMaxCustomDict);
    d.dict = static_cast<const uint8_t*>(dict) + (dict_size - tail); d.dict_size = tail;
  }
  return d;
}
inline BrotliAmdResult to_result(const BrotliAmdStreamStatus& s) {
  BrotliAmdResult r;
  r.result = s.result; r.error_code = s.error_code; r.decoded_size = s.decoded_size; r.consumed = s.consumed;
  r.produced = s.produced; r.num_metablocks = s.num_metablocks; r.spilled_metablocks = s.spilled_metablocks; r.num_commands = s.num_commands;
  r.engine_commands = s.engine_commands; r.reserved = 0;
  return r;
}

// The reference notices a full output buffer at its next ring-buffer flush (decode.rs:1693-1738): a second decode with room up to ONE BYTE SHORT
// of that point -- it flushes as soon as its ring of ring_bytes is full -- says what it would have reported for a buffer of `cap` bytes.
inline uint64_t flush_point_cap(uint64_t cap, uint64_t ring_bytes) { return (cap / ring_bytes + 1) * ring_bytes - 1; }
// ... and whether that decode's verdict replaces NEEDS_MORE_OUTPUT: an error, or the end of the input, in front of the flush point
inline bool second_verdict_wins(const BrotliAmdStreamStatus& st2, uint64_t cap2) {
  return st2.result == BROTLI_DECODER_RESULT_ERROR || (st2.result == BROTLI_DECODER_RESULT_NEEDS_MORE_INPUT && st2.produced <= cap2);
}

// h_descs[0..n) filled -> launched on `stream` (the plan, the probe where the plan wants one, the upload); BrotliAmdBatchWait brings the results
int submit(BrotliAmdBatch* b, uint32_t n, hipStream_t stream);
// ... and waited for, later passes included: h_status[0..n).  exact_limit: streams that ran out of output get the reference's verdict
// (settle_output_limits).  False: a HIP failure.
bool decode_descs(BrotliAmdBatch* b, uint32_t n, hipStream_t stream, bool exact_limit);
constexpr bool kExactLimitDefault = false;   // what a batch object's exact_limit is until a batch entry point says otherwise: the one-shot and streaming paths' value
// The DELIVERED bytes -- [out, out + decoded_size) -- of every stream of the last decode call on the object, where BrotliAmdBatchDigestOutputs and
// BrotliAmdBatchUnshuffleOutputs find them (batch.h says where; brotli_seg_call.cpp).  False, and g_last_error: no decode call yet, one that failed, a
// launch nobody has waited for.  A call of no streams: true and none.
struct DeliveredBytes { const uint8_t* ptr; uint64_t len; };
bool delivered_outputs(BrotliAmdBatch* b, std::vector<DeliveredBytes>* outs);
void drop_packed(BrotliAmdBatch* b);   // a decode call ends the validity of the last packed call's output

// ---- calls over a table of segments: the digests (brotli_digest.cpp) and the element filters (brotli_filters.cpp) ----
struct SegCallWhat { const char* alloc; const char* upload; const char* wait; };   // what hip_ok says of a failed step
// One call on `stream` (the object's device is current): room in c->d for the table, rounded up to 16 bytes, and `extra` bytes behind it; its
// first nev events; the table's upload; then launch(uint8_t* table, uint8_t* what lies behind it, const hipEvent_t* events) -> all of it was queued.  The stream is waited
// for IN ANY CASE: the upload reads pageable memory.  On success *total_ms is the time from the first event to the last and, where gap_ms is
// given, gap_ms[i] that from event i to event i + 1.  -> 0, or -1 and g_last_error.
template <class Launch>
int run_seg_call(SegCall* c, const SegCallWhat& what, const void* table, size_t table_bytes, size_t extra, uint32_t nev, hipStream_t stream,
                 Launch launch, float* total_ms, float* gap_ms = nullptr) {
  const size_t room = (table_bytes + 15u) & ~(size_t)15;
  if (!c->d.reserve(room + extra, what.alloc)) return -1;
  for (uint32_t i = 0; i < nev; i++)
    if (!c->ev[i] && !hip_ok(hipEventCreate(&c->ev[i]), "hipEventCreate")) return -1;
  bool ok = hip_ok(hipMemcpyAsync(c->d.get(), table, table_bytes, hipMemcpyHostToDevice, stream), what.upload);
  ok = ok && launch(c->d.get(), c->d.get() + room, c->ev);
  // (waited for in any case: the copies read and write the caller's pageable memory)
  if (!hip_ok(hipStreamSynchronize(stream), what.wait) || !ok) return -1;
  (void)hipEventElapsedTime(total_ms, c->ev[0], c->ev[nev - 1u]);
  for (uint32_t i = 0; gap_ms && i + 1u < nev; i++) (void)hipEventElapsedTime(&gap_ms[i], c->ev[i], c->ev[i + 1u]);
  return 0;
}

// `size` bytes placed `skew` past a 16-byte boundary in a room of this object's own, among bytes that are not theirs (whole foreign words in
// front and behind as well): where the BrotliAmdDebug*Host hooks keep what the device's functions read and write on the host.
class SkewedRoom {
 public:
  SkewedRoom(size_t size, uint32_t skew, uint8_t fill)
      : room_(size + 64u, fill), at_((((uint64_t)(uintptr_t)room_.data() + 15u) & ~(uint64_t)15) + 16u + skew) {}
  SkewedRoom(const SkewedRoom&) = delete;
  SkewedRoom& operator=(const SkewedRoom&) = delete;
  uint64_t at() const { return at_; }   // the address of the bytes
  void put(const uint8_t* from, size_t n) { if (n) std::memcpy(reinterpret_cast<void*>((uintptr_t)at_), from, n); }
  void get(uint8_t* to, size_t off, size_t n) const { if (n) std::memcpy(to, reinterpret_cast<const void*>((uintptr_t)(at_ + off)), n); }
  void snapshot() { before_ = room_; }
  // whether, since the snapshot, no byte of the room changed but bytes at offsets i past at() with inside(i)
  template <class Inside>
  bool changed_inside_only(Inside inside) const {
    const size_t off = (size_t)(at_ - (uint64_t)(uintptr_t)room_.data());
    for (size_t i = 0; i < room_.size(); i++)
      if (room_[i] != before_[i] && (i < off || !inside(i - off))) return false;
    return true;
  }

 private:
  std::vector<uint8_t> room_, before_;
  uint64_t at_;
};

}  // namespace brotli_amd_host
#endif  // BROTLI_AMD_HOST_H_
