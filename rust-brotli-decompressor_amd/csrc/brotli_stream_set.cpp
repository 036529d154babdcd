// brotli_stream_set.cpp -- stream sets: many streaming states advanced by ONE launch (include/brotli/batch.h).  Per state the call is
// BrotliDecoderDecompressStream's, phase by phase (brotli_stream.h: stream_begin ... stream_end); what differs is how the bytes travel and how
// many states a launch holds: the chunks of all states go to the device packed in one pinned staging buffer and a ragged copy
// (csrc/brotli_copy_kernels.hip) appends each to its state's input, one launch over the set's own batch object decodes them all, a ragged copy
// gathers every state's new output into staging and one transfer brings it back.
#include <new>

#include "brotli_stream.h"

extern "C" uint32_t brotli_amd_copy_tile_bytes(void);

using namespace brotli_amd_host;

// One direction's staging: the pinned host side and the device side of the same size.
struct SetStage {
  PinBuf<> h;
  DevBuf<> d;
  size_t capacity() const { return h.capacity(); }
};

struct BrotliAmdStreamSet {
  uint32_t max_states = 0;
  int device = -1;                       // bound at the first call that needs a device
  BrotliAmdBatch* batch = nullptr;
  PinBuf<BrotliAmdCopySeg> h_segs;       // max_states entries
  DevBuf<BrotliAmdCopySeg> d_segs;
  SetStage in, out;
  uint32_t last_launches = 0, last_transfers = 0;
};

namespace {

constexpr size_t kSetStageMax = (size_t)64 << 20;   // staging in each direction at most; a larger chunk or output part travels alone

bool set_bind(BrotliAmdStreamSet* set) {
  if (set->batch) return true;
  int dev = set->device;
  if (dev < 0 && !current_device(&dev)) return false;
  if (!hip_ok(hipSetDevice(dev), "hipSetDevice")) return false;
  BrotliAmdBatch* b = BrotliAmdBatchCreate(set->max_states, 0, 0);
  if (!b) return false;
  if (!set->h_segs.reserve(sizeof(BrotliAmdCopySeg) * set->max_states, "hipHostMalloc(copy segments)") ||
      !set->d_segs.reserve(sizeof(BrotliAmdCopySeg) * set->max_states, "hipMalloc(copy segments)")) {
    set->h_segs.release(); set->d_segs.release();
    BrotliAmdBatchDestroy(b);
    return false;
  }
  set->batch = b; set->device = dev;
  return true;
}

// Staging of `need` bytes: a power of two from 1 MiB, kSetStageMax at most.  The null stream is waited for before the old pair goes.
bool set_stage(SetStage& s, size_t need) {
  if (need <= s.capacity()) return true;
  size_t want = (size_t)1 << 20;
  while (want < need) want <<= 1;
  want = std::min(want, kSetStageMax);
  if (!hip_ok(hipStreamSynchronize(nullptr), "hipStreamSynchronize")) return false;
  s.h.release(); s.d.release();
  if (!s.h.reserve(want, "hipHostMalloc(staging)") || !s.d.reserve(want, "hipMalloc(staging)", kReaderSlack)) {
    s.h.release(); s.d.release();
    return false;
  }
  return true;
}

// One part of a staged move: `len` bytes between a state's device buffer at `dev` and host memory at `host`.
struct SetPart { uint8_t* dev; uint8_t* host; size_t len; };

// Moves the parts between host and device: those that fit the staging buffer together in one transfer and one ragged copy (several rounds of
// both where they add up to more than the buffer holds), a part larger than the buffer by a copy of its own.  Synchronous: done on return.
bool set_move(BrotliAmdStreamSet* set, const std::vector<SetPart>& parts, bool to_device) {
  SetStage& stage = to_device ? set->in : set->out;
  size_t staged = 0;
  for (const SetPart& p : parts) if (p.len <= kSetStageMax) staged += p.len;
  if (staged && !set_stage(stage, std::min(staged, kSetStageMax))) return false;
  uint8_t* const h = stage.h; uint8_t* const d = stage.d;
  size_t at = 0;
  while (at < parts.size()) {
    uint32_t m = 0; size_t bytes = 0, first = at;
    for (; at < parts.size() && m < set->max_states; at++) {
      const SetPart& p = parts[at];
      if (p.len == 0) continue;
      if (p.len > kSetStageMax) {
        if (!hip_ok(to_device ? hipMemcpy(p.dev, p.host, p.len, hipMemcpyHostToDevice) : hipMemcpy(p.host, p.dev, p.len, hipMemcpyDeviceToHost), "hipMemcpy(large part)")) return false;
        set->last_transfers++;
        continue;
      }
      if (bytes + p.len > stage.capacity()) break;
      if (to_device) { std::memcpy(h + bytes, p.host, p.len); set->h_segs[m] = BrotliAmdCopySeg{d + bytes, p.dev, p.len}; }
      else set->h_segs[m] = BrotliAmdCopySeg{p.dev, d + bytes, p.len};
      m++; bytes += p.len;
    }
    if (m == 0) continue;
    bool ok = hip_ok(hipMemcpyAsync(set->d_segs, set->h_segs, sizeof(BrotliAmdCopySeg) * m, hipMemcpyHostToDevice, nullptr), "hipMemcpyAsync(copy segments)");
    if (to_device) ok = ok && hip_ok(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, nullptr), "hipMemcpyAsync(staged input)");
    ok = ok && hip_ok(brotli_amd_launch_ragged_copy_sized(set->d_segs, m, bytes, nullptr), "brotli_amd_ragged_copy_kernel launch");
    if (!to_device) ok = ok && hip_ok(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, nullptr), "hipMemcpyAsync(staged output)");
    // (output is wanted on the host now; input only has to be out of the pinned buffer before it is filled again -- the launch that follows is
    // on the same stream, and so are the state buffers' re-base copies and frees, and the wait for the launch is the wait for this)
    if (!to_device || at < parts.size()) ok = ok && hip_ok(hipStreamSynchronize(nullptr), "hipStreamSynchronize(staging)");
    if (!ok) return false;
    set->last_transfers++;
    if (!to_device) {
      size_t off = 0;
      for (size_t k = first; k < at; k++) {
        const SetPart& p = parts[k];
        if (p.len == 0 || p.len > kSetStageMax) continue;
        std::memcpy(p.host, h + off, p.len); off += p.len;
      }
    }
  }
  return true;
}

}  // namespace

extern "C" BrotliAmdStreamSet* BrotliAmdStreamSetCreate(uint32_t max_states) {
  BrotliAmdStreamSet* set = new (std::nothrow) BrotliAmdStreamSet();
  if (!set) return nullptr;
  set->max_states = max_states ? max_states : 1u;
  return set;
}

extern "C" void BrotliAmdStreamSetDestroy(BrotliAmdStreamSet* set) {
  if (!set) return;
  if (set->batch) BrotliAmdBatchDestroy(set->batch);   // (waits for the device)
  if (set->device >= 0) {   // its buffers go with the set's device current
    DeviceGuard guard;
    (void)hipSetDevice(set->device);
    delete set;
  } else delete set;
}

extern "C" uint32_t BrotliAmdStreamSetLastLaunches(BrotliAmdStreamSet* set) { return set ? set->last_launches : 0; }
extern "C" uint32_t BrotliAmdStreamSetLastTransfers(BrotliAmdStreamSet* set) { return set ? set->last_transfers : 0; }

extern "C" int BrotliAmdStreamSetDecompress(BrotliAmdStreamSet* set, uint32_t n, BrotliDecoderState* const* states, size_t* available_in,
                                            const uint8_t** next_in, size_t* available_out, uint8_t** next_out, size_t* total_out,
                                            BrotliDecoderResult* results) {
  // failures of the call as a whole: nothing is touched
  if (!set) { g_last_error = "invalid stream set arguments"; return -1; }
  if (n == 0) { set->last_launches = set->last_transfers = 0; return 0; }
  if (!states || !results || !available_in || !next_in || !available_out || !next_out || n > set->max_states) { g_last_error = "invalid stream set arguments"; return -1; }
  {
    std::vector<const BrotliDecoderState*> seen(states, states + n);
    std::sort(seen.begin(), seen.end());
    if (seen[0] == nullptr || std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { g_last_error = "invalid stream set arguments"; return -1; }
    int dev = set->device;
    for (uint32_t i = 0; i < n; i++) {
      if (states[i]->device < 0) continue;
      if (dev < 0 && hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; break; }   // (the device the set would bind to)
      if (states[i]->device != dev) { g_last_error = "a state of the set is bound to another device"; return -1; }
    }
  }
  set->last_launches = set->last_transfers = 0;
  // the head of every state's call, on the host; what is left needs the device
  std::vector<uint32_t> act; std::vector<size_t> given(n, 0);
  for (uint32_t i = 0; i < n; i++) {
    BrotliDecoderState* s = states[i];
    size_t* tot = total_out ? &total_out[i] : nullptr;
    if (stream_begin(s, &available_in[i], &next_in[i], &available_out[i], &next_out[i], tot, &results[i])) continue;
    given[i] = available_in[i];
    if (stream_wants_device(s, given[i])) act.push_back(i);
    else results[i] = stream_end(s, &available_out[i], &next_out[i], tot);
  }
  if (act.empty()) return 0;
  DeviceGuard guard;
  const auto fail_all = [&](const std::vector<uint32_t>& which, const char* what) { for (uint32_t i : which) results[i] = stream_fail(states[i], what); };
  if (!set_bind(set)) { fail_all(act, "HIP device unavailable"); return 0; }
  if (!hip_ok(hipSetDevice(set->device), "hipSetDevice")) { fail_all(act, "HIP runtime failure"); return 0; }
  // input: every state's chunk behind what its device buffer holds
  {
    std::vector<uint32_t> ready; std::vector<SetPart> parts;
    for (uint32_t i : act) {
      BrotliDecoderState* s = states[i];
      if (s->device < 0) s->device = set->device;   // (no batch object of its own until it is first stepped alone)
      size_t fill = 0;
      if (!stream_upload_dictionary(s) || !stream_input_room(s, given[i], &fill)) { results[i] = stream_fail(s, "HIP runtime failure"); continue; }
      parts.push_back(SetPart{s->d_in + fill, const_cast<uint8_t*>(next_in[i]), given[i]});
      ready.push_back(i);
    }
    act.swap(ready);
    if (act.empty()) return 0;
    if (!set_move(set, parts, true)) { fail_all(act, "HIP runtime failure"); return 0; }
    for (uint32_t i : act) stream_took_input(states[i], &available_in[i], &next_in[i], given[i]);
  }
  // decode: one launch over all of them; the states whose device output buffer was full grow it and are launched again, they alone
  std::vector<uint32_t> cur = act;
  while (!cur.empty()) {
    {
      std::vector<uint32_t> ready;
      for (uint32_t i : cur) { if (stream_ensure_out(states[i])) ready.push_back(i); else results[i] = stream_fail(states[i], 1); }
      cur.swap(ready);
      if (cur.empty()) break;
    }
    const uint32_t m = (uint32_t)cur.size();
    for (uint32_t j = 0; j < m; j++) set->batch->h_descs[j] = stream_desc(states[cur[j]]);
    if (!decode_descs(set->batch, m, nullptr, kExactLimitDefault)) { for (uint32_t i : cur) results[i] = stream_fail(states[i], 1); break; }
    set->last_launches++;
    std::vector<BrotliAmdStreamStatus> sts(set->batch->h_status.get(), set->batch->h_status + m);
    // output: what the reference would have flushed by now (fetch_output's rule), off the device behind what each caller has not taken yet
    std::vector<uint32_t> got; std::vector<SetPart> parts;   // got: positions in cur
    for (uint32_t j = 0; j < m; j++) {
      BrotliDecoderState* s = states[cur[j]];
      stream_note_status(s, sts[j]);
      const size_t len = sts[j].decoded_size > s->fetched ? (size_t)(sts[j].decoded_size - s->fetched) : 0;
      if (!reserve_outq(s, len)) { results[cur[j]] = stream_fail(s, 2); continue; }
      parts.push_back(SetPart{s->d_out + (s->fetched - s->out_base), s->outq + s->outq_len, len});
      got.push_back(j);
    }
    if (!set_move(set, parts, false)) { for (uint32_t j : got) results[cur[j]] = stream_fail(states[cur[j]], 1); break; }
    std::vector<uint32_t> again;
    for (size_t k = 0; k < got.size(); k++) {
      const uint32_t j = got[k], i = cur[j];
      BrotliDecoderState* s = states[i];
      s->outq_len += parts[k].len; s->fetched += parts[k].len;
      if (sts[j].result == BROTLI_DECODER_RESULT_NEEDS_MORE_OUTPUT) {
        if (stream_grow_out(s)) again.push_back(i); else results[i] = stream_fail(s, 1);
        continue;
      }
      if (!stream_decoded(s, sts[j], &available_in[i], &next_in[i], given[i])) { results[i] = stream_fail(s, "HIP runtime failure"); continue; }
      results[i] = stream_end(s, &available_out[i], &next_out[i], total_out ? &total_out[i] : nullptr);
    }
    cur.swap(again);
  }
  return 0;
}

// Test hook: the ragged copy alone (host arrays of device pointers; launches, waits).
extern "C" int BrotliAmdDebugRaggedCopy(uint32_t n, const void* const* d_src, void* const* d_dst, const size_t* lens) {
  if (n == 0) return hip_ok(brotli_amd_launch_ragged_copy(nullptr, 0, nullptr), "brotli_amd_ragged_copy_kernel launch") ? 0 : -1;
  if (!d_src || !d_dst || !lens) { g_last_error = "invalid ragged copy arguments"; return -1; }
  std::vector<BrotliAmdCopySeg> segs(n);
  for (uint32_t i = 0; i < n; i++) segs[i] = BrotliAmdCopySeg{static_cast<const uint8_t*>(d_src[i]), static_cast<uint8_t*>(d_dst[i]), lens[i]};
  DevBuf<BrotliAmdCopySeg> d;
  bool ok = d.reserve(sizeof(BrotliAmdCopySeg) * n, "hipMalloc(copy segments)");
  ok = ok && hip_ok(hipMemcpy(d, segs.data(), sizeof(BrotliAmdCopySeg) * n, hipMemcpyHostToDevice), "hipMemcpy(copy segments)");
  ok = ok && hip_ok(brotli_amd_launch_ragged_copy(d, n, nullptr), "brotli_amd_ragged_copy_kernel launch");
  ok = ok && hip_ok(hipStreamSynchronize(nullptr), "hipStreamSynchronize(ragged copy)");
  return ok ? 0 : -1;
}
extern "C" uint32_t BrotliAmdDebugRaggedCopyTile(void) { return brotli_amd_copy_tile_bytes(); }
