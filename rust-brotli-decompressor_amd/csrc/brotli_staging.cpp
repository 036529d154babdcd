// brotli_staging.cpp -- the batch object's entry points beyond "device pointers in, device pointers out" (include/brotli/batch.h): host buffers
// through staging arenas and pinned memory (BrotliAmdBatchDecodeHostDict), the size walk on the device (BrotliAmdBatchSizeHints), and the
// packed decode, which needs no output sizes from its caller (BrotliAmdBatchDecodeDevicePacked / HostPacked).
#include <system_error>
#include <thread>

#include "brotli_host.h"
#include "brotli_size_walk.h"

// (csrc/brotli_size_kernels.hip: the size walk of n streams, one lane a stream)
extern "C" hipError_t brotli_amd_launch_size_walk(const BrotliAmdSizeDesc* d_descs, uint32_t n, uint32_t flags, BrotliAmdSizeHint* d_hints, hipStream_t stream);

using namespace brotli_amd_host;

namespace {

// streams [lo, hi) copied by up to sixteen threads, split by bytes: one(i, false) says stream i's bytes, one(i, true) copies them
template <class One>
void parallel_copy(uint32_t lo, uint32_t hi, One&& one) {
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  size_t bytes = 0; for (uint32_t i = lo; i < hi; i++) bytes += one(i, false);
  const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(hw, bytes >> 20));
  if (nt <= 1) { for (uint32_t i = lo; i < hi; i++) (void)one(i, true); return; }
  std::vector<std::thread> ts; const size_t per = (bytes + nt - 1) / nt; uint32_t i0 = lo;
  for (unsigned t = 0; t < nt && i0 < hi; t++) {
    uint32_t i1 = i0; size_t acc = 0;
    while (i1 < hi && (acc < per || t + 1 == nt)) acc += one(i1++, false);
    try { ts.emplace_back([=, &one]() { for (uint32_t i = i0; i < i1; i++) (void)one(i, true); }); }
    catch (const std::system_error&) { for (uint32_t i = i0; i < i1; i++) (void)one(i, true); }   // (no thread to be had: this one does the part)
    i0 = i1;
  }
  for (auto& t : ts) t.join();
}

// an arena's slots: 64-byte aligned, 64 bytes between them
size_t slot_bytes(size_t n) { return ((n + 63) & ~(size_t)63) + 64; }

// The host entry points' way to the device (BrotliAmdBatchDecodeHostDict, BrotliAmdBatchDecodeHostPacked): where each stream and each distinct
// dictionary lies in the batch object's staging arenas.
struct StagedInputs {
  std::vector<std::pair<const uint8_t*, size_t>> dict_of;   // distinct (pointer, size) pairs (what make_desc would keep of them), in order of appearance
  std::vector<size_t> dict_off, in_off;
  std::vector<int> dict_ix;                                 // per stream: its pair, -1 none
  size_t dict_total = 0, in_total = 0;
  const uint8_t* dict_ptr(const BrotliAmdBatch* b, uint32_t i) const { return dict_ix[i] >= 0 ? b->d_stage_dict + dict_off[(size_t)dict_ix[i]] : nullptr; }
  size_t dict_size(uint32_t i) const { return dict_ix[i] >= 0 ? dict_of[(size_t)dict_ix[i]].second : 0; }
};

// Lays the inputs out and makes the device arenas, the pinned host side and the copy stream.  *pinned: whether the host gave pinned memory for the
// inputs (where it has none to give, the transfers go stream by stream from the caller's own, pageable, buffers).
bool stage_prepare(BrotliAmdBatch* b, uint32_t n, const size_t* in_sizes, const uint8_t* const* dicts, const size_t* dict_sizes, StagedInputs& s, bool* pinned) {
  // custom dictionaries: every distinct (pointer, size) pair is uploaded once -- a batch of documents against one shared dictionary
  // reads one copy of it, which stays in the device's caches
  s.dict_ix.assign(n, -1); s.in_off.resize(n);
  if (dicts && dict_sizes) {
    for (uint32_t i = 0; i < n; i++) {
      if (dicts[i] == nullptr || dict_sizes[i] == 0) continue;
      const size_t tail = std::min(dict_sizes[i], kMaxCustomDict);
      const std::pair<const uint8_t*, size_t> key(dicts[i] + (dict_sizes[i] - tail), tail);
      size_t k = 0;
      if (i != 0 && s.dict_ix[i - 1] >= 0 && s.dict_of[(size_t)s.dict_ix[i - 1]] == key) k = (size_t)s.dict_ix[i - 1];   // (the rule: the stream before's)
      else k = (size_t)(std::find(s.dict_of.begin(), s.dict_of.end(), key) - s.dict_of.begin());
      if (k == s.dict_of.size()) { s.dict_of.push_back(key); s.dict_off.push_back(s.dict_total); s.dict_total += slot_bytes(tail); }
      s.dict_ix[i] = (int)k;
    }
  }
  if (!b->d_stage_dict.reserve(s.dict_total, "hipMalloc(dictionary arena)")) return false;
  // one input arena
  for (uint32_t i = 0; i < n; i++) { s.in_off[i] = s.in_total; s.in_total += slot_bytes(in_sizes[i]); }
  if (!b->d_stage_in.reserve(s.in_total, "hipMalloc(input arena)")) return false;
  *pinned = b->h_pin_in.reserve(s.in_total, nullptr);
  return b->copy_stream || hip_ok(hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking), "hipStreamCreate");
}

// The dictionaries and the inputs on their way (copy_stream; the caller waits on it): with pinned memory the inputs are packed into it by several
// threads, piece by piece, each piece's transfer behind it.
bool stage_upload(BrotliAmdBatch* b, uint32_t n, const uint8_t* const* in, const size_t* in_sizes, const StagedInputs& s, bool pinned) {
  for (size_t k = 0; k < s.dict_of.size(); k++)
    if (!hip_ok(hipMemcpyAsync(b->d_stage_dict + s.dict_off[k], s.dict_of[k].first, s.dict_of[k].second, hipMemcpyHostToDevice, b->copy_stream), "hipMemcpyAsync(dictionary)")) return false;
  if (!pinned) {
    for (uint32_t i = 0; i < n; i++)
      if (in_sizes[i] && !hip_ok(hipMemcpyAsync(b->d_stage_in + s.in_off[i], in[i], in_sizes[i], hipMemcpyHostToDevice, b->copy_stream), "hipMemcpyAsync(input)")) return false;
    return true;
  }
  uint32_t lo = 0;
  while (lo < n) {
    uint32_t hi = lo; size_t acc = 0;
    while (hi < n && acc < ((size_t)32 << 20)) acc += in_sizes[hi++];
    parallel_copy(lo, hi, [&](uint32_t i, bool go) -> size_t { if (go && in_sizes[i]) std::memcpy(b->h_pin_in + s.in_off[i], in[i], in_sizes[i]); return in_sizes[i]; });
    const size_t o0 = s.in_off[lo], o1 = hi < n ? s.in_off[hi] : s.in_total;
    if (!hip_ok(hipMemcpyAsync(b->d_stage_in + o0, b->h_pin_in + o0, o1 - o0, hipMemcpyHostToDevice, b->copy_stream), "hipMemcpyAsync(input)")) return false;
    lo = hi;
  }
  return true;
}

}  // namespace

extern "C" int BrotliAmdBatchDecodeHostDict(BrotliAmdBatch* b, uint32_t n, const uint8_t* const* in, const size_t* in_sizes, uint8_t* const* out,
                                            const size_t* out_caps, const uint8_t* const* dicts, const size_t* dict_sizes, uint32_t flags,
                                            BrotliAmdResult* results) {
  if (!b || n > b->max_streams || (n && (!in || !in_sizes || !out || !out_caps))) { g_last_error = "invalid batch arguments"; return -1; }
  drop_packed(b);
  if (n == 0) { b->outputs = BrotliAmdBatch::Outputs::None; return 0; }
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  StagedInputs staged;
  bool pinned = true;
  if (!stage_prepare(b, n, in_sizes, dicts, dict_sizes, staged, &pinned)) return -1;
  // one output arena, and its pinned host side
  std::vector<size_t> out_off(n);
  size_t out_total = 0;
  for (uint32_t i = 0; i < n; i++) { out_off[i] = out_total; out_total += slot_bytes(out_caps[i]); }
  if (!b->d_stage_out.reserve(out_total, "hipMalloc(output arena)")) return -1;
  pinned = pinned && b->h_pin_out.reserve(out_total, nullptr);
  if (!stage_upload(b, n, in, in_sizes, staged, pinned)) return -1;
  for (uint32_t i = 0; i < n; i++)
    b->h_descs[i] = make_desc(b->d_stage_in + staged.in_off[i], in_sizes[i], b->d_stage_out + out_off[i], out_caps[i], flags, staged.dict_ptr(b, i), staged.dict_size(i));
  b->exact_limit = !(flags & BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT);
  if (!hip_ok(hipStreamSynchronize(b->copy_stream), "hipStreamSynchronize(upload)")) return -1;
  if (submit(b, n, nullptr) != 0) return -1;
  std::vector<BrotliAmdResult> local;
  if (!results) { local.resize(n); results = local.data(); }
  if (BrotliAmdBatchWait(b, results) != 0) return -1;
  // download: pieces of about 32 MiB into pinned memory, the copies into the caller's buffers (several threads) side by side with the
  // next piece's transfer
  const auto got_of = [&](uint32_t i) { return (size_t)std::min<uint64_t>(results[i].decoded_size, out_caps[i]); };
  if (!pinned) {
    for (uint32_t i = 0; i < n; i++)
      if (got_of(i) && !hip_ok(hipMemcpyAsync(out[i], b->d_stage_out + out_off[i], got_of(i), hipMemcpyDeviceToHost, b->copy_stream), "hipMemcpyAsync(output)")) return -1;
    if (!hip_ok(hipStreamSynchronize(b->copy_stream), "hipStreamSynchronize(download)")) return -1;
  } else {
    std::vector<std::pair<uint32_t, uint32_t>> pieces; std::vector<hipEvent_t> evs;
    uint32_t lo = 0;
    bool ok = true;
    while (lo < n && ok) {
      uint32_t hi = lo; size_t acc = 0;
      while (hi < n && acc < ((size_t)32 << 20)) { acc += got_of(hi); hi++; }
      // a transfer per run of streams that filled their slots (the rule); a stream that stopped short of its slot ends a run, so that a
      // failed stream with a large buffer costs its decoded bytes, not its capacity
      for (uint32_t r0 = lo; r0 < hi && ok; ) {
        uint32_t r1 = r0;
        while (r1 + 1 < hi && got_of(r1) + 4096 >= out_caps[r1]) r1++;
        const size_t o0 = out_off[r0], o1 = out_off[r1] + got_of(r1);
        if (o1 > o0) ok = hip_ok(hipMemcpyAsync(b->h_pin_out + o0, b->d_stage_out + o0, o1 - o0, hipMemcpyDeviceToHost, b->copy_stream), "hipMemcpyAsync(output)");
        r0 = r1 + 1;
      }
      hipEvent_t ev = nullptr;
      ok = ok && hip_ok(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate") && hip_ok(hipEventRecord(ev, b->copy_stream), "hipEventRecord");
      evs.push_back(ev); pieces.emplace_back(lo, hi);
      lo = hi;
    }
    for (size_t k = 0; k < pieces.size() && ok; k++) {
      ok = hip_ok(hipEventSynchronize(evs[k]), "hipEventSynchronize");
      if (ok) parallel_copy(pieces[k].first, pieces[k].second, [&](uint32_t i, bool go) -> size_t {
        if (go && got_of(i)) std::memcpy(out[i], b->h_pin_out + out_off[i], got_of(i));
        return got_of(i); });
    }
    (void)hipStreamSynchronize(b->copy_stream);
    for (hipEvent_t ev : evs) if (ev) (void)hipEventDestroy(ev);
    if (!ok) return -1;
  }
  return 0;
}

extern "C" int BrotliAmdBatchDecodeHost(BrotliAmdBatch* b, uint32_t n, const uint8_t* const* in, const size_t* in_sizes, uint8_t* const* out,
                                        const size_t* out_caps, uint32_t flags, BrotliAmdResult* results) {
  return BrotliAmdBatchDecodeHostDict(b, n, in, in_sizes, out, out_caps, nullptr, nullptr, flags, results);
}

// ================================== size hints and the packed decode (batch.h) ==================================
namespace {

// the size walk of n streams on `stream`, waited for: hints[0..n) on the host
int size_hints_device(BrotliAmdBatch* b, uint32_t n, const void* const* d_in, const size_t* in_sizes, uint32_t flags, BrotliAmdSizeHint* hints,
                      hipStream_t stream) {
  const size_t descs_bytes = sizeof(BrotliAmdSizeDesc) * (size_t)n;
  if (!b->d_size.reserve(descs_bytes + sizeof(BrotliAmdSizeHint) * (size_t)n, "hipMalloc(size hints)")) return -1;
  BrotliAmdSizeDesc* d_descs = reinterpret_cast<BrotliAmdSizeDesc*>(b->d_size.get());
  BrotliAmdSizeHint* d_hints = reinterpret_cast<BrotliAmdSizeHint*>(b->d_size + descs_bytes);
  std::vector<BrotliAmdSizeDesc> descs(n);
  for (uint32_t i = 0; i < n; i++) descs[i] = BrotliAmdSizeDesc{static_cast<const uint8_t*>(d_in[i]), in_sizes[i]};
  bool ok = hip_ok(hipMemcpyAsync(d_descs, descs.data(), descs_bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(size descs)");
  ok = ok && hip_ok(brotli_amd_launch_size_walk(d_descs, n, flags & BROTLI_AMD_BATCH_LARGE_WINDOW, d_hints, stream), "brotli_amd_size_walk_kernel launch");
  ok = ok && hip_ok(hipMemcpyAsync(hints, d_hints, sizeof(BrotliAmdSizeHint) * (size_t)n, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(size hints)");
  // (waited for in any case: the copies read and write the caller's and this function's pageable memory)
  return hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize(size hints)") && ok ? 0 : -1;
}

// one ragged-copy launch of m segments on `stream` (the table is uploaded from pageable memory: the caller waits on the stream before `segs` goes)
bool packed_copy(BrotliAmdBatch* b, const std::vector<BrotliAmdCopySeg>& segs, uint64_t bytes, hipStream_t stream) {
  const uint32_t m = (uint32_t)segs.size();
  if (!b->d_pack_segs.reserve(sizeof(BrotliAmdCopySeg) * (size_t)m, "hipMalloc(copy segments)")) return false;
  BrotliAmdCopySeg* d_segs = reinterpret_cast<BrotliAmdCopySeg*>(b->d_pack_segs.get());
  return hip_ok(hipMemcpyAsync(d_segs, segs.data(), sizeof(BrotliAmdCopySeg) * (size_t)m, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(copy segments)") &&
         hip_ok(brotli_amd_launch_ragged_copy_sized(d_segs, m, bytes, stream), "brotli_amd_ragged_copy_kernel launch");
}

constexpr uint64_t kPackGrowRound = 65536;   // a grown slot is a multiple of this

// h_descs[0..m) filled: one launch, waited for (larger-arena passes included), no second look at full buffers
bool packed_launch(BrotliAmdBatch* b, uint32_t m, hipStream_t stream) {
  if (!decode_descs(b, m, stream, false)) return false;
  b->last_packed_launches++;
  const float ms = BrotliAmdBatchLastKernelMs(b);
  if (ms > 0.0f) b->packed_ms += ms;
  return true;
}

// A stream's counters over the launch that ran out of room and the one that went on in a larger slot: sums -- but a stream that had reached no
// boundary started again from byte 0, and its first launch does not count.
BrotliAmdStreamStatus sum_over_rounds(const BrotliAmdStreamStatus& first, BrotliAmdStreamStatus next) {
  if (first.resume.window_bits != 0u) {
    next.num_metablocks += first.num_metablocks; next.spilled_metablocks += first.spilled_metablocks;
    next.num_commands += first.num_commands; next.engine_commands += first.engine_commands;
  }
  return next;
}

// BrotliAmdBatchDecodeDevicePacked behind its argument checks (the steps: batch.h)
int packed_decode(BrotliAmdBatch* b, uint32_t n, const void* const* d_in, const size_t* in_sizes, const void* const* d_dicts,
                  const size_t* dict_sizes, uint64_t max_out_bytes, uint32_t flags, hipStream_t stream, BrotliAmdResult* results) {
  drop_packed(b);
  if (n == 0) { b->packed_offsets.assign(1, 0); b->packed_valid = true; b->n = 0; b->launched = false; return 0; }
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  // 1. the hints; 2. first capacities; the slots back to back
  std::vector<BrotliAmdSizeHint> hints(n);
  if (size_hints_device(b, n, d_in, in_sizes, flags, hints.data(), stream) != 0) return -1;
  const uint64_t limit = max_out_bytes ? max_out_bytes : ~(uint64_t)0;
  std::vector<uint64_t> cap(n);
  std::vector<uint8_t*> out(n);
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    const BrotliAmdSizeHint& h = hints[i];
    const uint64_t c = h.exact && h.status == BROTLI_AMD_SIZE_OK ? h.bytes
                                                                 : std::max<uint64_t>(kGuessOutFloor, h.bytes + kGuessOutFactor * ((uint64_t)in_sizes[i] - h.walked_in));
    cap[i] = std::min(c, limit);
    total += cap[i];
  }
  if (!b->d_pack_slots.reserve((size_t)total, "hipMalloc(packed slots)", kReaderSlack)) return -1;   // (the slack: a slot of no bytes at the end has an address as well)
  { uint64_t at = 0; for (uint32_t i = 0; i < n; i++) { out[i] = b->d_pack_slots + at; at += cap[i]; } }
  const bool dicts = d_dicts && dict_sizes;
  const auto desc_of = [&](uint32_t i) { return make_desc(d_in[i], in_sizes[i], out[i], cap[i], flags, dicts ? d_dicts[i] : nullptr, dicts ? dict_sizes[i] : 0); };
  std::vector<DevBuf<>> rounds;   // the growth rounds' slots: freed when the call is over, on every path
  const auto done = [&](int rc) {
    b->n = 0; b->launched = false;   // (nothing for BrotliAmdBatchWait or BrotliAmdBatchRelaunch to come back to)
    if (rc != 0) drop_packed(b);
    else b->packed_valid = true;
    return rc;
  };
  // 3. one launch over all of them
  for (uint32_t i = 0; i < n; i++) b->h_descs[i] = desc_of(i);
  if (!packed_launch(b, n, stream)) return done(-1);
  std::vector<BrotliAmdStreamStatus> st(b->h_status.get(), b->h_status + n);
  // 4. the streams whose slot was too small, and they alone: a larger slot, what they have decoded moved there, resumed
  bool moved = false;
  for (;;) {
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < n; i++) if (st[i].result == BROTLI_DECODER_RESULT_NEEDS_MORE_OUTPUT && cap[i] < limit) idx.push_back(i);
    if (idx.empty()) break;
    const uint32_t m = (uint32_t)idx.size();
    std::vector<uint64_t> ncap(m);
    uint64_t rtotal = 0;
    for (uint32_t j = 0; j < m; j++) {
      const uint32_t i = idx[j];
      uint64_t want = std::max<uint64_t>(2u * cap[i], 1u);
      const uint64_t at_in = st[i].resume.window_bits != 0u ? st[i].resume.bit_pos >> 3 : 0u;
      if (at_in != 0u) {   // what the stream's ratio up to its resume point says of the whole
        const unsigned __int128 est = (unsigned __int128)st[i].resume.out_pos * in_sizes[i] / at_in;
        want = std::max<uint64_t>(want, est > (unsigned __int128)limit ? limit : (uint64_t)est);
      }
      want = want > limit - (kPackGrowRound - 1u) ? limit : (want + kPackGrowRound - 1u) / kPackGrowRound * kPackGrowRound;
      ncap[j] = std::min(want, limit);
      rtotal += ncap[j];
    }
    rounds.emplace_back();
    if (!rounds.back().reserve((size_t)rtotal, "hipMalloc(grown packed slots)", kReaderSlack)) return done(-1);
    uint8_t* fresh = rounds.back();
    // everything below the resume point is final: the last metablock boundary, or the command boundary noted inside the metablock behind it
    std::vector<BrotliAmdCopySeg> segs(m);
    uint64_t at = 0, copy_bytes = 0;
    for (uint32_t j = 0; j < m; j++) {
      const uint32_t i = idx[j];
      const BrotliAmdResume& r = st[i].resume;
      uint64_t keep = r.window_bits == 0u ? 0u : std::max<uint64_t>(r.out_pos, r.mid_valid ? r.mid_out_pos : 0u);
      keep = std::min(keep, cap[i]);
      segs[j] = BrotliAmdCopySeg{out[i], fresh + at, keep};
      copy_bytes += keep;
      out[i] = fresh + at; cap[i] = ncap[j]; at += ncap[j];
    }
    if (!packed_copy(b, segs, copy_bytes, stream)) { (void)hipStreamSynchronize(stream); return done(-1); }
    b->last_packed_copies++;
    for (uint32_t j = 0; j < m; j++) {
      const uint32_t i = idx[j];
      BrotliAmdStreamDesc& d = b->h_descs[j];
      d = desc_of(i);
      if (st[i].resume.window_bits != 0u) { d.flags |= BROTLI_AMD_FLAG_RESUME; d.resume = st[i].resume; }   // (else: no boundary yet, from byte 0 again)
    }
    if (!packed_launch(b, m, stream)) return done(-1);
    for (uint32_t j = 0; j < m; j++) st[idx[j]] = sum_over_rounds(st[idx[j]], b->h_status[j]);
    moved = true;
  }
  // 5. pack
  b->packed_offsets.resize((size_t)n + 1);
  b->packed_offsets[0] = 0;
  bool in_place = !moved;
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t got = std::min(st[i].decoded_size, cap[i]);
    st[i].decoded_size = got;
    in_place = in_place && got == cap[i];
    b->packed_offsets[i + 1] = b->packed_offsets[i] + got;
  }
  if (in_place) b->packed_out = b->d_pack_slots;
  else {
    const uint64_t bytes = b->packed_offsets[n];
    if (!b->d_pack_tight.reserve((size_t)bytes, "hipMalloc(packed output)", kReaderSlack)) return done(-1);
    std::vector<BrotliAmdCopySeg> segs(n);
    for (uint32_t i = 0; i < n; i++) segs[i] = BrotliAmdCopySeg{out[i], b->d_pack_tight + b->packed_offsets[i], b->packed_offsets[i + 1] - b->packed_offsets[i]};
    const bool ok = packed_copy(b, segs, bytes, stream);
    if (!hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize(packed gather)") || !ok) return done(-1);
    b->last_packed_copies++;
    b->packed_out = b->d_pack_tight;
  }
  if (results) for (uint32_t i = 0; i < n; i++) results[i] = to_result(st[i]);
  return done(0);
}

}  // namespace

extern "C" int BrotliAmdDebugSizeWalk(const uint8_t* in, size_t n, uint32_t flags, BrotliAmdSizeHint* hint) {
  if (!hint || (n && !in)) return -1;
  *hint = brotli_amd_size_walk(BrotliAmdWalkBytes{in}, n, flags);
  return 0;
}

extern "C" int BrotliAmdBatchSizeHints(BrotliAmdBatch* b, uint32_t n, const void* const* d_in, const size_t* in_sizes, uint32_t flags,
                                       BrotliAmdSizeHint* hints, void* hip_stream) {
  if (!b || (n && (!d_in || !in_sizes || !hints))) { g_last_error = "invalid batch arguments"; return -1; }
  if (n == 0) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  return size_hints_device(b, n, d_in, in_sizes, flags, hints, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchDecodeDevicePacked(BrotliAmdBatch* b, uint32_t n, const void* const* d_in, const size_t* in_sizes,
                                                const void* const* d_dicts, const size_t* dict_sizes, uint64_t max_out_bytes, uint32_t flags,
                                                void* hip_stream, BrotliAmdResult* results) {
  if (!b || n > b->max_streams || (n && (!d_in || !in_sizes))) { g_last_error = "invalid batch arguments"; return -1; }
  DeviceGuard guard;
  return packed_decode(b, n, d_in, in_sizes, d_dicts, dict_sizes, max_out_bytes, flags, static_cast<hipStream_t>(hip_stream), results);
}

extern "C" const void* BrotliAmdBatchPackedOutput(BrotliAmdBatch* b, const uint64_t** offsets) {
  if (offsets) *offsets = b && !b->packed_offsets.empty() ? b->packed_offsets.data() : nullptr;
  return b ? b->packed_out : nullptr;
}

extern "C" int BrotliAmdBatchPackedFetch(BrotliAmdBatch* b, uint8_t* host_dst) {
  if (!b || b->packed_offsets.empty()) { g_last_error = "no packed output"; return -1; }
  const uint64_t bytes = b->packed_offsets.back();
  if (bytes == 0) return 0;
  if (!b->packed_out || !host_dst) { g_last_error = "no packed output"; return -1; }
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  return hip_ok(hipMemcpy(host_dst, b->packed_out, (size_t)bytes, hipMemcpyDeviceToHost), "hipMemcpy(packed output)") ? 0 : -1;
}

extern "C" uint32_t BrotliAmdBatchLastPackedLaunches(BrotliAmdBatch* b) { return b ? b->last_packed_launches : 0; }
extern "C" uint32_t BrotliAmdBatchLastPackedCopies(BrotliAmdBatch* b) { return b ? b->last_packed_copies : 0; }

extern "C" int BrotliAmdBatchDecodeHostPacked(BrotliAmdBatch* b, uint32_t n, const uint8_t* const* in, const size_t* in_sizes,
                                              const uint8_t* const* dicts, const size_t* dict_sizes, uint64_t max_out_bytes, uint32_t flags,
                                              BrotliAmdResult* results) {
  if (!b || n > b->max_streams || (n && (!in || !in_sizes))) { g_last_error = "invalid batch arguments"; return -1; }
  DeviceGuard guard;
  if (n == 0) return packed_decode(b, 0, nullptr, nullptr, nullptr, nullptr, max_out_bytes, flags, nullptr, results);
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  // the staging of BrotliAmdBatchDecodeHostDict: every distinct dictionary once into its arena, the streams into the input arena
  StagedInputs staged;
  bool pinned = true;
  if (!stage_prepare(b, n, in_sizes, dicts, dict_sizes, staged, &pinned)) return -1;
  const bool ok = stage_upload(b, n, in, in_sizes, staged, pinned);
  if (!hip_ok(hipStreamSynchronize(b->copy_stream), "hipStreamSynchronize(upload)") || !ok) return -1;
  std::vector<const void*> d_in(n), d_dict(n, nullptr);
  std::vector<size_t> d_dict_size(n, 0);
  for (uint32_t i = 0; i < n; i++) { d_in[i] = b->d_stage_in + staged.in_off[i]; d_dict[i] = staged.dict_ptr(b, i); d_dict_size[i] = staged.dict_size(i); }
  return packed_decode(b, n, d_in.data(), in_sizes, d_dict.data(), d_dict_size.data(), max_out_bytes, flags, nullptr, results);
}
