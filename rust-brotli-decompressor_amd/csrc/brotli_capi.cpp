// brotli_capi.cpp -- the reference's C ABI (include/brotli/decode.h) on top of the batch object (brotli_batch.cpp).
//
// Mirrors, by behaviour, reference src/ffi/mod.rs (entry points, argument validation, error latching),
// src/lib.rs:336-468 (one-shot helpers, BrotliDecoderReturnInfo) and the caller-visible contract of
// src/decode.rs:2779-3403 (BrotliDecompressStream: what is consumed, what is delivered, when each result is
// returned).  It owns no decoder: all decoding happens in brotli_kernels.hip.  The streaming entry point keeps
// the stream's compressed bytes and its output in device memory and re-launches the kernel from the last
// completed metablock boundary each time more input arrives (BrotliAmdResume), which is the device analogue
// of the reference's resumable state machine.  When no HIP device is usable every entry point fails with
// BROTLI_DECODER_ERROR_UNREACHABLE and a message -- there is no CPU path to fall back to.
#include <cstdio>
#include <cstdlib>
#include <new>

#include "brotli_stream.h"

using namespace brotli_amd_host;

// ============================================ error strings ============================================
// reference src/state.rs:533-578 (including the historical "FL_SPACE" spelling of CL_SPACE)
extern "C" const char* BrotliDecoderErrorString(BrotliDecoderErrorCode c) {
  switch ((int)c) {
    case 0: return "NO_ERROR";
    case 1: return "SUCCESS";
    case 2: return "NEEDS_MORE_INPUT";
    case 3: return "NEEDS_MORE_OUTPUT";
    case -1: return "ERROR_FORMAT_EXUBERANT_NIBBLE";
    case -2: return "ERROR_FORMAT_RESERVED";
    case -3: return "ERROR_FORMAT_EXUBERANT_META_NIBBLE";
    case -4: return "ERROR_FORMAT_SIMPLE_HUFFMAN_ALPHABET";
    case -5: return "ERROR_FORMAT_SIMPLE_HUFFMAN_SAME";
    case -6: return "ERROR_FORMAT_FL_SPACE";
    case -7: return "ERROR_FORMAT_HUFFMAN_SPACE";
    case -8: return "ERROR_FORMAT_CONTEXT_MAP_REPEAT";
    case -9: return "ERROR_FORMAT_BLOCK_LENGTH_1";
    case -10: return "ERROR_FORMAT_BLOCK_LENGTH_2";
    case -11: return "ERROR_FORMAT_TRANSFORM";
    case -12: return "ERROR_FORMAT_DICTIONARY";
    case -13: return "ERROR_FORMAT_WINDOW_BITS";
    case -14: return "ERROR_FORMAT_PADDING_1";
    case -15: return "ERROR_FORMAT_PADDING_2";
    case -16: return "ERROR_FORMAT_DISTANCE";
    case -19: return "ERROR_DICTIONARY_NOT_SET";
    case -20: return "ERROR_INVALID_ARGUMENTS";
    case -21: return "ERROR_ALLOC_CONTEXT_MODES";
    case -22: return "ERROR_ALLOC_TREE_GROUPS";
    case -25: return "ERROR_ALLOC_CONTEXT_MAP";
    case -26: return "ERROR_ALLOC_RING_BUFFER_1";
    case -27: return "ERROR_ALLOC_RING_BUFFER_2";
    case -30: return "ERROR_ALLOC_BLOCK_TYPE_TREES";
    case -31: return "ERROR_UNREACHABLE";
    default: return "ERROR_UNREACHABLE";
  }
}

extern "C" uint32_t BrotliDecoderVersion(void) { return 0x1000f00; }  // ffi/mod.rs:588-590

// ============================================== one-shot ==============================================
namespace {

// window bits announced by the first bytes of a stream (RFC 7932 section 9.1; same answer as the reference's
// lg_window_size, src/decode.rs:1221-1253).  0 when not decidable.
uint32_t peek_window_bits(const uint8_t* in, size_t n) {
  if (n == 0) return 0;
  uint8_t b = in[0];
  if ((b & 1) == 0) return 16;
  if ((b & 0xE) != 0) return 17 + ((b >> 1) & 7);
  uint32_t n3 = (b >> 4) & 7;
  if (n3 == 1) {  // large window: 6 bits of WBITS follow the reserved bit
    if (n < 2 || (b & 0x80)) return 0;
    uint32_t w = in[1] & 0x3F;
    return (w >= 10 && w <= 30) ? w : 0;
  }
  return n3 ? 8 + n3 : 17;
}

// Device resources of the one-shot entry points: one set per calling thread (the reference's one-shot calls share
// nothing -- src/lib.rs:447-468 builds a fresh state per call -- so concurrent callers must not serialise on a lock);
// freed when the thread ends.
struct OneShot {
  BrotliAmdBatch* batch = nullptr;
  DevBuf<> d_in, d_out;
  int device = -1;
  void release() {
    if (batch) BrotliAmdBatchDestroy(batch);   // (waits for the device)
    if (d_in || d_out) { DeviceGuard guard; if (device >= 0) (void)hipSetDevice(device); d_in.release(); d_out.release(); }
    batch = nullptr; device = -1;
  }
  // staging for `need` bytes: 4 KiB at least
  static bool grow(DevBuf<>& buf, size_t need) { return buf.reserve(std::max<size_t>(need, 4096), "hipMalloc(one-shot staging)", kReaderSlack); }
  ~OneShot() { release(); }
};
thread_local OneShot t_oneshot;

void fill_error(BrotliDecoderReturnInfo* r, BrotliDecoderErrorCode code, const char* msg) {
  std::memset(r, 0, sizeof *r);
  r->result = BROTLI_DECODER_RESULT_ERROR;
  r->code = code;
  std::snprintf(r->error, sizeof r->error, "%s", msg ? msg : BrotliDecoderErrorString(code));
}

// Decode with output capacity `cap` on the device; returns false on a runtime (HIP) failure.
bool run_once(OneShot& o, size_t n_in, size_t cap, uint32_t flags, BrotliAmdStreamStatus* st) {
  o.batch->h_descs[0] = make_desc(o.d_in, n_in, o.d_out, cap, flags);
  if (!decode_descs(o.batch, 1, nullptr, kExactLimitDefault)) return false;
  *st = o.batch->h_status[0];
  return true;
}

// reference src/lib.rs:447-468 (brotli_decode) + BrotliDecoderReturnInfo::new (lib.rs:343-370)
BrotliDecoderReturnInfo oneshot_decode(const uint8_t* in, size_t n_in, uint8_t* out, size_t cap, BrotliAmdStreamStatus* status_out = nullptr) {
  BrotliDecoderReturnInfo r;
  OneShot& o = t_oneshot;
  DeviceGuard guard;
  int dev = 0;
  if (!current_device(&dev)) { fill_error(&r, BROTLI_DECODER_ERROR_UNREACHABLE, ("HIP device unavailable: " + g_last_error).c_str()); return r; }
  if (o.batch && o.device != dev) o.release();  // the caller moved to another device
  if (!o.batch) { o.batch = BrotliAmdBatchCreate(1, 0, 0); o.device = dev; }
  if (!o.batch) { fill_error(&r, BROTLI_DECODER_ERROR_UNREACHABLE, ("HIP device unavailable: " + g_last_error).c_str()); return r; }
  const uint32_t flags = BROTLI_AMD_FLAG_LARGE_WINDOW;  // lib.rs:457 -> BrotliState::new -> large_window = true
  BrotliAmdStreamStatus st;
  bool ok = OneShot::grow(o.d_in, n_in) && OneShot::grow(o.d_out, cap);
  ok = ok && (n_in == 0 || hip_ok(hipMemcpy(o.d_in, in, n_in, hipMemcpyHostToDevice), "hipMemcpy(input)"));
  ok = ok && run_once(o, n_in, cap, flags, &st);
  if (ok && st.result == BROTLI_DECODER_RESULT_NEEDS_MORE_OUTPUT) {
    // The reference only notices a full output buffer at its next ring-buffer flush (decode.rs:1693-1738),
    // so what it reports depends on what the stream does up to the next multiple of the window size.  Decode
    // again with room up to that point and map the outcome (flush_point_cap, second_verdict_wins: as the batch's settle pass does).
    uint32_t wbits = peek_window_bits(in, n_in);
    if (wbits) {
      const uint64_t rb = st.ring_bytes ? st.ring_bytes : (uint64_t)1 << wbits;  // (the emulated ring: smaller than the window for a short last metablock)
      const size_t cap2 = (size_t)flush_point_cap(cap, rb);
      BrotliAmdStreamStatus st2;
      if (OneShot::grow(o.d_out, cap2) && run_once(o, n_in, cap2, flags, &st2)) {
        if (second_verdict_wins(st2, cap2)) {
          st = st2; st.decoded_size = std::min<uint64_t>(st2.decoded_size, cap);
        } else {
          st.result = BROTLI_DECODER_RESULT_NEEDS_MORE_OUTPUT; st.error_code = BROTLI_DECODER_NEEDS_MORE_OUTPUT; st.decoded_size = cap;
        }
      } else ok = false;
    }
  }
  if (!ok) { fill_error(&r, BROTLI_DECODER_ERROR_UNREACHABLE, ("HIP runtime failure: " + g_last_error).c_str()); return r; }
  size_t got = (size_t)std::min<uint64_t>(st.decoded_size, cap);
  if (got && !hip_ok(hipMemcpy(out, o.d_out, got, hipMemcpyDeviceToHost), "hipMemcpy(output)")) {
    fill_error(&r, BROTLI_DECODER_ERROR_UNREACHABLE, ("HIP runtime failure: " + g_last_error).c_str());
    return r;
  }
  if (status_out) *status_out = st;
  std::memset(&r, 0, sizeof r);
  r.decoded_size = got;
  r.result = (BrotliDecoderResult)st.result;
  r.code = (BrotliDecoderErrorCode)st.error_code;
  std::snprintf(r.error, sizeof r.error, "%s", BrotliDecoderErrorString(r.code));
  return r;
}

// reference src/ffi/mod.rs:45-61: pointer/length pairs that a slice could not be made of
template <typename T>
bool valid_slice(const T* p, size_t len) {
  if (len == 0) return true;
  if (!p) return false;
  if (((uintptr_t)p) % alignof(T) != 0) return false;
  if (len > (size_t)(PTRDIFF_MAX) / sizeof(T)) return false;
  return (uintptr_t)p + len * sizeof(T) >= (uintptr_t)p;
}

BrotliDecoderReturnInfo invalid_arguments() {
  BrotliDecoderReturnInfo r;
  fill_error(&r, BROTLI_DECODER_ERROR_INVALID_ARGUMENTS, nullptr);
  return r;
}

}  // namespace

extern "C" BrotliDecoderReturnInfo BrotliDecoderDecompressWithReturnInfo(size_t encoded_size, const uint8_t* encoded_buffer, size_t decoded_size,
                                                                         uint8_t* decoded_buffer) {
  if (!valid_slice(encoded_buffer, encoded_size) || !valid_slice(decoded_buffer, decoded_size)) return invalid_arguments();
  return oneshot_decode(encoded_buffer, encoded_size, decoded_buffer, decoded_size);
}

extern "C" BrotliDecoderResult BrotliDecoderDecompress(size_t encoded_size, const uint8_t* encoded_buffer, size_t* decoded_size,
                                                       uint8_t* decoded_buffer) {
  if (!valid_slice(decoded_size, 1)) return BROTLI_DECODER_RESULT_ERROR;  // ffi/mod.rs:269-271
  BrotliDecoderReturnInfo r = BrotliDecoderDecompressWithReturnInfo(encoded_size, encoded_buffer, *decoded_size, decoded_buffer);
  *decoded_size = r.decoded_size;
  return r.result == BROTLI_DECODER_RESULT_SUCCESS ? BROTLI_DECODER_RESULT_SUCCESS : BROTLI_DECODER_RESULT_ERROR;
}

extern "C" BrotliDecoderReturnInfo BrotliDecoderDecompressPrealloc(size_t encoded_size, const uint8_t* encoded_buffer, size_t decoded_size,
                                                                   uint8_t* decoded_buffer, size_t scratch_u8_size, uint8_t* scratch_u8_buffer,
                                                                   size_t scratch_u32_size, uint32_t* scratch_u32_buffer, size_t scratch_hc_size,
                                                                   HuffmanCode* scratch_hc_buffer) {
  if (!valid_slice(encoded_buffer, encoded_size) || !valid_slice(decoded_buffer, decoded_size) ||
      !valid_slice(scratch_u8_buffer, scratch_u8_size) || !valid_slice(scratch_u32_buffer, scratch_u32_size) ||
      !valid_slice(scratch_hc_buffer, scratch_hc_size))
    return invalid_arguments();
  // The reference decodes out of the three scratch slices (src/lib.rs:374-401: stack allocators over them) and a
  // request they cannot serve panics, which the C ABI reports as ERROR_UNREACHABLE with decoded_size 0
  // (src/ffi/mod.rs:686-713).  Nothing is decoded out of them here (the tables live in the GPU's LDS), but the same
  // requests are accounted: the context-map prefix code at creation (state.rs:395), block-type and block-length trees
  // at the first compressed metablock (decode.rs:2958-2969), per metablock its prefix codes (1080 cells and one u32
  // each, huffman/mod.rs:61-72), its context modes and maps (decode.rs:1295, 3155), and the ring buffer
  // (decode.rs:1843-1855).  The model is the peak of what is alive at once: a slice large enough for the peak but too
  // fragmented for the reference's first-fit allocator succeeds here and fails there (documented in decode.h).
  constexpr uint64_t kTable = 1080;  // BROTLI_HUFFMAN_MAX_TABLE_SIZE, huffman/mod.rs:36
  if (scratch_hc_size < kTable) { BrotliDecoderReturnInfo r; fill_error(&r, BROTLI_DECODER_ERROR_UNREACHABLE, "scratch exhausted (HuffmanCode)"); return r; }
  BrotliAmdStreamStatus st;
  std::memset(&st, 0, sizeof st);
  BrotliDecoderReturnInfo r = oneshot_decode(encoded_buffer, encoded_size, decoded_buffer, decoded_size, &st);
  if (r.code == BROTLI_DECODER_ERROR_UNREACHABLE || r.code == BROTLI_DECODER_ERROR_INVALID_ARGUMENTS) return r;
  const uint64_t need_hc = kTable + (st.any_compressed ? 6 * kTable : 0) + (uint64_t)st.peak_trees * kTable;
  const uint64_t need_u32 = st.peak_trees;
  const uint64_t need_u8 = (st.ring_bytes ? st.ring_bytes + 42 + 24 : 0) + st.peak_map_bytes;
  if (need_hc > scratch_hc_size || need_u32 > scratch_u32_size || need_u8 > scratch_u8_size) {
    fill_error(&r, BROTLI_DECODER_ERROR_UNREACHABLE, need_hc > scratch_hc_size ? "scratch exhausted (HuffmanCode)" : need_u32 > scratch_u32_size ? "scratch exhausted (u32)" : "scratch exhausted (u8)");
    return r;
  }
  return r;
}

// ============================================== streaming ==============================================
namespace {

void* st_alloc(BrotliDecoderState* s, size_t n) { return s->alloc_func ? s->alloc_func(s->opaque, n) : std::malloc(n); }
void st_free(BrotliDecoderState* s, void* p) { if (!p) return; if (s->free_func) s->free_func(s->opaque, p); else std::free(p); }

bool fatal(int code) { return code < 0; }

void set_runtime_error(BrotliDecoderState* s, const char* what) {
  s->error_code = BROTLI_DECODER_ERROR_UNREACHABLE;
  std::snprintf(s->error_text, sizeof s->error_text, "%s: %s", what, g_last_error.c_str());
  s->has_error_text = true;
}

// A device buffer of the state, at least `need` bytes, that starts with bytes [from, from + keep) of the old one: where a new one is needed it has
// twice the old one's bytes (from == 0: the buffer grows) or as many (from != 0: it is trimmed), 64 KiB at least.
bool dev_rebase(DevBuf<>& buf, size_t from, size_t keep, size_t need) {
  const size_t grown = std::max<size_t>(std::max<size_t>(need, from == 0 ? buf.capacity() * 2 : buf.capacity()), 1 << 16);
  return buf.rebase(from, keep, need, grown, "hipMalloc(stream buffer)", kReaderSlack);
}

size_t hand_over(BrotliDecoderState* s, uint8_t* dst, size_t room) {
  size_t n = std::min(room, s->outq_len - s->outq_off);
  if (n) { std::memcpy(dst, s->outq + s->outq_off, n); s->outq_off += n; s->total_out += n; }
  if (s->outq_off == s->outq_len) s->outq_off = s->outq_len = 0;
  return n;
}

// What lies in front of everything a later pass can touch is dropped: input below the last completed metablock
// boundary (with a margin: the reader fetches whole 256-byte pieces), output below both the bytes still to be copied
// off the device and one window (the farthest a back-reference reaches) in front of that boundary.  Memory of an
// instance stays O(window + one metablock), not O(stream).
bool trim_buffers(BrotliDecoderState* s, bool eager = false) {
  if (!s->have_resume || s->resume.window_bits == 0) return true;
  const uint64_t in_keep = (s->resume.bit_pos >> 3) > 1024 ? ((s->resume.bit_pos >> 3) - 1024) & ~(uint64_t)255 : 0;
  if (in_keep > s->in_base && in_keep - s->in_base >= std::max<uint64_t>(1 << 16, s->d_in.capacity() / 2)) {
    const size_t from = (size_t)(in_keep - s->in_base), keep = (size_t)(s->d_in_len - in_keep);
    if (!dev_rebase(s->d_in, from, keep, keep)) return false;
    s->in_base = in_keep;
  }
  const uint64_t window = 1ull << s->resume.window_bits;
  uint64_t out_keep = s->resume.out_pos > window ? s->resume.out_pos - window : 0;
  if (s->fetched < out_keep) out_keep = s->fetched;
  out_keep &= ~(uint64_t)255;
  if (out_keep > s->out_base && out_keep - s->out_base >= (eager ? std::max<uint64_t>(1 << 16, s->d_out.capacity() / 4) : std::max<uint64_t>(1 << 20, s->d_out.capacity() / 2))) {
    const size_t from = (size_t)(out_keep - s->out_base);
    const size_t keep = s->d_out.capacity() - from;  // (whatever the last pass wrote lies below the buffer's end)
    if (!dev_rebase(s->d_out, from, keep, s->d_out.capacity())) return false;
    s->out_base = out_keep;
  }
  return true;
}

}  // namespace

// ---- The phases of one BrotliDecoderDecompressStream call (brotli_stream.h) ----
bool brotli_amd_host::reserve_outq(BrotliDecoderState* s, size_t n) {
  if (s->outq_len + n <= s->outq_cap) return true;
  size_t ncap = std::max(s->outq_cap * 2, s->outq_len + n);
  uint8_t* nq = static_cast<uint8_t*>(st_alloc(s, ncap));
  if (!nq) return false;
  if (s->outq_len) std::memcpy(nq, s->outq, s->outq_len);
  st_free(s, s->outq);
  s->outq = nq; s->outq_cap = ncap;
  return true;
}

bool brotli_amd_host::stream_ensure_out(BrotliDecoderState* s) {
  const size_t pending_in = (size_t)(s->d_in_len - s->in_base);
  return dev_rebase(s->d_out, 0, s->d_out.capacity(), std::max<size_t>(s->d_out.capacity(), std::max<size_t>(kGuessOutFloor, kGuessOutFactor * pending_in)));
}

BrotliAmdStreamDesc brotli_amd_host::stream_desc(const BrotliDecoderState* s) {
  BrotliAmdStreamDesc d = make_desc(reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(s->d_in.get()) - (uintptr_t)s->in_base), s->d_in_len,
                                    reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(s->d_out.get()) - (uintptr_t)s->out_base), s->out_base + s->d_out.capacity(),
                                    (s->large_window ? BROTLI_AMD_FLAG_LARGE_WINDOW : 0u) | (s->canny ? 0u : BROTLI_AMD_FLAG_NO_CANNY), s->d_dict, s->dict_len);
  if (s->have_resume) { d.flags |= BROTLI_AMD_FLAG_RESUME; d.resume = s->resume; }
  return d;
}

void brotli_amd_host::stream_note_status(BrotliDecoderState* s, const BrotliAmdStreamStatus& st) {
  s->device_commands += st.num_commands;
  if (st.resume.window_bits != 0) { s->resume = st.resume; s->have_resume = true; }
}

bool brotli_amd_host::stream_grow_out(BrotliDecoderState* s) {
  const uint64_t before = s->out_base;
  if (!trim_buffers(s, true)) return false;
  const uint64_t live = (s->have_resume ? s->resume.out_pos : 0) > s->out_base ? (s->have_resume ? s->resume.out_pos : 0) - s->out_base : 0;
  if (s->out_base == before || live > s->d_out.capacity() / 2)
    if (!dev_rebase(s->d_out, 0, s->d_out.capacity(), s->d_out.capacity() * 2)) return false;
  return true;
}

namespace {

// Copies what the reference would have flushed by now off the device, behind what the caller has not taken yet.
// 0 = ok, 1 = HIP failure, 2 = allocation failure
int fetch_output(BrotliDecoderState* s, uint64_t deliverable) {
  if (deliverable <= s->fetched) return 0;
  size_t n = (size_t)(deliverable - s->fetched);
  if (!reserve_outq(s, n)) return 2;
  if (!hip_ok(hipMemcpy(s->outq + s->outq_len, s->d_out + (s->fetched - s->out_base), n, hipMemcpyDeviceToHost), "hipMemcpy(output)")) return 1;
  s->outq_len += n;
  s->fetched = deliverable;
  return 0;
}

// One decode pass over everything received so far, from the last completed metablock boundary.
// 0 = ok, 1 = HIP failure, 2 = allocation failure
int decode_pass(BrotliDecoderState* s, BrotliAmdStreamStatus* st) {
  for (;;) {
    if (!stream_ensure_out(s)) return 1;
    s->batch->h_descs[0] = stream_desc(s);
    if (!decode_descs(s->batch, 1, nullptr, kExactLimitDefault)) return 1;
    *st = s->batch->h_status[0];
    stream_note_status(s, *st);
    // bytes the reference would have flushed by now: all of them on success / needs-more-input, the part
    // below the last ring-buffer boundary on a fatal error (decode.rs:2835-2846, 2899-2913)
    if (int e = fetch_output(s, st->decoded_size)) return e;
    if (st->result != BROTLI_DECODER_RESULT_NEEDS_MORE_OUTPUT) return 0;
    if (!stream_grow_out(s)) return 1;
  }
}

}  // namespace

bool brotli_amd_host::stream_begin(BrotliDecoderState* s, size_t* available_in, const uint8_t** next_in, size_t* available_out, uint8_t** next_out, size_t* total_out,
                  BrotliDecoderResult* result) {
  *result = BROTLI_DECODER_RESULT_ERROR;
  if (!s || !available_in || !next_in || !available_out || !next_out) {  // ffi/mod.rs:397-407
    if (s) s->error_code = BROTLI_DECODER_ERROR_INVALID_ARGUMENTS;
    return true;
  }
  if (!valid_slice(*next_in, *available_in) || !valid_slice(*next_out, *available_out)) {
    s->error_code = BROTLI_DECODER_ERROR_INVALID_ARGUMENTS;
    return true;
  }
  if (fatal(s->error_code)) return true;  // decode.rs:2796-2798
  if ((uint64_t)*available_in >= (1ull << 32)) {                 // decode.rs:2799-2801
    s->error_code = BROTLI_DECODER_ERROR_INVALID_ARGUMENTS;
    return true;
  }
  // Output the decoder OWES comes first, and while it does not fit no input is consumed (a caller that sees
  // NEEDS_MORE_OUTPUT finds its input where it left it: bit_reader/mod.rs:295-306).  Owed is what the reference has to write
  // before it decodes on: the end of the stream (decode.rs:3382-3397), the bytes in front of a fatal error, and a full ring
  // buffer (decode.rs:1693-1738) -- this decoder keeps no ring, so "a window's worth not yet taken" stands for that.  What a
  // call that ended in NEEDS_MORE_INPUT had no room for is NOT owed: the reference wrote what fitted, took the call's input
  // and kept the rest for later calls (decode.rs:2835-2846), and so does this.
  if (s->outq_len != s->outq_off) {
    const uint64_t ring = (s->have_resume && s->resume.window_bits) ? (1ull << s->resume.window_bits) : ~0ull;
    if (s->finished || s->pending_error || (uint64_t)(s->outq_len - s->outq_off) >= ring) {
      size_t n0 = hand_over(s, *next_out, *available_out);
      *next_out += n0; *available_out -= n0;
      if (s->outq_len != s->outq_off) {
        if (total_out) *total_out = (size_t)s->total_out;
        s->error_code = BROTLI_DECODER_NEEDS_MORE_OUTPUT;
        *result = BROTLI_DECODER_RESULT_NEEDS_MORE_OUTPUT;
        return true;
      }
    }
  }
  return false;
}

BrotliDecoderResult brotli_amd_host::stream_fail(BrotliDecoderState* s, const char* what) { set_runtime_error(s, what); return BROTLI_DECODER_RESULT_ERROR; }
BrotliDecoderResult brotli_amd_host::stream_fail(BrotliDecoderState* s, int e) {  // (decode_pass's codes)
  if (e == 2) { s->error_code = BROTLI_DECODER_ERROR_ALLOC_RING_BUFFER_2; return BROTLI_DECODER_RESULT_ERROR; }
  return stream_fail(s, "HIP runtime failure");
}

bool brotli_amd_host::stream_upload_dictionary(BrotliDecoderState* s) {
  if (!s->h_dict) return true;
  if (!s->d_dict.reserve(s->dict_len, "hipMalloc(custom dictionary)", 64) ||
      !hip_ok(hipMemcpy(s->d_dict, s->h_dict, s->dict_len, hipMemcpyHostToDevice), "hipMemcpy(custom dictionary)")) {
    s->d_dict.release();
    return false;
  }
  st_free(s, s->h_dict); s->h_dict = nullptr;
  return true;
}

bool brotli_amd_host::stream_input_room(BrotliDecoderState* s, size_t given, size_t* fill) {
  *fill = (size_t)(s->d_in_len - s->in_base);
  return dev_rebase(s->d_in, 0, *fill, *fill + given);
}

void brotli_amd_host::stream_took_input(BrotliDecoderState* s, size_t* available_in, const uint8_t** next_in, size_t given) {
  s->d_in_len += given;
  *next_in += given; *available_in = 0;
  s->used = true;
}

bool brotli_amd_host::stream_decoded(BrotliDecoderState* s, const BrotliAmdStreamStatus& st, size_t* available_in, const uint8_t** next_in, size_t given) {
  if (st.result == BROTLI_DECODER_RESULT_SUCCESS) {
    s->finished = true;
    // give back what lies beyond the end of the stream (decode.rs:3374-3378); it is part of this call's input
    size_t unused = (size_t)(s->d_in_len - st.consumed);
    if (unused > given) unused = given;
    *next_in -= unused; *available_in += unused;
  } else if (st.result == BROTLI_DECODER_RESULT_ERROR) {
    s->pending_error = st.error_code;
  } else if (!trim_buffers(s)) {
    return false;
  }
  return true;
}

BrotliDecoderResult brotli_amd_host::stream_end(BrotliDecoderState* s, size_t* available_out, uint8_t** next_out, size_t* total_out) {
  size_t n = hand_over(s, *next_out, *available_out);
  *next_out += n; *available_out -= n;
  if (total_out) *total_out = (size_t)s->total_out;
  if (s->outq_len != s->outq_off && (s->finished || s->pending_error)) { s->error_code = BROTLI_DECODER_NEEDS_MORE_OUTPUT; return BROTLI_DECODER_RESULT_NEEDS_MORE_OUTPUT; }
  if (s->pending_error) { s->error_code = s->pending_error; return BROTLI_DECODER_RESULT_ERROR; }
  if (s->finished) { s->error_code = BROTLI_DECODER_SUCCESS; return BROTLI_DECODER_RESULT_SUCCESS; }
  s->error_code = BROTLI_DECODER_NEEDS_MORE_INPUT;
  return BROTLI_DECODER_RESULT_NEEDS_MORE_INPUT;
}

extern "C" BrotliDecoderState* BrotliDecoderCreateInstance(brotli_alloc_func alloc_func, brotli_free_func free_func, void* opaque) {
  if ((alloc_func == nullptr) != (free_func == nullptr)) return nullptr;  // ffi/mod.rs:132-135
  void* mem = alloc_func ? alloc_func(opaque, sizeof(BrotliDecoderStateStruct)) : std::malloc(sizeof(BrotliDecoderStateStruct));
  if (!mem) return nullptr;
  BrotliDecoderState* s = new (mem) BrotliDecoderStateStruct();   // (the caller's memory: constructed in place, destroyed explicitly)
  s->alloc_func = alloc_func; s->free_func = free_func; s->opaque = opaque;
  return s;
}

extern "C" void BrotliDecoderDestroyInstance(BrotliDecoderState* s) {
  if (!s) return;
  if (s->batch) BrotliAmdBatchDestroy(s->batch);   // (waits for the device)
  st_free(s, s->h_dict);
  st_free(s, s->outq);
  brotli_free_func f = s->free_func; void* opaque = s->opaque;
  if (s->d_in || s->d_out || s->d_dict) {   // its device buffers go with the state's device current
    DeviceGuard guard;
    if (s->device >= 0) (void)hipSetDevice(s->device);
    s->~BrotliDecoderStateStruct();
  } else s->~BrotliDecoderStateStruct();
  if (f) f(opaque, s); else std::free(s);
}

extern "C" BROTLI_BOOL BrotliDecoderSetParameter(BrotliDecoderState* s, BrotliDecoderParameter param, uint32_t value) {
  if (!s) return BROTLI_FALSE;
  if (s->used) return BROTLI_FALSE;  // only in the UNINITED state (ffi/mod.rs:163-166)
  switch (param) {
    case BROTLI_DECODER_PARAM_DISABLE_RING_BUFFER_REALLOCATION: s->canny = (value == 0); return BROTLI_TRUE;
    case BROTLI_DECODER_PARAM_LARGE_WINDOW: s->large_window = (value != 0); return BROTLI_TRUE;
  }
  return BROTLI_TRUE;
}

extern "C" BrotliDecoderResult BrotliDecoderDecompressStream(BrotliDecoderState* s, size_t* available_in, const uint8_t** next_in,
                                                             size_t* available_out, uint8_t** next_out, size_t* total_out) {
  BrotliDecoderResult early;
  if (stream_begin(s, available_in, next_in, available_out, next_out, total_out, &early)) return early;
  const size_t given = *available_in;
  if (stream_wants_device(s, given)) {
    DeviceGuard guard;
    // lazily bind to the current device (a state first stepped through a stream set is bound to the set's already, and has no batch object yet)
    if (!s->batch) {
      int dev = s->device;
      if (dev < 0 && !current_device(&dev)) return stream_fail(s, "HIP device unavailable");
      if (s->device >= 0 && !hip_ok(hipSetDevice(dev), "hipSetDevice")) return stream_fail(s, "HIP runtime failure");
      s->batch = BrotliAmdBatchCreate(1, 0, 0);
      if (!s->batch) return stream_fail(s, "HIP device unavailable");
      s->device = dev;
    }
    if (!hip_ok(hipSetDevice(s->device), "hipSetDevice")) return stream_fail(s, "HIP runtime failure");
    if (!stream_upload_dictionary(s)) return stream_fail(s, "HIP runtime failure");
    size_t fill = 0;
    if (!stream_input_room(s, given, &fill) || !hip_ok(hipMemcpy(s->d_in + fill, *next_in, given, hipMemcpyHostToDevice), "hipMemcpy(input)"))
      return stream_fail(s, "HIP runtime failure");
    stream_took_input(s, available_in, next_in, given);
    BrotliAmdStreamStatus st;
    if (int e = decode_pass(s, &st)) return stream_fail(s, e);
    if (!stream_decoded(s, st, available_in, next_in, given)) return stream_fail(s, "HIP runtime failure");
  }
  return stream_end(s, available_out, next_out, total_out);
}

extern "C" BrotliDecoderResult BrotliDecoderDecompressStreaming(BrotliDecoderState* s, size_t* available_in, const uint8_t* next_in,
                                                                size_t* available_out, uint8_t* next_out) {
  return BrotliDecoderDecompressStream(s, available_in, &next_in, available_out, &next_out, nullptr);
}

extern "C" BROTLI_BOOL BrotliDecoderHasMoreOutput(const BrotliDecoderState* s) {
  if (!s || fatal(s->error_code)) return BROTLI_FALSE;  // decode.rs:2259-2263
  return s->outq_len != s->outq_off ? BROTLI_TRUE : BROTLI_FALSE;
}

extern "C" const uint8_t* BrotliDecoderTakeOutput(BrotliDecoderState* s, size_t* size) {
  if (!s || !size) return nullptr;
  size_t want = *size ? *size : ((size_t)1 << 24);  // decode.rs:2273
  if (fatal(s->error_code) || s->outq_len == s->outq_off) { *size = 0; return nullptr; }
  size_t n = std::min(want, s->outq_len - s->outq_off);
  const uint8_t* p = s->outq + s->outq_off;
  s->outq_off += n; s->total_out += n;
  *size = n;
  return p;  // valid until the next call on this instance
}

// BrotliState::new_with_custom_dictionary (state.rs:400-411) for an instance of the C ABI: one dictionary, before the first byte is decoded.
extern "C" BROTLI_BOOL BrotliAmdDecoderAttachDictionary(BrotliDecoderState* s, const uint8_t* data, size_t size) {
  if (!s || s->used) return BROTLI_FALSE;
  if (size == 0) return BROTLI_TRUE;
  if (!data || s->h_dict || s->d_dict) return BROTLI_FALSE;
  const size_t tail = std::min(size, kMaxCustomDict);   // (no window reaches further back: decode.rs:1831-1839)
  uint8_t* copy = static_cast<uint8_t*>(st_alloc(s, tail));
  if (!copy) return BROTLI_FALSE;
  std::memcpy(copy, data + (size - tail), tail);
  s->h_dict = copy; s->dict_len = tail;
  return BROTLI_TRUE;
}

extern "C" uint64_t BrotliAmdDecoderDeviceCommands(const BrotliDecoderState* s) { return s ? s->device_commands : 0; }
extern "C" BROTLI_BOOL BrotliDecoderIsUsed(const BrotliDecoderState* s) { return (s && s->used) ? BROTLI_TRUE : BROTLI_FALSE; }
extern "C" BROTLI_BOOL BrotliDecoderIsFinished(const BrotliDecoderState* s) {
  return (s && s->finished && !s->pending_error && s->outq_len == s->outq_off) ? BROTLI_TRUE : BROTLI_FALSE;
}
extern "C" BrotliDecoderErrorCode BrotliDecoderGetErrorCode(const BrotliDecoderState* s) {
  return s ? (BrotliDecoderErrorCode)s->error_code : BROTLI_DECODER_ERROR_INVALID_ARGUMENTS;
}
extern "C" const char* BrotliDecoderGetErrorString(const BrotliDecoderState* s) {
  if (s && s->has_error_text) return s->error_text;  // ffi/mod.rs:571-580
  return BrotliDecoderErrorString(BrotliDecoderGetErrorCode(s));
}

extern "C" uint8_t* BrotliDecoderMallocU8(BrotliDecoderState* s, size_t size) { return s ? static_cast<uint8_t*>(st_alloc(s, size)) : nullptr; }
extern "C" void BrotliDecoderFreeU8(BrotliDecoderState* s, uint8_t* data, size_t) { if (s) st_free(s, data); }
extern "C" size_t* BrotliDecoderMallocUsize(BrotliDecoderState* s, size_t size) {
  if (!s || size > SIZE_MAX / sizeof(size_t)) return nullptr;  // ffi/mod.rs:507-510
  return static_cast<size_t*>(st_alloc(s, size * sizeof(size_t)));
}
extern "C" void BrotliDecoderFreeUsize(BrotliDecoderState* s, size_t* data, size_t) { if (s) st_free(s, data); }

// Debug aid for tests/ (not part of the public headers): device bytes a streaming instance holds at the moment.
extern "C" __attribute__((visibility("default"))) size_t brotli_amd_debug_stream_device_bytes(const BrotliDecoderState* s) {
  return s ? s->d_in.capacity() + s->d_out.capacity() : 0;
}

