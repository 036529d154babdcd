// brotli_stream.h -- the streaming state of the reference's C ABI and the phases of one BrotliDecoderDecompressStream call (brotli_capi.cpp).
// The solo entry point runs the phases for its one state, with its own batch object and synchronous copies; BrotliAmdStreamSetDecompress
// (brotli_stream_set.cpp) runs them for many states around ONE launch and ragged copies.
#ifndef BROTLI_AMD_STREAM_H_
#define BROTLI_AMD_STREAM_H_
#include "brotli_host.h"

// Lives in memory of the caller's allocator: constructed in place (BrotliDecoderCreateInstance), destroyed explicitly (DestroyInstance).
struct BrotliDecoderStateStruct {
  brotli_alloc_func alloc_func = nullptr; brotli_free_func free_func = nullptr; void* opaque = nullptr;
  bool large_window = false;   // ffi/mod.rs:127
  bool canny = true;           // state.rs: canny_ringbuffer_allocation = true
  bool used = false, finished = false, have_resume = false;
  int error_code = BROTLI_DECODER_SUCCESS;   // BrotliDecoderErrorCode, latched when fatal (decode.rs:2796-2798)
  int pending_error = 0;   // fatal code found by the device, reported once everything before it is delivered
  char error_text[256] = {}; bool has_error_text = false;
  BrotliAmdBatch* batch = nullptr;
  int device = -1;
  // Device copies of the part of the stream that can still matter: compressed bytes from a little in front of the last
  // completed metablock boundary (in_base = stream offset of d_in[0]; d_in_len = stream bytes received in all), output
  // from one window in front of that boundary or from the first byte not yet copied off the device, whichever is lower
  // (out_base = output offset of d_out[0]).  The kernel is handed pointers biased by the bases, so that it goes on
  // addressing the stream and the output from their beginnings.
  brotli_amd_host::DevBuf<> d_in; size_t d_in_len = 0; uint64_t in_base = 0;
  brotli_amd_host::DevBuf<> d_out; uint64_t out_base = 0;
  BrotliAmdResume resume = {};
  uint64_t fetched = 0;        // output bytes already copied off the device
  uint64_t total_out = 0;      // output bytes handed to the caller (partial_pos_out)
  uint8_t* outq = nullptr; size_t outq_len = 0, outq_off = 0, outq_cap = 0;  // fetched but not yet handed over
  uint64_t device_commands = 0; // commands the device has decoded for this stream in all its launches together (BrotliAmdDecoderDeviceCommands)
  // the custom dictionary (BrotliAmdDecoderAttachDictionary): the state's own copy on the host until the instance is bound to a
  // device, then on the device -- a buffer of its own, which no trim or re-base of the output touches: every launch names it
  uint8_t* h_dict = nullptr; brotli_amd_host::DevBuf<> d_dict; size_t dict_len = 0;
};

namespace brotli_amd_host {

// The head of a call, on the host: argument and slice checks, the latched error, the output the decoder owes.  True: the call is over (*result).
bool stream_begin(BrotliDecoderState* s, size_t* available_in, const uint8_t** next_in, size_t* available_out, uint8_t** next_out, size_t* total_out,
                  BrotliDecoderResult* result);
// Whether a call that got past its head has anything to decode: the others go straight to stream_end.
inline bool stream_wants_device(const BrotliDecoderState* s, size_t given) { return !s->finished && !s->pending_error && given != 0; }
BrotliDecoderResult stream_fail(BrotliDecoderState* s, const char* what);   // a runtime failure: g_last_error says which
BrotliDecoderResult stream_fail(BrotliDecoderState* s, int e);              // 1 = HIP failure, 2 = allocation failure
// The attached dictionary moves to the device the instance is bound to (the current one).
bool stream_upload_dictionary(BrotliDecoderState* s);
// Room for `given` more bytes behind what the state's device input buffer holds; *fill: where they go.
bool stream_input_room(BrotliDecoderState* s, size_t given, size_t* fill);
// The call's input is on the device (or on its way there): it counts as consumed.
void stream_took_input(BrotliDecoderState* s, size_t* available_in, const uint8_t** next_in, size_t given);
// The device's output buffer of the state before a launch: room for six times the compressed bytes not yet behind a metablock boundary.
bool stream_ensure_out(BrotliDecoderState* s);
// The state's descriptor of a launch: everything received so far, from the last completed metablock boundary.
BrotliAmdStreamDesc stream_desc(const BrotliDecoderState* s);
void stream_note_status(BrotliDecoderState* s, const BrotliAmdStreamStatus& st);
// Room for n more bytes behind what the caller has not taken yet (the state's own allocator).
bool reserve_outq(BrotliDecoderState* s, size_t n);
// A launch came back NEEDS_MORE_OUTPUT -- the device output buffer is exhausted: everything below the resume point is final.  What is dead is
// dropped; where that does not leave half the buffer free, the buffer doubles.
bool stream_grow_out(BrotliDecoderState* s);
// What the last launch of the call said.  False: a HIP failure while trimming.
bool stream_decoded(BrotliDecoderState* s, const BrotliAmdStreamStatus& st, size_t* available_in, const uint8_t** next_in, size_t given);
// The tail of a call: what there is goes out as far as there is room, and the result follows from what is left.
BrotliDecoderResult stream_end(BrotliDecoderState* s, size_t* available_out, uint8_t** next_out, size_t* total_out);

}  // namespace brotli_amd_host
#endif  // BROTLI_AMD_STREAM_H_
