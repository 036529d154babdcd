// brotli_filters.cpp -- the element filters on the device (include/brotli/batch.h): unshuffle (byte planes back into elements), undelta (deltas
// back into values, a wrapping running sum per segment), bit-unshuffle (bit planes back into elements), bit-unpack (k-bit fields back into
// elements), unvarint (LEB128 varints back into elements, with a result per segment), unrle (runs of the RLE / bit-packed hybrid back into
// elements, with a result per segment as well) and undbp (DELTA_BINARY_PACKED blocks back into elements, with a result per segment too).  Each takes n segments of device memory
// (BrotliAmdBatch*Segments) or the delivered bytes of every stream of the last decode call (BrotliAmdBatch*Outputs), in one launch -- undelta and
// unvarint in three --, and each has a hook that runs the device's functions of its header (csrc/brotli_unshuffle.h, brotli_undelta.h,
// brotli_bitunshuffle.h, brotli_bitunpack.h, brotli_unvarint.h) on the host as the kernel's lanes take them, for tests without a device.  What
// differs between the filters is a descriptor (kFilter), a check of a segment's shape, and the hook's loop; unvarint has a segment of its own
// (BrotliAmdUnvarintSeg: a source length and a capacity), whose units are its source's, and so has unrle (BrotliAmdUnrleSeg), whose units are
// one a segment and one an item of its destination; undbp (BrotliAmdUndbpSeg) is unrle's shape with items of deltas, four launches and five events.
#include "brotli_bitunpack.h"
#include "brotli_bitunshuffle.h"
#include "brotli_host.h"
#include "brotli_undbp.h"
#include "brotli_undelta.h"
#include "brotli_unrle.h"
#include "brotli_unshuffle.h"
#include "brotli_unvarint.h"

#include <numeric>

// (csrc/brotli_*_kernels.hip: units: the segments' units together; undelta's ev: four events around and between its three launches)
extern "C" hipError_t brotli_amd_launch_unshuffle(const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, hipStream_t stream);
extern "C" hipError_t brotli_amd_launch_bitunshuffle(const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, hipStream_t stream);
extern "C" hipError_t brotli_amd_launch_bitunpack(const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, hipStream_t stream);
extern "C" hipError_t brotli_amd_launch_undelta(const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream,
                                                const hipEvent_t* ev);
extern "C" hipError_t brotli_amd_launch_unvarint(const BrotliAmdUnvarintSeg* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream,
                                                 const hipEvent_t* ev);
extern "C" hipError_t brotli_amd_launch_unrle(const BrotliAmdUnrleSeg* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream,
                                              const hipEvent_t* ev);
extern "C" hipError_t brotli_amd_launch_undbp(const BrotliAmdUndbpSeg* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream,
                                              const hipEvent_t* ev);
extern "C" uint64_t brotli_amd_undbp_scratch_bytes(uint64_t units, uint32_t n);
extern "C" uint32_t brotli_amd_undbp_item_deltas(void);
extern "C" uint32_t brotli_amd_undbp_walk_chunk(void);
extern "C" uint64_t brotli_amd_unrle_scratch_bytes(uint64_t units, uint32_t n);
extern "C" uint32_t brotli_amd_unrle_item_elems(void);
extern "C" uint32_t brotli_amd_unrle_walk_chunk(void);
extern "C" uint64_t brotli_amd_undelta_scratch_bytes(uint64_t units);
extern "C" uint64_t brotli_amd_unvarint_scratch_bytes(uint64_t units, uint32_t n);
extern "C" uint64_t brotli_amd_unvarint_results_at(uint64_t units);
extern "C" uint32_t brotli_amd_unvarint_tile_bytes(void);
extern "C" uint32_t brotli_amd_unshuffle_tile_bytes(void);
extern "C" uint32_t brotli_amd_undelta_tile_bytes(void);
extern "C" uint32_t brotli_amd_undelta_carry_span(void);
extern "C" uint32_t brotli_amd_bitunshuffle_tile_bytes(void);
extern "C" uint32_t brotli_amd_bitunpack_tile_bytes(void);

using namespace brotli_amd_host;

namespace {

// What the host needs to know of a filter.  A filter of one launch (`launch`) has two events, recorded around it here; undelta and unvarint
// (`launch_timed`, `launch_counted`: unvarint's table has its own segments) have four, which their launchers record around and between their
// launches, and room behind the table that grows with the units -- unvarint's with the segments too, for their results.  Unrle (`launch_runs`)
// has three around and between its two launches, undbp (`launch_blocks`) five around and between its four.
struct FilterDesc {
  const char* name;   // in the texts of g_last_error
  SegCallWhat what;
  const char* launch_what;
  hipError_t (*launch)(const BrotliAmdUnshuffleSeg*, uint32_t, uint64_t, hipStream_t);
  hipError_t (*launch_timed)(const BrotliAmdUnshuffleSeg*, uint32_t, uint64_t, void*, hipStream_t, const hipEvent_t*);
  hipError_t (*launch_counted)(const BrotliAmdUnvarintSeg*, uint32_t, uint64_t, void*, hipStream_t, const hipEvent_t*);
  hipError_t (*launch_runs)(const BrotliAmdUnrleSeg*, uint32_t, uint64_t, void*, hipStream_t, const hipEvent_t*);
  hipError_t (*launch_blocks)(const BrotliAmdUndbpSeg*, uint32_t, uint64_t, void*, hipStream_t, const hipEvent_t*);
  uint64_t (*scratch_bytes)(uint64_t units, uint32_t n);   // behind the table (nullptr: nothing)
  uint32_t events;
};
const FilterDesc kFilter[kFilters] = {
    {"unshuffle", {"hipMalloc(unshuffle segments)", "hipMemcpyAsync(unshuffle segments)", "hipStreamSynchronize(unshuffle)"},
     "brotli_amd_unshuffle_kernel launch", brotli_amd_launch_unshuffle, nullptr, nullptr, nullptr, nullptr, nullptr, 2u},
    {"undelta", {"hipMalloc(undelta segments and tiles)", "hipMemcpyAsync(undelta segments)", "hipStreamSynchronize(undelta)"},
     "brotli_amd_undelta kernels launch", nullptr, brotli_amd_launch_undelta, nullptr, nullptr, nullptr, [](uint64_t units, uint32_t) { return brotli_amd_undelta_scratch_bytes(units); }, 4u},
    {"bit-unshuffle", {"hipMalloc(bit-unshuffle segments)", "hipMemcpyAsync(bit-unshuffle segments)", "hipStreamSynchronize(bit-unshuffle)"},
     "brotli_amd_bitunshuffle_kernel launch", brotli_amd_launch_bitunshuffle, nullptr, nullptr, nullptr, nullptr, nullptr, 2u},
    {"bit-unpack", {"hipMalloc(bit-unpack segments)", "hipMemcpyAsync(bit-unpack segments)", "hipStreamSynchronize(bit-unpack)"},
     "brotli_amd_bitunpack_kernel launch", brotli_amd_launch_bitunpack, nullptr, nullptr, nullptr, nullptr, nullptr, 2u},
    {"unvarint", {"hipMalloc(unvarint segments, tiles and results)", "hipMemcpyAsync(unvarint segments)", "hipStreamSynchronize(unvarint)"},
     "brotli_amd_unvarint kernels launch", nullptr, nullptr, brotli_amd_launch_unvarint, nullptr, nullptr, brotli_amd_unvarint_scratch_bytes, 4u},
    {"unrle", {"hipMalloc(unrle segments, results and checkpoints)", "hipMemcpyAsync(unrle segments)", "hipStreamSynchronize(unrle)"},
     "brotli_amd_unrle kernels launch", nullptr, nullptr, nullptr, brotli_amd_launch_unrle, nullptr, brotli_amd_unrle_scratch_bytes, 3u},
    {"undbp", {"hipMalloc(undbp segments, results, checkpoints and tiles)", "hipMemcpyAsync(undbp segments)", "hipStreamSynchronize(undbp)"},
     "brotli_amd_undbp kernels launch", nullptr, nullptr, nullptr, nullptr, brotli_amd_launch_undbp, brotli_amd_undbp_scratch_bytes, 5u},
};

typedef std::vector<BrotliAmdUnshuffleSeg> Segs;
typedef std::vector<BrotliAmdUnvarintSeg> VarintSegs;
typedef std::vector<BrotliAmdUnrleSeg> RleSegs;
typedef std::vector<BrotliAmdUndbpSeg> DbpSegs;

// a segment's units: its destination's words, unvarint's its source's (brotli_seg_walk.h), unrle's one for its walk and one for every item
inline uint64_t units_of(const BrotliAmdUnshuffleSeg& s) { return brotli_amd_seg_units((uint64_t)(uintptr_t)s.dst, s.len); }
inline uint64_t units_of(const BrotliAmdUnvarintSeg& s) { return brotli_amd_seg_units((uint64_t)(uintptr_t)s.src, s.len); }
inline uint64_t units_of(const BrotliAmdUnrleSeg& s) { return 1u + brotli_amd_unrle_items(s.cap, brotli_amd_unrle_item_elems()); }
inline uint64_t units_of(const BrotliAmdUndbpSeg& s) { return 1u + brotli_amd_undbp_items(s.cap, brotli_amd_undbp_item_deltas()); }
// a filter's launches over its table
inline hipError_t launch_of(const FilterDesc& d, const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  return d.launch_timed(d_segs, n, units, d_scratch, stream, ev);
}
inline hipError_t launch_of(const FilterDesc& d, const BrotliAmdUnvarintSeg* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  return d.launch_counted(d_segs, n, units, d_scratch, stream, ev);
}
inline hipError_t launch_of(const FilterDesc& d, const BrotliAmdUnrleSeg* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  return d.launch_runs(d_segs, n, units, d_scratch, stream, ev);
}
inline hipError_t launch_of(const FilterDesc& d, const BrotliAmdUndbpSeg* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev) {
  return d.launch_blocks(d_segs, n, units, d_scratch, stream, ev);
}
// ... of one launch (unvarint, unrle and undbp have none of these)
inline hipError_t launch_of(const FilterDesc& d, const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, hipStream_t stream) { return d.launch(d_segs, n, units, stream); }
inline hipError_t launch_of(const FilterDesc&, const BrotliAmdUnvarintSeg*, uint32_t, uint64_t, hipStream_t) { return hipErrorInvalidValue; }
inline hipError_t launch_of(const FilterDesc&, const BrotliAmdUnrleSeg*, uint32_t, uint64_t, hipStream_t) { return hipErrorInvalidValue; }
inline hipError_t launch_of(const FilterDesc&, const BrotliAmdUndbpSeg*, uint32_t, uint64_t, hipStream_t) { return hipErrorInvalidValue; }

int invalid_arguments(Filter f) { g_last_error = std::string("invalid ") + kFilter[f].name + " arguments"; return -1; }

// an entry point begins: no times of an earlier call
void no_times(BrotliAmdBatch* b, Filter f) {
  b->filter[f].ms = 0.0f;
  if (f == kUndelta) for (float& ms : b->undelta_phase_ms) ms = 0.0f;
  if (f == kUnvarint) for (float& ms : b->unvarint_phase_ms) ms = 0.0f;
  if (f == kUnrle) for (float& ms : b->unrle_phase_ms) ms = 0.0f;
  if (f == kUndbp) for (float& ms : b->undbp_phase_ms) ms = 0.0f;
}

// segs on `stream`, waited for (their shapes were checked).  units_out: their units together; scratch_out: the device memory behind the table,
// where unvarint's results lie until the next call (nullptr: nothing was launched)
template <class Seg>
int filter_device(BrotliAmdBatch* b, Filter f, const std::vector<Seg>& segs, hipStream_t stream, uint64_t* units_out = nullptr,
                  const uint8_t** scratch_out = nullptr) {
  if (scratch_out) *scratch_out = nullptr;
  if (segs.empty()) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const FilterDesc& d = kFilter[f];
  const uint32_t n = (uint32_t)segs.size();
  uint64_t units = 0;   // of all segments together (brotli_seg_walk.h)
  for (const Seg& s : segs) units += units_of(s);
  if (units_out) *units_out = units;
  if (units == 0u) return 0;   // (segments without bytes: nothing to launch)
  return run_seg_call(&b->filter[f].call, d.what, segs.data(), sizeof(Seg) * n, d.scratch_bytes ? d.scratch_bytes(units, n) : 0u, d.events, stream,
                      [&](uint8_t* d_table, uint8_t* d_scratch, const hipEvent_t* ev) {
    const Seg* d_segs = reinterpret_cast<Seg*>(d_table);
    if (scratch_out) *scratch_out = d_scratch;
    if (!d.launch) return hip_ok(launch_of(d, d_segs, n, units, d_scratch, stream, ev), d.launch_what);
    return hip_ok(hipEventRecord(ev[0], stream), "hipEventRecord") && hip_ok(launch_of(d, d_segs, n, units, stream), d.launch_what) &&
           hip_ok(hipEventRecord(ev[1], stream), "hipEventRecord");
  }, &b->filter[f].ms, f == kUndelta ? b->undelta_phase_ms : f == kUnvarint ? b->unvarint_phase_ms : f == kUnrle ? b->unrle_phase_ms : f == kUndbp ? b->undbp_phase_ms : nullptr);
}

// ---- a call's segments, each checked in front of everything that touches the device ----
// From the caller's arrays: shape(i, &seg) checks segment i and fills in seg's len, width and param -- false: g_last_error says why.  seg is
// the table's own entry: filled in where it stays, it is not copied once more (a table has a hundred thousand of them).
template <class Shape>
bool segments_of_arrays(uint32_t n, const void* const* d_src, void* const* d_dst, Shape shape, Segs* segs) {
  segs->reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    segs->push_back(BrotliAmdUnshuffleSeg{static_cast<const uint8_t*>(d_src[i]), static_cast<uint8_t*>(d_dst[i]), 0u, 0u, 0u});
    if (!shape(i, &segs->back())) return false;
  }
  return true;
}
// From the delivered bytes of the last decode call's streams: seg comes with the stream's bytes as src and len, and shape may change len.  A NULL
// destination skips the stream: none of its parameters are looked at.
template <class Shape>
bool segments_of_outputs(BrotliAmdBatch* b, void* const* d_dst, Shape shape, Segs* segs) {
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return false;
  segs->reserve(outs.size());
  for (size_t i = 0; i < outs.size(); i++) {
    if (d_dst[i] == nullptr) continue;
    segs->push_back(BrotliAmdUnshuffleSeg{outs[i].ptr, static_cast<uint8_t*>(d_dst[i]), outs[i].len, 0u, 0u});
    if (!shape(i, &segs->back())) return false;
  }
  return true;
}

// ---- unshuffle, undelta, bit-unshuffle: a width, and bit-unshuffle's block ----
// (a table has a hundred thousand segments: what passes costs a comparison, and the texts are built out of line)
bool refuse(const std::string& why) { g_last_error = why; return false; }
inline bool known_width(Filter f, uint32_t width) {
  return brotli_amd_unshuffle_width_ok(width) || refuse(std::string(kFilter[f].name) + " width is not 1, 2, 4 or 8");
}
inline bool known_block(uint32_t block) {
  return brotli_amd_bitunshuffle_block_ok(block) || refuse("bit-unshuffle block_elems is neither 0 nor a multiple of 8");
}
// undelta in place is allowed at an address that is a multiple of the width only: there a unit reads exactly the bytes it writes
inline bool placed_ok(uint64_t src, uint64_t dst, uint32_t width) {
  return src != dst || dst % width == 0u || refuse("undelta in place at an address that is not a multiple of the width");
}
// s.src and s.dst with this width and block (bit-unshuffle's; 0 elsewhere)
inline bool plane_shape(Filter f, BrotliAmdUnshuffleSeg* s, uint32_t width, uint32_t block) {
  if (!known_width(f, width) || (f == kBitUnshuffle && !known_block(block))) return false;
  if (f == kUndelta && !placed_ok((uint64_t)(uintptr_t)s->src, (uint64_t)(uintptr_t)s->dst, width)) return false;
  s->width = width; s->param = block;
  return true;
}

int plane_segments(Filter f, BrotliAmdBatch* b, uint32_t n, const void* const* d_src, void* const* d_dst, const size_t* lens, const uint8_t* widths,
                   const uint32_t* block_elems, void* hip_stream) {
  if (!b || (n && (!d_src || !d_dst || !lens || !widths))) return invalid_arguments(f);
  no_times(b, f);
  Segs segs;
  if (!segments_of_arrays(n, d_src, d_dst, [&](size_t i, BrotliAmdUnshuffleSeg* s) {
        s->len = lens[i];
        return plane_shape(f, s, widths[i], block_elems ? block_elems[i] : 0u);
      }, &segs)) return -1;
  return filter_device(b, f, segs, static_cast<hipStream_t>(hip_stream));
}

int plane_outputs(Filter f, BrotliAmdBatch* b, void* const* d_dst, const uint8_t* widths, const uint32_t* block_elems) {
  if (!b || !d_dst || !widths) return invalid_arguments(f);
  no_times(b, f);
  Segs segs;
  if (!segments_of_outputs(b, d_dst, [&](size_t i, BrotliAmdUnshuffleSeg* s) { return plane_shape(f, s, widths[i], block_elems ? block_elems[i] : 0u); }, &segs))
    return -1;
  return filter_device(b, f, segs, b->last_stream);
}

// ---- bit-unpack: k bits into w bytes by flags, and a count ----
// `who` names the segment or stream in the text
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
// a segment's len is its DESTINATION's bytes
void packed_shape(BrotliAmdUnshuffleSeg* s, uint64_t count, uint32_t bits, uint32_t width, uint32_t flags) {
  s->len = count * width; s->width = width; s->param = brotli_amd_bitunpack_param(bits, flags);
}

// ---- unvarint: a width, flags and a capacity; a result per segment ----
// `who` names the segment or stream in the text
bool known_varint(uint32_t width, uint32_t flags, uint64_t cap, bool has_dst, const char* who, size_t i) {
  const char* what = nullptr;
  if (!brotli_amd_unshuffle_width_ok(width)) what = "width is not 1, 2, 4 or 8";
  else if ((flags & ~BROTLI_AMD_UNVARINT_FLAGS) != 0u) what = "unknown flag bits";
  else if (cap > BROTLI_AMD_UNVARINT_MAX_CAP) what = "a capacity above 2^56 elements";
  else if (cap != 0u && !has_dst) what = "no destination for a capacity that is not 0";
  if (!what) return true;
  g_last_error = std::string("unvarint ") + who + " " + std::to_string(i) + ": " + what + " (width " + std::to_string(width) + ", flags " + std::to_string(flags) +
                 ", capacity " + std::to_string(cap) + ")";
  return false;
}

// segs on `stream`, waited for, and their results: segment j's to results[where[j]] of the n_results, the others zeros
int varint_device(BrotliAmdBatch* b, const VarintSegs& segs, const std::vector<size_t>& where, BrotliAmdUnvarintResult* results, size_t n_results,
                  hipStream_t stream) {
  std::fill(results, results + n_results, BrotliAmdUnvarintResult{0u, 0u, 0u});
  uint64_t units = 0;
  const uint8_t* d_scratch = nullptr;
  if (filter_device(b, kUnvarint, segs, stream, &units, &d_scratch) != 0) return -1;
  if (!d_scratch) return 0;   // (segments without bytes: their results are zeros)
  std::vector<BrotliAmdUnvarintResult> got(segs.size());
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice") ||
      !hip_ok(hipMemcpy(got.data(), d_scratch + brotli_amd_unvarint_results_at(units), sizeof(BrotliAmdUnvarintResult) * got.size(), hipMemcpyDeviceToHost),
              "hipMemcpy(unvarint results)"))
    return -1;
  for (size_t j = 0; j < got.size(); j++) results[where[j]] = got[j];
  return 0;
}

// ---- unrle: a field width, a width, flags and a capacity; a result per segment ----
// `who` names the segment or stream in the text
bool known_runs(uint32_t bits, uint32_t width, uint32_t flags, uint64_t cap, bool has_dst, const char* who, size_t i) {
  const char* what = nullptr;
  if (!brotli_amd_unshuffle_width_ok(width)) what = "width is not 1, 2, 4 or 8";
  else if ((flags & ~BROTLI_AMD_UNRLE_FLAGS) != 0u) what = "unknown flag bits";
  else if ((flags & BROTLI_AMD_UNRLE_WIDTH_BYTE) == 0u && bits > BROTLI_AMD_UNRLE_MAX_BITS) what = "field of more than 32 bits";
  else if ((flags & BROTLI_AMD_UNRLE_WIDTH_BYTE) == 0u && bits > 8u * width) what = "field is wider than the element";
  else if (cap > BROTLI_AMD_UNRLE_MAX_CAP) what = "a capacity above 2^56 elements";
  else if (cap != 0u && !has_dst) what = "no destination for a capacity that is not 0";
  if (!what) return true;
  g_last_error = std::string("unrle ") + who + " " + std::to_string(i) + ": " + what + " (bits " + std::to_string(bits) + ", width " + std::to_string(width) +
                 ", flags " + std::to_string(flags) + ", capacity " + std::to_string(cap) + ")";
  return false;
}
// a table's next entry: its first item is the number of items of the entries in front of it
void push_runs(RleSegs* segs, const void* src, void* dst, uint64_t len, uint64_t cap, uint32_t width, uint32_t bits, uint32_t flags) {
  const uint64_t first = segs->empty() ? 0u : segs->back().first_item + brotli_amd_unrle_items(segs->back().cap, brotli_amd_unrle_item_elems());
  segs->push_back(BrotliAmdUnrleSeg{static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), len, cap, first, width, bits, flags, 0u});
}

// segs on `stream`, waited for, and their results: segment j's to results[where[j]] of the n_results, the others zeros
int runs_device(BrotliAmdBatch* b, const RleSegs& segs, const std::vector<size_t>& where, BrotliAmdUnrleResult* results, size_t n_results, hipStream_t stream) {
  std::fill(results, results + n_results, BrotliAmdUnrleResult{0u, 0u, 0u, 0u, 0u});
  const uint8_t* d_scratch = nullptr;
  if (filter_device(b, kUnrle, segs, stream, nullptr, &d_scratch) != 0) return -1;
  if (!d_scratch) return 0;   // (no segments)
  // (a call without items is the walk alone: what lies between the events behind it is no launch's time)
  if (segs.back().first_item + brotli_amd_unrle_items(segs.back().cap, brotli_amd_unrle_item_elems()) == 0u) {
    b->unrle_phase_ms[1] = 0.0f;
    b->filter[kUnrle].ms = b->unrle_phase_ms[0];
  }
  std::vector<BrotliAmdUnrleResult> got(segs.size());
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice") ||
      !hip_ok(hipMemcpy(got.data(), d_scratch, sizeof(BrotliAmdUnrleResult) * got.size(), hipMemcpyDeviceToHost), "hipMemcpy(unrle results)"))
    return -1;
  for (size_t j = 0; j < got.size(); j++) results[where[j]] = got[j];
  return 0;
}

// ---- undbp: a width, no flags and a capacity; a result per segment ----
// `who` names the segment or stream in the text
bool known_blocks(uint32_t width, uint32_t flags, uint64_t cap, bool has_dst, const char* who, size_t i) {
  const char* what = nullptr;
  if (!brotli_amd_unshuffle_width_ok(width)) what = "width is not 1, 2, 4 or 8";
  else if (flags != 0u) what = "unknown flag bits";
  else if (cap > BROTLI_AMD_UNDBP_MAX_CAP) what = "a capacity above 2^56 elements";
  else if (cap != 0u && !has_dst) what = "no destination for a capacity that is not 0";
  if (!what) return true;
  g_last_error = std::string("undbp ") + who + " " + std::to_string(i) + ": " + what + " (width " + std::to_string(width) + ", flags " + std::to_string(flags) +
                 ", capacity " + std::to_string(cap) + ")";
  return false;
}
// a table's next entry: its first item is the number of items of the entries in front of it
void push_blocks(DbpSegs* segs, const void* src, void* dst, uint64_t len, uint64_t cap, uint32_t width) {
  const uint64_t first = segs->empty() ? 0u : segs->back().first_item + brotli_amd_undbp_items(segs->back().cap, brotli_amd_undbp_item_deltas());
  segs->push_back(BrotliAmdUndbpSeg{static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), len, cap, first, width, 0u});
}

// segs on `stream`, waited for, and their results: segment j's to results[where[j]] of the n_results, the others zeros
int blocks_device(BrotliAmdBatch* b, const DbpSegs& segs, const std::vector<size_t>& where, BrotliAmdUndbpResult* results, size_t n_results, hipStream_t stream) {
  std::fill(results, results + n_results, BrotliAmdUndbpResult{0u, 0u, 0u, 0u, 0u, 0u, 0u});
  const uint8_t* d_scratch = nullptr;
  if (filter_device(b, kUndbp, segs, stream, nullptr, &d_scratch) != 0) return -1;
  if (!d_scratch) return 0;   // (no segments)
  // (a call without items is the walk alone: what lies between the events behind it is no launch's time)
  if (segs.back().first_item + brotli_amd_undbp_items(segs.back().cap, brotli_amd_undbp_item_deltas()) == 0u) {
    b->undbp_phase_ms[1] = b->undbp_phase_ms[2] = b->undbp_phase_ms[3] = 0.0f;
    b->filter[kUndbp].ms = b->undbp_phase_ms[0];
  }
  std::vector<BrotliAmdUndbpResult> got(segs.size());
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice") ||
      !hip_ok(hipMemcpy(got.data(), d_scratch, sizeof(BrotliAmdUndbpResult) * got.size(), hipMemcpyDeviceToHost), "hipMemcpy(undbp results)"))
    return -1;
  for (size_t j = 0; j < got.size(); j++) results[where[j]] = got[j];
  return 0;
}

// ---- the hooks ----
// what a hook of one segment ends with: no byte beside the len bytes of the destination may have changed; they go to dst
int hook_result(Filter f, const SkewedRoom& droom, uint8_t* dst, size_t len) {
  if (!droom.changed_inside_only([len](size_t i) { return i < len; })) { g_last_error = std::string(kFilter[f].name) + " wrote outside its destination"; return -2; }
  droom.get(dst, 0u, len);
  return 0;
}

}  // namespace

extern "C" int BrotliAmdBatchUnshuffleSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, void* const* d_dst, const size_t* lens,
                                               const uint8_t* widths, void* hip_stream) {
  return plane_segments(kUnshuffle, b, n, d_src, d_dst, lens, widths, nullptr, hip_stream);
}
extern "C" int BrotliAmdBatchUnshuffleOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint8_t* widths) {
  return plane_outputs(kUnshuffle, b, d_dst, widths, nullptr);
}
extern "C" int BrotliAmdBatchUndeltaSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, void* const* d_dst, const size_t* lens,
                                             const uint8_t* widths, void* hip_stream) {
  return plane_segments(kUndelta, b, n, d_src, d_dst, lens, widths, nullptr, hip_stream);
}
extern "C" int BrotliAmdBatchUndeltaOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint8_t* widths) {
  return plane_outputs(kUndelta, b, d_dst, widths, nullptr);
}
extern "C" int BrotliAmdBatchBitUnshuffleSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, void* const* d_dst, const size_t* lens,
                                                  const uint8_t* widths, const uint32_t* block_elems, void* hip_stream) {
  return plane_segments(kBitUnshuffle, b, n, d_src, d_dst, lens, widths, block_elems, hip_stream);
}
extern "C" int BrotliAmdBatchBitUnshuffleOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint8_t* widths, const uint32_t* block_elems) {
  return plane_outputs(kBitUnshuffle, b, d_dst, widths, block_elems);
}

extern "C" int BrotliAmdBatchBitUnpackSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                               const uint64_t* counts, const uint8_t* bits, const uint8_t* widths, const uint8_t* flags, void* hip_stream) {
  if (!b || (n && (!d_src || !src_lens || !d_dst || !counts || !bits || !widths))) return invalid_arguments(kBitUnpack);
  no_times(b, kBitUnpack);
  Segs segs;
  if (!segments_of_arrays(n, d_src, d_dst, [&](size_t i, BrotliAmdUnshuffleSeg* s) {
        const uint32_t f = flags ? flags[i] : 0u;
        if (!known_shape(bits[i], widths[i], f, "segment", i) || !known_count(counts[i], bits[i], src_lens[i], "segment", i)) return false;
        packed_shape(s, counts[i], bits[i], widths[i], f);
        return true;
      }, &segs)) return -1;
  return filter_device(b, kBitUnpack, segs, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchBitUnpackOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint64_t* counts, const uint8_t* bits, const uint8_t* widths,
                                              const uint8_t* flags) {
  if (!b || !d_dst || !bits || !widths) return invalid_arguments(kBitUnpack);
  no_times(b, kBitUnpack);
  Segs segs;
  if (!segments_of_outputs(b, d_dst, [&](size_t i, BrotliAmdUnshuffleSeg* s) {
        const uint32_t f = flags ? flags[i] : 0u;
        if (!known_shape(bits[i], widths[i], f, "stream", i)) return false;
        // without a count: the whole fields that the delivered bytes hold (8 len cannot overflow: len is a size of memory)
        const uint64_t count = counts ? counts[i] : s->len * 8u / bits[i];
        if (!known_count(count, bits[i], s->len, "stream", i)) return false;
        packed_shape(s, count, bits[i], widths[i], f);
        return true;
      }, &segs)) return -1;
  return filter_device(b, kBitUnpack, segs, b->last_stream);
}

extern "C" int BrotliAmdBatchUnvarintSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                              const uint64_t* caps, const uint8_t* widths, const uint8_t* flags, BrotliAmdUnvarintResult* results, void* hip_stream) {
  if (!b || (n && (!d_src || !src_lens || !caps || !widths || !results))) return invalid_arguments(kUnvarint);
  no_times(b, kUnvarint);
  VarintSegs segs;
  std::vector<size_t> where(n);
  segs.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    void* dst = d_dst ? d_dst[i] : nullptr;   // (no array of destinations: a call that counts, where every capacity is 0)
    const uint32_t f = flags ? flags[i] : 0u;
    if (!known_varint(widths[i], f, caps[i], dst != nullptr, "segment", i)) return -1;
    segs.push_back(BrotliAmdUnvarintSeg{static_cast<const uint8_t*>(d_src[i]), static_cast<uint8_t*>(dst), src_lens[i], caps[i], widths[i], f});
    where[i] = i;
  }
  return varint_device(b, segs, where, results, n, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchUnvarintOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint64_t* caps, const uint8_t* widths, const uint8_t* flags,
                                             BrotliAmdUnvarintResult* results) {
  if (!b || !widths || !results) return invalid_arguments(kUnvarint);
  no_times(b, kUnvarint);
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  const bool count_only = !d_dst || !caps;   // every stream is counted and nothing is written
  VarintSegs segs;
  std::vector<size_t> where;
  segs.reserve(outs.size());
  for (size_t i = 0; i < outs.size(); i++) {
    if (!count_only && d_dst[i] == nullptr) continue;   // skipped: none of its parameters are looked at
    const uint32_t f = flags ? flags[i] : 0u;
    const uint64_t cap = count_only ? 0u : caps[i];
    if (!known_varint(widths[i], f, cap, !count_only, "stream", i)) return -1;
    segs.push_back(BrotliAmdUnvarintSeg{outs[i].ptr, count_only ? nullptr : static_cast<uint8_t*>(d_dst[i]), outs[i].len, cap, widths[i], f});
    where.push_back(i);
  }
  return varint_device(b, segs, where, results, outs.size(), b->last_stream);
}

extern "C" int BrotliAmdBatchUnrleSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                           const uint64_t* caps, const uint8_t* bits, const uint8_t* widths, const uint8_t* flags, BrotliAmdUnrleResult* results,
                                           void* hip_stream) {
  if (!b || (n && (!d_src || !src_lens || !caps || !bits || !widths || !results))) return invalid_arguments(kUnrle);
  no_times(b, kUnrle);
  RleSegs segs;
  std::vector<size_t> where(n);
  segs.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    void* dst = d_dst ? d_dst[i] : nullptr;   // (no array of destinations: a call that counts, where every capacity is 0)
    const uint32_t f = flags ? flags[i] : 0u;
    if (!known_runs(bits[i], widths[i], f, caps[i], dst != nullptr, "segment", i)) return -1;
    push_runs(&segs, d_src[i], dst, src_lens[i], caps[i], widths[i], bits[i], f);
    where[i] = i;
  }
  return runs_device(b, segs, where, results, n, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchUnrleOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint64_t* caps, const uint8_t* bits, const uint8_t* widths,
                                          const uint8_t* flags, BrotliAmdUnrleResult* results) {
  if (!b || !bits || !widths || !results) return invalid_arguments(kUnrle);
  no_times(b, kUnrle);
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  const bool count_only = !d_dst || !caps;   // every stream is counted and nothing is written
  RleSegs segs;
  std::vector<size_t> where;
  segs.reserve(outs.size());
  for (size_t i = 0; i < outs.size(); i++) {
    if (!count_only && d_dst[i] == nullptr) continue;   // skipped: none of its parameters are looked at
    const uint32_t f = flags ? flags[i] : 0u;
    const uint64_t cap = count_only ? 0u : caps[i];
    if (!known_runs(bits[i], widths[i], f, cap, !count_only, "stream", i)) return -1;
    push_runs(&segs, outs[i].ptr, count_only ? nullptr : d_dst[i], outs[i].len, cap, widths[i], bits[i], f);
    where.push_back(i);
  }
  return runs_device(b, segs, where, results, outs.size(), b->last_stream);
}

extern "C" int BrotliAmdBatchUndbpSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                           const uint64_t* caps, const uint8_t* widths, const uint8_t* flags, BrotliAmdUndbpResult* results, void* hip_stream) {
  if (!b || (n && (!d_src || !src_lens || !caps || !widths || !results))) return invalid_arguments(kUndbp);
  no_times(b, kUndbp);
  DbpSegs segs;
  std::vector<size_t> where(n);
  segs.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    void* dst = d_dst ? d_dst[i] : nullptr;   // (no array of destinations: a call that counts, where every capacity is 0)
    if (!known_blocks(widths[i], flags ? flags[i] : 0u, caps[i], dst != nullptr, "segment", i)) return -1;
    push_blocks(&segs, d_src[i], dst, src_lens[i], caps[i], widths[i]);
    where[i] = i;
  }
  return blocks_device(b, segs, where, results, n, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchUndbpOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint64_t* caps, const uint8_t* widths, const uint8_t* flags,
                                          BrotliAmdUndbpResult* results) {
  if (!b || !widths || !results) return invalid_arguments(kUndbp);
  no_times(b, kUndbp);
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  const bool count_only = !d_dst || !caps;   // every stream is counted and nothing is written
  DbpSegs segs;
  std::vector<size_t> where;
  segs.reserve(outs.size());
  for (size_t i = 0; i < outs.size(); i++) {
    if (!count_only && d_dst[i] == nullptr) continue;   // skipped: none of its parameters are looked at
    const uint64_t cap = count_only ? 0u : caps[i];
    if (!known_blocks(widths[i], flags ? flags[i] : 0u, cap, !count_only, "stream", i)) return -1;
    push_blocks(&segs, outs[i].ptr, count_only ? nullptr : d_dst[i], outs[i].len, cap, widths[i]);
    where.push_back(i);
  }
  return blocks_device(b, segs, where, results, outs.size(), b->last_stream);
}

extern "C" float BrotliAmdBatchLastUnshuffleMs(BrotliAmdBatch* b) { return b ? b->filter[kUnshuffle].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndeltaMs(BrotliAmdBatch* b) { return b ? b->filter[kUndelta].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndeltaPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return b && phase >= 1u && phase <= 3u ? b->undelta_phase_ms[phase - 1u] : 0.0f; }
extern "C" float BrotliAmdBatchLastBitUnshuffleMs(BrotliAmdBatch* b) { return b ? b->filter[kBitUnshuffle].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastBitUnpackMs(BrotliAmdBatch* b) { return b ? b->filter[kBitUnpack].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUnvarintMs(BrotliAmdBatch* b) { return b ? b->filter[kUnvarint].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUnvarintPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return b && phase >= 1u && phase <= 3u ? b->unvarint_phase_ms[phase - 1u] : 0.0f; }
extern "C" float BrotliAmdBatchLastUnrleMs(BrotliAmdBatch* b) { return b ? b->filter[kUnrle].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUnrlePhaseMs(BrotliAmdBatch* b, uint32_t phase) { return b && phase >= 1u && phase <= 2u ? b->unrle_phase_ms[phase - 1u] : 0.0f; }
extern "C" float BrotliAmdBatchLastUndbpMs(BrotliAmdBatch* b) { return b ? b->filter[kUndbp].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndbpPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return b && phase >= 1u && phase <= 4u ? b->undbp_phase_ms[phase - 1u] : 0.0f; }
extern "C" uint32_t BrotliAmdDebugUndbpItemDeltas(void) { return brotli_amd_undbp_item_deltas(); }
extern "C" uint32_t BrotliAmdDebugUndbpWalkChunk(void) { return brotli_amd_undbp_walk_chunk(); }
extern "C" uint32_t BrotliAmdDebugUnrleItemElems(void) { return brotli_amd_unrle_item_elems(); }
extern "C" uint32_t BrotliAmdDebugUnrleWalkChunk(void) { return brotli_amd_unrle_walk_chunk(); }
extern "C" uint32_t BrotliAmdDebugUnvarintTile(void) { return brotli_amd_unvarint_tile_bytes(); }
extern "C" uint32_t BrotliAmdDebugUnshuffleTile(void) { return brotli_amd_unshuffle_tile_bytes(); }
extern "C" uint32_t BrotliAmdDebugUndeltaTile(void) { return brotli_amd_undelta_tile_bytes(); }
extern "C" uint32_t BrotliAmdDebugUndeltaCarrySpan(void) { return brotli_amd_undelta_carry_span(); }
extern "C" uint32_t BrotliAmdDebugBitUnshuffleTile(void) { return brotli_amd_bitunshuffle_tile_bytes(); }
extern "C" uint32_t BrotliAmdDebugBitUnpackTile(void) { return brotli_amd_bitunpack_tile_bytes(); }

// The hooks run the device's functions on the host over every unit of a segment, source and destination each in a SkewedRoom (brotli_host.h).

extern "C" int BrotliAmdDebugUnshuffleHost(uint32_t width, const uint8_t* src, size_t len, uint8_t* dst, uint32_t src_skew, uint32_t dst_skew) {
  if (!known_width(kUnshuffle, width)) return -1;
  if ((len && (!src || !dst)) || src_skew > 15u || dst_skew > 15u) return invalid_arguments(kUnshuffle);
  SkewedRoom sroom(len, src_skew, 0xA5), droom(len, dst_skew, 0x5A);
  sroom.put(src, len);
  droom.snapshot();
  const uint64_t units = brotli_amd_seg_units(droom.at(), len);
  // (two units a step, as a lane takes them in a tile inside one segment; odd `len`s of units end in a single one)
  for (uint64_t k = 0; k < units; k += 2u) brotli_amd_unshuffle_two_units(sroom.at(), droom.at(), len, width, k, units);
  return hook_result(kUnshuffle, droom, dst, len);
}

// The work is taken as the kernel takes a tile inside one segment: tile after tile of the segment's units, in each the slots in the lanes' order.
extern "C" int BrotliAmdDebugBitUnshuffleHost(uint32_t width, uint32_t block_elems, const uint8_t* src, size_t len, uint8_t* dst, uint32_t src_skew,
                                              uint32_t dst_skew, uint64_t* fast_items) {
  if (!known_width(kBitUnshuffle, width) || !known_block(block_elems)) return -1;
  if ((len && (!src || !dst)) || src_skew > 15u || dst_skew > 15u) return invalid_arguments(kBitUnshuffle);
  SkewedRoom sroom(len, src_skew, 0xA5), droom(len, dst_skew, 0x5A);
  sroom.put(src, len);
  droom.snapshot();
  const uint64_t units = brotli_amd_seg_units(droom.at(), len), tile = brotli_amd_bitunshuffle_tile_bytes() / 16u, slot = 2u * width;
  uint64_t items = 0;
  for (uint64_t t0 = 0; t0 < units; t0 += tile) {
    const uint64_t t1 = std::min(t0 + tile, units);
    for (uint64_t s = t0 / slot; slot * s < t1; s++) {
      const uint64_t ka = std::max(slot * s, t0), kb = std::min(slot * (s + 1u), t1);
      items += brotli_amd_bitunshuffle_range(sroom.at(), droom.at(), len, width, block_elems, ka, kb);
    }
  }
  if (fast_items) *fast_items = items;
  return hook_result(kBitUnshuffle, droom, dst, len);
}

// ... tile after tile and slot after slot as well
extern "C" int BrotliAmdDebugBitUnpackHost(uint32_t bits, uint32_t width, uint32_t flags, const uint8_t* src, size_t src_len, uint64_t count, uint8_t* dst,
                                           uint32_t src_skew, uint32_t dst_skew, uint64_t* fast_items) {
  if (!known_shape(bits, width, flags, "segment", 0) || !known_count(count, bits, src_len, "segment", 0)) return -1;
  if ((src_len && !src) || (count && !dst) || src_skew > 15u || dst_skew > 15u) return invalid_arguments(kBitUnpack);
  const uint64_t len = count * width;
  if (len > ((uint64_t)1 << 40)) { g_last_error = "bit-unpack on the host: more than 2^40 destination bytes"; return -1; }
  SkewedRoom sroom(src_len, src_skew, 0xA5), droom(len, dst_skew, 0x5A);
  sroom.put(src, src_len);
  droom.snapshot();
  const uint64_t units = brotli_amd_seg_units(droom.at(), len), tile = brotli_amd_bitunpack_tile_bytes() / 16u, slot = 2u * width;
  uint64_t items = 0;
  for (uint64_t t0 = 0; t0 < units; t0 += tile) {
    const uint64_t t1 = std::min(t0 + tile, units);
    for (uint64_t s = t0 / slot; slot * s < t1; s++) items += brotli_amd_bitunpack_slot(sroom.at(), droom.at(), count, width, bits, flags, s, t0, t1);
  }
  if (fast_items) *fast_items = items;
  return hook_result(kBitUnpack, droom, dst, len);
}

// Undelta's three phases, tile by tile, over n segments given as offsets into one source and one destination buffer, each buffer in its room.  In
// place: one room, filled from src, with the segments at their DESTINATION offsets.
extern "C" int BrotliAmdDebugUndeltaHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                         const uint64_t* dst_offs, const uint64_t* lens, const uint8_t* widths, uint32_t src_skew, uint32_t dst_skew,
                                         uint32_t tile_units, uint32_t order_seed, int in_place) {
  if ((n && (!src_offs || !dst_offs || !lens || !widths)) || (src_size && !src) || (dst_size && !dst) || src_skew > 15u || dst_skew > 15u ||
      (in_place && src_size != dst_size))
    return invalid_arguments(kUndelta);
  for (uint32_t i = 0; i < n; i++) {
    if (!known_width(kUndelta, widths[i])) return -1;
    if (lens[i] > dst_size || dst_offs[i] > dst_size - lens[i] || lens[i] > src_size || (!in_place && src_offs[i] > src_size - lens[i])) {
      g_last_error = "invalid undelta arguments: a segment outside its buffer";
      return -1;
    }
  }
  if (tile_units == 0u) tile_units = brotli_amd_undelta_tile_bytes() / 16u;
  SkewedRoom sroom(in_place ? 0u : src_size, src_skew, 0xA5), droom(dst_size, dst_skew, 0x5A);
  SkewedRoom& from = in_place ? droom : sroom;
  from.put(src, src_size);
  Segs segs(n);
  std::vector<uint64_t> pre(n + 1u, 0u);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t s = from.at() + (in_place ? dst_offs[i] : src_offs[i]), d = droom.at() + dst_offs[i];
    if (!placed_ok(s, d, widths[i])) return -1;
    segs[i] = BrotliAmdUnshuffleSeg{reinterpret_cast<const uint8_t*>((uintptr_t)s), reinterpret_cast<uint8_t*>((uintptr_t)d), lens[i], widths[i], 0u};
    pre[i + 1u] = pre[i] + brotli_amd_seg_units(d, lens[i]);
  }
  droom.snapshot();
  const uint64_t units = pre[n], ntiles = (units + tile_units - 1u) / tile_units;
  // phases 1 and 3 take the tiles in an order shuffled by the seed: the result may not depend on it
  std::vector<uint64_t> order(ntiles);
  std::iota(order.begin(), order.end(), (uint64_t)0);
  uint32_t rnd = order_seed * 2654435761u + 1u;
  auto shuffle = [&]() {
    if (order_seed == 0u) return;
    for (uint64_t i = ntiles; i > 1u; i--) { rnd = rnd * 1664525u + 1013904223u; std::swap(order[i - 1u], order[(rnd >> 8) % i]); }
  };
  auto tile_end = [&](uint64_t t) { return std::min<uint64_t>((t + 1u) * tile_units, units); };
  std::vector<BrotliAmdUndeltaTile> tiles(ntiles);
  std::vector<uint64_t> carries(ntiles);
  shuffle();
  for (uint64_t t : order) tiles[t] = brotli_amd_undelta_host_summary(segs.data(), pre.data(), n, t * tile_units, tile_end(t));
  BrotliAmdUndeltaPair out = {0u, 0u};
  for (uint64_t t = 0; t < ntiles; t++) {
    carries[t] = brotli_amd_undelta_carry_in(out.sum, tiles[t]);
    out = brotli_amd_undelta_combine(out, brotli_amd_undelta_tile_pair(tiles[t]));
  }
  shuffle();
  for (uint64_t t : order) brotli_amd_undelta_host_apply(segs.data(), pre.data(), n, t * tile_units, tile_end(t), carries[t]);
  // no byte outside every segment's destination may have changed
  std::vector<uint8_t> inside(dst_size, 0);
  for (uint32_t i = 0; i < n; i++) std::fill(inside.begin() + dst_offs[i], inside.begin() + dst_offs[i] + lens[i], 1);
  if (!droom.changed_inside_only([&](size_t i) { return i < dst_size && inside[i]; })) { g_last_error = "undelta wrote outside its destination"; return -2; }
  for (uint32_t i = 0; i < n; i++) droom.get(dst + dst_offs[i], dst_offs[i], lens[i]);
  return 0;
}

// Unvarint's three phases, tile by tile, over n segments given as offsets into one source and one destination buffer, each buffer in its room.
extern "C" int BrotliAmdDebugUnvarintHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                          const uint64_t* src_lens, const uint64_t* dst_offs, const uint64_t* caps, const uint8_t* widths, const uint8_t* flags,
                                          uint32_t src_skew, uint32_t dst_skew, uint32_t tile_units, uint32_t order_seed, BrotliAmdUnvarintResult* results) {
  if ((n && (!src_offs || !src_lens || !dst_offs || !caps || !widths || !results)) || (src_size && !src) || (dst_size && !dst) || src_skew > 15u || dst_skew > 15u)
    return invalid_arguments(kUnvarint);
  for (uint32_t i = 0; i < n; i++) {
    if (!known_varint(widths[i], flags ? flags[i] : 0u, caps[i], true, "segment", i)) return -1;
    const uint64_t room = std::min<uint64_t>(caps[i], src_lens[i]) * widths[i];   // (a segment of len bytes holds len varints at the most)
    if (src_lens[i] > src_size || src_offs[i] > src_size - src_lens[i] || room > dst_size || dst_offs[i] > dst_size - room) {
      g_last_error = "invalid unvarint arguments: a segment outside its buffer";
      return -1;
    }
  }
  if (tile_units == 0u) tile_units = brotli_amd_unvarint_tile_bytes() / 16u;
  SkewedRoom sroom(src_size, src_skew, 0xA5), droom(dst_size, dst_skew, 0x5A);
  sroom.put(src, src_size);
  droom.put(dst, dst_size);
  VarintSegs segs(n);
  std::vector<uint64_t> pre(n + 1u, 0u);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t s = sroom.at() + src_offs[i], d = droom.at() + dst_offs[i];
    segs[i] = BrotliAmdUnvarintSeg{reinterpret_cast<const uint8_t*>((uintptr_t)s), reinterpret_cast<uint8_t*>((uintptr_t)d), src_lens[i], caps[i], widths[i],
                                   flags ? flags[i] : 0u};
    pre[i + 1u] = pre[i] + brotli_amd_seg_units(s, src_lens[i]);
  }
  droom.snapshot();
  const uint64_t units = pre[n], ntiles = (units + tile_units - 1u) / tile_units;
  // phases 1 and 3 take the tiles in an order shuffled by the seed: the result may not depend on it
  std::vector<uint64_t> order(ntiles);
  std::iota(order.begin(), order.end(), (uint64_t)0);
  uint32_t rnd = order_seed * 2654435761u + 1u;
  auto shuffle = [&]() {
    if (order_seed == 0u) return;
    for (uint64_t i = ntiles; i > 1u; i--) { rnd = rnd * 1664525u + 1013904223u; std::swap(order[i - 1u], order[(rnd >> 8) % i]); }
  };
  auto tile_end = [&](uint64_t t) { return std::min<uint64_t>((t + 1u) * tile_units, units); };
  std::vector<BrotliAmdUndeltaTile> tiles(ntiles);
  std::vector<uint64_t> carries(ntiles);
  std::vector<BrotliAmdUnvarintResult> got(n, BrotliAmdUnvarintResult{0u, 0u, 0u});
  shuffle();
  for (uint64_t t : order) tiles[t] = brotli_amd_unvarint_host_summary(segs.data(), pre.data(), n, t * tile_units, tile_end(t));
  BrotliAmdUndeltaPair out = {0u, 0u};
  for (uint64_t t = 0; t < ntiles; t++) {
    carries[t] = brotli_amd_undelta_carry_in(out.sum, tiles[t]);
    out = brotli_amd_undelta_combine(out, brotli_amd_undelta_tile_pair(tiles[t]));
  }
  shuffle();
  for (uint64_t t : order) brotli_amd_unvarint_host_emit(segs.data(), pre.data(), n, t * tile_units, tile_end(t), carries[t], got.data());
  // no byte outside every segment's elements may have changed
  std::vector<uint8_t> inside(dst_size, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t bytes = std::min(got[i].count, caps[i]) * widths[i];
    if (bytes > dst_size - dst_offs[i]) { g_last_error = "unvarint counted more varints than the segment has bytes"; return -2; }
    std::fill(inside.begin() + dst_offs[i], inside.begin() + dst_offs[i] + bytes, 1);
  }
  if (!droom.changed_inside_only([&](size_t i) { return i < dst_size && inside[i]; })) { g_last_error = "unvarint wrote outside its destination"; return -2; }
  droom.get(dst, 0u, dst_size);
  std::copy(got.begin(), got.end(), results);
  return 0;
}

// Unrle's two phases over n segments given as offsets into one source and one destination buffer, each buffer in its room: every segment's walk,
// then the items of all segments in an order shuffled by the seed.
extern "C" int BrotliAmdDebugUnrleHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                       const uint64_t* src_lens, const uint64_t* dst_offs, const uint64_t* caps, const uint8_t* bits, const uint8_t* widths,
                                       const uint8_t* flags, uint32_t src_skew, uint32_t dst_skew, uint32_t item_elems, uint32_t order_seed,
                                       BrotliAmdUnrleResult* results) {
  if ((n && (!src_offs || !src_lens || !dst_offs || !caps || !bits || !widths || !results)) || (src_size && !src) || (dst_size && !dst) || src_skew > 15u ||
      dst_skew > 15u)
    return invalid_arguments(kUnrle);
  if (item_elems == 0u) item_elems = brotli_amd_unrle_item_elems();
  for (uint32_t i = 0; i < n; i++) {
    if (!known_runs(bits[i], widths[i], flags ? flags[i] : 0u, caps[i], true, "segment", i)) return -1;
    if (src_lens[i] > src_size || src_offs[i] > src_size - src_lens[i] || dst_offs[i] > dst_size) {
      g_last_error = "invalid unrle arguments: a segment outside its buffer";
      return -1;
    }
  }
  SkewedRoom sroom(src_size, src_skew, 0xA5), droom(dst_size, dst_skew, 0x5A);
  sroom.put(src, src_size);
  droom.put(dst, dst_size);
  // the walks: they write nothing, and say how much room every segment needs
  RleSegs segs;
  std::vector<BrotliAmdUnrleResult> got(n);
  std::vector<std::vector<BrotliAmdUnrleCheckpoint>> ckpts(n);
  std::vector<std::pair<uint32_t, uint64_t>> order;   // (segment, item)
  for (uint32_t i = 0; i < n; i++) {
    // (the items of the elements there is room for: the walk marks no others, and a capacity of 2^56 needs no table of its own)
    const uint64_t room = (dst_size - dst_offs[i]) / widths[i], cap = std::min<uint64_t>(caps[i], room + 1u);
    segs.push_back(BrotliAmdUnrleSeg{reinterpret_cast<const uint8_t*>((uintptr_t)(sroom.at() + src_offs[i])), reinterpret_cast<uint8_t*>((uintptr_t)(droom.at() + dst_offs[i])),
                                     src_lens[i], cap, 0u, widths[i], bits[i], flags ? flags[i] : 0u, 0u});
    ckpts[i].assign(brotli_amd_unrle_items(cap, item_elems), BrotliAmdUnrleCheckpoint{BROTLI_AMD_UNRLE_NONE, BROTLI_AMD_UNRLE_NONE});
    got[i] = brotli_amd_unrle_host_walk(segs[i], item_elems, ckpts[i].data());
    if (std::min(got[i].count, caps[i]) > room) {
      g_last_error = "invalid unrle arguments: a segment outside its buffer";
      return -1;
    }
    for (uint64_t j = 0; j < ckpts[i].size(); j++) order.push_back({i, j});
  }
  droom.snapshot();
  uint32_t rnd = order_seed * 2654435761u + 1u;
  if (order_seed != 0u)
    for (size_t i = order.size(); i > 1u; i--) { rnd = rnd * 1664525u + 1013904223u; std::swap(order[i - 1u], order[(rnd >> 8) % i]); }
  for (const auto& it : order) brotli_amd_unrle_host_item(segs[it.first], got[it.first], ckpts[it.first][it.second], it.second, item_elems);
  // no byte outside every segment's elements may have changed
  std::vector<uint8_t> inside(dst_size, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t bytes = std::min(got[i].count, caps[i]) * widths[i];
    std::fill(inside.begin() + dst_offs[i], inside.begin() + dst_offs[i] + bytes, 1);
  }
  if (!droom.changed_inside_only([&](size_t i) { return i < dst_size && inside[i]; })) { g_last_error = "unrle wrote outside its destination"; return -2; }
  droom.get(dst, 0u, dst_size);
  std::copy(got.begin(), got.end(), results);
  return 0;
}

// Undbp's phases over n segments given as offsets into one source and one destination buffer, each buffer in its room: every segment's walk, the
// items' sums in an order shuffled by the seed, the carries as undelta's hook takes them, and the items' stores in another shuffled order.
extern "C" int BrotliAmdDebugUndbpHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                       const uint64_t* src_lens, const uint64_t* dst_offs, const uint64_t* caps, const uint8_t* widths, const uint8_t* flags,
                                       uint32_t src_skew, uint32_t dst_skew, uint32_t item_deltas, uint32_t order_seed, BrotliAmdUndbpResult* results) {
  if ((n && (!src_offs || !src_lens || !dst_offs || !caps || !widths || !results)) || (src_size && !src) || (dst_size && !dst) || src_skew > 15u || dst_skew > 15u)
    return invalid_arguments(kUndbp);
  if (item_deltas == 0u) item_deltas = brotli_amd_undbp_item_deltas();
  if (!brotli_amd_undbp_item_ok(item_deltas)) { g_last_error = "invalid undbp arguments: an item that is no multiple of 32 deltas"; return -1; }
  for (uint32_t i = 0; i < n; i++) {
    if (!known_blocks(widths[i], flags ? flags[i] : 0u, caps[i], true, "segment", i)) return -1;
    if (src_lens[i] > src_size || src_offs[i] > src_size - src_lens[i] || dst_offs[i] > dst_size) {
      g_last_error = "invalid undbp arguments: a segment outside its buffer";
      return -1;
    }
  }
  SkewedRoom sroom(src_size, src_skew, 0xA5), droom(dst_size, dst_skew, 0x5A);
  sroom.put(src, src_size);
  droom.put(dst, dst_size);
  // the walks: they write nothing, and say how much room every segment needs
  DbpSegs segs;
  std::vector<BrotliAmdUndbpResult> got(n);
  std::vector<uint64_t> firsts(n, 0u), pre(n + 1u, 0u);
  std::vector<BrotliAmdUndbpCheckpoint> ckpts;
  for (uint32_t i = 0; i < n; i++) {
    // (the items of the elements there is room for: the walk marks no others, and a capacity of 2^56 needs no table of its own)
    const uint64_t room = (dst_size - dst_offs[i]) / widths[i], cap = std::min<uint64_t>(caps[i], room + 1u);
    segs.push_back(BrotliAmdUndbpSeg{reinterpret_cast<const uint8_t*>((uintptr_t)(sroom.at() + src_offs[i])), reinterpret_cast<uint8_t*>((uintptr_t)(droom.at() + dst_offs[i])),
                                     src_lens[i], cap, pre[i], widths[i], 0u});
    pre[i + 1u] = pre[i] + brotli_amd_undbp_items(cap, item_deltas);
    ckpts.resize(pre[i + 1u], BrotliAmdUndbpCheckpoint{BROTLI_AMD_UNDBP_NONE, BROTLI_AMD_UNDBP_NONE});
    got[i] = brotli_amd_undbp_host_walk(segs[i], item_deltas, ckpts.data() + pre[i], &firsts[i]);
    if (std::min(got[i].count, caps[i]) > room) {
      g_last_error = "invalid undbp arguments: a segment outside its buffer";
      return -1;
    }
  }
  droom.snapshot();
  const uint64_t items = pre[n];
  std::vector<uint64_t> order(items);
  std::iota(order.begin(), order.end(), (uint64_t)0);
  uint32_t rnd = order_seed * 2654435761u + 1u;
  auto shuffle = [&]() {
    if (order_seed == 0u) return;
    for (uint64_t i = items; i > 1u; i--) { rnd = rnd * 1664525u + 1013904223u; std::swap(order[i - 1u], order[(rnd >> 8) % i]); }
  };
  std::vector<BrotliAmdUndeltaTile> tiles(items);
  std::vector<uint64_t> carries(items);
  shuffle();
  for (uint64_t g : order) {
    const uint32_t i = brotli_amd_seg_find(pre.data(), n, g);
    tiles[g] = brotli_amd_undbp_host_sum(segs[i], got[i], ckpts[g], firsts[i], g - pre[i], item_deltas);
  }
  BrotliAmdUndeltaPair out = {0u, 0u};
  for (uint64_t g = 0; g < items; g++) {
    carries[g] = brotli_amd_undelta_carry_in(out.sum, tiles[g]);
    out = brotli_amd_undelta_combine(out, brotli_amd_undelta_tile_pair(tiles[g]));
  }
  shuffle();
  for (uint64_t g : order) {
    const uint32_t i = brotli_amd_seg_find(pre.data(), n, g);
    brotli_amd_undbp_host_store(segs[i], got[i], ckpts[g], firsts[i], g - pre[i], item_deltas, carries[g]);
  }
  // no byte outside every segment's elements may have changed
  std::vector<uint8_t> inside(dst_size, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t bytes = std::min(got[i].count, caps[i]) * widths[i];
    std::fill(inside.begin() + dst_offs[i], inside.begin() + dst_offs[i] + bytes, 1);
  }
  if (!droom.changed_inside_only([&](size_t i) { return i < dst_size && inside[i]; })) { g_last_error = "undbp wrote outside its destination"; return -2; }
  droom.get(dst, 0u, dst_size);
  std::copy(got.begin(), got.end(), results);
  return 0;
}
