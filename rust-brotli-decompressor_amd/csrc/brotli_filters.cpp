// brotli_filters.cpp -- the element filters on the device (include/brotli/batch.h), each over n segments of device memory (BrotliAmdBatch*Segments)
// or over the delivered bytes of every stream of the last decode call (BrotliAmdBatch*Outputs).  In four parts:
//   the descriptor  kFilter: a filter's name in the texts, its launcher -- one signature for all --, its room behind the table, its events.
//                   filter_device runs any table through it and keeps the call's times with the batch object.
//   the plain path  unshuffle, undelta, bit-unshuffle, bit-unpack: a table of BrotliAmdUnshuffleSeg built from the caller's arrays or from the
//                   outputs by a shape check per filter; nothing comes back but the destination's bytes.
//   the counted path  unvarint, unrle, undbp, undict: a capacity per segment and a result per segment.  A traits struct a filter (its segment, its
//                   result, its shape check, how an entry is made, how many items a capacity gives, whether it has a dictionary) under three
//                   templates: counted_device, counted_segments, counted_outputs.
//   unnull          beside the counted path: two sources, two destinations and a level a segment are columns of its own; it shares the counted
//                   table's members and counted_device, and the four counted filters' templates do not know of it.
//   undict-bytes    beside them as well: two destinations a segment, and a second table -- the call's DISTINCT dictionaries -- behind the
//                   segments, so it has a launcher, a table and a device call of its own.
//   undlba          beside them too: two destinations a segment and no dictionary; its launcher wants the bound of the bytes its copies move.
//   undba           beside them too: undlba's segments and checks under its own name, a result of its own.
//   the hooks       BrotliAmdDebug*Host run the device's functions of a filter's header (csrc/brotli_<filter>.h) on the host as the kernel's lanes
//                   take them, for tests without a device.  They share the seeded orders, the serial carries, the argument checks and the
//                   counted filters' closing block; each keeps its own phase loops.
#include "brotli_bitunpack.h"
#include "brotli_bitunshuffle.h"
#include "brotli_host.h"
#include "brotli_undbp.h"
#include "brotli_undict.h"
#include "brotli_undict_bytes.h"
#include "brotli_undelta.h"
#include "brotli_undba.h"
#include "brotli_undlba.h"
#include "brotli_unnull.h"
#include "brotli_unrle.h"
#include "brotli_unshuffle.h"
#include "brotli_unvarint.h"

#include <map>
#include <numeric>
#include <tuple>

// (csrc/brotli_*_kernels.hip: d_segs: the filter's table on the device; units: the segments' units together; d_scratch: what lies behind the table;
// ev: the filter's events, recorded around and between its launches)
typedef hipError_t FilterLaunch(const void* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev);
extern "C" FilterLaunch brotli_amd_launch_unshuffle, brotli_amd_launch_undelta, brotli_amd_launch_bitunshuffle, brotli_amd_launch_bitunpack,
    brotli_amd_launch_unvarint, brotli_amd_launch_unrle, brotli_amd_launch_undbp, brotli_amd_launch_undict, brotli_amd_launch_unnull;
extern "C" uint64_t brotli_amd_unnull_scratch_bytes(uint64_t units, uint32_t n);
// (csrc/brotli_undict_bytes_kernels.hip: d_dicts: the call's nd distinct dictionaries, whose entry positions are `starts` together)
extern "C" uint64_t brotli_amd_undict_bytes_scratch_bytes(uint64_t units, uint32_t n, uint32_t nd, uint64_t starts);
extern "C" hipError_t brotli_amd_launch_undict_bytes(const void* d_segs, uint32_t n, uint64_t units, const void* d_dicts, uint32_t nd, void* d_scratch, hipStream_t stream,
                                                     const hipEvent_t* ev);
// (csrc/brotli_undlba_kernels.hip: max_bytes: what the segments' copies add up to at the most)
extern "C" uint64_t brotli_amd_undlba_scratch_bytes(uint64_t units, uint32_t n);
extern "C" hipError_t brotli_amd_launch_undlba(const void* d_segs, uint32_t n, uint64_t units, uint64_t max_bytes, void* d_scratch, hipStream_t stream, const hipEvent_t* ev);
// (csrc/brotli_undba_kernels.hip)
extern "C" uint64_t brotli_amd_undba_scratch_bytes(uint64_t units, uint32_t n);
extern "C" hipError_t brotli_amd_launch_undba(const void* d_segs, uint32_t n, uint64_t units, void* d_scratch, hipStream_t stream, const hipEvent_t* ev);
extern "C" uint32_t brotli_amd_undba_lds_string(void);
extern "C" uint32_t brotli_amd_undba_lds_carry(void);
extern "C" uint64_t brotli_amd_undelta_scratch_bytes(uint64_t units);
extern "C" uint64_t brotli_amd_unvarint_scratch_bytes(uint64_t units, uint32_t n);
extern "C" uint64_t brotli_amd_unrle_scratch_bytes(uint64_t units, uint32_t n);
extern "C" uint64_t brotli_amd_undbp_scratch_bytes(uint64_t units, uint32_t n);
extern "C" uint64_t brotli_amd_undict_scratch_bytes(uint64_t units, uint32_t n);
extern "C" uint32_t brotli_amd_undbp_item_deltas(void);
extern "C" uint32_t brotli_amd_undbp_walk_chunk(void);
extern "C" uint32_t brotli_amd_unrle_item_elems(void);
extern "C" uint32_t brotli_amd_unrle_walk_chunk(void);
extern "C" uint32_t brotli_amd_unvarint_tile_bytes(void);
extern "C" uint32_t brotli_amd_unshuffle_tile_bytes(void);
extern "C" uint32_t brotli_amd_undelta_tile_bytes(void);
extern "C" uint32_t brotli_amd_undelta_carry_span(void);
extern "C" uint32_t brotli_amd_bitunshuffle_tile_bytes(void);
extern "C" uint32_t brotli_amd_bitunpack_tile_bytes(void);

using namespace brotli_amd_host;

namespace {

// ---- the descriptor ----
// What the host needs to know of a filter.  A filter of one launch has two events; undelta and unvarint have four around and between their three
// launches, unrle and undict three, undbp and unnull five, undict-bytes six, undlba eight and undba ten -- the last three with launchers of their own
// signatures (undict_bytes_device, undlba_device, undba_device).  The counted filters' results lie first behind the table.
struct FilterDesc {
  const char* name;   // in the texts of g_last_error
  SegCallWhat what;
  const char* launch_what;
  FilterLaunch* launch;
  uint64_t (*scratch_bytes)(uint64_t units, uint32_t n);   // behind the table (nullptr: nothing)
  uint32_t events;
};
const FilterDesc kFilter[kFilters] = {
    {"unshuffle", {"hipMalloc(unshuffle segments)", "hipMemcpyAsync(unshuffle segments)", "hipStreamSynchronize(unshuffle)"},
     "brotli_amd_unshuffle_kernel launch", brotli_amd_launch_unshuffle, nullptr, 2u},
    {"undelta", {"hipMalloc(undelta segments and tiles)", "hipMemcpyAsync(undelta segments)", "hipStreamSynchronize(undelta)"},
     "brotli_amd_undelta kernels launch", brotli_amd_launch_undelta, [](uint64_t units, uint32_t) { return brotli_amd_undelta_scratch_bytes(units); }, 4u},
    {"bit-unshuffle", {"hipMalloc(bit-unshuffle segments)", "hipMemcpyAsync(bit-unshuffle segments)", "hipStreamSynchronize(bit-unshuffle)"},
     "brotli_amd_bitunshuffle_kernel launch", brotli_amd_launch_bitunshuffle, nullptr, 2u},
    {"bit-unpack", {"hipMalloc(bit-unpack segments)", "hipMemcpyAsync(bit-unpack segments)", "hipStreamSynchronize(bit-unpack)"},
     "brotli_amd_bitunpack_kernel launch", brotli_amd_launch_bitunpack, nullptr, 2u},
    {"unvarint", {"hipMalloc(unvarint segments, tiles and results)", "hipMemcpyAsync(unvarint segments)", "hipStreamSynchronize(unvarint)"},
     "brotli_amd_unvarint kernels launch", brotli_amd_launch_unvarint, brotli_amd_unvarint_scratch_bytes, 4u},
    {"unrle", {"hipMalloc(unrle segments, results and checkpoints)", "hipMemcpyAsync(unrle segments)", "hipStreamSynchronize(unrle)"},
     "brotli_amd_unrle kernels launch", brotli_amd_launch_unrle, brotli_amd_unrle_scratch_bytes, 3u},
    {"undbp", {"hipMalloc(undbp segments, results, checkpoints and tiles)", "hipMemcpyAsync(undbp segments)", "hipStreamSynchronize(undbp)"},
     "brotli_amd_undbp kernels launch", brotli_amd_launch_undbp, brotli_amd_undbp_scratch_bytes, 5u},
    {"undict", {"hipMalloc(undict segments, results and checkpoints)", "hipMemcpyAsync(undict segments)", "hipStreamSynchronize(undict)"},
     "brotli_amd_undict kernels launch", brotli_amd_launch_undict, brotli_amd_undict_scratch_bytes, 3u},
    {"unnull", {"hipMalloc(unnull segments, results, checkpoints and tiles)", "hipMemcpyAsync(unnull segments)", "hipStreamSynchronize(unnull)"},
     "brotli_amd_unnull kernels launch", brotli_amd_launch_unnull, brotli_amd_unnull_scratch_bytes, 5u},
    {"undict-bytes", {"hipMalloc(undict-bytes segments, dictionaries, results, checkpoints, tiles and entry positions)", "hipMemcpyAsync(undict-bytes segments)",
                      "hipStreamSynchronize(undict-bytes)"},
     "brotli_amd_undict_bytes kernels launch", nullptr, nullptr, 6u},
    {"undlba", {"hipMalloc(undlba segments, results, checkpoints, tiles and copies)", "hipMemcpyAsync(undlba segments)", "hipStreamSynchronize(undlba)"},
     "brotli_amd_undlba kernels launch", nullptr, nullptr, 8u},
    {"undba", {"hipMalloc(undba segments, results, checkpoints, tiles and last elements)", "hipMemcpyAsync(undba segments)", "hipStreamSynchronize(undba)"},
     "brotli_amd_undba kernels launch", nullptr, nullptr, 10u},
};

typedef std::vector<BrotliAmdUnshuffleSeg> Segs;

// a segment's units: its destination's words, unvarint's its source's (brotli_seg_walk.h), unrle's and undbp's one for its walk and one for every item
inline uint64_t units_of(const BrotliAmdUnshuffleSeg& s) { return brotli_amd_seg_units((uint64_t)(uintptr_t)s.dst, s.len); }
inline uint64_t units_of(const BrotliAmdUnvarintSeg& s) { return brotli_amd_seg_units((uint64_t)(uintptr_t)s.src, s.len); }
inline uint64_t units_of(const BrotliAmdUnrleSeg& s) { return 1u + brotli_amd_unrle_items(s.cap, brotli_amd_unrle_item_elems()); }
inline uint64_t units_of(const BrotliAmdUndbpSeg& s) { return 1u + brotli_amd_undbp_items(s.cap, brotli_amd_undbp_item_deltas()); }
inline uint64_t units_of(const BrotliAmdUndictSeg& s) { return 1u + brotli_amd_unrle_items(s.cap, brotli_amd_unrle_item_elems()); }
inline uint64_t units_of(const BrotliAmdUnnullSeg& s) { return 1u + brotli_amd_unrle_items(s.cap, brotli_amd_unrle_item_elems()); }
inline uint64_t units_of(const BrotliAmdUndictBytesSeg& s) { return 1u + brotli_amd_unrle_items(s.cap, brotli_amd_unrle_item_elems()); }

int invalid_arguments(Filter f) { g_last_error = std::string("invalid ") + kFilter[f].name + " arguments"; return -1; }

// an entry point begins: no times of an earlier call
void no_times(BrotliAmdBatch* b, Filter f) {
  b->filter[f].ms = 0.0f;
  for (float& ms : b->filter[f].phase_ms) ms = 0.0f;
}
// the time of launch `phase` (1 ..) of filter f's last call; 0 for a phase it does not have
float phase_ms(const BrotliAmdBatch* b, Filter f, uint32_t phase) { return b && phase >= 1u && phase < kFilter[f].events ? b->filter[f].phase_ms[phase - 1u] : 0.0f; }

// segs on `stream`, waited for (their shapes were checked).  scratch_out: the device memory behind the table, where a counted filter's results
// lie until the next call (nullptr: nothing was launched)
template <class Seg>
int filter_device(BrotliAmdBatch* b, Filter f, const std::vector<Seg>& segs, hipStream_t stream, const uint8_t** scratch_out = nullptr) {
  if (scratch_out) *scratch_out = nullptr;
  if (segs.empty()) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const FilterDesc& d = kFilter[f];
  const uint32_t n = (uint32_t)segs.size();
  uint64_t units = 0;   // of all segments together (brotli_seg_walk.h)
  for (const Seg& s : segs) units += units_of(s);
  if (units == 0u) return 0;   // (segments without bytes: nothing to launch)
  return run_seg_call(&b->filter[f].call, d.what, segs.data(), sizeof(Seg) * n, d.scratch_bytes ? d.scratch_bytes(units, n) : 0u, d.events, stream,
                      [&](uint8_t* d_table, uint8_t* d_scratch, const hipEvent_t* ev) {
    if (scratch_out) *scratch_out = d_scratch;
    return hip_ok(d.launch(d_table, n, units, d_scratch, stream, ev), d.launch_what);
  }, &b->filter[f].ms, d.events > 2u ? b->filter[f].phase_ms : nullptr);
}

// ---- the plain path: a call's segments, each checked in front of everything that touches the device ----
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

// ---- the counted path: a width, flags and a capacity (unrle: a field width too); a result per segment ----
// What differs between the counted filters.  kFlags: the flag bits it knows; kMaxCap: the largest capacity; kBits: it has a column of field widths
// and names it in its texts; kItems: its units are items of its destination; field_fault: what is wrong with a field width (nullptr: nothing); items: the items a capacity gives (unvarint: none, its
// units are its source's); make: a table entry, first_item being the items of the entries in front of it; kDict: it has the two dictionary
// columns, and make takes what they say; empty: the result of a segment that was not looked at.
struct Dict { const void* ptr; uint64_t entries; };   // a segment's dictionary (undict's; nothing elsewhere)
struct Unvarint {
  typedef BrotliAmdUnvarintSeg Seg;
  typedef BrotliAmdUnvarintResult Result;
  static constexpr Filter kId = kUnvarint;
  static constexpr uint32_t kFlags = BROTLI_AMD_UNVARINT_FLAGS;
  static constexpr uint64_t kMaxCap = BROTLI_AMD_UNVARINT_MAX_CAP;
  static constexpr bool kBits = false, kItems = false, kDict = false;
  static const char* field_fault(uint32_t, uint32_t, uint32_t) { return nullptr; }
  static uint64_t items(uint64_t) { return 0u; }
  static Seg make(const uint8_t* src, uint8_t* dst, uint64_t len, uint64_t cap, uint32_t width, uint32_t, uint32_t flags, uint64_t, Dict) {
    return Seg{src, dst, len, cap, width, flags};
  }
};
struct Unrle {
  typedef BrotliAmdUnrleSeg Seg;
  typedef BrotliAmdUnrleResult Result;
  static constexpr Filter kId = kUnrle;
  static constexpr uint32_t kFlags = BROTLI_AMD_UNRLE_FLAGS;
  static constexpr uint64_t kMaxCap = BROTLI_AMD_UNRLE_MAX_CAP;
  static constexpr bool kBits = true, kItems = true, kDict = false;
  static const char* field_fault(uint32_t bits, uint32_t width, uint32_t flags) {
    if ((flags & BROTLI_AMD_UNRLE_WIDTH_BYTE) != 0u) return nullptr;   // (the field width is in the source, and bits is not looked at)
    return bits > BROTLI_AMD_UNRLE_MAX_BITS ? "field of more than 32 bits" : bits > 8u * width ? "field is wider than the element" : nullptr;
  }
  static uint64_t items(uint64_t cap) { return brotli_amd_unrle_items(cap, brotli_amd_unrle_item_elems()); }
  static Seg make(const uint8_t* src, uint8_t* dst, uint64_t len, uint64_t cap, uint32_t width, uint32_t bits, uint32_t flags, uint64_t first_item, Dict) {
    return Seg{src, dst, len, cap, first_item, width, bits, flags, 0u};
  }
};
struct Undbp {
  typedef BrotliAmdUndbpSeg Seg;
  typedef BrotliAmdUndbpResult Result;
  static constexpr Filter kId = kUndbp;
  static constexpr uint32_t kFlags = 0u;
  static constexpr uint64_t kMaxCap = BROTLI_AMD_UNDBP_MAX_CAP;
  static constexpr bool kBits = false, kItems = true, kDict = false;
  static const char* field_fault(uint32_t, uint32_t, uint32_t) { return nullptr; }
  static uint64_t items(uint64_t cap) { return brotli_amd_undbp_items(cap, brotli_amd_undbp_item_deltas()); }
  static Seg make(const uint8_t* src, uint8_t* dst, uint64_t len, uint64_t cap, uint32_t width, uint32_t, uint32_t, uint64_t first_item, Dict) {
    return Seg{src, dst, len, cap, first_item, width, 0u};
  }
};
struct Undict {
  typedef BrotliAmdUndictSeg Seg;
  typedef BrotliAmdUndictResult Result;
  static constexpr Filter kId = kUndict;
  static constexpr uint32_t kFlags = BROTLI_AMD_UNDICT_FLAGS;
  static constexpr uint64_t kMaxCap = BROTLI_AMD_UNDICT_MAX_CAP;
  static constexpr bool kBits = true, kItems = true, kDict = true;
  static const char* field_fault(uint32_t bits, uint32_t, uint32_t flags) {   // (an index is not bound by the element's width)
    return (flags & BROTLI_AMD_UNDICT_WIDTH_BYTE) == 0u && bits > BROTLI_AMD_UNRLE_MAX_BITS ? "field of more than 32 bits" : nullptr;
  }
  static uint64_t items(uint64_t cap) { return brotli_amd_unrle_items(cap, brotli_amd_unrle_item_elems()); }
  static Seg make(const uint8_t* src, uint8_t* dst, uint64_t len, uint64_t cap, uint32_t width, uint32_t bits, uint32_t flags, uint64_t first_item, Dict d) {
    return Seg{src, dst, len, cap, first_item, width, bits, flags, 0u, static_cast<const uint8_t*>(d.ptr), d.entries};
  }
};
// the result of a segment that was not looked at: zeros, and of undict no first bad element
template <class T> typename T::Result empty_result() { return typename T::Result{}; }
template <> BrotliAmdUndictResult empty_result<Undict>() { return BrotliAmdUndictResult{0u, 0u, 0u, 0u, 0u, 0u, BROTLI_AMD_UNDICT_NONE}; }

// the shape check.  (A table has a hundred thousand segments: what passes costs a few comparisons in the caller's loop, and the text -- it names
// the first clause that fails, and `who` names the segment or stream -- is built out of line.)
template <class T>
__attribute__((noinline)) bool refuse_counted(const char* what, uint32_t bits, uint32_t width, uint32_t flags, uint64_t cap, Dict d, const char* who, size_t i) {
  g_last_error = std::string(kFilter[T::kId].name) + " " + who + " " + std::to_string(i) + ": " + what + " (" + (T::kBits ? "bits " + std::to_string(bits) + ", " : "") +
                 "width " + std::to_string(width) + ", flags " + std::to_string(flags) + ", capacity " + std::to_string(cap) +
                 (T::kDict ? ", dictionary entries " + std::to_string(d.entries) : "") + ")";
  return false;
}
template <class T>
inline bool known_counted(uint32_t bits, uint32_t width, uint32_t flags, uint64_t cap, bool has_dst, const char* who, size_t i, Dict d = Dict{nullptr, 0u}) {
  const char* what = nullptr;
  if (!brotli_amd_unshuffle_width_ok(width)) what = "width is not 1, 2, 4 or 8";
  else if ((flags & ~T::kFlags) != 0u) what = "unknown flag bits";
  else if ((what = T::field_fault(bits, width, flags)) != nullptr) {}
  else if (cap > T::kMaxCap) what = "a capacity above 2^56 elements";
  else if (cap != 0u && !has_dst) what = "no destination for a capacity that is not 0";
  else if (T::kDict && d.entries > BROTLI_AMD_UNDICT_MAX_ENTRIES) what = "a dictionary of more than 2^56 entries";
  else if (T::kDict && cap != 0u && d.entries != 0u && !d.ptr) what = "no dictionary for entries and a capacity that are not 0";
  return !what || refuse_counted<T>(what, bits, width, flags, cap, d, who, i);
}

// a call's columns, by segment or stream: flags may be NULL (zeros), bits is looked at where the filter has field widths, and dicts and
// dict_entries where it has dictionaries (NULL: none, and no entries)
struct Columns {
  const uint64_t* caps; const uint8_t* bits; const uint8_t* widths; const uint8_t* flags;
  const void* const* dicts = nullptr; const uint64_t* dict_entries = nullptr;
  Dict dict(size_t i) const { return Dict{dicts ? dicts[i] : nullptr, dict_entries ? dict_entries[i] : 0u}; }
};

// A counted call's table, entry by entry: each checked, then made where it stays.  `where`: the index of every entry's result.
template <class T>
struct CountedTable {
  std::vector<typename T::Seg> segs;
  std::vector<size_t> where;
  uint64_t items = 0;   // of all entries so far
  void reserve(size_t n) { segs.reserve(n); where.reserve(n); }
  // entry i of the call, with a capacity and a destination that its caller has settled -- false: g_last_error says why.  (In the caller's loop:
  // as a function of its own it cost a call with nine arguments a segment, 0.25 ms in a table of a hundred thousand -- profiles/filter_host_paths.txt.)
  __attribute__((always_inline)) bool push(const Columns& c, size_t i, const void* src, void* dst, uint64_t len, uint64_t cap, bool has_dst, const char* who, Dict d = Dict{nullptr, 0u}) {
    const uint32_t bits = T::kBits ? c.bits[i] : 0u, flags = c.flags ? c.flags[i] : 0u;
    if (!known_counted<T>(bits, c.widths[i], flags, cap, has_dst, who, i, d)) return false;
    segs.push_back(T::make(static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), len, cap, c.widths[i], bits, flags, items, d));
    where.push_back(i);
    items += T::items(cap);
    return true;
  }
};

// the table on `stream`, waited for, and its results: entry j's to results[where[j]] of the n_results, the others zeros
template <class T>
int counted_device(BrotliAmdBatch* b, const CountedTable<T>& t, typename T::Result* results, size_t n_results, hipStream_t stream) {
  std::fill(results, results + n_results, empty_result<T>());
  const uint8_t* d_scratch = nullptr;
  if (filter_device(b, T::kId, t.segs, stream, &d_scratch) != 0) return -1;
  if (!d_scratch) return 0;   // (no segments, or segments without bytes: their results are zeros)
  // (a call of a filter with items that has none is the walk alone: what lies between the events behind it is no launch's time)
  BrotliAmdBatch::FilterCall& call = b->filter[T::kId];
  if (T::kItems && t.items == 0u) {
    std::fill(call.phase_ms + 1, std::end(call.phase_ms), 0.0f);
    call.ms = call.phase_ms[0];
  }
  std::vector<typename T::Result> got(t.segs.size());
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice") ||
      !hip_ok(hipMemcpy(got.data(), d_scratch, sizeof(typename T::Result) * got.size(), hipMemcpyDeviceToHost),
              (std::string("hipMemcpy(") + kFilter[T::kId].name + " results)").c_str()))
    return -1;
  for (size_t j = 0; j < got.size(); j++) results[t.where[j]] = got[j];
  return 0;
}

template <class T>
int counted_segments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst, const Columns& c,
                     typename T::Result* results, void* hip_stream) {
  if (!b || (n && (!d_src || !src_lens || !c.caps || (T::kBits && !c.bits) || !c.widths || !results))) return invalid_arguments(T::kId);
  no_times(b, T::kId);
  CountedTable<T> t;
  t.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    void* dst = d_dst ? d_dst[i] : nullptr;   // (no array of destinations: a call that counts, where every capacity is 0)
    if (T::kDict && c.caps[i] != 0u && (!c.dicts || !c.dict_entries)) return invalid_arguments(T::kId);   // (no arrays of dictionaries: the same)
    if (!t.push(c, i, d_src[i], dst, src_lens[i], c.caps[i], dst != nullptr, "segment", T::kDict ? c.dict(i) : Dict{nullptr, 0u})) return -1;
  }
  return counted_device(b, t, results, n, static_cast<hipStream_t>(hip_stream));
}

// the dictionary of stream i of the outputs: what stream dict_streams[i] of the same call delivered, as entries of stream i's width, or -- for
// BROTLI_AMD_UNDICT_NO_STREAM and without dict_streams -- the columns' own.  False: g_last_error says why.
__attribute__((noinline)) bool refuse_dict_stream(size_t i, uint32_t j, size_t n) {
  g_last_error = "undict stream " + std::to_string(i) + ": its dictionary stream " + std::to_string(j) +
                 (j == i ? " is the stream itself" : " is none of the " + std::to_string(n) + " streams of the last decode call");
  return false;
}
inline bool dict_of_outputs(const std::vector<DeliveredBytes>& outs, const Columns& c, const uint32_t* dict_streams, size_t i, Dict* d) {
  const uint32_t j = dict_streams ? dict_streams[i] : BROTLI_AMD_UNDICT_NO_STREAM;
  if (j == BROTLI_AMD_UNDICT_NO_STREAM) { *d = c.dict(i); return true; }
  if (j == i || j >= outs.size()) return refuse_dict_stream(i, j, outs.size());
  const uint32_t w = c.widths[i];
  *d = Dict{outs[j].ptr, brotli_amd_unshuffle_width_ok(w) ? outs[j].len / w : 0u};   // (a width that is none is refused by the shape check)
  return true;
}

template <class T>
int counted_outputs(BrotliAmdBatch* b, void* const* d_dst, const Columns& c, typename T::Result* results, const uint32_t* dict_streams = nullptr) {
  if (!b || (T::kBits && !c.bits) || !c.widths || !results) return invalid_arguments(T::kId);
  no_times(b, T::kId);
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  const bool count_only = !d_dst || !c.caps;   // every stream is counted and nothing is written
  CountedTable<T> t;
  t.reserve(outs.size());
  for (size_t i = 0; i < outs.size(); i++) {
    if (!count_only && d_dst[i] == nullptr) continue;   // skipped: none of its parameters are looked at
    Dict d = {nullptr, 0u};
    if (T::kDict && !count_only && !dict_of_outputs(outs, c, dict_streams, i, &d)) return -1;
    if (!t.push(c, i, outs[i].ptr, count_only ? nullptr : d_dst[i], outs[i].len, count_only ? 0u : c.caps[i], !count_only, "stream", d)) return -1;
  }
  return counted_device(b, t, results, outs.size(), b->last_stream);
}

// ---- unnull: a path of its own beside the counted one ----
// It has two sources a segment -- levels and values --, two destinations -- slots and a bitmap -- and a level, so its columns are its own; what
// it shares with the counted filters is the table (entries, where, items) and counted_device.  The four counted filters pay nothing for it.
struct Unnull {
  typedef BrotliAmdUnnullSeg Seg;
  typedef BrotliAmdUnnullResult Result;
  static constexpr Filter kId = kUnnull;
  static constexpr bool kItems = true;
};
__attribute__((noinline)) bool refuse_unnull(const char* what, const BrotliAmdUnnullSeg& s, const char* who, size_t i) {
  g_last_error = std::string("unnull ") + who + " " + std::to_string(i) + ": " + what + " (bits " + std::to_string(s.bits) + ", level " + std::to_string(s.level) + ", width " +
                 std::to_string(s.width) + ", flags " + std::to_string(s.flags) + ", capacity " + std::to_string(s.cap) + ", values " + std::to_string(s.values_count) + ")";
  return false;
}
// the shape check of one entry, in the order of batch.h's list (has_dst: the call has a destination for it)
inline bool known_unnull(const BrotliAmdUnnullSeg& s, bool has_dst, const char* who, size_t i) {
  const char* what = nullptr;
  const bool follow = (s.flags & BROTLI_AMD_UNNULL_VALUES_FOLLOW) != 0u;
  if (!brotli_amd_unshuffle_width_ok(s.width)) what = "width is not 1, 2, 4 or 8";
  else if ((s.flags & ~BROTLI_AMD_UNNULL_FLAGS) != 0u) what = "unknown flag bits";
  else if (follow && (s.flags & BROTLI_AMD_UNNULL_LENGTH_PREFIX) == 0u) what = "values that follow the levels without a length prefix";
  else if (s.bits > BROTLI_AMD_UNRLE_MAX_BITS) what = "field of more than 32 bits";
  else if (s.cap > BROTLI_AMD_UNNULL_MAX_CAP) what = "a capacity above 2^56 elements";
  else if (s.values_count > BROTLI_AMD_UNNULL_MAX_VALUES) what = "more than 2^56 values";
  else if (s.cap != 0u && !has_dst) what = "no destination for a capacity that is not 0";
  else if (!follow && s.cap != 0u && s.values_count != 0u && !s.values) what = "no values for a count and a capacity that are not 0";
  return !what || refuse_unnull(what, s, who, i);
}
// entry i of a call into its table: checked, then given its place among the items
inline bool push_unnull(CountedTable<Unnull>* t, BrotliAmdUnnullSeg s, size_t i, bool has_dst, const char* who) {
  if (!known_unnull(s, has_dst, who, i)) return false;
  s.first_item = t->items;
  t->segs.push_back(s);
  t->where.push_back(i);
  t->items += brotli_amd_unrle_items(s.cap, brotli_amd_unrle_item_elems());
  return true;
}

// ---- undict for byte arrays: a path of its own beside the counted one ----
// A segment has two destinations, a data capacity and an offset base, and its dictionary is bytes and a bound, not entries of a width: its
// columns are its own.  Behind the segments the call's table has a record for every DISTINCT dictionary -- (pointer, length, bound) --, which the
// device walks once however many segments name it.
struct BytesDict { const void* ptr; uint64_t len, bound; };
typedef BrotliAmdUndictBytesResult BytesResult;
BytesResult empty_bytes_result() { return brotli_amd_undict_bytes_result(BrotliAmdUnrleResult{0u, 0u, 0u, 0u, 0u}, BrotliAmdUndictBytesDictResult{0u, 0u, 0u, 0u}); }

__attribute__((noinline)) bool refuse_bytes(const char* what, const BrotliAmdUndictBytesSeg& s, BytesDict d, const char* who, size_t i) {
  g_last_error = std::string("undict-bytes ") + who + " " + std::to_string(i) + ": " + what + " (bits " + std::to_string(s.bits) + ", flags " + std::to_string(s.flags) +
                 ", capacity " + std::to_string(s.cap) + ", data capacity " + std::to_string(s.data_cap) + ", dictionary bytes " + std::to_string(d.len) + ")";
  return false;
}
// the shape check of one entry, in the order of batch.h's list
inline bool known_bytes(const BrotliAmdUndictBytesSeg& s, BytesDict d, const char* who, size_t i) {
  const char* what = nullptr;
  if ((s.flags & ~BROTLI_AMD_UNDICT_BYTES_FLAGS) != 0u) what = "unknown flag bits";
  else if ((s.flags & BROTLI_AMD_UNDICT_BYTES_WIDTH_BYTE) == 0u && s.bits > BROTLI_AMD_UNRLE_MAX_BITS) what = "field of more than 32 bits";
  else if (s.cap > BROTLI_AMD_UNDICT_BYTES_MAX_CAP) what = "a capacity above 2^56 elements";
  else if (s.data_cap != 0u && !s.data) what = "no data destination for a data capacity that is not 0";
  else if (s.cap != 0u && d.len != 0u && !d.ptr) what = "no dictionary for bytes and a capacity that are not 0";
  else if (d.len >= BROTLI_AMD_UNDICT_BYTES_MAX_DICT) what = "a dictionary of 2^32 bytes or more";
  return !what || refuse_bytes(what, s, d, who, i);
}

// the call's distinct dictionaries, and where each one's entry positions begin
struct BytesDicts {
  std::vector<BrotliAmdUndictBytesDict> recs;
  uint64_t starts = 0;   // of all records together
  uint32_t index(BytesDict d) {
    if (!recs.empty() && recs.back().dict == d.ptr && recs.back().len == d.len && recs.back().bound == d.bound) return (uint32_t)recs.size() - 1u;   // (the pages of a chunk)
    const auto at = known_.emplace(std::make_tuple(d.ptr, d.len, d.bound), (uint32_t)recs.size());
    if (at.second) {
      recs.push_back(BrotliAmdUndictBytesDict{static_cast<const uint8_t*>(d.ptr), d.len, d.bound, starts});
      starts += brotli_amd_undict_bytes_starts(d.len, d.bound);
    }
    return at.first->second;
  }
 private:
  std::map<std::tuple<const void*, uint64_t, uint64_t>, uint32_t> known_;
};

struct BytesTable {
  std::vector<BrotliAmdUndictBytesSeg> segs;
  std::vector<size_t> where;
  uint64_t items = 0;
  BytesDicts dicts;
  // entry i of a call: checked, then given its place among the items and its dictionary's record (a segment that only counts has none)
  bool push(BrotliAmdUndictBytesSeg s, BytesDict d, size_t i, const char* who) {
    if (!known_bytes(s, d, who, i)) return false;
    s.first_item = items;
    s.dict = s.cap != 0u ? dicts.index(d) : BROTLI_AMD_UNDICT_BYTES_NO_DICT;
    segs.push_back(s);
    where.push_back(i);
    items += brotli_amd_unrle_items(s.cap, brotli_amd_unrle_item_elems());
    return true;
  }
};

// the table on `stream`, waited for, and its results: entry j's to results[where[j]] of the n_results, the others zeros
int undict_bytes_device(BrotliAmdBatch* b, const BytesTable& t, BytesResult* results, size_t n_results, hipStream_t stream) {
  std::fill(results, results + n_results, empty_bytes_result());
  if (t.segs.empty()) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const FilterDesc& d = kFilter[kUndictBytes];
  BrotliAmdBatch::FilterCall& call = b->filter[kUndictBytes];
  const uint32_t n = (uint32_t)t.segs.size(), nd = (uint32_t)t.dicts.recs.size();
  const uint64_t units = n + t.items;
  // the segments, and behind them -- at a multiple of 16 -- the dictionaries' records
  const size_t seg_bytes = (sizeof(BrotliAmdUndictBytesSeg) * n + 15u) & ~(size_t)15;
  std::vector<uint8_t> table(seg_bytes + sizeof(BrotliAmdUndictBytesDict) * nd, 0);
  std::memcpy(table.data(), t.segs.data(), sizeof(BrotliAmdUndictBytesSeg) * n);
  if (nd) std::memcpy(table.data() + seg_bytes, t.dicts.recs.data(), sizeof(BrotliAmdUndictBytesDict) * nd);
  const uint8_t* d_results = nullptr;
  if (run_seg_call(&call.call, d.what, table.data(), table.size(), brotli_amd_undict_bytes_scratch_bytes(units, n, nd, t.dicts.starts), d.events, stream,
                   [&](uint8_t* d_table, uint8_t* d_scratch, const hipEvent_t* ev) {
    d_results = d_scratch;
    return hip_ok(brotli_amd_launch_undict_bytes(d_table, n, units, d_table + seg_bytes, nd, d_scratch, stream, ev), d.launch_what);
  }, &call.ms, call.phase_ms) != 0) return -1;
  if (t.items == 0u) {   // (the RLE walk alone: what lies between the other events is no launch's time)
    const float walk = call.phase_ms[1];
    std::fill(std::begin(call.phase_ms), std::end(call.phase_ms), 0.0f);
    call.ms = call.phase_ms[1] = walk;
  }
  std::vector<BytesResult> got(n);
  if (!hip_ok(hipMemcpy(got.data(), d_results, sizeof(BytesResult) * n, hipMemcpyDeviceToHost), "hipMemcpy(undict-bytes results)")) return -1;
  for (size_t j = 0; j < got.size(); j++) results[t.where[j]] = got[j];
  return 0;
}

// ---- undlba: a path of its own beside the counted one ----
// A segment has undict-bytes' two destinations, data capacity and offset base, and no dictionary and no field width.  What the host knows of
// the bytes that the call's copies move is a bound: min(len, data_cap) a segment that has a data destination.
typedef BrotliAmdUndlbaResult DlbaResult;
DlbaResult empty_dlba_result() { return brotli_amd_undlba_result(BrotliAmdUndbpResult{0u, 0u, 0u, 0u, 0u, 0u, 0u}, 0u); }

__attribute__((noinline)) bool refuse_dlba(const char* what, const BrotliAmdUndlbaSeg& s, const char* who, size_t i) {
  g_last_error = std::string("undlba ") + who + " " + std::to_string(i) + ": " + what + " (flags " + std::to_string(s.flags) + ", capacity " + std::to_string(s.cap) +
                 ", data capacity " + std::to_string(s.data_cap) + ")";
  return false;
}
// the shape check of one entry, in the order of batch.h's list (the outputs call has taken its skipped streams out in front of it)
inline bool known_dlba(const BrotliAmdUndlbaSeg& s, const char* who, size_t i) {
  const char* what = nullptr;
  if ((s.flags & BROTLI_AMD_UNDLBA_SKIP) != 0u) what = "BROTLI_AMD_UNDLBA_SKIP is for the outputs of a decode call";
  else if ((s.flags & ~BROTLI_AMD_UNDLBA_FLAGS) != 0u) what = "unknown flag bits";
  else if (s.cap > BROTLI_AMD_UNDLBA_MAX_CAP) what = "a capacity above 2^56 elements";
  else if (s.data_cap != 0u && !s.data) what = "no data destination for a data capacity that is not 0";
  return !what || refuse_dlba(what, s, who, i);
}

struct DlbaTable {
  std::vector<BrotliAmdUndlbaSeg> segs;
  std::vector<size_t> where;
  uint64_t items = 0, max_bytes = 0;
  void reserve(size_t n) { segs.reserve(n); where.reserve(n); }
  // entry i of a call: checked, then given its place among the items
  bool push(BrotliAmdUndlbaSeg s, size_t i, const char* who) {
    if (!known_dlba(s, who, i)) return false;
    s.first_item = items;
    segs.push_back(s);
    where.push_back(i);
    items += brotli_amd_undbp_items(s.cap, brotli_amd_undbp_item_deltas());
    if (s.cap != 0u && s.data) max_bytes += std::min(s.len, s.data_cap);
    return true;
  }
};

// the table on `stream`, waited for, and its results: entry j's to results[where[j]] of the n_results, the others zeros
int undlba_device(BrotliAmdBatch* b, const DlbaTable& t, DlbaResult* results, size_t n_results, hipStream_t stream) {
  std::fill(results, results + n_results, empty_dlba_result());
  if (t.segs.empty()) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const FilterDesc& d = kFilter[kUndlba];
  BrotliAmdBatch::FilterCall& call = b->filter[kUndlba];
  const uint32_t n = (uint32_t)t.segs.size();
  const uint64_t units = n + t.items;
  const uint8_t* d_results = nullptr;
  if (run_seg_call(&call.call, d.what, t.segs.data(), sizeof(BrotliAmdUndlbaSeg) * n, brotli_amd_undlba_scratch_bytes(units, n), d.events, stream,
                   [&](uint8_t* d_table, uint8_t* d_scratch, const hipEvent_t* ev) {
    d_results = d_scratch;
    return hip_ok(brotli_amd_launch_undlba(d_table, n, units, t.max_bytes, d_scratch, stream, ev), d.launch_what);
  }, &call.ms, call.phase_ms) != 0) return -1;
  if (t.items == 0u) {   // (the walk alone: what lies between the other events is no launch's time)
    std::fill(call.phase_ms + 1, std::end(call.phase_ms), 0.0f);
    call.ms = call.phase_ms[0];
  }
  std::vector<DlbaResult> got(n);
  if (!hip_ok(hipMemcpy(got.data(), d_results, sizeof(DlbaResult) * n, hipMemcpyDeviceToHost), "hipMemcpy(undlba results)")) return -1;
  for (size_t j = 0; j < got.size(); j++) results[t.where[j]] = got[j];
  return 0;
}

// ---- undba: undlba's segments and checks under its own name, a result and a launcher of its own ----
typedef BrotliAmdUndbaResult DbaResult;
DbaResult empty_dba_result() { const BrotliAmdUndbpResult none = {0u, 0u, 0u, 0u, 0u, 0u, 0u}; return brotli_amd_undba_result(none, none, 0u); }

__attribute__((noinline)) bool refuse_dba(const char* what, const BrotliAmdUndbaSeg& s, const char* who, size_t i) {
  g_last_error = std::string("undba ") + who + " " + std::to_string(i) + ": " + what + " (flags " + std::to_string(s.flags) + ", capacity " + std::to_string(s.cap) +
                 ", data capacity " + std::to_string(s.data_cap) + ")";
  return false;
}
// the shape check of one entry, in the order of batch.h's list (the outputs call has taken its skipped streams out in front of it)
inline bool known_dba(const BrotliAmdUndbaSeg& s, const char* who, size_t i) {
  const char* what = nullptr;
  if ((s.flags & BROTLI_AMD_UNDBA_SKIP) != 0u) what = "BROTLI_AMD_UNDBA_SKIP is for the outputs of a decode call";
  else if ((s.flags & ~BROTLI_AMD_UNDBA_FLAGS) != 0u) what = "unknown flag bits";
  else if (s.cap > BROTLI_AMD_UNDBA_MAX_CAP) what = "a capacity above 2^56 elements";
  else if (s.data_cap != 0u && !s.data) what = "no data destination for a data capacity that is not 0";
  return !what || refuse_dba(what, s, who, i);
}

struct DbaTable {
  std::vector<BrotliAmdUndbaSeg> segs;
  std::vector<size_t> where;
  uint64_t items = 0;
  void reserve(size_t n) { segs.reserve(n); where.reserve(n); }
  // entry i of a call: checked, then given its place among the items
  bool push(BrotliAmdUndbaSeg s, size_t i, const char* who) {
    if (!known_dba(s, who, i)) return false;
    s.first_item = items;
    segs.push_back(s);
    where.push_back(i);
    items += brotli_amd_undbp_items(s.cap, brotli_amd_undbp_item_deltas());
    return true;
  }
};

// the table on `stream`, waited for, and its results: entry j's to results[where[j]] of the n_results, the others zeros
int undba_device(BrotliAmdBatch* b, const DbaTable& t, DbaResult* results, size_t n_results, hipStream_t stream) {
  std::fill(results, results + n_results, empty_dba_result());
  if (t.segs.empty()) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const FilterDesc& d = kFilter[kUndba];
  BrotliAmdBatch::FilterCall& call = b->filter[kUndba];
  const uint32_t n = (uint32_t)t.segs.size();
  const uint64_t units = n + t.items;
  const uint8_t* d_results = nullptr;
  if (run_seg_call(&call.call, d.what, t.segs.data(), sizeof(BrotliAmdUndbaSeg) * n, brotli_amd_undba_scratch_bytes(units, n), d.events, stream,
                   [&](uint8_t* d_table, uint8_t* d_scratch, const hipEvent_t* ev) {
    d_results = d_scratch;
    return hip_ok(brotli_amd_launch_undba(d_table, n, units, d_scratch, stream, ev), d.launch_what);
  }, &call.ms, call.phase_ms) != 0) return -1;
  if (t.items == 0u) {   // (the walks alone: what lies between the other events is no launch's time)
    std::fill(call.phase_ms + 1, std::end(call.phase_ms), 0.0f);
    call.ms = call.phase_ms[0];
  }
  std::vector<DbaResult> got(n);
  if (!hip_ok(hipMemcpy(got.data(), d_results, sizeof(DbaResult) * n, hipMemcpyDeviceToHost), "hipMemcpy(undba results)")) return -1;
  for (size_t j = 0; j < got.size(); j++) results[t.where[j]] = got[j];
  return 0;
}

// ---- what the hooks share ----
// The hooks run the device's functions on the host over every unit of a segment, source and destination each in a SkewedRoom (brotli_host.h).
// a hook's buffers and skews
inline bool rooms_ok(const uint8_t* src, size_t src_size, const uint8_t* dst, size_t dst_size, uint32_t src_skew, uint32_t dst_skew) {
  return !(src_size && !src) && !(dst_size && !dst) && src_skew <= 15u && dst_skew <= 15u;
}
// len bytes at off lie in a buffer of size bytes
inline bool lies_in(uint64_t off, uint64_t len, uint64_t size) { return len <= size && off <= size - len; }
int outside_buffer(Filter f) { g_last_error = std::string("invalid ") + kFilter[f].name + " arguments: a segment outside its buffer"; return -1; }

// The order in which a hook takes its tiles or items: shuffled by the seed (0: left as it is), and shuffled on from there by every later call.  No
// result may depend on it.
struct SeededOrder {
  explicit SeededOrder(uint32_t seed) : seed_(seed), rnd_(seed * 2654435761u + 1u) {}
  template <class Item>
  void shuffle(std::vector<Item>* order) {
    if (seed_ == 0u) return;
    for (uint64_t i = order->size(); i > 1u; i--) { rnd_ = rnd_ * 1664525u + 1013904223u; std::swap((*order)[i - 1u], (*order)[(rnd_ >> 8) % i]); }
  }
 private:
  uint32_t seed_, rnd_;
};
std::vector<uint64_t> first_numbers(uint64_t n) {
  std::vector<uint64_t> order(n);
  std::iota(order.begin(), order.end(), (uint64_t)0);
  return order;
}

// the carry launch, serially: every tile record's carry_in
std::vector<uint64_t> carries_of(const std::vector<BrotliAmdUndeltaTile>& tiles) {
  std::vector<uint64_t> carries(tiles.size());
  BrotliAmdUndeltaPair out = {0u, 0u};
  for (size_t t = 0; t < tiles.size(); t++) {
    carries[t] = brotli_amd_undelta_carry_in(out.sum, tiles[t]);
    out = brotli_amd_undelta_combine(out, brotli_amd_undelta_tile_pair(tiles[t]));
  }
  return carries;
}

// what a hook of one segment ends with: no byte beside the len bytes of the destination may have changed; they go to dst
int hook_result(Filter f, const SkewedRoom& droom, uint8_t* dst, size_t len) {
  if (!droom.changed_inside_only([len](size_t i) { return i < len; })) { g_last_error = std::string(kFilter[f].name) + " wrote outside its destination"; return -2; }
  droom.get(dst, 0u, len);
  return 0;
}
// ... and a counted hook: no byte outside every segment's elements -- min(count, cap) of them -- may have changed; the whole room goes to dst
template <class Result>
int counted_hook_result(Filter f, const SkewedRoom& droom, uint32_t n, uint8_t* dst, size_t dst_size, const uint64_t* dst_offs, const uint64_t* caps,
                        const uint8_t* widths, const std::vector<Result>& got, Result* results) {
  std::vector<uint8_t> inside(dst_size, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t bytes = std::min(got[i].count, caps[i]) * widths[i];
    std::fill(inside.begin() + dst_offs[i], inside.begin() + dst_offs[i] + bytes, 1);
  }
  if (!droom.changed_inside_only([&](size_t i) { return i < dst_size && inside[i]; })) { g_last_error = std::string(kFilter[f].name) + " wrote outside its destination"; return -2; }
  droom.get(dst, 0u, dst_size);
  std::copy(got.begin(), got.end(), results);
  return 0;
}

// The destination's side of the arguments of a hook whose segments are walked and then taken item by item.
struct ItemHookDst { uint8_t* dst; size_t dst_size; const uint64_t* dst_offs; const uint64_t* caps; const uint8_t* widths; };

// What such a hook's walks leave -- the items' prefix array, and every item's checkpoint --, and the order its items are taken in.
template <class Checkpoint>
struct HookItems {
  std::vector<uint64_t> pre;
  std::vector<Checkpoint> ckpts;
  // Every segment's walk: walk(i, ckpts) -> got[i].  It writes nothing, and says how much room the segment needs; fits(i, m): the segment's other
  // rooms hold its m elements.  A segment's capacity becomes the elements there is room for and one more: the walk marks the items of no
  // others, and a capacity of 2^56 needs no table of its own.  items_of(cap): the items of a capacity.
  template <class Seg, class Result, class Items, class Walk, class Fits>
  int walks(Filter f, std::vector<Seg>& segs, std::vector<Result>& got, const ItemHookDst& d, Items items_of, Walk walk, Fits fits) {
    static_assert(BROTLI_AMD_UNDBP_NONE == BROTLI_AMD_UNRLE_NONE, "one checkpoint of an item beyond count");
    pre.assign(segs.size() + 1u, 0u);
    for (uint32_t i = 0; i < segs.size(); i++) {
      const uint64_t room = (d.dst_size - d.dst_offs[i]) / d.widths[i];
      segs[i].cap = std::min<uint64_t>(d.caps[i], room + 1u);
      segs[i].first_item = pre[i];
      pre[i + 1u] = pre[i] + items_of(segs[i].cap);
      ckpts.resize(pre[i + 1u], Checkpoint{BROTLI_AMD_UNRLE_NONE, BROTLI_AMD_UNRLE_NONE});
      got[i] = walk(i, ckpts.data() + pre[i]);
      const uint64_t m = std::min(got[i].count, d.caps[i]);
      if (m > room || !fits(i, m)) return outside_buffer(f);
    }
    return 0;
  }
  // each(i, checkpoint, j, g) for item j of segment i, the g-th of all, in the order that `seeded` shuffles next
  template <class Each>
  void shuffled(SeededOrder* seeded, Each each) const {
    std::vector<uint64_t> order = first_numbers(pre.back());
    seeded->shuffle(&order);
    for (uint64_t g : order) {
      const uint32_t i = brotli_amd_seg_find(pre.data(), (uint32_t)pre.size() - 1u, g);
      each(i, ckpts[g], g - pre[i], g);
    }
  }
};

// A hook of two phases (unrle, undict) over segs, whose capacities are the caller's: the walks, then the items of all segments in an order
// shuffled by the seed: item(i, &result, checkpoint, j).
template <class Seg, class Result, class Walk, class Item>
int walk_items_hook(Filter f, std::vector<Seg>& segs, SkewedRoom& droom, const ItemHookDst& d, uint32_t item_elems, uint32_t order_seed, Walk walk, Item item,
                    Result* results) {
  std::vector<Result> got(segs.size());
  HookItems<BrotliAmdUnrleCheckpoint> items;
  const int walked = items.walks(f, segs, got, d, [&](uint64_t cap) { return brotli_amd_unrle_items(cap, item_elems); }, walk, [](uint32_t, uint64_t) { return true; });
  if (walked != 0) return walked;
  droom.snapshot();
  SeededOrder seeded(order_seed);
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUnrleCheckpoint cp, uint64_t j, uint64_t) { item(i, &got[i], cp, j); });
  return counted_hook_result(f, droom, (uint32_t)segs.size(), d.dst, d.dst_size, d.dst_offs, d.caps, d.widths, got, results);
}

// The phases of a hook of four (undbp, unnull) up to its stores: the walks, the items' records in an order shuffled by the seed --
// count(i, checkpoint, j) --, the carries as undelta's hook takes them, and the items' stores in another shuffled order:
// store(i, checkpoint, j, carry_in).  The caller ends with counted_hook_result.
template <class Checkpoint, class Seg, class Result, class Items, class Walk, class Fits, class Count, class Store>
int walk_count_store_hook(Filter f, std::vector<Seg>& segs, std::vector<Result>& got, SkewedRoom& droom, const ItemHookDst& d, uint32_t order_seed, Items items_of,
                          Walk walk, Fits fits, Count count, Store store) {
  HookItems<Checkpoint> items;
  const int walked = items.walks(f, segs, got, d, items_of, walk, fits);
  if (walked != 0) return walked;
  droom.snapshot();
  SeededOrder seeded(order_seed);
  std::vector<BrotliAmdUndeltaTile> tiles(items.pre.back());
  items.shuffled(&seeded, [&](uint32_t i, Checkpoint cp, uint64_t j, uint64_t g) { tiles[g] = count(i, cp, j); });
  const std::vector<uint64_t> carries = carries_of(tiles);
  items.shuffled(&seeded, [&](uint32_t i, Checkpoint cp, uint64_t j, uint64_t g) { store(i, cp, j, carries[g]); });
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
  return counted_segments<Unvarint>(b, n, d_src, src_lens, d_dst, Columns{caps, nullptr, widths, flags}, results, hip_stream);
}
extern "C" int BrotliAmdBatchUnvarintOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint64_t* caps, const uint8_t* widths, const uint8_t* flags,
                                             BrotliAmdUnvarintResult* results) {
  return counted_outputs<Unvarint>(b, d_dst, Columns{caps, nullptr, widths, flags}, results);
}
extern "C" int BrotliAmdBatchUnrleSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                           const uint64_t* caps, const uint8_t* bits, const uint8_t* widths, const uint8_t* flags, BrotliAmdUnrleResult* results,
                                           void* hip_stream) {
  return counted_segments<Unrle>(b, n, d_src, src_lens, d_dst, Columns{caps, bits, widths, flags}, results, hip_stream);
}
extern "C" int BrotliAmdBatchUnrleOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint64_t* caps, const uint8_t* bits, const uint8_t* widths,
                                          const uint8_t* flags, BrotliAmdUnrleResult* results) {
  return counted_outputs<Unrle>(b, d_dst, Columns{caps, bits, widths, flags}, results);
}
extern "C" int BrotliAmdBatchUndbpSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                           const uint64_t* caps, const uint8_t* widths, const uint8_t* flags, BrotliAmdUndbpResult* results, void* hip_stream) {
  return counted_segments<Undbp>(b, n, d_src, src_lens, d_dst, Columns{caps, nullptr, widths, flags}, results, hip_stream);
}
extern "C" int BrotliAmdBatchUndbpOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint64_t* caps, const uint8_t* widths, const uint8_t* flags,
                                          BrotliAmdUndbpResult* results) {
  return counted_outputs<Undbp>(b, d_dst, Columns{caps, nullptr, widths, flags}, results);
}

extern "C" int BrotliAmdBatchUndictSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                            const uint64_t* caps, const uint8_t* bits, const uint8_t* widths, const uint8_t* flags, const void* const* d_dicts,
                                            const uint64_t* dict_entries, BrotliAmdUndictResult* results, void* hip_stream) {
  return counted_segments<Undict>(b, n, d_src, src_lens, d_dst, Columns{caps, bits, widths, flags, d_dicts, dict_entries}, results, hip_stream);
}
extern "C" int BrotliAmdBatchUndictOutputs(BrotliAmdBatch* b, void* const* d_dst, const uint64_t* caps, const uint8_t* bits, const uint8_t* widths,
                                           const uint8_t* flags, const uint32_t* dict_streams, const void* const* d_dicts, const uint64_t* dict_entries,
                                           BrotliAmdUndictResult* results) {
  return counted_outputs<Undict>(b, d_dst, Columns{caps, bits, widths, flags, d_dicts, dict_entries}, results, dict_streams);
}

extern "C" int BrotliAmdBatchUnnullSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_levels, const size_t* level_lens, const void* const* d_values,
                                            const uint64_t* value_counts, void* const* d_dst, void* const* d_valid, const uint64_t* caps, const uint8_t* bits,
                                            const uint32_t* levels, const uint8_t* widths, const uint8_t* flags, BrotliAmdUnnullResult* results, void* hip_stream) {
  if (!b || (n && (!d_levels || !level_lens || !caps || !bits || !levels || !widths || !results))) return invalid_arguments(kUnnull);
  no_times(b, kUnnull);
  CountedTable<Unnull> t;
  t.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    void* dst = d_dst ? d_dst[i] : nullptr;   // (no array of destinations: a call that counts, where every capacity is 0)
    const uint32_t f = flags ? flags[i] : 0u;
    // (no arrays of values: the same, but for segments whose values follow their levels)
    if (caps[i] != 0u && (f & BROTLI_AMD_UNNULL_VALUES_FOLLOW) == 0u && (!d_values || !value_counts)) return invalid_arguments(kUnnull);
    const BrotliAmdUnnullSeg s = {static_cast<const uint8_t*>(d_levels[i]), static_cast<uint8_t*>(dst), level_lens[i], caps[i], 0u, widths[i], bits[i], f, levels[i],
                                  static_cast<const uint8_t*>(d_values ? d_values[i] : nullptr), value_counts ? value_counts[i] : 0u,
                                  static_cast<uint8_t*>(d_valid ? d_valid[i] : nullptr)};
    if (!push_unnull(&t, s, i, dst != nullptr, "segment")) return -1;
  }
  return counted_device(b, t, results, n, static_cast<hipStream_t>(hip_stream));
}
extern "C" int BrotliAmdBatchUnnullOutputs(BrotliAmdBatch* b, void* const* d_dst, void* const* d_valid, const uint64_t* caps, const uint8_t* bits, const uint32_t* levels,
                                           const uint8_t* widths, const void* const* d_levels, const size_t* level_lens, BrotliAmdUnnullResult* results) {
  if (!b || !bits || !levels || !widths || !results || (d_levels && !level_lens)) return invalid_arguments(kUnnull);
  no_times(b, kUnnull);
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  const bool count_only = !d_dst || !caps;   // every stream is counted and nothing is written
  CountedTable<Unnull> t;
  t.reserve(outs.size());
  for (size_t i = 0; i < outs.size(); i++) {
    if (!count_only && d_dst[i] == nullptr) continue;   // skipped: none of its parameters are looked at
    uint8_t* dst = count_only ? nullptr : static_cast<uint8_t*>(d_dst[i]);
    uint8_t* valid = count_only || !d_valid ? nullptr : static_cast<uint8_t*>(d_valid[i]);
    const uint64_t cap = count_only ? 0u : caps[i];
    const uint32_t w = widths[i];
    BrotliAmdUnnullSeg s;
    if (d_levels && d_levels[i]) {   // v2: the caller's levels, and the stream's bytes as the values (a width that is none is refused by the shape check)
      s = BrotliAmdUnnullSeg{static_cast<const uint8_t*>(d_levels[i]), dst, level_lens[i], cap, 0u, w, bits[i], 0u, levels[i], outs[i].ptr,
                             brotli_amd_unshuffle_width_ok(w) ? outs[i].len / w : 0u, valid};
    } else {   // a v1 body: prefix, levels, values
      s = BrotliAmdUnnullSeg{outs[i].ptr, dst, outs[i].len, cap, 0u, w, bits[i], BROTLI_AMD_UNNULL_FLAGS, levels[i], nullptr, 0u, valid};
    }
    if (!push_unnull(&t, s, i, !count_only, "stream")) return -1;
  }
  return counted_device(b, t, results, outs.size(), b->last_stream);
}

extern "C" int BrotliAmdBatchUndictBytesSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_offsets, void* const* d_data,
                                                 const uint64_t* data_caps, const uint64_t* caps, const uint8_t* bits, const uint8_t* flags, const uint64_t* offset_bases,
                                                 const void* const* d_dicts, const uint64_t* dict_lens, const uint64_t* dict_entries, BrotliAmdUndictBytesResult* results,
                                                 void* hip_stream) {
  if (!b || (n && (!d_src || !src_lens || !caps || !bits || !results))) return invalid_arguments(kUndictBytes);
  no_times(b, kUndictBytes);
  BytesTable t;
  t.segs.reserve(n); t.where.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    if (caps[i] != 0u && (!d_dicts || !dict_lens)) return invalid_arguments(kUndictBytes);   // (no arrays of dictionaries: a call that counts, where every capacity is 0)
    const BytesDict d = {d_dicts ? d_dicts[i] : nullptr, dict_lens ? dict_lens[i] : 0u, dict_entries ? dict_entries[i] : BROTLI_AMD_UNDICT_BYTES_ALL};
    const BrotliAmdUndictBytesSeg s = {static_cast<const uint8_t*>(d_src[i]), static_cast<uint8_t*>(d_data ? d_data[i] : nullptr), src_lens[i], caps[i], 0u, 0u, bits[i],
                                       flags ? flags[i] : 0u, 0u, static_cast<uint8_t*>(d_offsets ? d_offsets[i] : nullptr), data_caps ? data_caps[i] : 0u,
                                       offset_bases ? offset_bases[i] : 0u};
    if (!t.push(s, d, i, "segment")) return -1;
  }
  return undict_bytes_device(b, t, results, n, static_cast<hipStream_t>(hip_stream));
}
__attribute__((noinline)) static bool refuse_bytes_dict_stream(size_t i, uint32_t j, size_t n) {
  g_last_error = "undict-bytes stream " + std::to_string(i) + ": its dictionary stream " + std::to_string(j) +
                 (j == i ? " is the stream itself" : " is none of the " + std::to_string(n) + " streams of the last decode call");
  return false;
}
extern "C" int BrotliAmdBatchUndictBytesOutputs(BrotliAmdBatch* b, void* const* d_offsets, void* const* d_data, const uint64_t* data_caps, const uint64_t* caps,
                                                const uint8_t* bits, const uint8_t* flags, const uint64_t* offset_bases, const uint32_t* dict_streams,
                                                const void* const* d_dicts, const uint64_t* dict_lens, const uint64_t* dict_entries, BrotliAmdUndictBytesResult* results) {
  if (!b || !bits || !results) return invalid_arguments(kUndictBytes);
  no_times(b, kUndictBytes);
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  BytesTable t;
  t.segs.reserve(outs.size()); t.where.reserve(outs.size());
  for (size_t i = 0; i < outs.size(); i++) {
    uint32_t f = flags ? flags[i] : 0u;
    if ((f & BROTLI_AMD_UNDICT_BYTES_SKIP) != 0u) continue;   // skipped: none of its other parameters are looked at
    const uint64_t cap = caps ? caps[i] : 0u;   // (without capacities every stream is counted, and nothing of a dictionary is looked at)
    BytesDict d = {nullptr, 0u, dict_entries ? dict_entries[i] : BROTLI_AMD_UNDICT_BYTES_ALL};
    if (cap != 0u) {
      const uint32_t j = dict_streams ? dict_streams[i] : BROTLI_AMD_UNDICT_NO_STREAM;
      if (j == BROTLI_AMD_UNDICT_NO_STREAM) { d.ptr = d_dicts ? d_dicts[i] : nullptr; d.len = dict_lens ? dict_lens[i] : 0u; }
      else if (j == i || j >= outs.size()) { refuse_bytes_dict_stream(i, j, outs.size()); return -1; }
      else { d.ptr = outs[j].ptr; d.len = outs[j].len; }
    }
    const BrotliAmdUndictBytesSeg s = {outs[i].ptr, static_cast<uint8_t*>(caps && d_data ? d_data[i] : nullptr), outs[i].len, cap, 0u, 0u, bits[i], f, 0u,
                                       static_cast<uint8_t*>(caps && d_offsets ? d_offsets[i] : nullptr), caps && data_caps ? data_caps[i] : 0u,
                                       offset_bases ? offset_bases[i] : 0u};
    if (!t.push(s, d, i, "stream")) return -1;
  }
  return undict_bytes_device(b, t, results, outs.size(), b->last_stream);
}

extern "C" int BrotliAmdBatchUndlbaSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_offsets, void* const* d_data,
                                            const uint64_t* data_caps, const uint64_t* caps, const uint8_t* flags, const uint64_t* offset_bases, BrotliAmdUndlbaResult* results,
                                            void* hip_stream) {
  if (!b || (n && (!d_src || !src_lens || !caps || !results))) return invalid_arguments(kUndlba);
  no_times(b, kUndlba);
  DlbaTable t;
  t.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    const BrotliAmdUndlbaSeg s = {static_cast<const uint8_t*>(d_src[i]), static_cast<uint8_t*>(d_data ? d_data[i] : nullptr), src_lens[i], caps[i], 0u, flags ? flags[i] : 0u, 0u,
                                  static_cast<uint8_t*>(d_offsets ? d_offsets[i] : nullptr), data_caps ? data_caps[i] : 0u, offset_bases ? offset_bases[i] : 0u};
    if (!t.push(s, i, "segment")) return -1;
  }
  return undlba_device(b, t, results, n, static_cast<hipStream_t>(hip_stream));
}
extern "C" int BrotliAmdBatchUndlbaOutputs(BrotliAmdBatch* b, void* const* d_offsets, void* const* d_data, const uint64_t* data_caps, const uint64_t* caps,
                                           const uint8_t* flags, const uint64_t* offset_bases, BrotliAmdUndlbaResult* results) {
  if (!b || !results) return invalid_arguments(kUndlba);
  no_times(b, kUndlba);
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  DlbaTable t;
  t.reserve(outs.size());
  for (size_t i = 0; i < outs.size(); i++) {
    const uint32_t f = flags ? flags[i] : 0u;
    if ((f & BROTLI_AMD_UNDLBA_SKIP) != 0u) continue;   // skipped: none of its other parameters are looked at
    // (without capacities every stream is counted, and no destination is looked at)
    const BrotliAmdUndlbaSeg s = {outs[i].ptr, static_cast<uint8_t*>(caps && d_data ? d_data[i] : nullptr), outs[i].len, caps ? caps[i] : 0u, 0u, f, 0u,
                                  static_cast<uint8_t*>(caps && d_offsets ? d_offsets[i] : nullptr), caps && data_caps ? data_caps[i] : 0u,
                                  offset_bases ? offset_bases[i] : 0u};
    if (!t.push(s, i, "stream")) return -1;
  }
  return undlba_device(b, t, results, outs.size(), b->last_stream);
}

extern "C" int BrotliAmdBatchUndbaSegments(BrotliAmdBatch* b, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_offsets, void* const* d_data,
                                           const uint64_t* data_caps, const uint64_t* caps, const uint8_t* flags, const uint64_t* offset_bases, BrotliAmdUndbaResult* results,
                                           void* hip_stream) {
  if (!b || (n && (!d_src || !src_lens || !caps || !results))) return invalid_arguments(kUndba);
  no_times(b, kUndba);
  DbaTable t;
  t.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    const BrotliAmdUndbaSeg s = {static_cast<const uint8_t*>(d_src[i]), static_cast<uint8_t*>(d_data ? d_data[i] : nullptr), src_lens[i], caps[i], 0u, flags ? flags[i] : 0u, 0u,
                                 static_cast<uint8_t*>(d_offsets ? d_offsets[i] : nullptr), data_caps ? data_caps[i] : 0u, offset_bases ? offset_bases[i] : 0u};
    if (!t.push(s, i, "segment")) return -1;
  }
  return undba_device(b, t, results, n, static_cast<hipStream_t>(hip_stream));
}
extern "C" int BrotliAmdBatchUndbaOutputs(BrotliAmdBatch* b, void* const* d_offsets, void* const* d_data, const uint64_t* data_caps, const uint64_t* caps,
                                          const uint8_t* flags, const uint64_t* offset_bases, BrotliAmdUndbaResult* results) {
  if (!b || !results) return invalid_arguments(kUndba);
  no_times(b, kUndba);
  std::vector<DeliveredBytes> outs;
  if (!delivered_outputs(b, &outs)) return -1;
  DbaTable t;
  t.reserve(outs.size());
  for (size_t i = 0; i < outs.size(); i++) {
    const uint32_t f = flags ? flags[i] : 0u;
    if ((f & BROTLI_AMD_UNDBA_SKIP) != 0u) continue;   // skipped: none of its other parameters are looked at
    // (without capacities every stream is counted, and no destination is looked at)
    const BrotliAmdUndbaSeg s = {outs[i].ptr, static_cast<uint8_t*>(caps && d_data ? d_data[i] : nullptr), outs[i].len, caps ? caps[i] : 0u, 0u, f, 0u,
                                 static_cast<uint8_t*>(caps && d_offsets ? d_offsets[i] : nullptr), caps && data_caps ? data_caps[i] : 0u,
                                 offset_bases ? offset_bases[i] : 0u};
    if (!t.push(s, i, "stream")) return -1;
  }
  return undba_device(b, t, results, outs.size(), b->last_stream);
}

extern "C" float BrotliAmdBatchLastUndbaMs(BrotliAmdBatch* b) { return b ? b->filter[kUndba].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndbaPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return phase_ms(b, kUndba, phase); }
extern "C" float BrotliAmdBatchLastUnnullMs(BrotliAmdBatch* b) { return b ? b->filter[kUnnull].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUnnullPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return phase_ms(b, kUnnull, phase); }
extern "C" float BrotliAmdBatchLastUnshuffleMs(BrotliAmdBatch* b) { return b ? b->filter[kUnshuffle].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndeltaMs(BrotliAmdBatch* b) { return b ? b->filter[kUndelta].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndeltaPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return phase_ms(b, kUndelta, phase); }
extern "C" float BrotliAmdBatchLastBitUnshuffleMs(BrotliAmdBatch* b) { return b ? b->filter[kBitUnshuffle].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastBitUnpackMs(BrotliAmdBatch* b) { return b ? b->filter[kBitUnpack].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUnvarintMs(BrotliAmdBatch* b) { return b ? b->filter[kUnvarint].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUnvarintPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return phase_ms(b, kUnvarint, phase); }
extern "C" float BrotliAmdBatchLastUnrleMs(BrotliAmdBatch* b) { return b ? b->filter[kUnrle].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUnrlePhaseMs(BrotliAmdBatch* b, uint32_t phase) { return phase_ms(b, kUnrle, phase); }
extern "C" float BrotliAmdBatchLastUndbpMs(BrotliAmdBatch* b) { return b ? b->filter[kUndbp].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndbpPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return phase_ms(b, kUndbp, phase); }
extern "C" float BrotliAmdBatchLastUndictMs(BrotliAmdBatch* b) { return b ? b->filter[kUndict].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndictPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return phase_ms(b, kUndict, phase); }
extern "C" float BrotliAmdBatchLastUndictBytesMs(BrotliAmdBatch* b) { return b ? b->filter[kUndictBytes].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndictBytesPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return phase_ms(b, kUndictBytes, phase); }
extern "C" float BrotliAmdBatchLastUndlbaMs(BrotliAmdBatch* b) { return b ? b->filter[kUndlba].ms : 0.0f; }
extern "C" float BrotliAmdBatchLastUndlbaPhaseMs(BrotliAmdBatch* b, uint32_t phase) { return phase_ms(b, kUndlba, phase); }
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

// ---- the hooks ----

extern "C" int BrotliAmdDebugUnshuffleHost(uint32_t width, const uint8_t* src, size_t len, uint8_t* dst, uint32_t src_skew, uint32_t dst_skew) {
  if (!known_width(kUnshuffle, width)) return -1;
  if (!rooms_ok(src, len, dst, len, src_skew, dst_skew)) return invalid_arguments(kUnshuffle);
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
  if (!rooms_ok(src, len, dst, len, src_skew, dst_skew)) return invalid_arguments(kBitUnshuffle);
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
  if (!rooms_ok(src, src_len, dst, count, src_skew, dst_skew)) return invalid_arguments(kBitUnpack);
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
  if ((n && (!src_offs || !dst_offs || !lens || !widths)) || !rooms_ok(src, src_size, dst, dst_size, src_skew, dst_skew) || (in_place && src_size != dst_size))
    return invalid_arguments(kUndelta);
  for (uint32_t i = 0; i < n; i++) {
    if (!known_width(kUndelta, widths[i])) return -1;
    if (!lies_in(dst_offs[i], lens[i], dst_size) || !lies_in(in_place ? 0u : src_offs[i], lens[i], src_size)) return outside_buffer(kUndelta);
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
  // phases 1 and 3 take the tiles in an order shuffled by the seed
  std::vector<uint64_t> order = first_numbers(ntiles);
  SeededOrder seeded(order_seed);
  auto tile_end = [&](uint64_t t) { return std::min<uint64_t>((t + 1u) * tile_units, units); };
  std::vector<BrotliAmdUndeltaTile> tiles(ntiles);
  seeded.shuffle(&order);
  for (uint64_t t : order) tiles[t] = brotli_amd_undelta_host_summary(segs.data(), pre.data(), n, t * tile_units, tile_end(t));
  const std::vector<uint64_t> carries = carries_of(tiles);
  seeded.shuffle(&order);
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
  if ((n && (!src_offs || !src_lens || !dst_offs || !caps || !widths || !results)) || !rooms_ok(src, src_size, dst, dst_size, src_skew, dst_skew))
    return invalid_arguments(kUnvarint);
  for (uint32_t i = 0; i < n; i++) {
    if (!known_counted<Unvarint>(0u, widths[i], flags ? flags[i] : 0u, caps[i], true, "segment", i)) return -1;
    const uint64_t room = std::min<uint64_t>(caps[i], src_lens[i]) * widths[i];   // (a segment of len bytes holds len varints at the most)
    if (!lies_in(src_offs[i], src_lens[i], src_size) || !lies_in(dst_offs[i], room, dst_size)) return outside_buffer(kUnvarint);
  }
  if (tile_units == 0u) tile_units = brotli_amd_unvarint_tile_bytes() / 16u;
  SkewedRoom sroom(src_size, src_skew, 0xA5), droom(dst_size, dst_skew, 0x5A);
  sroom.put(src, src_size);
  droom.put(dst, dst_size);
  std::vector<BrotliAmdUnvarintSeg> segs(n);
  std::vector<uint64_t> pre(n + 1u, 0u);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t s = sroom.at() + src_offs[i], d = droom.at() + dst_offs[i];
    segs[i] = BrotliAmdUnvarintSeg{reinterpret_cast<const uint8_t*>((uintptr_t)s), reinterpret_cast<uint8_t*>((uintptr_t)d), src_lens[i], caps[i], widths[i],
                                   flags ? flags[i] : 0u};
    pre[i + 1u] = pre[i] + brotli_amd_seg_units(s, src_lens[i]);
  }
  droom.snapshot();
  const uint64_t units = pre[n], ntiles = (units + tile_units - 1u) / tile_units;
  // phases 1 and 3 take the tiles in an order shuffled by the seed
  std::vector<uint64_t> order = first_numbers(ntiles);
  SeededOrder seeded(order_seed);
  auto tile_end = [&](uint64_t t) { return std::min<uint64_t>((t + 1u) * tile_units, units); };
  std::vector<BrotliAmdUndeltaTile> tiles(ntiles);
  std::vector<BrotliAmdUnvarintResult> got(n, BrotliAmdUnvarintResult{0u, 0u, 0u});
  seeded.shuffle(&order);
  for (uint64_t t : order) tiles[t] = brotli_amd_unvarint_host_summary(segs.data(), pre.data(), n, t * tile_units, tile_end(t));
  const std::vector<uint64_t> carries = carries_of(tiles);
  seeded.shuffle(&order);
  for (uint64_t t : order) brotli_amd_unvarint_host_emit(segs.data(), pre.data(), n, t * tile_units, tile_end(t), carries[t], got.data());
  for (uint32_t i = 0; i < n; i++)
    if (std::min(got[i].count, caps[i]) * widths[i] > dst_size - dst_offs[i]) { g_last_error = "unvarint counted more varints than the segment has bytes"; return -2; }
  return counted_hook_result(kUnvarint, droom, n, dst, dst_size, dst_offs, caps, widths, got, results);
}

// Unrle's two phases over n segments given as offsets into one source and one destination buffer, each buffer in its room: every segment's walk,
// then the items of all segments in an order shuffled by the seed.
extern "C" int BrotliAmdDebugUnrleHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                       const uint64_t* src_lens, const uint64_t* dst_offs, const uint64_t* caps, const uint8_t* bits, const uint8_t* widths,
                                       const uint8_t* flags, uint32_t src_skew, uint32_t dst_skew, uint32_t item_elems, uint32_t order_seed,
                                       BrotliAmdUnrleResult* results) {
  if ((n && (!src_offs || !src_lens || !dst_offs || !caps || !bits || !widths || !results)) || !rooms_ok(src, src_size, dst, dst_size, src_skew, dst_skew))
    return invalid_arguments(kUnrle);
  if (item_elems == 0u) item_elems = brotli_amd_unrle_item_elems();
  for (uint32_t i = 0; i < n; i++) {
    if (!known_counted<Unrle>(bits[i], widths[i], flags ? flags[i] : 0u, caps[i], true, "segment", i)) return -1;
    if (!lies_in(src_offs[i], src_lens[i], src_size) || dst_offs[i] > dst_size) return outside_buffer(kUnrle);
  }
  SkewedRoom sroom(src_size, src_skew, 0xA5), droom(dst_size, dst_skew, 0x5A);
  sroom.put(src, src_size);
  droom.put(dst, dst_size);
  std::vector<BrotliAmdUnrleSeg> segs;
  for (uint32_t i = 0; i < n; i++)
    segs.push_back(BrotliAmdUnrleSeg{reinterpret_cast<const uint8_t*>((uintptr_t)(sroom.at() + src_offs[i])), reinterpret_cast<uint8_t*>((uintptr_t)(droom.at() + dst_offs[i])),
                                     src_lens[i], caps[i], 0u, widths[i], bits[i], flags ? flags[i] : 0u, 0u});
  return walk_items_hook(
      kUnrle, segs, droom, ItemHookDst{dst, dst_size, dst_offs, caps, widths}, item_elems, order_seed,
      [&](uint32_t i, BrotliAmdUnrleCheckpoint* ckpts) { return brotli_amd_unrle_host_walk(segs[i], item_elems, ckpts); },
      [&](uint32_t i, BrotliAmdUnrleResult* res, BrotliAmdUnrleCheckpoint cp, uint64_t j) { brotli_amd_unrle_host_item(segs[i], *res, cp, j, item_elems); }, results);
}

// Undbp's phases over n segments given as offsets into one source and one destination buffer, each buffer in its room: every segment's walk, the
// items' sums in an order shuffled by the seed, the carries as undelta's hook takes them, and the items' stores in another shuffled order.
extern "C" int BrotliAmdDebugUndbpHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                       const uint64_t* src_lens, const uint64_t* dst_offs, const uint64_t* caps, const uint8_t* widths, const uint8_t* flags,
                                       uint32_t src_skew, uint32_t dst_skew, uint32_t item_deltas, uint32_t order_seed, BrotliAmdUndbpResult* results) {
  if ((n && (!src_offs || !src_lens || !dst_offs || !caps || !widths || !results)) || !rooms_ok(src, src_size, dst, dst_size, src_skew, dst_skew))
    return invalid_arguments(kUndbp);
  if (item_deltas == 0u) item_deltas = brotli_amd_undbp_item_deltas();
  if (!brotli_amd_undbp_item_ok(item_deltas)) { g_last_error = "invalid undbp arguments: an item that is no multiple of 32 deltas"; return -1; }
  for (uint32_t i = 0; i < n; i++) {
    if (!known_counted<Undbp>(0u, widths[i], flags ? flags[i] : 0u, caps[i], true, "segment", i)) return -1;
    if (!lies_in(src_offs[i], src_lens[i], src_size) || dst_offs[i] > dst_size) return outside_buffer(kUndbp);
  }
  SkewedRoom sroom(src_size, src_skew, 0xA5), droom(dst_size, dst_skew, 0x5A);
  sroom.put(src, src_size);
  droom.put(dst, dst_size);
  std::vector<BrotliAmdUndbpSeg> segs;
  for (uint32_t i = 0; i < n; i++)
    segs.push_back(BrotliAmdUndbpSeg{reinterpret_cast<const uint8_t*>((uintptr_t)(sroom.at() + src_offs[i])), reinterpret_cast<uint8_t*>((uintptr_t)(droom.at() + dst_offs[i])),
                                     src_lens[i], caps[i], 0u, widths[i], 0u});
  std::vector<BrotliAmdUndbpResult> got(n);
  std::vector<uint64_t> firsts(n, 0u);
  const int r = walk_count_store_hook<BrotliAmdUndbpCheckpoint>(
      kUndbp, segs, got, droom, ItemHookDst{dst, dst_size, dst_offs, caps, widths}, order_seed, [&](uint64_t cap) { return brotli_amd_undbp_items(cap, item_deltas); },
      [&](uint32_t i, BrotliAmdUndbpCheckpoint* ckpts) { return brotli_amd_undbp_host_walk(segs[i], item_deltas, ckpts, &firsts[i]); }, [](uint32_t, uint64_t) { return true; },
      [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j) { return brotli_amd_undbp_host_sum(segs[i], got[i], cp, firsts[i], j, item_deltas); },
      [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t carry) { brotli_amd_undbp_host_store(segs[i], got[i], cp, firsts[i], j, item_deltas, carry); });
  return r != 0 ? r : counted_hook_result(kUndbp, droom, n, dst, dst_size, dst_offs, caps, widths, got, results);
}

// Undict's two phases over n segments given as offsets into one source, one destination and one dictionary buffer, each buffer in its room:
// every segment's walk -- unrle's --, then the items of all segments in an order shuffled by the seed, each adding its bad elements to its
// segment's result.
extern "C" int BrotliAmdDebugUndictHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint8_t* dict, size_t dict_size,
                                        const uint64_t* src_offs, const uint64_t* src_lens, const uint64_t* dst_offs, const uint64_t* caps, const uint64_t* dict_offs,
                                        const uint64_t* dict_entries, const uint8_t* bits, const uint8_t* widths, const uint8_t* flags, uint32_t src_skew,
                                        uint32_t dst_skew, uint32_t dict_skew, uint32_t item_elems, uint32_t order_seed, BrotliAmdUndictResult* results) {
  if ((n && (!src_offs || !src_lens || !dst_offs || !caps || !dict_offs || !dict_entries || !bits || !widths || !results)) ||
      !rooms_ok(src, src_size, dst, dst_size, src_skew, dst_skew) || (dict_size && !dict) || dict_skew > 15u)
    return invalid_arguments(kUndict);
  if (item_elems == 0u) item_elems = brotli_amd_unrle_item_elems();
  for (uint32_t i = 0; i < n; i++) {
    if (!known_counted<Undict>(bits[i], widths[i], flags ? flags[i] : 0u, caps[i], true, "segment", i, Dict{dict ? dict : src, dict_entries[i]})) return -1;
    if (!lies_in(src_offs[i], src_lens[i], src_size) || dst_offs[i] > dst_size) return outside_buffer(kUndict);
    if (dict_entries[i] != 0u && !lies_in(dict_offs[i], dict_entries[i] * widths[i], dict_size)) {
      g_last_error = "invalid undict arguments: a dictionary outside its buffer";
      return -1;
    }
  }
  SkewedRoom sroom(src_size, src_skew, 0xA5), droom(dst_size, dst_skew, 0x5A), troom(dict_size, dict_skew, 0x3C);
  sroom.put(src, src_size);
  droom.put(dst, dst_size);
  troom.put(dict, dict_size);
  std::vector<BrotliAmdUndictSeg> segs;
  for (uint32_t i = 0; i < n; i++)
    segs.push_back(BrotliAmdUndictSeg{reinterpret_cast<const uint8_t*>((uintptr_t)(sroom.at() + src_offs[i])), reinterpret_cast<uint8_t*>((uintptr_t)(droom.at() + dst_offs[i])),
                                      src_lens[i], caps[i], 0u, widths[i], bits[i], flags ? flags[i] : 0u, 0u,
                                      reinterpret_cast<const uint8_t*>((uintptr_t)(troom.at() + dict_offs[i])), dict_entries[i]});
  return walk_items_hook(
      kUndict, segs, droom, ItemHookDst{dst, dst_size, dst_offs, caps, widths}, item_elems, order_seed,
      [&](uint32_t i, BrotliAmdUnrleCheckpoint* ckpts) { return brotli_amd_undict_host_walk(segs[i], item_elems, ckpts); },
      [&](uint32_t i, BrotliAmdUndictResult* res, BrotliAmdUnrleCheckpoint cp, uint64_t j) { brotli_amd_undict_host_item(segs[i], res, cp, j, item_elems); }, results);
}

// Unnull's four phases over n segments given as offsets into one source, one destination, one values and one validity buffer, each buffer in its
// room: every segment's walk behind its prefix, the items' counts in an order shuffled by the seed, the carries as undelta's hook takes them,
// and the items' slots and validity bytes in another shuffled order, each adding its present and missing slots to its segment's result.
extern "C" int BrotliAmdDebugUnnullHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint8_t* values, size_t values_size,
                                        uint8_t* valid, size_t valid_size, const uint64_t* src_offs, const uint64_t* src_lens, const uint64_t* dst_offs,
                                        const uint64_t* caps, const uint64_t* value_offs, const uint64_t* value_counts, const uint64_t* valid_offs, const uint32_t* levels,
                                        const uint8_t* bits, const uint8_t* widths, const uint8_t* flags, uint32_t src_skew, uint32_t dst_skew, uint32_t values_skew,
                                        uint32_t valid_skew, uint32_t item_elems, uint32_t order_seed, BrotliAmdUnnullResult* results) {
  if ((n && (!src_offs || !src_lens || !dst_offs || !caps || !value_offs || !value_counts || !valid_offs || !levels || !bits || !widths || !results)) ||
      !rooms_ok(src, src_size, dst, dst_size, src_skew, dst_skew) || !rooms_ok(values, values_size, valid, valid_size, values_skew, valid_skew))
    return invalid_arguments(kUnnull);
  if (item_elems == 0u) item_elems = brotli_amd_unrle_item_elems();
  if (!brotli_amd_unnull_item_ok(item_elems)) { g_last_error = "invalid unnull arguments: an item that is no multiple of 8 slots"; return -1; }
  SkewedRoom sroom(src_size, src_skew, 0xA5), droom(dst_size, dst_skew, 0x5A), vroom(values_size, values_skew, 0x3C), broom(valid_size, valid_skew, 0xC3);
  std::vector<BrotliAmdUnnullSeg> segs;
  for (uint32_t i = 0; i < n; i++) {
    const bool has_valid = valid_offs[i] != ~(uint64_t)0;
    const BrotliAmdUnnullSeg s = {reinterpret_cast<const uint8_t*>((uintptr_t)(sroom.at() + src_offs[i])), reinterpret_cast<uint8_t*>((uintptr_t)(droom.at() + dst_offs[i])),
                                  src_lens[i], caps[i], 0u, widths[i], bits[i], flags ? flags[i] : 0u, levels[i],
                                  reinterpret_cast<const uint8_t*>((uintptr_t)(vroom.at() + value_offs[i])), value_counts[i],
                                  has_valid ? reinterpret_cast<uint8_t*>((uintptr_t)(broom.at() + valid_offs[i])) : nullptr};
    if (!known_unnull(s, true, "segment", i)) return -1;
    if (!lies_in(src_offs[i], src_lens[i], src_size) || dst_offs[i] > dst_size || (has_valid && valid_offs[i] > valid_size)) return outside_buffer(kUnnull);
    if ((s.flags & BROTLI_AMD_UNNULL_VALUES_FOLLOW) == 0u && value_counts[i] != 0u && !lies_in(value_offs[i], value_counts[i] * widths[i], values_size)) {
      g_last_error = "invalid unnull arguments: values outside their buffer";
      return -1;
    }
    segs.push_back(s);
  }
  sroom.put(src, src_size);
  droom.put(dst, dst_size);
  vroom.put(values, values_size);
  broom.put(valid, valid_size);
  broom.snapshot();   // (the walks write nothing)
  std::vector<BrotliAmdUnnullResult> got(n);
  std::vector<BrotliAmdUnnullRuns> runs(n);
  std::vector<uint32_t> masks((item_elems + BROTLI_AMD_UNNULL_LANE_SLOTS - 1u) / BROTLI_AMD_UNNULL_LANE_SLOTS);
  const int walked = walk_count_store_hook<BrotliAmdUnrleCheckpoint>(
      kUnnull, segs, got, droom, ItemHookDst{dst, dst_size, dst_offs, caps, widths}, order_seed, [&](uint64_t cap) { return brotli_amd_unrle_items(cap, item_elems); },
      [&](uint32_t i, BrotliAmdUnrleCheckpoint* ckpts) { return brotli_amd_unnull_host_walk(segs[i], item_elems, ckpts, &runs[i]); },
      [&](uint32_t i, uint64_t m) { return !segs[i].valid || (m + 7u) / 8u <= valid_size - valid_offs[i]; },
      [&](uint32_t i, BrotliAmdUnrleCheckpoint cp, uint64_t j) {
        std::fill(masks.begin(), masks.end(), 0u);
        return brotli_amd_unnull_host_count(segs[i], runs[i], got[i], cp, j, item_elems, masks.data());
      },
      [&](uint32_t i, BrotliAmdUnrleCheckpoint cp, uint64_t j, uint64_t carry) {
        std::fill(masks.begin(), masks.end(), 0u);
        brotli_amd_unnull_host_expand(segs[i], runs[i], &got[i], cp, j, item_elems, carry, masks.data());
      });
  if (walked != 0) return walked;
  // no byte outside every segment's validity bytes may have changed; the slots' room is judged by the counted hooks' closing block
  std::vector<uint8_t> inside(valid_size, 0);
  for (uint32_t i = 0; i < n; i++)
    if (segs[i].valid) std::fill(inside.begin() + valid_offs[i], inside.begin() + valid_offs[i] + (std::min(got[i].count, caps[i]) + 7u) / 8u, 1);
  if (!broom.changed_inside_only([&](size_t i) { return i < valid_size && inside[i]; })) { g_last_error = "unnull wrote outside its bitmap"; return -2; }
  const int r = counted_hook_result(kUnnull, droom, n, dst, dst_size, dst_offs, caps, widths, got, results);
  if (r == 0) broom.get(valid, 0u, valid_size);
  return r;
}

// Undict-bytes' five phases over n segments given as offsets into one source, one offsets, one data and one dictionary buffer, each buffer in
// its room: every distinct dictionary's walk, every segment's walk -- unrle's --, the items' byte counts in an order shuffled by the seed, the
// carries as undelta's hook takes them, and the items' offsets and bytes in another shuffled order, every item's destination words in an
// order shuffled by word_seed.
extern "C" int BrotliAmdDebugUndictBytesHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* offsets, size_t offsets_size, uint8_t* data, size_t data_size,
                                             const uint8_t* dict, size_t dict_size, const uint64_t* src_offs, const uint64_t* src_lens, const uint64_t* offsets_offs,
                                             const uint64_t* data_offs, const uint64_t* data_caps, const uint64_t* caps, const uint64_t* offset_bases,
                                             const uint64_t* dict_offs, const uint64_t* dict_lens, const uint64_t* dict_entries, const uint8_t* bits, const uint8_t* flags,
                                             uint32_t src_skew, uint32_t offsets_skew, uint32_t data_skew, uint32_t dict_skew, uint32_t item_elems, uint32_t order_seed,
                                             uint32_t word_seed, BrotliAmdUndictBytesResult* results, uint64_t* dict_walks) {
  const uint64_t none = ~(uint64_t)0;
  if ((n && (!src_offs || !src_lens || !offsets_offs || !data_offs || !data_caps || !caps || !offset_bases || !dict_offs || !dict_lens || !dict_entries || !bits || !results)) ||
      !rooms_ok(src, src_size, offsets, offsets_size, src_skew, offsets_skew) || !rooms_ok(dict, dict_size, data, data_size, dict_skew, data_skew))
    return invalid_arguments(kUndictBytes);
  if (item_elems == 0u) item_elems = brotli_amd_unrle_item_elems();
  SkewedRoom sroom(src_size, src_skew, 0xA5), oroom(offsets_size, offsets_skew, 0x5A), droom(data_size, data_skew, 0x69), troom(dict_size, dict_skew, 0x3C);
  std::vector<BrotliAmdUndictBytesSeg> segs;
  std::vector<BytesDict> dicts;
  for (uint32_t i = 0; i < n; i++) {
    const bool has_offsets = offsets_offs[i] != none, has_data = data_offs[i] != none;
    const BytesDict d = {dict_lens[i] ? reinterpret_cast<const void*>((uintptr_t)(troom.at() + dict_offs[i])) : nullptr, dict_lens[i], dict_entries[i]};
    const BrotliAmdUndictBytesSeg s = {reinterpret_cast<const uint8_t*>((uintptr_t)(sroom.at() + src_offs[i])),
                                       has_data ? reinterpret_cast<uint8_t*>((uintptr_t)(droom.at() + data_offs[i])) : nullptr, src_lens[i], caps[i], 0u,
                                       BROTLI_AMD_UNDICT_BYTES_NO_DICT, bits[i], flags ? flags[i] : 0u, 0u,
                                       has_offsets ? reinterpret_cast<uint8_t*>((uintptr_t)(oroom.at() + offsets_offs[i])) : nullptr, data_caps[i], offset_bases[i]};
    if (!known_bytes(s, d, "segment", i)) return -1;
    if (!lies_in(src_offs[i], src_lens[i], src_size) || (has_offsets && offsets_offs[i] > offsets_size) || (has_data && data_offs[i] > data_size)) return outside_buffer(kUndictBytes);
    if (caps[i] != 0u && dict_lens[i] != 0u && !lies_in(dict_offs[i], dict_lens[i], dict_size)) {
      g_last_error = "invalid undict-bytes arguments: a dictionary outside its buffer";
      return -1;
    }
    segs.push_back(s);
    dicts.push_back(d);
  }
  sroom.put(src, src_size);
  oroom.put(offsets, offsets_size);
  droom.put(data, data_size);
  troom.put(dict, dict_size);
  // phase 1: every distinct dictionary once
  BytesDicts table;
  for (uint32_t i = 0; i < n; i++)
    if (caps[i] != 0u) segs[i].dict = table.index(dicts[i]);
  std::vector<uint32_t> starts(table.starts);
  std::vector<BrotliAmdUndictBytesDictResult> dict_results;
  for (const BrotliAmdUndictBytesDict& r : table.recs)
    dict_results.push_back(brotli_amd_undict_bytes_host_dict((uint64_t)(uintptr_t)r.dict, r.len, r.bound, starts.data() + r.first_start));
  if (dict_walks) *dict_walks = table.recs.size();
  // phase 2: the walks.  A segment's capacity becomes its count and one more at the most: the walk marks the items of no other elements, and a
  // capacity of 2^56 needs no table of its own.
  HookItems<BrotliAmdUnrleCheckpoint> items;
  std::vector<BytesResult> got(n);
  items.pre.assign(n + 1u, 0u);
  for (uint32_t i = 0; i < n; i++) {
    const BrotliAmdUndictBytesDictResult dr = segs[i].dict != BROTLI_AMD_UNDICT_BYTES_NO_DICT ? dict_results[segs[i].dict] : BrotliAmdUndictBytesDictResult{0u, 0u, 0u, 0u};
    BrotliAmdUndictBytesSeg counting = segs[i];
    counting.cap = 0u;
    segs[i].cap = std::min<uint64_t>(caps[i], brotli_amd_undict_bytes_host_walk(counting, dr, item_elems, nullptr).count + 1u);
    segs[i].first_item = items.pre[i];
    items.pre[i + 1u] = items.pre[i] + brotli_amd_unrle_items(segs[i].cap, item_elems);
    items.ckpts.resize(items.pre[i + 1u], BrotliAmdUnrleCheckpoint{BROTLI_AMD_UNRLE_NONE, BROTLI_AMD_UNRLE_NONE});
    got[i] = brotli_amd_undict_bytes_host_walk(segs[i], dr, item_elems, items.ckpts.data() + items.pre[i]);
    const uint64_t slots = std::min(got[i].count, caps[i]) + ((segs[i].flags & BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY) != 0u || caps[i] == 0u ? 0u : 1u);
    if (segs[i].offsets && slots * brotli_amd_undict_bytes_offset_width(segs[i].flags) > offsets_size - offsets_offs[i]) return outside_buffer(kUndictBytes);
  }
  oroom.snapshot();
  droom.snapshot();
  // phases 3 and 4
  SeededOrder seeded(order_seed), word_order(word_seed);
  std::vector<BrotliAmdUndeltaTile> tiles(items.pre.back());
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUnrleCheckpoint cp, uint64_t j, uint64_t g) {
    tiles[g] = brotli_amd_undict_bytes_host_count(segs[i], starts.data() + table.recs[segs[i].dict].first_start, &got[i], cp, j, item_elems);
  });
  const std::vector<uint64_t> carries = carries_of(tiles);
  std::vector<uint64_t> kept(n, 0u);   // the bytes of every segment that its data capacity leaves
  for (uint32_t i = 0; i < n; i++) {
    uint64_t bytes = 0;
    for (uint64_t g = items.pre[i]; g < items.pre[i + 1u]; g++) bytes += tiles[g].sum;
    kept[i] = segs[i].data ? std::min(bytes, segs[i].data_cap) : 0u;
    if (segs[i].data && kept[i] > data_size - data_offs[i]) return outside_buffer(kUndictBytes);
  }
  // phase 5
  std::vector<uint64_t> ends(item_elems + 1u);
  std::vector<uint32_t> pos(item_elems);
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUnrleCheckpoint cp, uint64_t j, uint64_t g) {
    const BrotliAmdUndictBytesDict& r = table.recs[segs[i].dict];
    brotli_amd_undict_bytes_host_expand(segs[i], (uint64_t)(uintptr_t)r.dict, starts.data() + r.first_start, &got[i], cp, j, item_elems, carries[g], ends.data(), pos.data(),
                                        [&](uint64_t count, auto each) {
      std::vector<uint64_t> order = first_numbers(count);
      word_order.shuffle(&order);
      for (uint64_t q : order) each(q);
    });
  });
  // no byte outside every segment's offsets and bytes may have changed
  std::vector<uint8_t> in_offsets(offsets_size, 0), in_data(data_size, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t slots = std::min(got[i].count, caps[i]) + ((segs[i].flags & BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY) != 0u || caps[i] == 0u ? 0u : 1u);
    if (segs[i].offsets) std::fill(in_offsets.begin() + offsets_offs[i], in_offsets.begin() + offsets_offs[i] + slots * brotli_amd_undict_bytes_offset_width(segs[i].flags), 1);
    if (segs[i].data) std::fill(in_data.begin() + data_offs[i], in_data.begin() + data_offs[i] + kept[i], 1);
  }
  if (!oroom.changed_inside_only([&](size_t i) { return i < offsets_size && in_offsets[i]; })) { g_last_error = "undict-bytes wrote outside its offsets"; return -2; }
  if (!droom.changed_inside_only([&](size_t i) { return i < data_size && in_data[i]; })) { g_last_error = "undict-bytes wrote outside its data"; return -2; }
  oroom.get(offsets, 0u, offsets_size);
  droom.get(data, 0u, data_size);
  std::copy(got.begin(), got.end(), results);
  return 0;
}

// Undlba's phases over n segments given as offsets into one source, one offsets and one data buffer, each buffer in its room: every segment's
// walk -- undbp's --, the items' delta sums in an order shuffled by the seed, the carries as undelta's hook takes them, the items' lengths in
// another shuffled order, the carries of their bytes, the items' offsets in a third, and the segments' copies in a fourth.
extern "C" int BrotliAmdDebugUndlbaHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* offsets, size_t offsets_size, uint8_t* data, size_t data_size,
                                        const uint64_t* src_offs, const uint64_t* src_lens, const uint64_t* offsets_offs, const uint64_t* data_offs,
                                        const uint64_t* data_caps, const uint64_t* caps, const uint64_t* offset_bases, const uint8_t* flags, uint32_t src_skew,
                                        uint32_t offsets_skew, uint32_t data_skew, uint32_t item_deltas, uint32_t order_seed, BrotliAmdUndlbaResult* results) {
  const uint64_t none = ~(uint64_t)0;
  if ((n && (!src_offs || !src_lens || !offsets_offs || !data_offs || !data_caps || !caps || !offset_bases || !results)) ||
      !rooms_ok(src, src_size, offsets, offsets_size, src_skew, offsets_skew) || (data_size && !data) || data_skew > 15u)
    return invalid_arguments(kUndlba);
  if (item_deltas == 0u) item_deltas = brotli_amd_undbp_item_deltas();
  if (!brotli_amd_undbp_item_ok(item_deltas)) { g_last_error = "invalid undlba arguments: an item that is no multiple of 32 deltas"; return -1; }
  SkewedRoom sroom(src_size, src_skew, 0xA5), oroom(offsets_size, offsets_skew, 0x5A), droom(data_size, data_skew, 0x69);
  std::vector<BrotliAmdUndlbaSeg> segs;
  for (uint32_t i = 0; i < n; i++) {
    const bool has_offsets = offsets_offs[i] != none, has_data = data_offs[i] != none;
    const BrotliAmdUndlbaSeg s = {reinterpret_cast<const uint8_t*>((uintptr_t)(sroom.at() + src_offs[i])),
                                  has_data ? reinterpret_cast<uint8_t*>((uintptr_t)(droom.at() + data_offs[i])) : nullptr, src_lens[i], caps[i], 0u, flags ? flags[i] : 0u, 0u,
                                  has_offsets ? reinterpret_cast<uint8_t*>((uintptr_t)(oroom.at() + offsets_offs[i])) : nullptr, data_caps[i], offset_bases[i]};
    if (!known_dlba(s, "segment", i)) return -1;
    if (!lies_in(src_offs[i], src_lens[i], src_size) || (has_offsets && offsets_offs[i] > offsets_size) || (has_data && data_offs[i] > data_size)) return outside_buffer(kUndlba);
    segs.push_back(s);
  }
  sroom.put(src, src_size);
  oroom.put(offsets, offsets_size);
  droom.put(data, data_size);
  // phase 1: the walks.  A segment's capacity becomes its count and one more at the most: the walk marks the items of no other elements, and a
  // capacity of 2^56 needs no table of its own.
  HookItems<BrotliAmdUndbpCheckpoint> items;
  std::vector<DlbaResult> got(n);
  std::vector<uint64_t> firsts(n, 0u);
  items.pre.assign(n + 1u, 0u);
  auto slots_of = [&](uint32_t i) { return std::min(got[i].count, caps[i]) + ((segs[i].flags & BROTLI_AMD_UNDLBA_ENDS_ONLY) != 0u || caps[i] == 0u ? 0u : 1u); };
  for (uint32_t i = 0; i < n; i++) {
    BrotliAmdUndlbaSeg counting = segs[i];
    counting.cap = 0u;
    segs[i].cap = std::min<uint64_t>(caps[i], brotli_amd_undlba_host_walk(counting, item_deltas, nullptr, &firsts[i]).count + 1u);
    segs[i].first_item = items.pre[i];
    items.pre[i + 1u] = items.pre[i] + brotli_amd_undbp_items(segs[i].cap, item_deltas);
    items.ckpts.resize(items.pre[i + 1u], BrotliAmdUndbpCheckpoint{BROTLI_AMD_UNDBP_NONE, BROTLI_AMD_UNDBP_NONE});
    got[i] = brotli_amd_undlba_host_walk(segs[i], item_deltas, items.ckpts.data() + items.pre[i], &firsts[i]);
    if (segs[i].offsets && slots_of(i) * brotli_amd_undlba_offset_width(segs[i].flags) > offsets_size - offsets_offs[i]) return outside_buffer(kUndlba);
  }
  oroom.snapshot();
  droom.snapshot();
  // phases 2 to 5
  SeededOrder seeded(order_seed);
  std::vector<BrotliAmdUndeltaTile> tiles(items.pre.back()), byte_tiles(items.pre.back());
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g) {
    tiles[g] = brotli_amd_undlba_host_sum(segs[i], got[i], cp, firsts[i], j, item_deltas);
  });
  const std::vector<uint64_t> carries = carries_of(tiles);
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g) {
    byte_tiles[g] = brotli_amd_undlba_host_lengths(segs[i], &got[i], cp, firsts[i], j, item_deltas, carries[g]);
  });
  const std::vector<uint64_t> byte_carries = carries_of(byte_tiles);
  std::vector<uint64_t> kept(n, 0u);   // the bytes of every segment that its source and its data capacity leave
  for (uint32_t i = 0; i < n; i++) {
    uint64_t bytes = 0;
    for (uint64_t g = items.pre[i]; g < items.pre[i + 1u]; g++) bytes += byte_tiles[g].sum;
    kept[i] = segs[i].data && segs[i].cap != 0u ? std::min({bytes, got[i].data_avail, segs[i].data_cap}) : 0u;
    if (kept[i] > data_size - (segs[i].data ? data_offs[i] : 0u)) return outside_buffer(kUndlba);
  }
  // phases 6 and 7: the table of copies starts as zeros
  std::vector<BrotliAmdCopySeg> copies(n, BrotliAmdCopySeg{nullptr, nullptr, 0u});
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g) {
    brotli_amd_undlba_host_expand(segs[i], &got[i], cp, firsts[i], j, item_deltas, carries[g], byte_carries[g], &copies[i]);
  });
  std::vector<uint64_t> order = first_numbers(n);
  seeded.shuffle(&order);
  for (uint64_t i : order) brotli_amd_undlba_host_copy(copies[i]);
  // no byte outside every segment's offsets and bytes may have changed
  std::vector<uint8_t> in_offsets(offsets_size, 0), in_data(data_size, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (segs[i].offsets) std::fill(in_offsets.begin() + offsets_offs[i], in_offsets.begin() + offsets_offs[i] + slots_of(i) * brotli_amd_undlba_offset_width(segs[i].flags), 1);
    if (segs[i].data) std::fill(in_data.begin() + data_offs[i], in_data.begin() + data_offs[i] + kept[i], 1);
  }
  if (!oroom.changed_inside_only([&](size_t i) { return i < offsets_size && in_offsets[i]; })) { g_last_error = "undlba wrote outside its offsets"; return -2; }
  if (!droom.changed_inside_only([&](size_t i) { return i < data_size && in_data[i]; })) { g_last_error = "undlba wrote outside its data"; return -2; }
  oroom.get(offsets, 0u, offsets_size);
  droom.get(data, 0u, data_size);
  std::copy(got.begin(), got.end(), results);
  return 0;
}

// Undba's phases over n segments given as offsets into one source, one offsets and one data buffer, each buffer in its room: every segment's
// two walks -- undbp's --, the items' delta sums of both streams in an order shuffled by the seed, the carries as undelta's hook takes them, the
// items' tests and sums in another shuffled order, their carries, the offsets in a third, phase A in a fourth, phase B segment by segment in a
// shuffled order of the segments, and phase C in a sixth.
extern "C" int BrotliAmdDebugUndbaHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* offsets, size_t offsets_size, uint8_t* data, size_t data_size,
                                       const uint64_t* src_offs, const uint64_t* src_lens, const uint64_t* offsets_offs, const uint64_t* data_offs,
                                       const uint64_t* data_caps, const uint64_t* caps, const uint64_t* offset_bases, const uint8_t* flags, uint32_t src_skew,
                                       uint32_t offsets_skew, uint32_t data_skew, uint32_t item_deltas, uint32_t order_seed, BrotliAmdUndbaResult* results) {
  const uint64_t none = ~(uint64_t)0;
  if ((n && (!src_offs || !src_lens || !offsets_offs || !data_offs || !data_caps || !caps || !offset_bases || !results)) ||
      !rooms_ok(src, src_size, offsets, offsets_size, src_skew, offsets_skew) || (data_size && !data) || data_skew > 15u)
    return invalid_arguments(kUndba);
  if (item_deltas == 0u) item_deltas = brotli_amd_undbp_item_deltas();
  if (!brotli_amd_undbp_item_ok(item_deltas)) { g_last_error = "invalid undba arguments: an item that is no multiple of 32 deltas"; return -1; }
  SkewedRoom sroom(src_size, src_skew, 0xA5), oroom(offsets_size, offsets_skew, 0x5A), droom(data_size, data_skew, 0x69);
  std::vector<BrotliAmdUndbaSeg> segs;
  for (uint32_t i = 0; i < n; i++) {
    const bool has_offsets = offsets_offs[i] != none, has_data = data_offs[i] != none;
    const BrotliAmdUndbaSeg s = {reinterpret_cast<const uint8_t*>((uintptr_t)(sroom.at() + src_offs[i])),
                                 has_data ? reinterpret_cast<uint8_t*>((uintptr_t)(droom.at() + data_offs[i])) : nullptr, src_lens[i], caps[i], 0u, flags ? flags[i] : 0u, 0u,
                                 has_offsets ? reinterpret_cast<uint8_t*>((uintptr_t)(oroom.at() + offsets_offs[i])) : nullptr, data_caps[i], offset_bases[i]};
    if (!known_dba(s, "segment", i)) return -1;
    if (!lies_in(src_offs[i], src_lens[i], src_size) || (has_offsets && offsets_offs[i] > offsets_size) || (has_data && data_offs[i] > data_size)) return outside_buffer(kUndba);
    segs.push_back(s);
  }
  sroom.put(src, src_size);
  oroom.put(offsets, offsets_size);
  droom.put(data, data_size);
  // phase 1: the walks.  A segment's capacity becomes its values and one more at the most: the walks mark the items of no other elements, and
  // a capacity of 2^56 needs no table of its own.  P's checkpoints, and S's beside them.
  HookItems<BrotliAmdUndbpCheckpoint> items;
  std::vector<BrotliAmdUndbpCheckpoint> ckpts_s;
  std::vector<DbaResult> got(n);
  std::vector<uint64_t> firsts_p(n, 0u), firsts_s(n, 0u);
  items.pre.assign(n + 1u, 0u);
  auto slots_of = [&](uint32_t i) {
    return brotli_amd_undba_m(got[i].count_p, got[i].count_s, caps[i]) + ((segs[i].flags & BROTLI_AMD_UNDBA_ENDS_ONLY) != 0u || caps[i] == 0u ? 0u : 1u);
  };
  for (uint32_t i = 0; i < n; i++) {
    BrotliAmdUndbaSeg counting = segs[i];
    counting.cap = 0u;
    const DbaResult counted = brotli_amd_undba_host_walk(counting, item_deltas, nullptr, nullptr, &firsts_p[i], &firsts_s[i]);
    segs[i].cap = std::min<uint64_t>(caps[i], std::max(counted.count_p, counted.count_s) + 1u);
    segs[i].first_item = items.pre[i];
    items.pre[i + 1u] = items.pre[i] + brotli_amd_undbp_items(segs[i].cap, item_deltas);
    items.ckpts.resize(items.pre[i + 1u], BrotliAmdUndbpCheckpoint{BROTLI_AMD_UNDBP_NONE, BROTLI_AMD_UNDBP_NONE});
    ckpts_s.resize(items.pre[i + 1u], BrotliAmdUndbpCheckpoint{BROTLI_AMD_UNDBP_NONE, BROTLI_AMD_UNDBP_NONE});
    got[i] = brotli_amd_undba_host_walk(segs[i], item_deltas, items.ckpts.data() + items.pre[i], ckpts_s.data() + items.pre[i], &firsts_p[i], &firsts_s[i]);
    if (segs[i].offsets && slots_of(i) * brotli_amd_undlba_offset_width(segs[i].flags) > offsets_size - offsets_offs[i]) return outside_buffer(kUndba);
  }
  oroom.snapshot();
  droom.snapshot();
  // phases 2 to 5
  SeededOrder seeded(order_seed);
  const uint64_t all = items.pre.back();
  std::vector<BrotliAmdUndeltaTile> tiles_p(all), tiles_s(all), tiles_l(all), tiles_x(all);
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g) {
    brotli_amd_undba_host_sum(segs[i], got[i], cp, ckpts_s[g], firsts_p[i], firsts_s[i], j, item_deltas, &tiles_p[g], &tiles_s[g]);
  });
  const std::vector<uint64_t> carries_p = carries_of(tiles_p), carries_s = carries_of(tiles_s);
  auto item_of = [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g) {
    return brotli_amd_undba_host_item(segs[i], got[i], cp, ckpts_s[g], firsts_p[i], firsts_s[i], j, item_deltas, carries_p[g], carries_s[g]);
  };
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g) {
    brotli_amd_undba_host_lengths(item_of(i, cp, j, g), j, &got[i], &tiles_l[g], &tiles_x[g]);
  });
  const std::vector<uint64_t> carries_l = carries_of(tiles_l), carries_x = carries_of(tiles_x);
  // what item g, whose first element is lo, has in front of it of L and of s
  auto sums_in = [&](uint32_t i, uint64_t g, uint64_t lo, uint64_t* bytes_in, uint64_t* suffix_in) {
    const uint64_t fb = got[i].first_bad, gb = lo > fb ? items.pre[i] + brotli_amd_undba_item_of(fb, item_deltas) : g;
    *bytes_in = brotli_amd_undba_sum_in(fb, lo, carries_l[g], carries_l[gb], tiles_l[gb].sum);
    *suffix_in = brotli_amd_undba_sum_in(fb, lo, carries_x[g], carries_x[gb], tiles_x[gb].sum);
  };
  // phase 6
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g) {
    const BrotliAmdUndbaHostItem it = item_of(i, cp, j, g);
    uint64_t bytes_in, suffix_in;
    sums_in(i, g, it.lo, &bytes_in, &suffix_in);
    brotli_amd_undba_host_expand(segs[i], &got[i], it, j, item_deltas, bytes_in, suffix_in);
  });
  std::vector<uint64_t> kept(n, 0u);   // the bytes of every segment that its data capacity leaves
  for (uint32_t i = 0; i < n; i++) {
    kept[i] = segs[i].cap != 0u ? brotli_amd_undba_keep(segs[i], got[i].bytes) : 0u;
    if (kept[i] > data_size - (segs[i].data ? data_offs[i] : 0u)) return outside_buffer(kUndba);
  }
  // phases 7 to 9
  std::vector<BrotliAmdUndbaLast> lasts(all, BrotliAmdUndbaLast{0u, 0u, 0u});
  std::vector<uint8_t> string(brotli_amd_undba_lds_string()), carried(brotli_amd_undba_lds_carry());
  auto lens_of = [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g, uint64_t* bytes_in, uint64_t* suffix_in) {
    const BrotliAmdUndbaHostItem it = item_of(i, cp, j, g);
    sums_in(i, g, it.lo, bytes_in, suffix_in);
    return brotli_amd_undba_host_lens(it, got[i].first_bad);
  };
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g) {
    if (kept[i] == 0u) return;
    uint64_t bytes_in, suffix_in;
    const BrotliAmdUndbaHostLens lens = lens_of(i, cp, j, g, &bytes_in, &suffix_in);
    lasts[g] = brotli_amd_undba_host_a((uint64_t)(uintptr_t)segs[i].data, kept[i], (uint64_t)(uintptr_t)segs[i].src + got[i].consumed_p + got[i].consumed_s, got[i].data_avail,
                                       lens.p.data(), lens.s.data(), (uint32_t)lens.p.size(), bytes_in, suffix_in, string.data(), (uint32_t)string.size());
  });
  std::vector<uint64_t> order = first_numbers(n);
  seeded.shuffle(&order);
  for (uint64_t i : order)
    if (kept[i] != 0u)
      brotli_amd_undba_host_b((uint64_t)(uintptr_t)segs[i].data, kept[i], lasts.data() + items.pre[i], items.pre[i + 1u] - items.pre[i], carried.data(), (uint32_t)carried.size());
  items.shuffled(&seeded, [&](uint32_t i, BrotliAmdUndbpCheckpoint cp, uint64_t j, uint64_t g) {
    if (kept[i] == 0u || j == 0u) return;
    uint64_t bytes_in, suffix_in;
    const BrotliAmdUndbaHostLens lens = lens_of(i, cp, j, g, &bytes_in, &suffix_in);
    brotli_amd_undba_host_c((uint64_t)(uintptr_t)segs[i].data, kept[i], lasts[g - 1u], lens.p.data(), lens.s.data(), (uint32_t)lens.p.size(), bytes_in);
  });
  // no byte outside every segment's offsets and bytes may have changed
  std::vector<uint8_t> in_offsets(offsets_size, 0), in_data(data_size, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (segs[i].offsets) std::fill(in_offsets.begin() + offsets_offs[i], in_offsets.begin() + offsets_offs[i] + slots_of(i) * brotli_amd_undlba_offset_width(segs[i].flags), 1);
    if (segs[i].data) std::fill(in_data.begin() + data_offs[i], in_data.begin() + data_offs[i] + kept[i], 1);
  }
  if (!oroom.changed_inside_only([&](size_t i) { return i < offsets_size && in_offsets[i]; })) { g_last_error = "undba wrote outside its offsets"; return -2; }
  if (!droom.changed_inside_only([&](size_t i) { return i < data_size && in_data[i]; })) { g_last_error = "undba wrote outside its data"; return -2; }
  oroom.get(offsets, 0u, offsets_size);
  droom.get(data, 0u, data_size);
  std::copy(got.begin(), got.end(), results);
  return 0;
}
