// Host <-> kernel contract of the batch decoder (plain C structs, no HIP types).
//
// One StreamDesc per .br stream, one StreamStatus written back per stream.  A stream is the unit of
// work the reference calls "one BrotliState" (src/state.rs:156-278): its own window, distance ring and
// output.  Streams never share anything, so a batch partitions freely over wavefronts and over GPUs.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// flags
#define BROTLI_AMD_FLAG_LARGE_WINDOW 1u  // accept the 14-bit large-window header (state.rs:394, ffi/mod.rs:127)
#define BROTLI_AMD_FLAG_NO_CANNY 2u      // BROTLI_DECODER_PARAM_DISABLE_RING_BUFFER_REALLOCATION (ffi/mod.rs:167-169)
#define BROTLI_AMD_FLAG_RESUME 4u        // start from the metablock boundary stored in `resume`
#define BROTLI_AMD_FLAG_NO_SPILL 8u      // a metablock whose tables do not fit the LDS arena ends the decode with result
                                         // BROTLI_AMD_RESULT_RETRY_ARENA at the boundary before it (the host then
                                         // resumes the stream in a launch with a larger arena) instead of spilling
#define BROTLI_AMD_FLAG_ENGINE_ONLY 32u  // set by the host where sixteen-wave blocks (one per CU) serve more streams than
                                         // there are CUs: a large metablock the command engine cannot take (literals that
                                         // depend on context) ends the decode the same way, and the stream continues in a
                                         // launch of small blocks, several to a CU -- one wave decodes such a metablock
                                         // wherever it runs, so what counts for it is streams in flight
#define BROTLI_AMD_FLAG_PROBE 128u       // nothing is decoded: the stream's header is read up to the literal context map of its first compressed
                                         // metablock, and the status says what kind of stream this is (result BROTLI_AMD_RESULT_PROBE,
                                         // engine_commands = bit 0: such a metablock exists, bit 1: its literals do not depend on context,
                                         // bit 2: it is large enough for a command engine): the host picks the launch shape by it
#define BROTLI_AMD_FLAG_DEFER 256u       // the stream is not this launch's: reported as BROTLI_AMD_RESULT_RETRY_ARENA at once (it is decoded, from
                                         // its first byte, in the launch of small blocks that follows)
#define BROTLI_AMD_RESULT_RETRY_ARENA 4  // (never reaches the caller of the C ABI)
#define BROTLI_AMD_RESULT_PROBE 5        // (never reaches the caller of the C ABI)
#define BROTLI_AMD_GANG_POOL_FLAG 0x100u  // queue[2] of a POOL launch (with 8 in the low bits: the blocks a stream may gather); a gang launch: 2, 4, 8 or 16 blocks a stream
#define BROTLI_AMD_GANG_CTL_BYTES 50176u // a gang's control block in memory, one per stream of a gang launch (brotli_kernels.hip: GC_*): queue[2] = blocks of a
                                         // gang (0 or 1: none), queue[4], queue[5] = the address of the first stream's block, the host zeroes them before the launch
#define BROTLI_AMD_SPEC_SCRATCH 65536u   // bytes at the end of each block's global scratch that the helper waves use for
                                         // speculatively decoded literals (the table arena is the part in front of it)

// State at a metablock boundary: everything that survives from one metablock to the next in the
// reference (state.rs:422-450 resets the rest).  The kernel stores it after every completed metablock;
// the streaming ABI feeds it back so that a stream delivered in pieces is decoded metablock by metablock
// instead of from byte 0 (the device analogue of the reference's resumable state machine).
typedef struct BrotliAmdResume {
  uint64_t bit_pos;       // absolute bit position in the compressed stream
  uint64_t out_pos;       // bytes produced so far
  int32_t dist_rb[4];     // last four distances, most recent first (state.rs:295-296 as a shift register)
  int32_t dist_rb_idx;    // unused (always 0): the ring is stored already rotated
  uint32_t window_bits;   // 0 = stream header not parsed yet
  uint32_t large_window;  // stream carries the large-window header
  uint32_t rb_size_log2;  // emulated ring size (0 = not allocated yet), decode.rs:1808-1871
  uint32_t is_last_done;  // last metablock completed (stream finished up to the final padding)
  uint32_t reserved;
  // A command boundary inside the metablock that starts at bit_pos (mid_valid != 0): where a launch that ran out of
  // input had got to.  The next launch parses that metablock's header again (the prefix codes are not kept) and goes
  // on from here instead of from the metablock's first command, so a stream fed in small pieces costs what its bytes
  // cost, not (pieces x metablock).  The reference keeps the same things across calls in its state (state.rs:255-330:
  // block lengths and types, distance ring, meta_block_remaining_len, the bit reader).
  uint32_t mid_valid;
  int32_t mid_mlen;        // bytes of the metablock still to be produced
  uint64_t mid_bit_pos;    // bit position of the next command
  uint64_t mid_out_pos;    // bytes produced in front of it
  uint32_t mid_bl[3];      // literals / commands / distances left in the current blocks
  uint32_t mid_types[6];   // second last and last block type, per category (state.rs:429-435)
  int32_t mid_dist_rb[4];  // last four distances, most recent first
  uint32_t mid_reserved;
} BrotliAmdResume;

typedef struct BrotliAmdStreamDesc {
  const uint8_t* in;      // device pointer, any alignment
  uint64_t in_size;
  uint8_t* out;           // device pointer
  uint64_t out_cap;
  uint32_t flags;
  uint32_t reserved;
  BrotliAmdResume resume; // only read when BROTLI_AMD_FLAG_RESUME is set
  // Custom (LZ77 prefix) dictionary (state.rs:400-411): device pointer and size, 0 = none.  Its bytes lie in front of output
  // position 0 for back-references only -- the kernel reads position v < 0 at dict + dict_size + v; nothing else sees them
  // (the first two literals' context is (0, 0): decode.rs:2466-2476).  Streams of one launch may name the same dictionary,
  // different ones or none; every launch of a stream (resumed, larger arena, second decode into scratch) names it again.
  const uint8_t* dict;
  uint64_t dict_size;
} BrotliAmdStreamDesc;

typedef struct BrotliAmdStreamStatus {
  int32_t result;         // BrotliResult: 0 error, 1 success, 2 needs more input, 3 needs more output
  int32_t error_code;     // BrotliDecoderErrorCode (state.rs:22-65)
  uint64_t decoded_size;  // bytes the reference would have delivered to the caller (lib.rs:466)
  uint64_t consumed;      // input bytes consumed
  uint64_t produced;      // bytes written to `out` (>= decoded_size on errors)
  uint32_t num_metablocks;
  uint32_t spilled_metablocks;  // metablocks whose tables did not fit the LDS part of the arena
  uint64_t num_commands;
  BrotliAmdResume resume; // last completed metablock boundary
  // What the reference's three allocators would have been asked for (BrotliDecoderDecompressPrealloc accounts its scratch
  // slices with these): prefix codes alive in one metablock at most (each BROTLI_HUFFMAN_MAX_TABLE_SIZE HuffmanCode cells
  // and one u32, huffman/mod.rs:61-72), bytes of context modes and maps alive in one metablock at most (decode.rs:1295,
  // 3155), the emulated ring buffer (decode.rs:1843-1855), and whether any compressed metablock was started (the block
  // type and block length trees, decode.rs:2958-2969)
  uint32_t peak_trees, peak_map_bytes, any_compressed;
  uint32_t engine_commands;  // of num_commands, how many a command engine took (blocks of sixteen waves): lets tests prove which path ran
  uint64_t ring_bytes;
} BrotliAmdStreamStatus;

// One segment of a ragged copy (csrc/brotli_copy_kernels.hip): len bytes from src to dst, device addresses of any alignment, len 0 included.
// The segments of one launch do not overlap each other.  Nothing outside [dst, dst + len) is written; nothing outside the 16-byte-aligned
// span around [src, src + len) is read.
typedef struct BrotliAmdCopySeg {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t len;
} BrotliAmdCopySeg;
#define BROTLI_AMD_COPY_TILE_BYTES 16384u  // destination bytes of one tile: the blocks of a launch take the segments' bytes tile by tile

// One segment of an unshuffle launch (csrc/brotli_unshuffle_kernels.hip, csrc/brotli_unshuffle.h): the len bytes at src are `width` byte planes
// (and len % width left-over bytes), the len bytes at dst become the elements; device addresses of any alignment, len 0 included, width 1, 2, 4
// or 8.  No destination range overlaps a source range or another destination range.  Nothing outside [dst, dst + len) is written; nothing
// outside the 16-byte-aligned span around [src, src + len) is read.  `param` is the one parameter a filter has beside the width: 0 for unshuffle
// and undelta, bit-unshuffle's block size, bit-unpack's field width and flags (below).
typedef struct BrotliAmdUnshuffleSeg {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t len;
  uint32_t width;
  uint32_t param;
} BrotliAmdUnshuffleSeg;
#define BROTLI_AMD_UNSHUFFLE_TILE_BYTES 16384u  // destination bytes of one tile

// An undelta call (csrc/brotli_undelta_kernels.hip, csrc/brotli_undelta.h) takes the segments of an unshuffle launch -- here len bytes of deltas
// at src become len bytes of values at dst; dst == src is allowed at a multiple of width -- and cuts their destination into tiles of
#define BROTLI_AMD_UNDELTA_TILE_BYTES 16384u  // destination bytes: a tile's carry-in comes from the tiles in front of it

// A bit-unshuffle launch (csrc/brotli_bitunshuffle_kernels.hip, csrc/brotli_bitunshuffle.h) takes the segments of an unshuffle launch too -- here
// the len bytes at src are blocks of 8 `width` bit rows -- with the block size in elements in `param` (0: one block; otherwise a multiple of
// 8).  A fast item of that kernel is 2 `width` words, so its tile is larger: sixteen words a thread.
#define BROTLI_AMD_BITUNSHUFFLE_TILE_BYTES 65536u  // destination bytes of one tile

// A bit-unpack launch (csrc/brotli_bitunpack_kernels.hip, csrc/brotli_bitunpack.h) takes the segments of an unshuffle launch as well, with one
// difference: `len` is the DESTINATION's bytes -- m elements of `width` bytes, m `width` --, and the units are the destination's; the source is
// the ceil(m k / 8) bytes at src that hold m fields of k bits.  `param` is k | flags << 8 (k: 1 .. 8 `width`; flags: bit 0 MSB-first, bit 1
// sign-extended).  A fast item of that kernel is 2 `width` words too, so it has the bit-unshuffle's tile: sixteen words a thread.
#define BROTLI_AMD_BITUNPACK_TILE_BYTES 65536u  // destination bytes of one tile

// One segment of an unvarint call (csrc/brotli_unvarint_kernels.hip, csrc/brotli_unvarint.h): the len bytes at src are LEB128 varints, and the
// first `cap` of them become elements of `width` bytes (1, 2, 4 or 8) at dst, by `flags` (bit 0: zigzag); device addresses of any alignment,
// len 0 and cap 0 included (cap 0: dst is not looked at).  The number of elements depends on the bytes, so the units are the words of SOURCE
// memory, and every segment has a result (BrotliAmdUnvarintResult, include/brotli/batch.h) behind the table.  No destination range overlaps a
// source range or another destination range.  Nothing outside [dst, dst + min(count, cap) width) is written; nothing outside the
// 16-byte-aligned span around [src, src + len) is read.
typedef struct BrotliAmdUnvarintSeg {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t len;
  uint64_t cap;
  uint32_t width;
  uint32_t flags;
} BrotliAmdUnvarintSeg;
#define BROTLI_AMD_UNVARINT_TILE_BYTES 16384u  // source bytes of one tile: a tile's carry-in is the number of varints that end in front of it

// One segment of an unrle call (csrc/brotli_unrle_kernels.hip, csrc/brotli_unrle.h): the len bytes at src are runs of the RLE / bit-packed
// hybrid with fields of `bits` bits (0 .. 32), and the first `cap` of their values become elements of `width` bytes (1, 2, 4 or 8) at dst, by
// `flags` (bit 0: the segment's first byte is the field width); device addresses of any alignment, len 0 and cap 0 included (cap 0: dst is not
// looked at).  The destination is cut into ITEMS of BROTLI_AMD_UNRLE_ITEM_ELEMS elements; first_item is the number of items of the segments in
// front of this one, so a call's units are one a segment -- its walk -- and one an item.  Every segment has a result (BrotliAmdUnrleResult,
// include/brotli/batch.h) and every item a checkpoint behind the table.  No destination range overlaps a source range or another destination
// range.  Nothing outside [dst, dst + min(count, cap) width) is written; nothing outside the 16-byte-aligned span around [src, src + len) is read.
typedef struct BrotliAmdUnrleSeg {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t len;
  uint64_t cap;
  uint64_t first_item;
  uint32_t width;
  uint32_t bits;
  uint32_t flags;
  uint32_t reserved;
} BrotliAmdUnrleSeg;
#define BROTLI_AMD_UNRLE_ITEM_ELEMS 1024u  // elements of one item of the expansion: a wave's share of a destination
#define BROTLI_AMD_UNRLE_WALK_CHUNK 1024u  // source bytes that a wave stages in LDS at a time: one 16-byte load a lane

// One segment of an undbp call (csrc/brotli_undbp_kernels.hip, csrc/brotli_undbp.h): the len bytes at src are a DELTA_BINARY_PACKED stream, and
// the first `cap` of its values become elements of `width` bytes (1, 2, 4 or 8) at dst; device addresses of any alignment, len 0 and cap 0
// included (cap 0: dst is not looked at).  The deltas are cut into ITEMS of BROTLI_AMD_UNDBP_ITEM_DELTAS deltas; first_item is the number of
// items of the segments in front of this one, so a call's units are one a segment -- its walk -- and one an item.  Every segment has a result
// (BrotliAmdUndbpResult, include/brotli/batch.h) and its first value behind the table, and every item a checkpoint, a tile record and a carry.
// No destination range overlaps a source range or another destination range.  Nothing outside [dst, dst + min(count, cap) width) is written;
// nothing outside the 16-byte-aligned span around [src, src + len) is read.
typedef struct BrotliAmdUndbpSeg {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t len;
  uint64_t cap;
  uint64_t first_item;
  uint32_t width;
  uint32_t reserved;
} BrotliAmdUndbpSeg;
#define BROTLI_AMD_UNDBP_ITEM_DELTAS 2048u  // deltas of one item: 64 groups of 32 fields, a group a lane

// One segment of an undict call (csrc/brotli_undict_kernels.hip, csrc/brotli_undict.h): an unrle segment whose values are INDICES into the
// dict_entries entries of `width` bytes at dict, device memory of any alignment; the first `cap` of the entries they name become the elements
// at dst, and an index at or above dict_entries gives 0 and is counted.  `bits` is bound by 32 alone.  Items, first_item and the checkpoints
// are unrle's; every segment has a result (BrotliAmdUndictResult, include/brotli/batch.h) behind the table, whose bad and first_bad the items
// add to.  No destination range overlaps a source range, a dictionary or another destination range.  Nothing outside
// [dst, dst + min(count, cap) width) is written; nothing outside the 16-byte-aligned spans around [src, src + len) and
// [dict, dict + dict_entries width) is read.
typedef struct BrotliAmdUndictSeg {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t len;
  uint64_t cap;
  uint64_t first_item;
  uint32_t width;
  uint32_t bits;
  uint32_t flags;
  uint32_t reserved;
  const uint8_t* dict;
  uint64_t dict_entries;
} BrotliAmdUndictSeg;

// One segment of an unnull call (csrc/brotli_unnull_kernels.hip, csrc/brotli_unnull.h): the len bytes at src are unrle runs of DEFINITION
// LEVELS of `bits` bits -- behind a 4-byte length with flag bit 0 --, and the first `cap` of them become slots of `width` bytes at dst and
// validity bits at valid (NULL: no bitmap): a slot whose level is `level` gets the next of the values_count dense values at `values` -- with
// flag bit 1 what lies behind the runs in the segment itself --, every other slot 0.  Device addresses of any alignment.  Items, first_item and
// the checkpoints are unrle's; every segment has a result (BrotliAmdUnnullResult, include/brotli/batch.h) and its runs' length behind the
// table, and every item a checkpoint, a tile record and a carry.  No destination or bitmap range overlaps a source range, a values range or
// another destination or bitmap range.  Nothing outside [dst, dst + min(count, cap) width) and [valid, valid + ceil(min(count, cap) / 8)) is
// written; nothing outside the 16-byte-aligned spans around [src, src + len) and [values, values + values_count width) is read.
typedef struct BrotliAmdUnnullSeg {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t len;
  uint64_t cap;
  uint64_t first_item;
  uint32_t width;
  uint32_t bits;
  uint32_t flags;
  uint32_t level;
  const uint8_t* values;
  uint64_t values_count;
  uint8_t* valid;
} BrotliAmdUnnullSeg;

// One segment of an undict-bytes call (csrc/brotli_undict_bytes_kernels.hip, csrc/brotli_undict_bytes.h): an unrle segment whose values are
// INDICES into a dictionary of PLAIN byte arrays -- record `dict` of the call's table of distinct dictionaries (BROTLI_AMD_UNDICT_BYTES_NO_DICT:
// none, cap is 0) --; the first `cap` of the entries they name become an Arrow string column: their running byte offsets on top of offset_base at
// `offsets` (NULL: none), 4 bytes each or 8 by flags, and their bytes one behind the other at `data`, cut at data_cap.  Items, first_item and the
// checkpoints are unrle's; every segment has a result (BrotliAmdUndictBytesResult, include/brotli/batch.h) behind the table, and every item a
// checkpoint, a tile record and a carry.  No destination range overlaps a source range, a dictionary or another destination range.  Nothing
// outside [data, data + min(bytes, data_cap)) and the offsets that batch.h names is written; nothing outside the 16-byte-aligned spans around
// [src, src + len) and the dictionary is read.
typedef struct BrotliAmdUndictBytesSeg {
  const uint8_t* src;
  uint8_t* data;
  uint64_t len;
  uint64_t cap;
  uint64_t first_item;
  uint32_t dict;
  uint32_t bits;
  uint32_t flags;
  uint32_t reserved;
  uint8_t* offsets;
  uint64_t data_cap;
  uint64_t offset_base;
} BrotliAmdUndictBytesSeg;
#define BROTLI_AMD_UNDICT_BYTES_NO_DICT 0xFFFFFFFFu

// One DISTINCT dictionary of such a call: `len` bytes (below 2^32) at `dict`, device memory of any alignment, of which at most `bound` entries
// are taken; first_start is where its entries' positions begin in the call's array of them, min(bound, len / 4) + 1 of them.  The records lie
// behind the segments in the call's table; every record has a result (BrotliAmdUndictBytesDictResult, csrc/brotli_undict_bytes.h) in the scratch.
typedef struct BrotliAmdUndictBytesDict {
  const uint8_t* dict;
  uint64_t len;
  uint64_t bound;
  uint64_t first_start;
} BrotliAmdUndictBytesDict;

// One segment of an undlba call (csrc/brotli_undlba_kernels.hip, csrc/brotli_undlba.h): the len bytes at src are a DELTA_BINARY_PACKED stream
// of lengths and, directly behind it, the values' bytes; the first `cap` lengths become an Arrow string column: their running sums on top of
// offset_base at `offsets` (NULL: none), 4 bytes each or 8 by flags, and the bytes one behind the other at `data` (NULL: none), cut at
// data_cap.  Items, first_item and the checkpoints are undbp's; every segment has a result (BrotliAmdUndlbaResult, include/brotli/batch.h), its
// first value and an entry of the table of copies behind the table, and every item a checkpoint, two tile records and two carries.  No
// destination range overlaps a source range or another destination range.  Nothing outside [data, data + min(bytes, data_avail, data_cap))
// and the offsets that batch.h names is written; nothing outside the 16-byte-aligned span around [src, src + len) is read.
typedef struct BrotliAmdUndlbaSeg {
  const uint8_t* src;
  uint8_t* data;
  uint64_t len;
  uint64_t cap;
  uint64_t first_item;
  uint32_t flags;
  uint32_t reserved;
  uint8_t* offsets;
  uint64_t data_cap;
  uint64_t offset_base;
} BrotliAmdUndlbaSeg;

// One segment of an undba call (csrc/brotli_undba_kernels.hip, csrc/brotli_undba.h) has undlba's fields with undlba's meanings: the len bytes
// at src are a DELTA_BINARY_PACKED stream of prefix lengths, one of suffix lengths directly behind it, and the suffix bytes behind that.  Items
// and first_item are undbp's, for both streams alike; behind the table every segment has a result (BrotliAmdUndbaResult, include/brotli/batch.h),
// both streams as undbp segments and undbp results, and two first values, and every item two checkpoints, four tile records, four carries and
// the record of its last element.  No destination range overlaps a source range or another destination range.  Nothing outside
// [data, data + min(bytes, data_cap)) and the offsets that batch.h names is written; nothing outside the 16-byte-aligned span around
// [src, src + len) and the call's own destinations is read.
typedef BrotliAmdUndlbaSeg BrotliAmdUndbaSeg;
// What phase A leaves of an item for phases B and C: its LAST element's place in the segment's data, its length and r = min(p) over the item.
typedef struct BrotliAmdUndbaLast {
  uint64_t at;
  uint32_t len;
  uint32_t r;
} BrotliAmdUndbaLast;

#ifdef __cplusplus
}
#endif
