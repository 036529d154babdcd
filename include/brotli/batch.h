/* brotli/batch.h -- batch extension of the C ABI: many independent .br streams per call.
 *
 * Not in the reference: its API decodes one stream per BrotliState (src/state.rs:156-278).  A GPU only
 * pays off when many streams decode at once, so the same decode path is also exposed in batch form.  The
 * per-stream outcome has exactly the meaning of the reference's one-shot return info (src/lib.rs:336-370):
 * result, error code and the number of bytes the reference would have delivered.
 *
 * Threading: a batch object may be used by one thread at a time; different batch objects are independent.
 * One batch object is bound to the HIP device that was current when it was created.
 */
#ifndef BROTLI_AMD_BATCH_H_
#define BROTLI_AMD_BATCH_H_

#include <stddef.h>
#include <stdint.h>

#include "decode.h" /* BrotliDecoderResult, the states of a stream set */

#if defined(__cplusplus)
extern "C" {
#endif

#ifndef BROTLI_DEC_API
#define BROTLI_DEC_API __attribute__((visibility("default")))
#endif

typedef struct BrotliAmdBatch BrotliAmdBatch;

/* per-stream outcome (same fields as BrotliAmdStreamStatus without the resume block) */
typedef struct BrotliAmdResult {
  int32_t result;        /* BrotliDecoderResult */
  int32_t error_code;    /* BrotliDecoderErrorCode */
  uint64_t decoded_size; /* bytes delivered (reference: BrotliDecoderReturnInfo.decoded_size) */
  uint64_t consumed;     /* input bytes consumed */
  uint64_t produced;     /* bytes written to the output buffer (>= decoded_size after an error) */
  uint32_t num_metablocks;
  uint32_t spilled_metablocks; /* metablocks whose tables did not fit the LDS arena (slower path; raise lds_arena_bytes) */
  uint64_t num_commands;
  uint32_t engine_commands;    /* of num_commands, how many a command engine took (blocks of sixteen waves, one stream a CU) */
  uint32_t reserved;
} BrotliAmdResult;

#define BROTLI_AMD_BATCH_LARGE_WINDOW 1u /* accept large-window streams (reference one-shot default, lib.rs:457) */
#define BROTLI_AMD_BATCH_NO_CANNY 2u     /* BROTLI_DECODER_PARAM_DISABLE_RING_BUFFER_REALLOCATION */
#define BROTLI_AMD_BATCH_SPILL_IN_PLACE 16u /* no second launch with a larger LDS arena for streams whose prefix-code tables
                                              do not fit the arena of the first: they spill to global memory (slower) */
#define BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT 64u /* A stream whose output buffer is too small is reported NEEDS_MORE_OUTPUT as soon
                                              as the buffer is full.  Without this flag such streams get the reference's
                                              verdict: the reference decodes into its ring buffer and only notices the full
                                              buffer at the next flush point (decode.rs:1693-1738), so an error or the end of
                                              the input in front of that point is what it reports; the batch decodes those
                                              streams a second time, into scratch memory with room up to that point (up to
                                              one window per stream, 2 GiB at a time), inside BrotliAmdBatchWait. */

/* Creates a batch context on the current HIP device for up to max_streams streams per call.
 * lds_arena_bytes = 0 and grid_blocks = 0 select the defaults.  NULL when no device is usable. */
BROTLI_DEC_API BrotliAmdBatch* BrotliAmdBatchCreate(uint32_t max_streams, uint32_t lds_arena_bytes, uint32_t grid_blocks);
BROTLI_DEC_API void BrotliAmdBatchDestroy(BrotliAmdBatch* batch);

/* Decodes n streams whose compressed bytes and output buffers already live in DEVICE memory.
 * d_in[i]/d_out[i] are device pointers (any alignment).  The launch is asynchronous on hip_stream
 * (a hipStream_t, NULL = default stream); call BrotliAmdBatchWait before reading results.
 * One case is NOT asynchronous: a batch of more streams than the device has compute units and at most four times as many, of a mean
 * compressed size of 8 KiB or more, is PROBED first -- a short launch that reads every stream's header and tells the host which streams
 * the command engines can take -- and the call waits on hip_stream for its answer (some tens of microseconds of kernel; it cannot be
 * captured into a graph).  The answer is kept with the batch object: the same descriptors again (pointers, sizes, flags) are not probed
 * again, and BrotliAmdBatchRelaunch never probes.  BrotliAmdBatchLastProbeMs says what the last call spent there.
 * Returns 0 on success, a negative value if the arguments or the device are unusable. */
BROTLI_DEC_API int BrotliAmdBatchDecodeDevice(BrotliAmdBatch* batch, uint32_t n, const void* const* d_in, const size_t* in_sizes,
                                             void* const* d_out, const size_t* out_caps, uint32_t flags, void* hip_stream);

/* Re-launches the decode of the streams described by the previous BrotliAmdBatchDecodeDevice call
 * (descriptors stay resident in device memory); used to time the kernel with inputs already in HBM. */
BROTLI_DEC_API int BrotliAmdBatchRelaunch(BrotliAmdBatch* batch, void* hip_stream);

/* Waits for the last launch and copies the per-stream results to the host. */
BROTLI_DEC_API int BrotliAmdBatchWait(BrotliAmdBatch* batch, BrotliAmdResult* results /* n entries, may be NULL */);

/* Convenience for host buffers: upload, decode, download.  Same per-stream semantics. */
BROTLI_DEC_API int BrotliAmdBatchDecodeHost(BrotliAmdBatch* batch, uint32_t n, const uint8_t* const* in, const size_t* in_sizes,
                                           uint8_t* const* out, const size_t* out_caps, uint32_t flags, BrotliAmdResult* results);

/* Custom (LZ77 prefix) dictionaries -- the batch form of the reference's BrotliDecompressCustomDict (src/lib.rs:101, 202) and
 * BrotliState::new_with_custom_dictionary (src/state.rs:400-411).  BrotliAmdBatchDecodeDevice plus, per stream, a DEVICE pointer to its
 * dictionary and its size: d_dicts == NULL, dict_sizes == NULL, d_dicts[i] == NULL or dict_sizes[i] == 0 mean no dictionary for that
 * stream, and a call without any is BrotliAmdBatchDecodeDevice exactly.  Streams of one call may name the same dictionary (the rule: thousands
 * of small documents against one shared dictionary, which the device then reads out of its caches), different ones or none; the
 * dictionaries are only read and must stay where they are until BrotliAmdBatchWait has returned (and through every BrotliAmdBatchRelaunch,
 * which keeps them).  A dictionary's bytes lie in front of output position 0 for back-references alone; one longer than the stream's window
 * counts with its last (1 << window_bits) - 16 bytes (decode.rs:1831-1839).  Result, error code, decoded_size and every output byte are the
 * reference's with that dictionary.  Same asynchrony and the same probe rule; the probe's memory of a batch includes the dictionaries.
 * Launch shapes are PLANNED as for the same batch without dictionaries -- gangs and pools included (BrotliAmdBatchLastGang, BrotliAmdBatchLastPool say
 * what they say without).  A command whose copy starts in the dictionary is always decoded by the block that owns its stream: a gang stops in
 * front of it and is invoked again behind it, so while a stream's window still reaches its dictionary the helper blocks have work only between
 * such commands. */
BROTLI_DEC_API int BrotliAmdBatchDecodeDeviceDict(BrotliAmdBatch* batch, uint32_t n, const void* const* d_in, const size_t* in_sizes,
                                                 void* const* d_out, const size_t* out_caps, const void* const* d_dicts,
                                                 const size_t* dict_sizes, uint32_t flags, void* hip_stream);

/* The same for host buffers: BrotliAmdBatchDecodeHost plus per-stream HOST pointers to the dictionaries.  Each distinct (pointer, size)
 * pair is uploaded once per call, not once per stream. */
BROTLI_DEC_API int BrotliAmdBatchDecodeHostDict(BrotliAmdBatch* batch, uint32_t n, const uint8_t* const* in, const size_t* in_sizes,
                                               uint8_t* const* out, const size_t* out_caps, const uint8_t* const* dicts,
                                               const size_t* dict_sizes, uint32_t flags, BrotliAmdResult* results);

/* ---- Batches whose decoded sizes are NOT known: size hints and the packed decode ----
 *
 * Every entry point above takes out_caps[]: the caller has to know how large each stream decodes, and Brotli has no size field.  The two
 * calls below lift that.
 *
 * THE SIZE WALK.  A stream's headers say more than one would guess (csrc/brotli_size_walk.h): metadata and stored metablocks carry their own
 * byte lengths, so they can be stepped over, and the first compressed metablock states its MLEN and ISLAST in front of its prefix codes.
 * The walk reads the stream header (every WBITS encoding; the 14-bit large-window form with BROTLI_AMD_BATCH_LARGE_WINDOW), then metablock
 * headers, and stops at the first compressed metablock, at an empty last metablock, at the end of the input or at a header the decoder
 * rejects (a reserved bit, an exuberant nibble or meta nibble, non-zero padding, invalid window bits).  No prefix code is decoded.
 *
 * The contract of a hint is weak on purpose -- the packed decode's correctness never depends on it:
 *   - `bytes` is a LOWER BOUND on the decoded size of every stream that decodes successfully;
 *   - it is the exact size where exact == 1 && status == 0 (of such a stream);
 *   - status == 2 only where the decoder reports an error;
 *   - the walk need not find every error. */
typedef struct BrotliAmdSizeHint {
  uint64_t bytes;      /* sum of MLEN over every stored metablock walked, plus MLEN of the first compressed one reached */
  uint64_t walked_in;  /* input bytes in front of the point where the walk stopped: the header of the compressed metablock reached or of the
                          metablock the walk could not finish; behind the last metablock where the walk reached the stream's end */
  uint32_t exact;      /* 1: the walk reached the stream's last metablock, so nothing can follow `bytes` */
  uint32_t status;     /* 0 ok, 1 the input ended inside the walk, 2 a header the decoder rejects */
} BrotliAmdSizeHint;

/* The hints of n streams in DEVICE memory (d_in[i]: any alignment) by one launch of one lane a stream (csrc/brotli_size_kernels.hip) on
 * hip_stream; the call waits on that stream and copies the hints to `hints` (host, n entries).  n is not bound by the batch object's
 * max_streams.  flags: BROTLI_AMD_BATCH_LARGE_WINDOW.  n == 0 returns 0; in_sizes[i] == 0 gives {0, 0, 0, 1}.  Negative on failure. */
BROTLI_DEC_API int BrotliAmdBatchSizeHints(BrotliAmdBatch* batch, uint32_t n, const void* const* d_in, const size_t* in_sizes,
                                          uint32_t flags, BrotliAmdSizeHint* hints, void* hip_stream);

/* Test hook (no device needed): the same function on the host, over n bytes at `in`.  Returns 0; negative for NULL arguments. */
BROTLI_DEC_API int BrotliAmdDebugSizeWalk(const uint8_t* in, size_t n, uint32_t flags, BrotliAmdSizeHint* hint);

/* THE PACKED DECODE: n streams in DEVICE memory, no output buffers and no sizes from the caller.  The library sizes, allocates, decodes --
 * growing what it guessed too small -- and leaves all outputs back to back in ONE device buffer of its own.
 *
 * The contract:
 *   - the call is synchronous: everything is decoded when it returns;
 *   - result, error_code, decoded_size, consumed and produced of results[i] are what BrotliAmdBatchDecodeDevice(Dict) reports for the same
 *     stream with out_caps[i] = max_out_bytes and flags | BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT -- with max_out_bytes == 0: with a buffer large
 *     enough that no stream ends NEEDS_MORE_OUTPUT.  (The counters -- num_metablocks, num_commands, engine_commands, spilled_metablocks -- are
 *     sums over the launches a stream took: a stream that had to grow decodes the metablock it stopped in a second time.)
 *   - stream i's delivered bytes are [offsets[i], offsets[i + 1]) of BrotliAmdBatchPackedOutput's buffer; the packing is tight:
 *     offsets[i + 1] - offsets[i] == results[i].decoded_size, and no alignment padding sits between streams;
 *   - the buffer and the offsets stay valid until the next decode call on the batch object or BrotliAmdBatchDestroy;
 *   - where a hipMalloc fails the call as a whole fails: a negative value, BrotliAmdLastError says why, and there are no partial results
 *     (BrotliAmdBatchPackedOutput then returns NULL).  n > max_streams and NULL arrays fail the same way; n == 0 returns 0.
 * d_dicts / dict_sizes: custom dictionaries as in BrotliAmdBatchDecodeDeviceDict (NULL: none).  max_out_bytes: per stream, 0 = no limit.
 * WITHOUT A LIMIT NOTHING BOUNDS THE GROWTH: a few hundred compressed bytes can state gigabytes of output, and a stream's slot is doubled until
 * it decodes or a hipMalloc fails (which fails the call).  Give input that is not trusted a max_out_bytes.
 * "The next decode call" is any of BrotliAmdBatchDecodeDevice(Dict), BrotliAmdBatchDecodeHost(Dict) and the packed calls on the same object, whatever it
 * returns: from its entry on BrotliAmdBatchPackedOutput returns NULL (offsets NULL), BrotliAmdBatchPackedFetch fails, and the two counters and
 * BrotliAmdBatchLastKernelMs no longer speak of the packed call.  After a packed call BrotliAmdBatchLastKernelMs is the time of all its decode launches
 * together; BrotliAmdBatchWait and BrotliAmdBatchRelaunch have nothing to come back to (0, and a failure).
 *
 * How a call runs:
 *  1. the size hints of all streams (above);
 *  2. each stream's first capacity: `bytes` where the hint is exact, else max(64 KiB, bytes + 6 x (in_size - walked_in)) -- the streaming
 *     decoder's first guess for input it has not seen decoded --, clamped to max_out_bytes;
 *  3. the slots lie back to back in one allocation, and ONE launch decodes the batch -- through the path of BrotliAmdBatchDecodeDeviceDict and
 *     BrotliAmdBatchWait: dictionaries, probe, gangs and pools (planned from the same in_sizes), the second pass with a larger LDS arena;
 *  4. streams that came back NEEDS_MORE_OUTPUT below their limit get a new slot of max(2 x cap, out_pos x in_size / consumed) -- the output and input positions of the resume point --, rounded up to
 *     64 KiB and clamped; the new slots are one allocation a round, one ragged-copy launch (csrc/brotli_copy_kernels.hip) moves what each of
 *     these streams has decoded up to its last metablock boundary, and they ALONE are launched again, resumed from that boundary; and so on
 *     until no stream is in that state;
 *  5. where every stream filled its slot exactly -- the rule for single-metablock documents, whose hints are exact -- the first allocation
 *     IS the packed output: one decode launch, no copy.  Otherwise one ragged-copy launch gathers the delivered bytes into a tight buffer. */
BROTLI_DEC_API int BrotliAmdBatchDecodeDevicePacked(BrotliAmdBatch* batch, uint32_t n, const void* const* d_in, const size_t* in_sizes,
                                                   const void* const* d_dicts, const size_t* dict_sizes, uint64_t max_out_bytes,
                                                   uint32_t flags, void* hip_stream, BrotliAmdResult* results);
/* The packed output of the last packed call (a DEVICE pointer; NULL where there is none) and its n + 1 offsets (host memory of the batch object). */
BROTLI_DEC_API const void* BrotliAmdBatchPackedOutput(BrotliAmdBatch* batch, const uint64_t** offsets);
/* Copies the whole packed output (offsets[n] bytes) to host memory.  Returns 0 on success. */
BROTLI_DEC_API int BrotliAmdBatchPackedFetch(BrotliAmdBatch* batch, uint8_t* host_dst);
/* The same for HOST buffers: the streams (and each distinct dictionary once) are uploaded through the staging of BrotliAmdBatchDecodeHostDict,
 * then the device form runs.  The caller reads the offsets, allocates, and calls BrotliAmdBatchPackedFetch. */
BROTLI_DEC_API int BrotliAmdBatchDecodeHostPacked(BrotliAmdBatch* batch, uint32_t n, const uint8_t* const* in, const size_t* in_sizes,
                                                 const uint8_t* const* dicts, const size_t* dict_sizes, uint64_t max_out_bytes,
                                                 uint32_t flags, BrotliAmdResult* results);
/* Decode launches of the last packed call (1 where no stream had to grow; the size walk is not counted) and ragged-copy launches in it
 * (0 where the first allocation was the packed output). */
BROTLI_DEC_API uint32_t BrotliAmdBatchLastPackedLaunches(BrotliAmdBatch* batch);
BROTLI_DEC_API uint32_t BrotliAmdBatchLastPackedCopies(BrotliAmdBatch* batch);

/* ---- Digests on the device: CRC-32 and CRC-32C of segments of device memory and of a decode call's outputs ----
 *
 * Decoded bytes stay in device memory, and so may compressed payloads; a caller who has to know that they are the right bytes -- a store's
 * recorded checksum, a framing format's CRC over a payload -- asks for their digests instead of copying them to the host.  Both kinds are
 * the reflected 32-bit CRCs with init and final XOR 0xFFFFFFFF: CRC32 is 0xEDB88320 (zlib, gzip, PNG, the `crc` of a Parquet page), CRC32C
 * is 0x82F63B78 (Castagnoli).  "123456789" gives 0xCBF43926 and 0xE3069283; a segment of no bytes gives 0.  A CRC is linear, so one long
 * segment is spread over the whole device like a thousand short ones (csrc/brotli_crc.h, csrc/brotli_crc_kernels.hip), and a digest does not
 * depend on how the work was shared out. */
#define BROTLI_AMD_DIGEST_CRC32 1u
#define BROTLI_AMD_DIGEST_CRC32C 2u

/* The digests of n segments in DEVICE memory -- lens[i] bytes at d_ptrs[i], any alignment, any length, 0 included; n is not bound by the batch
 * object's max_streams; segments may overlap or repeat --: one launch on hip_stream, the call waits on that stream and copies the n digests to
 * `digests` (host).  Nothing outside the 16-byte-aligned span around [d_ptrs[i], d_ptrs[i] + lens[i]) is read.  n == 0 returns 0.  A negative
 * value, and a BrotliAmdLastError text, for a NULL batch, a NULL array with n != 0, and a kind that is neither of the two. */
BROTLI_DEC_API int BrotliAmdBatchDigestSegments(BrotliAmdBatch* batch, uint32_t kind, uint32_t n, const void* const* d_ptrs, const size_t* lens,
                                               uint32_t* digests, void* hip_stream);

/* The digests of the DELIVERED bytes -- [out, out + decoded_size) -- of every stream of the last decode call on the object, into digests[0..n) of
 * that call's n:
 *   - after BrotliAmdBatchDecodeDevice(Dict) or BrotliAmdBatchRelaunch, once BrotliAmdBatchWait has returned: the caller's d_out[i];
 *   - after BrotliAmdBatchDecodeHost(Dict): the streams' slots in the object's device staging, which it keeps -- the bytes the call copied out;
 *   - after BrotliAmdBatchDecodeDevicePacked / HostPacked: [offsets[i], offsets[i + 1]) of the packed output.
 * A stream that ended in an error or NEEDS_MORE_OUTPUT is digested over its decoded_size bytes too (not over `produced`).  The launch runs on
 * the stream of that decode call and the call waits for it.  It is not a decode call itself: BrotliAmdBatchPackedOutput stays valid, and
 * BrotliAmdBatchRelaunch and the Last* accessors say what they said before.  A negative value, and a BrotliAmdLastError text, for a NULL batch or
 * NULL digests, a kind that is neither of the two, an object without a decode call, a last decode call that failed behind its argument checks (it has no
 * outputs; one of no streams returns 0), and a launch that BrotliAmdBatchWait has not been called for. */
BROTLI_DEC_API int BrotliAmdBatchDigestOutputs(BrotliAmdBatch* batch, uint32_t kind, uint32_t* digests);

/* Milliseconds the digest kernel took in the last of the two calls above (HIP events around its launch). */
BROTLI_DEC_API float BrotliAmdBatchLastDigestMs(BrotliAmdBatch* batch);

/* Test hooks (no device needed).  The bytes of source memory in one tile of a digest launch (the unit in which its blocks share the work); */
BROTLI_DEC_API uint32_t BrotliAmdDebugDigestTile(void);
/* the digest of data[0, n) by the device's functions on the host, cut the way the kernel cuts: the bytes placed at `skew` (0..15) past a
 * 16-byte boundary among bytes that are not theirs, 16-byte units, a piece for every run of run_units units (0: the kernel's own number), the
 * pieces combined by a multiplication each and XOR; 0, and a BrotliAmdLastError text, for an unknown kind or skew > 15; */
BROTLI_DEC_API uint32_t BrotliAmdDebugDigestHost(uint32_t kind, const uint8_t* data, size_t n, uint32_t skew, uint32_t run_units);
/* crc x^(8 nbytes) mod the kind's polynomial, for any 64-bit nbytes: crc(A B) == BrotliAmdDebugDigestShift(kind, crc(A), |B|) ^ crc(B). */
BROTLI_DEC_API uint32_t BrotliAmdDebugDigestShift(uint32_t kind, uint32_t crc, uint64_t nbytes);

/* ---- Unshuffle on the device: byte planes of outputs back into elements ----
 *
 * Numeric data that is compressed with Brotli is, as a rule, not stored as the bytes of the array but SHUFFLED into byte planes first -- plane
 * 0 holds byte 0 of every element, plane 1 byte 1, and so on --, which puts the exponent bytes of floats next to each other: Parquet's
 * BYTE_STREAM_SPLIT encoding under its BROTLI codec, the shuffle filter of Blosc and HDF5, the byte grouping of checkpoint compressors.  The
 * decoded bytes are then one step away from the tensor, and these calls take it where the bytes lie.
 *
 * THE TRANSFORM.  A segment of len bytes and a width w: m = len / w elements and r = len % w bytes left over.  For p < w m
 *     dst[p] = src[(p % w) m + p / w],
 * and for w m <= p < len, dst[p] = src[p]: the r left-over bytes stay in place at the end (Blosc's rule; Parquet never has r != 0).  The widths
 * are 1, 2, 4 and 8; width 1 is a copy.  The width is PER SEGMENT: a checkpoint mixes int8 with wider types.  Only this direction -- planes to
 * elements -- exists.
 *
 * OUT OF PLACE: no destination range may overlap any source range or any other destination range of the call.
 *
 * One launch does all segments, the work split by bytes as the ragged copy's is (csrc/brotli_unshuffle.h, csrc/brotli_unshuffle_kernels.hip): one
 * tensor of a gigabyte is spread over the whole device like a hundred thousand pages of a hundred bytes. */

/* n segments in DEVICE memory -- lens[i] bytes of planes at d_src[i] become lens[i] bytes of elements of width widths[i] at d_dst[i]; any
 * alignment, any length, 0 included; n is not bound by the batch object's max_streams --: one launch on hip_stream, and the call waits on that
 * stream.  No byte outside [d_dst[i], d_dst[i] + lens[i]) is written; nothing outside the 16-byte-aligned span around
 * [d_src[i], d_src[i] + lens[i]) is read.  n == 0 returns 0.  A negative value, and a BrotliAmdLastError text, for a NULL batch, a NULL array with
 * n != 0 and any width that is not 1, 2, 4 or 8: the widths are checked on the host in front of everything else, so nothing is launched and no
 * byte is written. */
BROTLI_DEC_API int BrotliAmdBatchUnshuffleSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, void* const* d_dst,
                                                  const size_t* lens, const uint8_t* widths, void* hip_stream);

/* The same for the DELIVERED bytes -- [out, out + decoded_size) -- of every stream of the last decode call on the object: stream i's go to
 * d_dst[i] (device memory of decoded_size bytes, any alignment) by widths[i]; d_dst[i] == NULL skips stream i (its width is not looked at).
 * Where the sources are, and when they are valid, is BrotliAmdBatchDigestOutputs' rule exactly:
 *   - after BrotliAmdBatchDecodeDevice(Dict) or BrotliAmdBatchRelaunch, once BrotliAmdBatchWait has returned: the caller's d_out[i];
 *   - after BrotliAmdBatchDecodeHost(Dict): the streams' slots in the object's device staging, which it keeps;
 *   - after BrotliAmdBatchDecodeDevicePacked / HostPacked: [offsets[i], offsets[i + 1]) of the packed output.
 * A stream that ended in an error or NEEDS_MORE_OUTPUT is transformed over its decoded_size bytes by the rule above (m = decoded_size / w).
 * The launch runs on the stream of that decode call and the call waits for it.  It is not a decode call itself: BrotliAmdBatchPackedOutput stays
 * valid, and BrotliAmdBatchRelaunch and the Last* accessors say what they said before.  A negative value, and a BrotliAmdLastError text, for a NULL
 * batch or a NULL array, a width that is not 1, 2, 4 or 8 (nothing is launched), an object without a decode call, a last decode call that
 * failed behind its argument checks (one of no streams returns 0), and a launch that BrotliAmdBatchWait has not been called for. */
BROTLI_DEC_API int BrotliAmdBatchUnshuffleOutputs(BrotliAmdBatch* batch, void* const* d_dst, const uint8_t* widths);

/* Milliseconds the unshuffle kernel took in the last of the two calls above (HIP events around its launch). */
BROTLI_DEC_API float BrotliAmdBatchLastUnshuffleMs(BrotliAmdBatch* batch);

/* Test hooks (no device needed).  The bytes of destination memory in one tile of an unshuffle launch (the unit in which its blocks share the
 * work); */
BROTLI_DEC_API uint32_t BrotliAmdDebugUnshuffleTile(void);
/* the transform of src[0, len) into dst[0, len) by the device's unit function on the host, over every 16-byte unit of the segment: source and
 * destination are placed at src_skew and dst_skew (0..15) past a 16-byte boundary among bytes that are not theirs.  0; negative, a
 * BrotliAmdLastError text and an untouched dst for a width that is not 1, 2, 4 or 8, a skew > 15, or a byte written outside the destination. */
BROTLI_DEC_API int BrotliAmdDebugUnshuffleHost(uint32_t width, const uint8_t* src, size_t len, uint8_t* dst, uint32_t src_skew, uint32_t dst_skew);

/* ---- Undelta on the device: running sums of deltas back into values ----
 *
 * The filter that stands beside shuffle in front of a general-purpose codec is DELTA: sorted timestamps, offsets and index arrays are stored as
 * differences, TIFF's horizontal predictor and PNG's Sub filter store a sample minus its neighbour, and array containers put a delta or a
 * byte-delta stage next to their shuffle stage (byte-delta is a width-1 delta per byte plane, undone in front of the unshuffle).  Undoing it is a
 * running sum, and these calls take it where the decoded bytes lie.
 *
 * THE TRANSFORM.  A segment of len bytes and a width w: m = len / w elements, read as little-endian unsigned integers of w bytes, and r = len % w
 * bytes left over.  For k < m
 *     dst_elem[k] = (src_elem[0] + src_elem[1] + ... + src_elem[k]) mod 2^(8 w),
 * and the r left-over bytes behind the last whole element are copied unchanged: unshuffle's rule, so a pipeline of the two agrees on them.  The
 * widths are 1, 2, 4 and 8; width 1 is a running sum of bytes, not a copy.  The width is PER SEGMENT.  Only this direction -- deltas to values --
 * exists.  Out of scope: signed or zigzag forms, deltas of order 2, strided or multi-sample deltas (PNG's Sub at 3 bytes a pixel) and XOR
 * deltas.
 *
 * OUT OF PLACE: no destination range overlaps any source range or any other destination range of the call.  IN PLACE: d_dst[i] == d_src[i]
 * exactly is allowed where that address is a multiple of widths[i].  In place at an address that is no multiple of the width is REJECTED on the
 * host.  Any other overlap is UNDEFINED.
 *
 * A running sum is not local: a segment of a gigabyte is spread over the whole device and still comes out as one sum.  A call is three launches
 * in stream order over tiles of destination bytes, the work split by bytes as the ragged copy's is -- the tiles' sums, one small launch that
 * turns them into every tile's carry-in, and the running sums themselves --, and no block ever waits for another block's result
 * (csrc/brotli_undelta.h, csrc/brotli_undelta_kernels.hip). */

/* n segments in DEVICE memory -- lens[i] bytes of deltas at d_src[i] become lens[i] bytes of values of width widths[i] at d_dst[i]; any
 * alignment, any length, 0 included; n is not bound by the batch object's max_streams --: the launches run on hip_stream, and the call waits on
 * that stream.  No byte outside [d_dst[i], d_dst[i] + lens[i]) is written; nothing outside the 16-byte-aligned span around
 * [d_src[i], d_src[i] + lens[i]) is read.  n == 0 returns 0.  A negative value, and a BrotliAmdLastError text, for a NULL batch, a NULL array with
 * n != 0, any width that is not 1, 2, 4 or 8, and an in-place segment at an address that is not a multiple of its width: all of these are
 * checked on the host in front of everything else, so nothing is launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchUndeltaSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, void* const* d_dst,
                                                const size_t* lens, const uint8_t* widths, void* hip_stream);

/* The same for the DELIVERED bytes -- [out, out + decoded_size) -- of every stream of the last decode call on the object: stream i's go to
 * d_dst[i] (device memory of decoded_size bytes, any alignment) by widths[i]; d_dst[i] == NULL skips stream i (its width is not looked at).
 * Where the sources are, and when they are valid, is BrotliAmdBatchUnshuffleOutputs' rule exactly, for the three kinds of decode call.  A stream
 * that ended in an error or NEEDS_MORE_OUTPUT is transformed over its decoded_size bytes by the rule above (m = decoded_size / w).  The launches
 * run on the stream of that decode call and the call waits for it.  It is not a decode call itself: BrotliAmdBatchPackedOutput stays valid, and
 * BrotliAmdBatchRelaunch and the Last* accessors say what they said before.  A negative value, and a BrotliAmdLastError text, for a NULL batch or
 * a NULL array, a width that is not 1, 2, 4 or 8 or a misaligned in-place destination (nothing is launched), an object without a decode call, a
 * last decode call that failed behind its argument checks (one of no streams returns 0), and a launch that BrotliAmdBatchWait has not been
 * called for. */
BROTLI_DEC_API int BrotliAmdBatchUndeltaOutputs(BrotliAmdBatch* batch, void* const* d_dst, const uint8_t* widths);

/* Milliseconds the undelta kernels took in the last of the two calls above (HIP events around all its launches together), */
BROTLI_DEC_API float BrotliAmdBatchLastUndeltaMs(BrotliAmdBatch* batch);
/* and those of phase 1 (the tiles' sums), 2 (the carries) or 3 (the running sums) alone; another phase: 0. */
BROTLI_DEC_API float BrotliAmdBatchLastUndeltaPhaseMs(BrotliAmdBatch* batch, uint32_t phase);

/* Test hooks (no device needed).  The bytes of destination memory in one tile of an undelta call; */
BROTLI_DEC_API uint32_t BrotliAmdDebugUndeltaTile(void);
/* the tiles whose carries the one block of the carry launch takes in one pass of its loop; */
BROTLI_DEC_API uint32_t BrotliAmdDebugUndeltaCarrySpan(void);
/* all three phases by the device's unit and tile functions on the host, over n segments given as offsets into one source buffer src[0, src_size)
 * and one destination buffer dst[0, dst_size): the buffers are placed at src_skew and dst_skew (0..15) past a 16-byte boundary among bytes that
 * are not theirs.  tile_units: the 16-byte units of a tile, 0 for the kernel's own.  order_seed != 0: phases 1 and 3 take the tiles in an order
 * shuffled by it (the result may not depend on it).  in_place != 0: src_size == dst_size, one room is filled from src and every segment's source
 * is its destination (src_offs is not looked at).  0, and the segments' bytes of dst written (no other byte of dst is); negative, a
 * BrotliAmdLastError text and an untouched dst for a width that is not 1, 2, 4 or 8, a skew > 15, a segment outside its buffer, in place at an
 * address that is not a multiple of the width, or a byte changed outside every segment's destination. */
BROTLI_DEC_API int BrotliAmdDebugUndeltaHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size,
                                            const uint64_t* src_offs, const uint64_t* dst_offs, const uint64_t* lens, const uint8_t* widths,
                                            uint32_t src_skew, uint32_t dst_skew, uint32_t tile_units, uint32_t order_seed, int in_place);

/* ---- Bit-unshuffle on the device: bit planes of outputs back into elements ----
 *
 * The third filter that array containers put in front of a general-purpose codec is BITSHUFFLE: the bit transpose of the bitshuffle library and
 * HDF5 filter 32008, the bit-shuffle mode of Blosc-style containers, the Bitshuffle stage of codec chains in zarr-like stores.  It is what
 * quantised integers, sensor counts, masks and the low mantissa bits of floats go through where the byte shuffle does not compress well
 * enough.  Undoing it is an 8 x 8 bit transpose per byte column on top of the unshuffle's byte interleave, and these calls take it where the
 * decoded bytes lie.
 *
 * THE SEGMENT AND ITS PARAMETERS.  A segment has len bytes and a width w in {1, 2, 4, 8}.  It also has a block size B in elements: B == 0
 * means the whole segment is one block; otherwise B is a multiple of 8, and any other value is rejected on the host.  m = len / w is the
 * number of elements.
 *
 * BLOCKS.  The elements are cut into blocks of B, at the same byte offsets in source and destination: block b starts at element b B and byte
 * offset o = b B w.  A full block transposes c = B elements.  The last, shorter block transposes c = (m - b B) rounded down to a multiple of
 * 8; that can be 0.  So the last m % 8 elements and the len % w bytes behind them are always copied unchanged: dst[p] = src[p] for
 * p >= 8 (m / 8) w.  (The blocked rule of the bitshuffle library; with B == 0 it is Blosc's rule: one block, left-over elements copied.)
 *
 * THE FORMULA.  Inside a block, for element i < c, byte j < w and bit k < 8 (bit 0 is the least significant):
 *     bit k of dst[o + i w + j]  =  bit (i % 8) of src[o + (8 j + k) (c / 8) + i / 8]
 * The source of a block is 8 w bit rows of c / 8 bytes each; row 8 j + k holds bit k of byte j of every element; element i sits in bit i % 8
 * of byte i / 8 of its row.
 *
 * Width 1 is a real transform: 8 x 8 bit transposes of rows of c / 8 bytes.  The width and B are PER SEGMENT.  Only this direction -- planes
 * to elements -- exists on the device.  B == 0 means "one block", NOT the library's "default block size": a caller with HDF5 data passes the
 * file's block size, which is 8192 / w by default.
 *
 * OUT OF PLACE: no destination range overlaps any source range or any other destination range of the call.  This is stated, not checked.
 *
 * One launch does all segments, the work split by bytes as the unshuffle's is (csrc/brotli_bitunshuffle.h, csrc/brotli_bitunshuffle_kernels.hip).
 * Blocks whose destination begins at a multiple of 16 bytes and that hold 32 elements or more go 32 elements a lane; every other word of
 * destination is gathered bit by bit. */

/* n segments in DEVICE memory -- lens[i] bytes of bit planes at d_src[i] become lens[i] bytes of elements of width widths[i], in blocks of
 * block_elems[i] elements (block_elems == NULL: all 0), at d_dst[i]; any alignment, any length, 0 included; n is not bound by the batch object's
 * max_streams --: one launch on hip_stream, and the call waits on that stream.  No byte outside [d_dst[i], d_dst[i] + lens[i]) is written;
 * nothing outside the 16-byte-aligned span around [d_src[i], d_src[i] + lens[i]) is read.  n == 0 returns 0.  A negative value, and a
 * BrotliAmdLastError text that names what was wrong, for a NULL batch, a NULL array (but block_elems) with n != 0, any width that is not 1, 2, 4 or
 * 8 and any block_elems that is neither 0 nor a multiple of 8: all of these are checked on the host in front of everything else, so nothing is
 * launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchBitUnshuffleSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, void* const* d_dst,
                                                     const size_t* lens, const uint8_t* widths, const uint32_t* block_elems /* n entries, or NULL: all 0 */,
                                                     void* hip_stream);

/* The same for the DELIVERED bytes -- [out, out + decoded_size) -- of every stream of the last decode call on the object: stream i's go to
 * d_dst[i] (device memory of decoded_size bytes, any alignment) by widths[i] and block_elems[i] (one entry per stream, or NULL: all 0);
 * d_dst[i] == NULL skips stream i (its width and block are not looked at).  Where the sources are, and when they are valid, is
 * BrotliAmdBatchUnshuffleOutputs' rule exactly, for the three kinds of decode call.  A stream that ended in an error or NEEDS_MORE_OUTPUT is
 * transformed over its decoded_size bytes by the rule above (m = decoded_size / w).  The launch runs on the stream of that decode call and the
 * call waits for it.  It is not a decode call itself: BrotliAmdBatchPackedOutput stays valid, and BrotliAmdBatchRelaunch and the Last* accessors say
 * what they said before.  A negative value, and a BrotliAmdLastError text, for a NULL batch, a NULL d_dst or widths, a bad width or block (nothing
 * is launched), an object without a decode call, a last decode call that failed behind its argument checks (one of no streams returns 0), and a
 * launch that BrotliAmdBatchWait has not been called for. */
BROTLI_DEC_API int BrotliAmdBatchBitUnshuffleOutputs(BrotliAmdBatch* batch, void* const* d_dst, const uint8_t* widths, const uint32_t* block_elems /* or NULL */);

/* Milliseconds the bit-unshuffle kernel took in the last of the two calls above (HIP events around its launch). */
BROTLI_DEC_API float BrotliAmdBatchLastBitUnshuffleMs(BrotliAmdBatch* batch);

/* Test hooks (no device needed).  The bytes of destination memory in one tile of a bit-unshuffle launch; */
BROTLI_DEC_API uint32_t BrotliAmdDebugBitUnshuffleTile(void);
/* the transform of src[0, len) into dst[0, len) by the device's functions on the host, the segment's words taken in the order and by the items
 * the kernel's lanes would take them: source and destination are placed at src_skew and dst_skew (0..15) past a 16-byte boundary among bytes
 * that are not theirs.  *fast_items (may be NULL): the runs of 32 elements that went the fast way.  0; negative, a BrotliAmdLastError text and an
 * untouched dst for a width that is not 1, 2, 4 or 8, a block_elems that is neither 0 nor a multiple of 8, a skew > 15, or a byte written outside
 * the destination. */
BROTLI_DEC_API int BrotliAmdDebugBitUnshuffleHost(uint32_t width, uint32_t block_elems, const uint8_t* src, size_t len, uint8_t* dst,
                                                 uint32_t src_skew, uint32_t dst_skew, uint64_t* fast_items /* may be NULL */);

/* ---- Bit-unpack on the device: k-bit fields of outputs back into elements ----
 *
 * The fourth layout that the same users put in front of the codec is FIXED-WIDTH BIT PACKING: values of k bits stored back to back, k no
 * multiple of 8.  Parquet writes it for dictionary indices, levels and the miniblocks of DELTA_BINARY_PACKED, Arrow for validity bitmaps
 * (k = 1); quantised checkpoints store 4-, 3- and 2-bit weights this way; numpy.packbits, numcodecs' PackBits and the sub-byte samples of PNG
 * and TIFF are the MSB-first variant; frame-of-reference columns are packed deltas, which the undelta calls above then sum up.  It is the one
 * filter here whose destination is LARGER than its source.
 *
 * THE SEGMENT AND ITS PARAMETERS.  A segment has source bytes src[0, src_len), a count m of elements, a field width k with 1 <= k <= 64, an
 * element width w in {1, 2, 4, 8} with k <= 8 w, and flags.  The destination is exactly m w bytes: element i is a little-endian unsigned
 * integer of w bytes at dst + i w.
 *
 * THE FORMULA.  Read the source as a string of bits.  Element i is the field of bits i k .. i k + k - 1.
 *   LSB-first (flags bit 0 clear: Parquet RLE/bit-packed, Arrow, int4 weight packing): stream bit b is bit b % 8 of src[b / 8], bit 0 being
 *     the least significant, and the first bit of a field is the value's bit 0.
 *   MSB-first (BROTLI_AMD_BITUNPACK_MSB_FIRST: numpy.packbits' default, PackBits, PNG/TIFF, Parquet's deprecated BIT_PACKED): stream bit b is
 *     bit 7 - b % 8 of src[b / 8], and the first bit of a field is the value's bit k - 1.
 *   BROTLI_AMD_BITUNPACK_SIGNED: the value is sign-extended from bit k - 1 to 8 w bits.  Otherwise it is zero-extended.
 * k == 8 w is a copy with LSB-first, and a byte reversal per element with MSB-first; both are allowed.  Example (the two of the Parquet format
 * text): the values 0 .. 7 at k = 3 are 88 c6 fa LSB-first and 05 39 77 MSB-first.
 *
 * The transform reads ceil(m k / 8) source bytes.  Pad bits in the last one are ignored, and so are source bytes behind it.  k, w and the flags
 * are PER SEGMENT.  Only this direction -- fields to elements -- exists on the device.
 *
 * OUT OF PLACE ONLY: no destination range overlaps any source range or any other destination range of the call.  This is stated, not checked.
 *
 * REFUSED ON THE HOST, in front of everything that touches the device: k == 0, k > 8 w, a width outside {1, 2, 4, 8}; unknown flag bits;
 * ceil(m k / 8) > src_len; m > 2^56 (so that neither m k nor m w can overflow).
 *
 * One launch does all segments, the work split by the destination's bytes as the unshuffle's is (csrc/brotli_bitunpack.h,
 * csrc/brotli_bitunpack_kernels.hip).  Where a destination begins at a multiple of 16 bytes, every whole group of 32 elements goes 32 elements
 * a lane; every other word of destination is put together byte by byte. */
#define BROTLI_AMD_BITUNPACK_MSB_FIRST 1u
#define BROTLI_AMD_BITUNPACK_SIGNED 2u

/* n segments in DEVICE memory -- the first counts[i] fields of bits[i] bits of the src_lens[i] bytes at d_src[i] become counts[i] elements of
 * widths[i] bytes at d_dst[i], by flags[i] (flags == NULL: all 0); any alignment, any count, 0 included; n is not bound by the batch object's
 * max_streams --: one launch on hip_stream, and the call waits on that stream.  No byte outside [d_dst[i], d_dst[i] + counts[i] widths[i]) is
 * written; nothing outside the 16-byte-aligned span around the ceil(counts[i] bits[i] / 8) source bytes is read.  n == 0 and segments of no
 * elements launch nothing and return 0.  A negative value, and a BrotliAmdLastError text that names the segment and what was wrong, for a NULL
 * batch, a NULL array (but flags) with n != 0, and everything in the list above: all of these are checked on the host in front of everything
 * else, so nothing is launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchBitUnpackSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                                  const uint64_t* counts, const uint8_t* bits, const uint8_t* widths,
                                                  const uint8_t* flags /* n entries, or NULL: all 0 */, void* hip_stream);

/* The same for the DELIVERED bytes -- [out, out + decoded_size) -- of every stream of the last decode call on the object: stream i's source is
 * its decoded_size delivered bytes, and its elements go to d_dst[i] (device memory of counts[i] widths[i] bytes, any alignment) by bits[i],
 * widths[i] and flags[i] (one entry per stream each; flags may be NULL: all 0).  counts == NULL: stream i's count is floor(8 decoded_size /
 * bits[i]), the whole fields that were delivered.  A given counts[i] that needs more bytes than were delivered fails the whole call: nothing is
 * launched, and the error text names the stream.  d_dst[i] == NULL skips stream i (none of its parameters are looked at).  Where the sources
 * are, and when they are valid, is BrotliAmdBatchUnshuffleOutputs' rule exactly, for the three kinds of decode call.  A stream that ended in an
 * error or NEEDS_MORE_OUTPUT is transformed over its decoded_size bytes by the rule above.  The launch runs on the stream of that decode call
 * and the call waits for it.  It is not a decode call itself: BrotliAmdBatchPackedOutput stays valid, and BrotliAmdBatchRelaunch and the Last*
 * accessors say what they said before.  A negative value, and a BrotliAmdLastError text, for a NULL batch, a NULL d_dst, bits or widths, a
 * refused shape or count (nothing is launched), an object without a decode call, a last decode call that failed behind its argument checks (one
 * of no streams returns 0), and a launch that BrotliAmdBatchWait has not been called for. */
BROTLI_DEC_API int BrotliAmdBatchBitUnpackOutputs(BrotliAmdBatch* batch, void* const* d_dst, const uint64_t* counts /* or NULL */, const uint8_t* bits,
                                                 const uint8_t* widths, const uint8_t* flags /* or NULL */);

/* Milliseconds the bit-unpack kernel took in the last of the two calls above (HIP events around its launch). */
BROTLI_DEC_API float BrotliAmdBatchLastBitUnpackMs(BrotliAmdBatch* batch);

/* Test hooks (no device needed).  The bytes of destination memory in one tile of a bit-unpack launch; */
BROTLI_DEC_API uint32_t BrotliAmdDebugBitUnpackTile(void);
/* the transform of the first `count` fields of src[0, src_len) into dst[0, count width) by the device's functions on the host, the segment's
 * words taken in the order and by the items the kernel's lanes would take them: source and destination are placed at src_skew and dst_skew
 * (0..15) past a 16-byte boundary among bytes that are not theirs.  *fast_items (may be NULL): the runs of 32 elements that went the fast way.
 * 0; negative, a BrotliAmdLastError text and an untouched dst for a refused shape or count (the list above), a skew > 15, or a byte written
 * outside the destination. */
BROTLI_DEC_API int BrotliAmdDebugBitUnpackHost(uint32_t bits, uint32_t width, uint32_t flags, const uint8_t* src, size_t src_len, uint64_t count,
                                              uint8_t* dst, uint32_t src_skew, uint32_t dst_skew, uint64_t* fast_items /* may be NULL */);

/* ---- Unvarint on the device: LEB128 varints of outputs back into elements ----
 *
 * The fifth layout in front of the codec is the VARIABLE-LENGTH INTEGER -- LEB128, protobuf's base-128 varint, plain or zigzag: protobuf packed
 * repeated fields, the block and miniblock headers and first values of Parquet's DELTA_BINARY_PACKED and DELTA_LENGTH_BYTE_ARRAY (a whole stream of which is the undbp calls' below), the run headers
 * of its RLE / bit-packed hybrid (a whole stream of which is the unrle calls' below), ORC's integer runs, Avro's zigzag longs, the postings lists and offset tables of search indexes, sorted ids
 * stored as varint deltas (which the undelta calls above then sum up).  It is the one filter here whose output size DEPENDS ON THE DATA: every
 * segment has a capacity and gets a result.
 *
 * THE SEGMENT AND ITS PARAMETERS.  A segment is the bytes src[0, len), with a width w in {1, 2, 4, 8}, flags, and a capacity cap in elements.
 *
 * END.  A byte with bit 7 clear ENDS a varint.  Call the positions of such bytes in the segment e_0 < e_1 < ... < e_{m-1}.  Varint i is the bytes
 * (e_{i-1}, e_i], from the segment's start for i = 0; its length L_i is the number of those bytes.  A varint never reaches back across the
 * segment's first byte, whatever lies in memory in front of it.
 *
 * VALUE.  Byte j of the varint contributes its low 7 bits at bit 7 j of a 64-bit value (little-endian groups).  For L_i <= 10, bits at and above
 * bit 64 are dropped: only bit 0 of the tenth byte counts, and nothing is reported.  For L_i > 10 the varint is OVERLONG: its element is 0 and
 * it is counted in `overlong`.  So an end byte needs at most the ten bytes in front of it; no look-back is unbounded.
 *
 * BROTLI_AMD_UNVARINT_ZIGZAG: v = (v >> 1) ^ (0 - (v & 1)) on the 64-bit value, in front of the truncation.  An overlong element stays 0.
 *
 * ELEMENT.  Element i is the value truncated to 8 w bits and stored little-endian at dst + i w, for i < min(m, cap).  dst has any alignment and
 * need not be a multiple of w.  No byte outside [dst, dst + min(m, cap) w) is written; nothing outside the 16-byte-aligned span around
 * [src, src + len) is read.
 *
 * RESULT.  Every segment gets a BrotliAmdUnvarintResult in host memory: count is m, also where cap < m (the way to size a second call);
 * consumed is e_{m-1} + 1, or 0 where m == 0 (len - consumed unfinished bytes trail the last end); overlong is the number of overlong varints
 * among all m.  All three are independent of cap, and of how the work was shared out.
 *
 * Examples: 96 01 ac 02 e5 8e 26 is 150, 300, 624485 (consumed 7); ff x 9 then 01, and ff x 9 then 7f, are both 2^64 - 1 at w = 8; 01 02 03 04
 * fe ff ff ff 0f with zigzag at w = 4 is -1, 1, -2, 2, 2147483647; 80 x 10 then 01 05 80 80 is 0 and 5 with count 2, consumed 12, overlong 1.
 *
 * OUT OF PLACE ONLY: no destination range overlaps any source range or any other destination range of the call.  This is stated, not checked.
 *
 * REFUSED ON THE HOST, in front of everything that touches the device: a width outside {1, 2, 4, 8}; unknown flag bits; cap > 2^56; a NULL
 * d_dst[i] with caps[i] != 0.
 *
 * A call is three launches in stream order over tiles of SOURCE bytes, the work split by bytes as the ragged copy's is: the number of ends in
 * every tile, undelta's carry launch over those numbers, and the elements themselves -- no block ever waits for another block's result
 * (csrc/brotli_unvarint.h, csrc/brotli_unvarint_kernels.hip). */
#define BROTLI_AMD_UNVARINT_ZIGZAG 1u

typedef struct BrotliAmdUnvarintResult {
  uint64_t count;     /* the varints that end in the segment, whatever cap was */
  uint64_t consumed;  /* the bytes up to and including the last end */
  uint64_t overlong;  /* the varints of more than ten bytes among them (their elements are 0) */
} BrotliAmdUnvarintResult;

/* n segments in DEVICE memory -- the varints in the src_lens[i] bytes at d_src[i] become elements of widths[i] bytes at d_dst[i], the first
 * caps[i] of them, by flags[i] (flags == NULL: all 0); results[i] says what segment i held; any alignment, any length, 0 included; n is not
 * bound by the batch object's max_streams --: the launches run on hip_stream, and the call waits on that stream.  caps[i] == 0 needs no
 * destination (d_dst[i] is not looked at, and d_dst itself may be NULL where every capacity is 0): a call of such segments only counts.  n == 0
 * returns 0.  A negative value, and a BrotliAmdLastError text that names the segment and what was wrong, for a NULL batch, a NULL array (but flags
 * and d_dst) with n != 0, and everything in the list above: all
 * of these are checked on the host in front of everything else, so nothing is launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchUnvarintSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                                 const uint64_t* caps, const uint8_t* widths, const uint8_t* flags /* n entries, or NULL: all 0 */,
                                                 BrotliAmdUnvarintResult* results, void* hip_stream);

/* The same for the DELIVERED bytes -- [out, out + decoded_size) -- of every stream of the last decode call on the object: stream i's varints go
 * to d_dst[i] (device memory of caps[i] widths[i] bytes, any alignment) by widths[i] and flags[i] (one entry per stream each; flags may be NULL:
 * all 0), and results[i] (one entry per stream) says what it held.  d_dst[i] == NULL skips stream i: none of its parameters are looked at and
 * its result is zeros.  d_dst == NULL or caps == NULL: every stream is counted and nothing is written.  Where the sources are, and when they are
 * valid, is BrotliAmdBatchUnshuffleOutputs' rule exactly, for the three kinds of decode call.  A stream that ended in an error or
 * NEEDS_MORE_OUTPUT is taken over its decoded_size bytes.  The launches run on the stream of that decode call and the call waits for it.  It is
 * not a decode call itself: BrotliAmdBatchPackedOutput stays valid, and BrotliAmdBatchRelaunch and the Last* accessors say what they said before.
 * A negative value, and a BrotliAmdLastError text, for a NULL batch, widths or results, a refused width, flag or cap (nothing is launched), an
 * object without a decode call, a last decode call that failed behind its argument checks (one of no streams returns 0), and a launch that
 * BrotliAmdBatchWait has not been called for. */
BROTLI_DEC_API int BrotliAmdBatchUnvarintOutputs(BrotliAmdBatch* batch, void* const* d_dst /* or NULL */, const uint64_t* caps /* or NULL */,
                                                const uint8_t* widths, const uint8_t* flags /* or NULL */, BrotliAmdUnvarintResult* results);

/* Milliseconds the unvarint kernels took in the last of the two calls above (HIP events around all its launches together), */
BROTLI_DEC_API float BrotliAmdBatchLastUnvarintMs(BrotliAmdBatch* batch);
/* and those of phase 1 (the tiles' counts), 2 (the carries) or 3 (the elements) alone; another phase: 0. */
BROTLI_DEC_API float BrotliAmdBatchLastUnvarintPhaseMs(BrotliAmdBatch* batch, uint32_t phase);

/* Test hooks (no device needed).  The bytes of SOURCE memory in one tile of an unvarint call; */
BROTLI_DEC_API uint32_t BrotliAmdDebugUnvarintTile(void);
/* all three phases by the device's unit and tile functions on the host, over n segments given as offsets into one source buffer src[0, src_size)
 * and one destination buffer dst[0, dst_size): the buffers are placed at src_skew and dst_skew (0..15) past a 16-byte boundary among bytes that
 * are not theirs.  Segment i is src_lens[i] bytes at src_offs[i]; its elements go to dst_offs[i], where there must be room for
 * min(caps[i], src_lens[i]) of them.  tile_units: the 16-byte units of a tile, 0 for the kernel's own.  order_seed != 0: phases 1 and 3 take
 * the tiles in an order shuffled by it (the result may not depend on it).  0, results[0..n) filled and the elements' bytes of dst written (no
 * other byte of dst is); -1, a BrotliAmdLastError text and an untouched dst for a refused width, flag or cap, a skew > 15 or a segment outside
 * its buffer; -2 where a byte outside the elements' destinations changed. */
BROTLI_DEC_API int BrotliAmdDebugUnvarintHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                             const uint64_t* src_lens, const uint64_t* dst_offs, const uint64_t* caps, const uint8_t* widths,
                                             const uint8_t* flags /* or NULL */, uint32_t src_skew, uint32_t dst_skew, uint32_t tile_units,
                                             uint32_t order_seed, BrotliAmdUnvarintResult* results);

/* ---- Unrle on the device: RLE / bit-packed hybrid runs of outputs back into elements ----
 *
 * The sixth layout in front of the codec is the RUN: Parquet's RLE / bit-packed hybrid, which holds the dictionary indices of every
 * dictionary-encoded column, the definition and repetition levels, and the booleans of v2 pages.  It is a varint header and then either
 * bit-unpack's packed fields or one repeated value; where a header lies depends on every header in front of it, so neither of the two calls
 * above can take it.  Like unvarint, its output size DEPENDS ON THE DATA: every segment has a capacity and gets a result.
 *
 * THE SEGMENT AND ITS PARAMETERS.  A segment is the bytes src[0, len), with a field width k in bits (0 .. 32), an element width w in
 * {1, 2, 4, 8} with k <= 8 w, flags, and a capacity cap in elements.  It is a sequence of RUNS, decoded from offset 0 (offset 1 with
 * BROTLI_AMD_UNRLE_WIDTH_BYTE) until the segment's end or the first STOP.
 *
 * HEADER.  h is a LEB128 varint of 1 .. 5 bytes, low group first.  Its up to 35 bits are taken as they are: nothing is dropped.
 * BIT-PACKED RUN, h & 1 == 1: g = h >> 1 groups, 8 g values.  The payload is g k bytes: fields of k bits, LSB-first, zero-extended --
 *   bit-unpack's default form.
 * RLE RUN, h & 1 == 0: c = h >> 1 values.  The payload is ceil(k / 8) bytes: a little-endian value, repeated c times.  The value is NOT
 *   masked to k bits; it is zero-extended to w bytes.
 * k == 0: both payloads are empty and every value is 0 (a dictionary of one entry).
 * BROTLI_AMD_UNRLE_WIDTH_BYTE: the segment's first byte is k (Parquet's dictionary-index page body); the `bits` argument is not looked at.  A
 *   k above 32 or above 8 w stops the decode, and so does an empty segment.
 *
 * STORES.  Element i of the concatenated runs, truncated to w bytes, goes to dst + i w, little-endian, for i < min(count, cap).  dst has any
 * alignment.  No byte outside [dst, dst + min(count, cap) w) is written; nothing outside the 16-byte-aligned span around [src, src + len)
 * is read.
 *
 * STOPS.  The decode ends at the first stop; everything in front of it is delivered.
 *   status                        when                                       values counted                              consumed
 *   BROTLI_AMD_UNRLE_OK           the runs end exactly at len                all                                         len
 *   BROTLI_AMD_UNRLE_BAD_HEADER   a header's fifth byte has bit 7 set        the runs in front                           that header's offset
 *   BROTLI_AMD_UNRLE_ZERO_RUN     h >> 1 == 0                                the runs in front                           that header's offset
 *   BROTLI_AMD_UNRLE_TRUNCATED    a header's continuation reaches len        the runs in front                           that header's offset
 *   BROTLI_AMD_UNRLE_TRUNCATED    an RLE value reaches len                   the runs in front                           that header's offset
 *   BROTLI_AMD_UNRLE_TRUNCATED    a bit-packed payload reaches len           the runs in front, and floor(8 r / k) values len
 *                                                                            of the r payload bytes that are there
 *   BROTLI_AMD_UNRLE_BAD_WIDTH    only with WIDTH_BYTE, see above            0                                           0
 * (The bit-packed TRUNCATED row exists because some writers cut the last group's padding: those values are counted and delivered.)
 *
 * RESULT.  Every segment gets a BrotliAmdUnrleResult in host memory.  count, consumed, runs, status and bits are independent of cap, and of how
 * the work was shared out.
 *
 * Examples (k, bytes, values): 3, 03 88 C6 FA: 0 .. 7;  3, 10 05: 8 x 5;  9, 06 2C 01: 3 x 300;  3, 90 03 07: 200 x 7;  0, 07: 24 x 0.
 *
 * OUT OF PLACE ONLY: no destination range overlaps any source range or any other destination range of the call.  This is stated, not checked.
 *
 * REFUSED ON THE HOST, in front of everything that touches the device: a width outside {1, 2, 4, 8}; unknown flag bits; k > 32 or k > 8 w
 * without WIDTH_BYTE; cap > 2^56; a NULL d_dst[i] with caps[i] != 0.
 *
 * A call is two launches in stream order, and no block ever waits for another.  1. THE WALK, one wave a segment: the wave stages the source
 * through LDS in aligned chunks and takes the headers one after the other -- it never reads a packed payload --, writes the segment's result,
 * and for every ITEM of the destination (BrotliAmdDebugUnrleItemElems() elements) a checkpoint: the header offset and first element of the
 * run that holds the item's first element.  2. THE EXPANSION, one wave an item, over the items of all segments in one list: the wave starts at
 * its checkpoint, collects the runs that cover the item and stores its elements, a lane's elements neighbours.  So one segment with a gigabyte
 * of destination is expanded by every CU; its walk is one wave's.  A call that only counts is the first launch alone
 * (csrc/brotli_unrle.h, csrc/brotli_unrle_kernels.hip).
 *
 * OUT OF SCOPE: a speculative parallel walk of one long segment; page framing -- thrift headers, and the 4-byte length in front of v1 levels,
 * where the caller passes src + 4 --; ORC's and PackBits' run formats; MSB-first fields; sign extension.  The dictionary gather is the
 * undict calls' below: runs in, values out. */
#define BROTLI_AMD_UNRLE_WIDTH_BYTE 1u

#define BROTLI_AMD_UNRLE_OK 0u
#define BROTLI_AMD_UNRLE_BAD_HEADER 1u
#define BROTLI_AMD_UNRLE_ZERO_RUN 2u
#define BROTLI_AMD_UNRLE_TRUNCATED 3u
#define BROTLI_AMD_UNRLE_BAD_WIDTH 4u

typedef struct BrotliAmdUnrleResult {
  uint64_t count;     /* values in all runs, whatever cap was */
  uint64_t consumed;  /* the table above */
  uint64_t runs;      /* runs that gave at least one value */
  uint32_t status;    /* BROTLI_AMD_UNRLE_* */
  uint32_t bits;      /* the k that was used */
} BrotliAmdUnrleResult;

/* n segments in DEVICE memory -- the runs in the src_lens[i] bytes at d_src[i], of fields of bits[i] bits, become elements of widths[i] bytes
 * at d_dst[i], the first caps[i] of them, by flags[i] (flags == NULL: all 0); results[i] says what segment i held; any alignment, any length,
 * 0 included; n is not bound by the batch object's max_streams --: the launches run on hip_stream, and the call waits on that stream.
 * caps[i] == 0 needs no destination (d_dst[i] is not looked at, and d_dst itself may be NULL where every capacity is 0): a call of such
 * segments only counts.  n == 0 returns 0.  A negative value, and a BrotliAmdLastError text that names the segment and what was wrong, for a
 * NULL batch, a NULL array (but flags and d_dst) with n != 0, and everything in the list above: all of these are checked on the host in front
 * of everything else, so nothing is launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchUnrleSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                              const uint64_t* caps, const uint8_t* bits, const uint8_t* widths,
                                              const uint8_t* flags /* n entries, or NULL: all 0 */, BrotliAmdUnrleResult* results, void* hip_stream);

/* The same for the DELIVERED bytes -- [out, out + decoded_size) -- of every stream of the last decode call on the object: stream i's values go
 * to d_dst[i] (device memory of caps[i] widths[i] bytes, any alignment) by bits[i], widths[i] and flags[i] (one entry per stream each; flags
 * may be NULL: all 0), and results[i] (one entry per stream) says what it held.  d_dst[i] == NULL skips stream i: none of its parameters are
 * looked at and its result is zeros.  d_dst == NULL or caps == NULL: every stream is counted and nothing is written.  Where the sources are,
 * and when they are valid, is BrotliAmdBatchUnshuffleOutputs' rule exactly, for the three kinds of decode call.  A stream that ended in an
 * error or NEEDS_MORE_OUTPUT is taken over its decoded_size bytes.  The launches run on the stream of that decode call and the call waits for
 * it.  It is not a decode call itself: BrotliAmdBatchPackedOutput stays valid, and BrotliAmdBatchRelaunch and the Last* accessors say what they
 * said before.  A negative value, and a BrotliAmdLastError text, for a NULL batch, bits, widths or results, a refused shape, flag or cap
 * (nothing is launched), an object without a decode call, a last decode call that failed behind its argument checks (one of no streams
 * returns 0), and a launch that BrotliAmdBatchWait has not been called for. */
BROTLI_DEC_API int BrotliAmdBatchUnrleOutputs(BrotliAmdBatch* batch, void* const* d_dst /* or NULL */, const uint64_t* caps /* or NULL */,
                                             const uint8_t* bits, const uint8_t* widths, const uint8_t* flags /* or NULL */,
                                             BrotliAmdUnrleResult* results);

/* Milliseconds the unrle kernels took in the last of the two calls above (HIP events around its launches together), */
BROTLI_DEC_API float BrotliAmdBatchLastUnrleMs(BrotliAmdBatch* batch);
/* and those of phase 1 (the walk) or 2 (the expansion) alone; another phase: 0. */
BROTLI_DEC_API float BrotliAmdBatchLastUnrlePhaseMs(BrotliAmdBatch* batch, uint32_t phase);

/* Test hooks (no device needed).  The elements of one item of the expansion, and the source bytes that the walk stages at a time; */
BROTLI_DEC_API uint32_t BrotliAmdDebugUnrleItemElems(void);
BROTLI_DEC_API uint32_t BrotliAmdDebugUnrleWalkChunk(void);
/* both phases by the functions of csrc/brotli_unrle.h on the host, over n segments given as offsets into one source buffer src[0, src_size)
 * and one destination buffer dst[0, dst_size): the buffers are placed at src_skew and dst_skew (0..15) past a 16-byte boundary among bytes that
 * are not theirs.  Segment i is src_lens[i] bytes at src_offs[i]; its elements go to dst_offs[i], where there must be room for
 * min(caps[i], count) of them.  item_elems: the elements of an item, 0 for the device's own.  order_seed != 0: the items are taken in an order
 * shuffled by it (the result may not depend on it).  0, results[0..n) filled and the elements' bytes of dst written (no other byte of dst
 * is); -1, a BrotliAmdLastError text and an untouched dst for a refused shape, flag or cap, a skew > 15 or a segment outside its buffer; -2
 * where a byte outside the elements' destinations changed. */
BROTLI_DEC_API int BrotliAmdDebugUnrleHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                          const uint64_t* src_lens, const uint64_t* dst_offs, const uint64_t* caps, const uint8_t* bits,
                                          const uint8_t* widths, const uint8_t* flags /* or NULL */, uint32_t src_skew, uint32_t dst_skew,
                                          uint32_t item_elems, uint32_t order_seed, BrotliAmdUnrleResult* results);

/* ---- Undbp on the device: DELTA_BINARY_PACKED blocks of outputs back into elements ----
 *
 * The seventh layout in front of the codec is the DELTA BLOCK: Parquet's DELTA_BINARY_PACKED, which v2 writers use for INT32 and INT64 columns
 * -- timestamps, ids, offsets --, for the lengths of DELTA_LENGTH_BYTE_ARRAY and for the prefix and suffix lengths of DELTA_BYTE_ARRAY.  It is
 * unvarint's varints, bit-unpack's fields and undelta's running sum in one stream; where a block lies depends on every block header in front of
 * it, and the values are a running sum across all blocks, so none of those three calls can take it.  Its output size DEPENDS ON THE DATA: every
 * segment has a capacity and gets a result.
 *
 * THE SEGMENT AND ITS PARAMETERS.  A segment is the bytes src[0, len), with an element width w in {1, 2, 4, 8} and a capacity cap in elements.
 * There are no flags yet: every bit of a flags array is refused.
 *
 * HEADER.  Four LEB128 varints by unvarint's value rule, each of at most ten bytes, padded forms such as 80 00 included: B, the values per
 * block; M, the miniblocks per block; N, the total values; first, zigzag.  The header is BAD_HEADER where a varint is longer than ten bytes,
 * B == 0, B % 128 != 0, B > 65536, M == 0, B % M != 0 or (B / M) % 32 != 0; the varints are judged first, in their order, then their values.
 * V = B / M is the values per miniblock.  (Writers use B = 128 or 256 and M = 4; 65536 is this contract's limit.)
 *
 * BLOCKS.  Value 0 is `first`.  The N - 1 deltas lie in ceil((N - 1) / B) blocks; N == 0 and N == 1 have none, and N == 0 gives count 0.  A block
 * is min_delta, a zigzag varint of at most ten bytes; M width bytes; and the payloads of its miniblocks, miniblock j being V fields of width[j]
 * bits, LSB-first and zero-extended -- bit-unpack's default form -- in V width[j] / 8 bytes.  In the last block only the ceil(remaining / V)
 * NEEDED miniblocks have payloads; the width bytes of the others are present and are not looked at, whatever they hold; the last needed
 * miniblock is padded to V fields.
 *
 * VALUE.  v_i = v_(i-1) + min_delta(block) + field, wrapping at 64 bits.  Element i is the low 8 w bits of v_i, little-endian at dst + i w, for
 * i < min(count, cap); with w = 4 this is Parquet's INT32 arithmetic, which wraps at 32 bits.  dst has any alignment.  No byte outside
 * [dst, dst + min(count, cap) w) is written; nothing outside the 16-byte-aligned span around [src, src + len) is read.
 *
 * STOPS.  The decode ends at the first stop; everything in front of it is delivered.
 *   status                        when                                              count                                     consumed
 *   BROTLI_AMD_UNDBP_OK           all N values decoded                              N                                         the end of the last needed miniblock
 *                                                                                                                             (N <= 1: of the header)
 *   BROTLI_AMD_UNDBP_BAD_HEADER   the list above; a min_delta of more than          0; the values in front of that block      0; that block's offset
 *                                 ten bytes
 *   BROTLI_AMD_UNDBP_BAD_WIDTH    a NEEDED miniblock's width byte is above 64       the values in front of that block         that block's offset
 *   BROTLI_AMD_UNDBP_TRUNCATED    the header, a block's min_delta or its width      0; the values in front of that block      0; that block's offset
 *                                 bytes reach len
 *   BROTLI_AMD_UNDBP_TRUNCATED    a needed miniblock's payload reaches len          the values in front, the block's whole    len
 *                                                                                   miniblocks in front of it, and
 *                                                                                   floor(8 r / k) values (never more than
 *                                                                                   are still needed) of the r payload
 *                                                                                   bytes that are there
 * (With a header that was read and N != 0, `first` is a value in front of every block.  A width above 64 stops its block whatever payload in
 * front of it is cut: the width bytes come first.)  OK with consumed < len is no error: the byte data of DELTA_LENGTH_BYTE_ARRAY follows the
 * lengths, and `consumed` is how the caller finds it.
 *
 * RESULT.  Every segment gets a BrotliAmdUndbpResult in host memory.  All of its fields are independent of cap, and of how the work was shared
 * out.  declared, block_values and miniblocks are as read where the header's four varints were read (a value above 2^32 - 1 as 2^32 - 1), 0
 * elsewhere.
 *
 * Examples (bytes: values; consumed):
 *   80 01 04 05 0e 02 00 00 00 00: 7, 8, 9, 10, 11; 10
 *   80 01 04 08 0e 03 02 00 00 00 c0 3f 00 00 00 00 00 00: 7, 5, 3, 1, 2, 3, 4, 5; 18 (the format text's second example)
 *   80 01 04 01 01: -1; 5
 *   80 01 04 02 00 ff ff ff ff ff ff ff ff ff 01 00 ee ee ee: 0, -2^63; 19 (a ten-byte min_delta, junk in the unneeded width bytes)
 *
 * OUT OF PLACE ONLY: no destination range overlaps any source range or any other destination range of the call.  This is stated, not checked.
 *
 * REFUSED ON THE HOST, in front of everything that touches the device: a width outside {1, 2, 4, 8}; any flag bit; cap > 2^56; a NULL d_dst[i]
 * with caps[i] != 0.
 *
 * A call is four launches in stream order, and no block ever waits for another.  1. THE WALK, one wave a segment, on unrle's walk: it reads the
 * header and every block's min_delta and width bytes -- never a payload --, writes the segment's result, and for every ITEM of the deltas
 * (BrotliAmdDebugUndbpItemDeltas() deltas) a checkpoint: the offset and first delta of the block that holds the item's first delta.  2. THE
 * ITEMS' SUMS, one wave an item over the items of all segments: from its checkpoint the wave reads the few block headers that cover the item and
 * gives each lane a group of 32 fields; the item's sum is an undelta tile record, the first item of a segment a head that carries `first`.
 * 3. UNDELTA'S CARRY LAUNCH over those records.  4. THE EXPANSION, the same item function, a running sum inside the wave on top of the carry-in,
 * and the stores.  So one long segment is expanded by every CU; its walk is one wave's.  A call that only counts is the first launch alone
 * (csrc/brotli_undbp.h, csrc/brotli_undbp_kernels.hip).
 *
 * OUT OF SCOPE: page framing -- thrift headers, v2's level sections --; a speculative parallel walk of one
 * long segment; sign extension of elements narrower than 8 bytes.  Byte arrays behind a DICTIONARY are the undict-bytes calls' below, and the
 * lengths AND bytes of DELTA_LENGTH_BYTE_ARRAY the undlba calls', and DELTA_BYTE_ARRAY the undba calls'. */
#define BROTLI_AMD_UNDBP_OK 0u
#define BROTLI_AMD_UNDBP_BAD_HEADER 1u
#define BROTLI_AMD_UNDBP_BAD_WIDTH 2u
#define BROTLI_AMD_UNDBP_TRUNCATED 3u

typedef struct BrotliAmdUndbpResult {
  uint64_t count;         /* values decoded, whatever cap was */
  uint64_t consumed;      /* the table above */
  uint64_t declared;      /* N */
  uint64_t blocks;        /* blocks that gave at least one value */
  uint32_t status;        /* BROTLI_AMD_UNDBP_* */
  uint32_t block_values;  /* B */
  uint32_t miniblocks;    /* M */
} BrotliAmdUndbpResult;

/* n segments in DEVICE memory -- the stream in the src_lens[i] bytes at d_src[i] becomes elements of widths[i] bytes at d_dst[i], the first
 * caps[i] of them; flags == NULL or all 0; results[i] says what segment i held; any alignment, any length, 0 included; n is not bound by the
 * batch object's max_streams --: the launches run on hip_stream, and the call waits on that stream.  caps[i] == 0 needs no destination
 * (d_dst[i] is not looked at, and d_dst itself may be NULL where every capacity is 0): a call of such segments only counts.  n == 0 returns 0.
 * A negative value, and a BrotliAmdLastError text that names the segment and what was wrong, for a NULL batch, a NULL array (but flags and
 * d_dst) with n != 0, and everything in the list above: all of these are checked on the host in front of everything else, so nothing is
 * launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchUndbpSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                              const uint64_t* caps, const uint8_t* widths, const uint8_t* flags /* n entries, or NULL: all 0 */,
                                              BrotliAmdUndbpResult* results, void* hip_stream);

/* The same for the DELIVERED bytes -- [out, out + decoded_size) -- of every stream of the last decode call on the object: stream i's values go
 * to d_dst[i] (device memory of caps[i] widths[i] bytes, any alignment), and results[i] (one entry per stream) says what it held.
 * d_dst[i] == NULL skips stream i: none of its parameters are looked at and its result is zeros.  d_dst == NULL or caps == NULL: every stream is
 * counted and nothing is written.  Where the sources are, and when they are valid, is BrotliAmdBatchUnshuffleOutputs' rule exactly, for the
 * three kinds of decode call.  A stream that ended in an error or NEEDS_MORE_OUTPUT is taken over its decoded_size bytes.  The launches run on
 * the stream of that decode call and the call waits for it.  It is not a decode call itself: BrotliAmdBatchPackedOutput stays valid, and
 * BrotliAmdBatchRelaunch and the Last* accessors say what they said before.  A negative value, and a BrotliAmdLastError text, for a NULL batch,
 * widths or results, a refused width, flag or cap (nothing is launched), an object without a decode call, a last decode call that failed behind
 * its argument checks (one of no streams returns 0), and a launch that BrotliAmdBatchWait has not been called for. */
BROTLI_DEC_API int BrotliAmdBatchUndbpOutputs(BrotliAmdBatch* batch, void* const* d_dst /* or NULL */, const uint64_t* caps /* or NULL */,
                                             const uint8_t* widths, const uint8_t* flags /* or NULL */, BrotliAmdUndbpResult* results);

/* Milliseconds the undbp kernels took in the last of the two calls above (HIP events around its launches together), */
BROTLI_DEC_API float BrotliAmdBatchLastUndbpMs(BrotliAmdBatch* batch);
/* and those of phase 1 (the walk), 2 (the items' sums), 3 (the carries) or 4 (the expansion) alone; another phase: 0. */
BROTLI_DEC_API float BrotliAmdBatchLastUndbpPhaseMs(BrotliAmdBatch* batch, uint32_t phase);

/* Test hooks (no device needed).  The deltas of one item, and the source bytes that the walk stages at a time; */
BROTLI_DEC_API uint32_t BrotliAmdDebugUndbpItemDeltas(void);
BROTLI_DEC_API uint32_t BrotliAmdDebugUndbpWalkChunk(void);
/* all phases by the functions of csrc/brotli_undbp.h on the host, over n segments given as offsets into one source buffer src[0, src_size) and
 * one destination buffer dst[0, dst_size): the buffers are placed at src_skew and dst_skew (0..15) past a 16-byte boundary among bytes that are
 * not theirs.  Segment i is src_lens[i] bytes at src_offs[i]; its elements go to dst_offs[i], where there must be room for min(caps[i], count)
 * of them.  item_deltas: the deltas of an item, a multiple of 32, 0 for the device's own.  order_seed != 0: the items are taken in an order
 * shuffled by it, in the sums and in the expansion (the result may not depend on it).  0, results[0..n) filled and the elements' bytes of dst
 * written (no other byte of dst is); -1, a BrotliAmdLastError text and an untouched dst for a refused width, flag, cap or item size, a skew > 15
 * or a segment outside its buffer; -2 where a byte outside the elements' destinations changed. */
BROTLI_DEC_API int BrotliAmdDebugUndbpHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint64_t* src_offs,
                                          const uint64_t* src_lens, const uint64_t* dst_offs, const uint64_t* caps, const uint8_t* widths,
                                          const uint8_t* flags /* or NULL */, uint32_t src_skew, uint32_t dst_skew, uint32_t item_deltas,
                                          uint32_t order_seed, BrotliAmdUndbpResult* results);

/* ---- Undict on the device: dictionary-index runs of outputs back into VALUES ----
 *
 * Writers dictionary-encode almost every column by default (Parquet's RLE_DICTIONARY): a column chunk is one dictionary page -- the distinct
 * values, PLAIN, D entries of w bytes -- and data pages whose body is a width byte k and then the RLE / bit-packed hybrid of k-bit INDICES
 * into that dictionary.  The unrle calls above turn such a body into indices; these calls turn it into the values themselves, in one pass:
 * the indices never reach memory, every one of them is checked against D before it is used as an address, and every segment's result says
 * how many were out of range and where the first one was.
 *
 * THE SEGMENT AND ITS PARAMETERS.  A segment is the bytes src[0, len), read by unrle's grammar EXACTLY: headers, the two payload kinds,
 * k == 0, the stops, and count, consumed, runs, status and bits of the result.  It has a field width `bits` of 0 .. 32 (or
 * BROTLI_AMD_UNDICT_WIDTH_BYTE: the segment's first byte is k, unrle's meaning), an element width w in {1, 2, 4, 8}, a capacity cap in
 * elements, a destination dst, and a DICTIONARY: dict, device memory of any alignment, and dict_entries = D.  The index width is NOT bound by
 * w: the only bound is k <= 32, for the argument and for the width byte alike -- a uint8 dictionary addressed by 12-bit fields is legal.
 *
 * VALUE.  Element i, i < min(count, cap), is the w bytes at dict + idx_i w, copied as they are, where idx_i < D.  Where idx_i >= D the element
 * is 0, nothing is read through that index, and the element is counted as bad.  An RLE run's value is not masked to k bits (unrle's rule), so
 * it may be out of range like any other index.  With D == 0 every element is bad and dict is not looked at.
 *
 * RESULT.  BrotliAmdUndictResult, 48 bytes: unrle's five fields in unrle's order and meaning -- independent of cap and of how the work was
 * shared out --, then bad, the DELIVERED elements whose index was >= D, and first_bad, the smallest such element index (UINT64_MAX: none).
 * bad and first_bad are about delivered elements only: they depend on cap, and a call that only counts gives 0 and UINT64_MAX; they do not
 * depend on how the work was shared out.  A skipped stream's result is zeros, with first_bad UINT64_MAX.
 *
 * LOADS AND STORES.  No byte outside [dst, dst + min(count, cap) w) is written.  Nothing outside the 16-byte-aligned span around
 * [src, src + len) is read, and nothing outside the 16-byte-aligned span around [dict, dict + D w): an entry is one load of w bytes where
 * dict is a multiple of w, and single bytes elsewhere.  OUT OF PLACE: no destination overlaps a source, a dictionary or another destination.
 * This is stated, not checked.
 *
 * Examples (k, bytes, dictionary): 3, 03 88 C6 FA over eight uint16 entries: the eight entries in order;  3, 10 05 with D = 5: 8 zeros,
 * bad 8, first_bad 0;  the same with D = 6: 8 x entry 5, bad 0;  0, 07: 24 x entry 0.
 *
 * REFUSED ON THE HOST, in front of everything that touches the device, with a text that names the segment: a width outside {1, 2, 4, 8};
 * unknown flag bits; bits > 32 without the width-byte flag; cap > 2^56; a NULL destination with cap != 0; a NULL dict with dict_entries != 0
 * and cap != 0; dict_entries > 2^56.
 *
 * A call is two launches in stream order, and no block ever waits for another.  1. THE WALK: unrle's, as it is.  2. THE EXPANSION WITH THE
 * LOOKUP, one wave an item over the items of all segments: a lane forms the indices of a group of its 16 neighbouring elements, issues their dictionary
 * loads together -- inside an RLE run one lookup serves every element of the run that the lane holds --, and puts the aligned 16-byte words
 * together.  The dictionary is read through the caches.  Bad indices are summed up inside the wave; an item that has some adds them to its
 * segment's result with one atomic add and one atomic minimum (csrc/brotli_undict.h, csrc/brotli_undict_kernels.hip).
 *
 * OUT OF SCOPE: FIXED_LEN_BYTE_ARRAY and INT96 dictionaries (entries of 12 or 16 bytes); page framing; plain index arrays (a framework's
 * gather does those); a parallel walk of one long segment.  BYTE_ARRAY dictionaries -- entries of variable bytes -- are the undict-bytes
 * calls' below.  Definition levels and the spreading of values over nulls are the unnull calls' below. */
#define BROTLI_AMD_UNDICT_WIDTH_BYTE 1u          /* BROTLI_AMD_UNRLE_WIDTH_BYTE's meaning */
#define BROTLI_AMD_UNDICT_NO_STREAM 0xFFFFFFFFu  /* dict_streams[i]: the dictionary is d_dicts[i], not a stream of the decode call */

typedef struct BrotliAmdUndictResult {
  uint64_t count;      /* values in all runs, whatever cap was */
  uint64_t consumed;   /* unrle's table */
  uint64_t runs;       /* runs that gave at least one value */
  uint32_t status;     /* BROTLI_AMD_UNRLE_* */
  uint32_t bits;       /* the k that was used */
  uint64_t bad;        /* delivered elements whose index was >= D */
  uint64_t first_bad;  /* the smallest such element index; UINT64_MAX: none */
} BrotliAmdUndictResult;

/* n segments in DEVICE memory -- the runs in the src_lens[i] bytes at d_src[i], of fields of bits[i] bits, index the dict_entries[i] entries of
 * widths[i] bytes at d_dicts[i], and the first caps[i] values go to d_dst[i], by flags[i] (flags == NULL: all 0); results[i] says what
 * segment i held; any alignment, any length, 0 included; n is not bound by the batch object's max_streams --: the launches run on hip_stream,
 * and the call waits on that stream.  caps[i] == 0 only counts: d_dst[i], d_dicts[i] and dict_entries[i] are not looked at but for the
 * refusals above, and d_dst, d_dicts and dict_entries themselves may be NULL where every capacity is 0.  n == 0 returns 0.  A negative value,
 * and a BrotliAmdLastError text that names the segment and what was wrong, for a NULL batch, a NULL array (but flags, and the three just
 * named) with n != 0, and everything in the list above: all of these are checked on the host in front of everything else, so nothing is
 * launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchUndictSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, const size_t* src_lens, void* const* d_dst,
                                               const uint64_t* caps, const uint8_t* bits, const uint8_t* widths,
                                               const uint8_t* flags /* n entries, or NULL: all 0 */, const void* const* d_dicts,
                                               const uint64_t* dict_entries, BrotliAmdUndictResult* results, void* hip_stream);

/* The same for the DELIVERED bytes of every stream of the last decode call on the object, by BrotliAmdBatchUnrleOutputs' rules for the three
 * kinds of decode call, for skipped streams (d_dst[i] == NULL: none of the stream's parameters are looked at) and for counting (d_dst == NULL
 * or caps == NULL).  dict_streams[i] below the call's stream count names the stream OF THE SAME DECODE CALL whose delivered bytes are stream
 * i's dictionary -- the Brotli-compressed dictionary page in the same batch --, with D = floor(decoded_size / widths[i]); such a stream is
 * normally skipped as a data stream itself.  BROTLI_AMD_UNDICT_NO_STREAM, or dict_streams == NULL, takes d_dicts[i] and dict_entries[i]: a
 * dictionary that an earlier call decoded (d_dicts and dict_entries may be NULL where no stream that writes takes them).  A stream that names
 * itself, and an index at or above the stream count that is not BROTLI_AMD_UNDICT_NO_STREAM, are refused.  A negative value, and a
 * BrotliAmdLastError text, for a NULL batch, bits, widths or results, a refusal (nothing is launched), an object without a decode call, a last
 * decode call that failed behind its argument checks (one of no streams returns 0), and a launch that BrotliAmdBatchWait has not been called
 * for. */
BROTLI_DEC_API int BrotliAmdBatchUndictOutputs(BrotliAmdBatch* batch, void* const* d_dst /* or NULL */, const uint64_t* caps /* or NULL */,
                                              const uint8_t* bits, const uint8_t* widths, const uint8_t* flags /* or NULL */,
                                              const uint32_t* dict_streams /* or NULL */, const void* const* d_dicts /* or NULL */,
                                              const uint64_t* dict_entries /* or NULL */, BrotliAmdUndictResult* results);

/* Milliseconds the undict kernels took in the last of the two calls above (HIP events around its launches together), */
BROTLI_DEC_API float BrotliAmdBatchLastUndictMs(BrotliAmdBatch* batch);
/* and those of phase 1 (the walk) or 2 (the expansion with the lookup) alone; another phase: 0. */
BROTLI_DEC_API float BrotliAmdBatchLastUndictPhaseMs(BrotliAmdBatch* batch, uint32_t phase);

/* Test hook (no device needed): both phases by the functions of csrc/brotli_unrle.h and csrc/brotli_undict.h on the host.  It has
 * BrotliAmdDebugUnrleHost's shape -- and its item size, BrotliAmdDebugUnrleItemElems() -- plus one dictionary buffer dict[0, dict_size), placed
 * at dict_skew (0..15) past a 16-byte boundary in a room of its own: segment i's dictionary is dict_entries[i] entries of widths[i] bytes at
 * dict_offs[i].  The items are taken in an order shuffled by order_seed (bad and first_bad may not depend on it).  0, -1 and -2 as there; -1
 * also for a dictionary outside its buffer. */
BROTLI_DEC_API int BrotliAmdDebugUndictHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint8_t* dict,
                                           size_t dict_size, const uint64_t* src_offs, const uint64_t* src_lens, const uint64_t* dst_offs,
                                           const uint64_t* caps, const uint64_t* dict_offs, const uint64_t* dict_entries, const uint8_t* bits,
                                           const uint8_t* widths, const uint8_t* flags /* or NULL */, uint32_t src_skew, uint32_t dst_skew,
                                           uint32_t dict_skew, uint32_t item_elems, uint32_t order_seed, BrotliAmdUndictResult* results);

/* ---- Undict for byte arrays on the device: dictionary-index runs of outputs back into OFFSETS AND BYTES ----
 *
 * String columns are the columns that writers dictionary-encode most reliably: a column chunk is one dictionary page -- PLAIN BYTE_ARRAY: per
 * entry a 4-byte little-endian length, then that many bytes -- and data pages whose body is what undict walks: a width byte k, then RLE /
 * bit-packed runs of k-bit indices.  These calls take the index runs and such a dictionary and write an Arrow string column, (offsets, data),
 * in one call: the indices never reach memory, and every one of them is checked against D before it becomes an address.
 *
 * THE SEGMENT AND ITS PARAMETERS.  A segment is an undict segment: src[0, len) is read by unrle's grammar EXACTLY -- headers, the two payload
 * kinds, k == 0, the stops, and count, consumed, runs, status and bits of the result --, with `bits` of 0 .. 32 (or
 * BROTLI_AMD_UNDICT_BYTES_WIDTH_BYTE: the segment's first byte is k) and a capacity cap in ELEMENTS.  Instead of an element width it has:
 *
 * THE DICTIONARY.  dict_len bytes at dict, device memory of any alignment, read as PLAIN byte arrays: entry e is a little-endian uint32 length
 * L_e, then L_e bytes.  dict_entries bounds how many entries are taken -- the page header's num_values --; BROTLI_AMD_UNDICT_BYTES_ALL: as many
 * as the bytes hold.  The dictionary ends at dict_entries entries, at dict_len exactly (dict_status BROTLI_AMD_UNDICT_BYTES_DICT_OK), or at
 * the first entry whose 4 length bytes or L_e value bytes the end cuts: BROTLI_AMD_UNDICT_BYTES_DICT_CUT; the entries in front of the cut
 * count, and D is their number.  Bytes left over behind dict_entries whole entries are no error.  Entry positions are 32-bit: dict_len >= 2^32
 * is refused, and a length that does not fit is simply a cut.
 *
 * THE OUTPUTS.  m = min(count, cap); element i < m has the index idx_i, by unrle's rule (an RLE run's value is not masked to k bits).  Where
 * idx_i < D the element's bytes are entry idx_i's, L_i of them; where idx_i >= D the element is EMPTY (L_i = 0), nothing is read through the
 * index, and the element is counted as bad.  bytes = the sum of L_i over i < m, 64 bits, independent of data_cap.
 *   OFFSETS  offsets[i] = offset_base + the sum of L_j over j < i, for i = 0 .. m, little-endian integers of 4 bytes -- of 8 with
 *            BROTLI_AMD_UNDICT_BYTES_OFFSETS64 --, truncated to that width, at d_offsets.  With BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY offsets[0] is
 *            not written, d_offsets points at offsets[1], and m entries are written: the pages of one column chunk append into one Arrow array
 *            without two segments writing the same word.  d_offsets == NULL: no offsets.
 *   DATA     d_data[0, min(bytes, data_cap)) is the concatenation of the elements' bytes, cut at data_cap byte-exactly.  d_data == NULL needs
 *            data_cap == 0.
 * A call with cap != 0 and neither destination only MEASURES: the caller knows its rows from the page header but not its bytes, and
 * result.bytes is how it sizes d_data for a second call.  (cap is the page's rows, not a large constant: as in unrle, a call's room on the
 * device grows with the items that its capacities name.)  cap == 0 only counts, as in unrle: nothing of the dictionary is looked at.
 *
 * RESULT.  BrotliAmdUndictBytesResult, 80 bytes: undict's seven fields in undict's order and meaning, then bytes, dict_entries (the D that was
 * used), dict_consumed (the bytes of the D entries), dict_status and a reserved 0.  Nothing in it depends on how the work was shared out.  A
 * skipped stream gives zeros with first_bad UINT64_MAX.
 *
 * LOADS AND STORES.  No byte outside [d_data, d_data + min(bytes, data_cap)) and outside the offsets named above is written.  Nothing outside
 * the 16-byte-aligned spans around [src, src + len) and [dict, dict + dict_len) is read.  OUT OF PLACE: no destination overlaps a source, a
 * dictionary or another destination.  This is stated, not checked.
 *
 * Examples (k, bytes, dictionary): 3, 03 88 C6 FA over the eight entries "", "a", "bc", ...: the eight in order;  3, 10 05 with D = 5: eight
 * empty elements, bad 8, first_bad 0, bytes 0;  the same with D = 6: 8 x entry 5;  0, 07: 24 x entry 0;  a dictionary whose third entry is cut
 * inside its length bytes: D = 2, DICT_CUT.
 *
 * REFUSED ON THE HOST, in front of everything that touches the device, with a text that names the segment: unknown flag bits; bits > 32
 * without the width-byte flag; cap > 2^56; data_cap != 0 with a NULL d_data; a NULL dict with dict_len != 0 and cap != 0; dict_len >= 2^32.
 *
 * A call is five launches in stream order, and no block ever waits for another -- no spins, no flags, no atomics on offsets or data.
 * 1. THE DICTIONARY WALK: the host makes the table of the call's DISTINCT dictionaries -- segments that name the same (pointer, length, bound)
 * share one record, the normal case for the pages of a chunk --; one wave a dictionary follows its length chain and writes starts[e], the
 * position of entry e's first value byte, for e = 0 .. D -- a sentinel behind the last, so that L_e = starts[e + 1] - 4 - starts[e] for every
 * e < D.  2. THE RLE WALK: unrle's, as it is.  3. THE LENGTHS, one wave an item: the indices, each compared with D in 64 bits by the one function
 * that turns (starts, D, idx) into (position, length, bad), the lengths summed into the item's tile record; bad elements go to the segment's
 * result with one atomic add and one atomic minimum.  4. THE CARRIES: undelta's carry launch.  5. THE EXPANSION, one wave an item: the lanes
 * redo indices and lengths, a scan on top of the item's carry-in gives every element its offset; offsets go out as aligned 16-byte stores, single
 * elements at the edges; the BYTES are written with the work split by the DESTINATION: the lanes stride over the aligned 16-byte words of the
 * item's range, each finds its word's first element by a binary search of the item's offsets in LDS, puts the word together from consecutive
 * elements' bytes and stores it once; the range's head and tail are single bytes (csrc/brotli_undict_bytes.h,
 * csrc/brotli_undict_bytes_kernels.hip).  A measuring call runs the same launches with every store predicated off.
 *
 * One item -- 1024 elements -- is one wave's work whatever its bytes: splitting an item of very long strings over several waves is out of
 * scope.  ALSO OUT OF SCOPE: PLAIN (non-dictionary) byte-array data pages (DELTA_LENGTH_BYTE_ARRAY is the undlba calls' below, DELTA_BYTE_ARRAY the undba calls'); FIXED_LEN_BYTE_ARRAY
 * and INT96 dictionaries; nullable string columns in one call -- unnull over byte arrays; a caller uses BrotliAmdBatchUnnullOutputs' counting
 * call to find where a v1 index body begins --; page framing; keeping a dictionary's starts from one call to the next; a parallel walk of one
 * long dictionary or segment. */
#define BROTLI_AMD_UNDICT_BYTES_WIDTH_BYTE 1u   /* BROTLI_AMD_UNRLE_WIDTH_BYTE's meaning */
#define BROTLI_AMD_UNDICT_BYTES_OFFSETS64 2u    /* offsets of 8 bytes */
#define BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY 4u    /* offsets[0] is not written, and d_offsets points at offsets[1] */
#define BROTLI_AMD_UNDICT_BYTES_SKIP 8u         /* BrotliAmdBatchUndictBytesOutputs: the stream is skipped */
#define BROTLI_AMD_UNDICT_BYTES_ALL 0xFFFFFFFFFFFFFFFFull   /* dict_entries: as many entries as the bytes hold */
#define BROTLI_AMD_UNDICT_BYTES_DICT_OK 0u
#define BROTLI_AMD_UNDICT_BYTES_DICT_CUT 1u

typedef struct BrotliAmdUndictBytesResult {
  uint64_t count;          /* values in all runs, whatever cap was */
  uint64_t consumed;       /* unrle's table */
  uint64_t runs;           /* runs that gave at least one value */
  uint32_t status;         /* BROTLI_AMD_UNRLE_* */
  uint32_t bits;           /* the k that was used */
  uint64_t bad;            /* delivered elements whose index was >= D */
  uint64_t first_bad;      /* the smallest such element index; UINT64_MAX: none */
  uint64_t bytes;          /* of the delivered elements together, whatever data_cap was */
  uint64_t dict_entries;   /* the D that was used */
  uint64_t dict_consumed;  /* the dictionary's bytes that those entries take */
  uint32_t dict_status;    /* BROTLI_AMD_UNDICT_BYTES_DICT_* */
  uint32_t reserved;       /* 0 */
} BrotliAmdUndictBytesResult;

/* n segments in DEVICE memory: the runs in the src_lens[i] bytes at d_src[i], of fields of bits[i] bits, index the byte arrays of the
 * dict_lens[i] bytes at d_dicts[i], at most dict_entries[i] of them (dict_entries == NULL: all ALL); the first caps[i] elements' offsets go to
 * d_offsets[i] on top of offset_bases[i] (NULL: all 0) and their bytes to d_data[i], at most data_caps[i] of them, by flags[i] (NULL: all 0);
 * results[i] says what segment i held.  d_offsets and d_data, or single entries of them, may be NULL (data_caps too, where d_data is): that
 * destination is not written.  caps[i] == 0 only counts: d_dicts and dict_lens may be NULL where every capacity is 0.  The launches run on
 * hip_stream, and the call waits on that stream.  n == 0 returns 0.  A negative value, and a BrotliAmdLastError text that names the segment
 * and what was wrong, for a NULL batch, a NULL array (but those named) with n != 0, BROTLI_AMD_UNDICT_BYTES_SKIP and everything in the list
 * above: all checked on the host in front of everything else, so nothing is launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchUndictBytesSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, const size_t* src_lens,
                                                    void* const* d_offsets /* or NULL */, void* const* d_data /* or NULL */,
                                                    const uint64_t* data_caps /* or NULL */, const uint64_t* caps, const uint8_t* bits,
                                                    const uint8_t* flags /* or NULL */, const uint64_t* offset_bases /* or NULL */,
                                                    const void* const* d_dicts, const uint64_t* dict_lens, const uint64_t* dict_entries /* or NULL */,
                                                    BrotliAmdUndictBytesResult* results, void* hip_stream);

/* The same for the DELIVERED bytes of every stream of the last decode call on the object, by BrotliAmdBatchUndictOutputs' rules for the three
 * kinds of decode call.  A stream with BROTLI_AMD_UNDICT_BYTES_SKIP in flags[i] is skipped: none of its other parameters are looked at and
 * its result is zeros -- the dictionary pages of the batch.  caps == NULL counts every stream and nothing else.  dict_streams[i] below the
 * call's stream count names the stream OF THE SAME DECODE CALL whose delivered bytes are stream i's dictionary, dict_len being its delivered
 * size: a dictionary stream that was delivered truncated is simply a shorter dictionary.  BROTLI_AMD_UNDICT_NO_STREAM, or dict_streams ==
 * NULL, takes d_dicts[i] and dict_lens[i].  dict_entries[i] bounds either kind.  A stream that names itself, and an index at or above the
 * stream count that is not BROTLI_AMD_UNDICT_NO_STREAM, are refused.  A negative value, and a BrotliAmdLastError text, as there. */
BROTLI_DEC_API int BrotliAmdBatchUndictBytesOutputs(BrotliAmdBatch* batch, void* const* d_offsets /* or NULL */, void* const* d_data /* or NULL */,
                                                   const uint64_t* data_caps /* or NULL */, const uint64_t* caps /* or NULL */, const uint8_t* bits,
                                                   const uint8_t* flags /* or NULL */, const uint64_t* offset_bases /* or NULL */,
                                                   const uint32_t* dict_streams /* or NULL */, const void* const* d_dicts /* or NULL */,
                                                   const uint64_t* dict_lens /* or NULL */, const uint64_t* dict_entries /* or NULL */,
                                                   BrotliAmdUndictBytesResult* results);

/* Milliseconds the undict-bytes kernels took in the last of the two calls above (HIP events around its launches together), */
BROTLI_DEC_API float BrotliAmdBatchLastUndictBytesMs(BrotliAmdBatch* batch);
/* and those of phase 1 (the dictionary walk), 2 (the RLE walk), 3 (the lengths), 4 (the carries) or 5 (the expansion) alone; another: 0. */
BROTLI_DEC_API float BrotliAmdBatchLastUndictBytesPhaseMs(BrotliAmdBatch* batch, uint32_t phase);

/* Test hook (no device needed): all five phases by the functions of csrc/brotli_unrle.h and csrc/brotli_undict_bytes.h on the host.  It has
 * BrotliAmdDebugUndictHost's shape with four buffers, each placed at its skew (0..15) past a 16-byte boundary in a room of its own: the source,
 * the offsets, the data and the dictionaries.  Segment i's runs are src_lens[i] bytes at src_offs[i], its offsets go to offsets_offs[i] and
 * its bytes to data_offs[i] (UINT64_MAX: that destination is NULL), its dictionary is dict_lens[i] bytes at dict_offs[i].  Segments that name
 * the same (offset, length, bound) share one dictionary walk, and *dict_walks (where not NULL) is the number of walks.  The items are taken in
 * orders shuffled by order_seed, and an item's destination words in an order shuffled by word_seed: no result and no byte may depend on
 * either.  0; -1 and a BrotliAmdLastError text for arguments that are refused or a segment, destination or dictionary outside its buffer; -2
 * where a byte outside the destinations named above changed. */
BROTLI_DEC_API int BrotliAmdDebugUndictBytesHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* offsets, size_t offsets_size, uint8_t* data,
                                                size_t data_size, const uint8_t* dict, size_t dict_size, const uint64_t* src_offs,
                                                const uint64_t* src_lens, const uint64_t* offsets_offs, const uint64_t* data_offs,
                                                const uint64_t* data_caps, const uint64_t* caps, const uint64_t* offset_bases,
                                                const uint64_t* dict_offs, const uint64_t* dict_lens, const uint64_t* dict_entries,
                                                const uint8_t* bits, const uint8_t* flags /* or NULL */, uint32_t src_skew, uint32_t offsets_skew,
                                                uint32_t data_skew, uint32_t dict_skew, uint32_t item_elems, uint32_t order_seed, uint32_t word_seed,
                                                BrotliAmdUndictBytesResult* results, uint64_t* dict_walks /* or NULL */);

/* ---- Undlba on the device: DELTA_LENGTH_BYTE_ARRAY of outputs back into OFFSETS AND BYTES ----
 *
 * DELTA_LENGTH_BYTE_ARRAY is the one string encoding of Parquet that is parallel by construction: all lengths first, as one DELTA_BINARY_PACKED
 * stream, then all values' bytes back to back.  A writer uses it for strings that are not dictionary-encoded.  These calls turn such a page
 * body into an Arrow string column -- (offsets, data) -- in one call: the lengths are never an array in memory, every length is checked, and
 * the bytes are one contiguous copy that is spread over the whole device.
 *
 * THE SEGMENT AND ITS PARAMETERS.  A segment is src[0, len) in device memory, at any alignment: a DELTA_BINARY_PACKED stream of N lengths and,
 * directly behind it, the values' bytes.  Per segment: a capacity cap in ELEMENTS, flags, offset_base, the destinations d_offsets and d_data,
 * and data_cap in bytes.
 *
 * LENGTHS.  The front part is read by undbp's grammar EXACTLY: the header, the blocks, the stops, the 64-bit wrapping value rule.  The
 * result's first seven fields -- count, consumed, declared, blocks, status, block_values, miniblocks -- are those of BrotliAmdUndbpResult for
 * the same bytes and the same cap, with undbp's meaning and undbp's status codes.  m = min(count, cap).  The length of element i < m is L_i,
 * the low 32 bits of v_i as a signed int32: Parquet's INT32 arithmetic, and what Arrow's decoder computes.  L_i < 0 makes the element BAD: it
 * is EMPTY (its length counts as 0), it is counted in `bad`, and the smallest such i is first_bad (UINT64_MAX: none).  `bytes` is the sum of
 * the good L_i over i < m, in 64 bits, whatever data_cap is.
 *
 * DATA.  The data begins at src + consumed, whatever the status is, and data_avail = len - consumed.  data_status is
 * BROTLI_AMD_UNDLBA_DATA_OK where bytes <= data_avail and BROTLI_AMD_UNDLBA_DATA_SHORT otherwise.  Delivered is
 * d_data[0, min(bytes, data_avail, data_cap)), and it equals src[consumed, ...) byte for byte; the cut is exact to the byte.
 * data_avail > bytes is no error where cap < count; where cap >= count it is the caller's to judge -- a page of a nullable column is one such
 * case --, and both numbers are in the result.
 *
 * OFFSETS.  offsets[i] = offset_base + the sum of L_j over j < i, for i = 0 .. m: little-endian integers of 4 bytes, or of 8 with
 * BROTLI_AMD_UNDLBA_OFFSETS64, truncated to that width.  They follow the lengths also where the data is SHORT or cut.  With
 * BROTLI_AMD_UNDLBA_ENDS_ONLY offsets[0] is not written, d_offsets points at offsets[1] and m entries are written -- as in undict-bytes, so
 * that the pages of a chunk append into one Arrow array.  With cap != 0, a d_offsets that is not NULL and no ENDS_ONLY, offsets[0] is written
 * even where m == 0: a page with N == 0 is one such case.
 *
 * KINDS OF CALL.  cap == 0 only COUNTS and is the walk alone: the seven undbp fields and data_avail are filled, bytes and bad are 0 and
 * first_bad is UINT64_MAX.  This is how a caller sizes d_data: a well-formed page has bytes == data_avail.  cap != 0 with neither destination
 * only MEASURES: the same launches with every store off.  BROTLI_AMD_UNDLBA_SKIP is for BrotliAmdBatchUndlbaOutputs alone: the stream is
 * skipped, and its result is zeros with first_bad UINT64_MAX.
 *
 * RESULT.  BrotliAmdUndlbaResult, 80 bytes.  Nothing in it depends on data_cap or on how the work was shared out; only bad, first_bad and
 * bytes depend on cap.
 *
 * Examples (bytes: elements; offsets; other results):
 *   80 01 04 04 00 02 00 00 00 00 61 62 62 63 63 63: "", "a", "bb", "ccc"; 0 0 1 3 6; consumed 10, bytes 6, data_avail 6
 *   80 01 04 01 06 78 79 7a: "xyz"; 0 3; consumed 5
 *   80 01 04 01 01 61 62: one length of -1; 0 0; bad 1, first_bad 0, bytes 0, data_avail 2, DATA_OK, no data byte written
 *   80 01 04 01 0a 61 62: one length of 5 over 2 bytes; 0 5; bytes 5, data_avail 2, DATA_SHORT, data "ab"
 *   80 01 04 00 00: none (N = 0); offset_base alone; count 0, consumed 5
 *
 * LOADS AND STORES.  No byte is written outside [d_data, d_data + min(bytes, data_avail, data_cap)) and outside the offsets named above;
 * nothing is read outside the 16-byte-aligned span around [src, src + len).  OUT OF PLACE ONLY: stated, not checked.
 *
 * REFUSED ON THE HOST, in front of everything that touches the device, with a BrotliAmdLastError text that names the segment: unknown flag
 * bits; BROTLI_AMD_UNDLBA_SKIP in the Segments call; cap > 2^56; data_cap != 0 with a NULL d_data; a NULL array with n != 0, but those named
 * as optional.
 *
 * A call is seven launches in stream order, and no block ever waits for another: no spins, no flags, no atomics on offsets or data.  1. THE
 * WALK, undbp's as it is, one wave a segment: the result's first seven fields, data_avail, the first value and the items' checkpoints.
 * 2. THE DELTA SUMS, undbp's item function and group sum, one wave an item of BrotliAmdDebugUndbpItemDeltas() deltas: an undelta tile record
 * an item.  3. UNDELTA'S CARRY LAUNCH: the value in front of every item's first delta.  4. THE LENGTHS, one wave an item: the lanes redo their
 * 32 values on top of the carry-in and turn each into (L, bad) by one function; the wave's sum of good lengths is a second tile record, and
 * the item's bad elements go to the result with one atomic add and one atomic minimum.  5. UNDELTA'S CARRY LAUNCH again, over the byte sums:
 * the bytes in front of every item.  6. THE OFFSETS, one wave an item: a scan over the lanes' byte sums on top of the carry-in gives a lane
 * its first offset; it stores its 32 neighbouring entries as aligned 16-byte words wherever it has a whole word, and singly at its two ends.
 * The item that holds the segment's last delivered element writes bytes, data_status and the segment's entry of a table of copies on the
 * device: src + consumed, d_data, min(bytes, data_avail, data_cap).  7. THE DATA: the ragged copy kernel itself over that table, the work
 * split by bytes -- one page of a gigabyte of strings is spread over every CU, and an item of very long strings is nobody's single wave
 * (csrc/brotli_undlba.h, csrc/brotli_undlba_kernels.hip).
 *
 * OUT OF SCOPE: PLAIN byte-array pages (DELTA_BYTE_ARRAY is the undba calls' below); nullable string columns in one call; repetition levels; page
 * framing; a parallel walk of one long segment; lengths wider than INT32. */
#define BROTLI_AMD_UNDLBA_OFFSETS64 2u    /* offsets of 8 bytes */
#define BROTLI_AMD_UNDLBA_ENDS_ONLY 4u    /* offsets[0] is not written, and d_offsets points at offsets[1] */
#define BROTLI_AMD_UNDLBA_SKIP 8u         /* BrotliAmdBatchUndlbaOutputs: the stream is skipped */
#define BROTLI_AMD_UNDLBA_DATA_OK 0u
#define BROTLI_AMD_UNDLBA_DATA_SHORT 1u

typedef struct BrotliAmdUndlbaResult {
  uint64_t count;         /* lengths decoded, whatever cap was */
  uint64_t consumed;      /* undbp's: where the data begins */
  uint64_t declared;      /* N */
  uint64_t blocks;        /* blocks that gave at least one length */
  uint32_t status;        /* BROTLI_AMD_UNDBP_* */
  uint32_t block_values;  /* B */
  uint32_t miniblocks;    /* M */
  uint32_t data_status;   /* BROTLI_AMD_UNDLBA_DATA_* */
  uint64_t bad;           /* delivered elements whose length was negative */
  uint64_t first_bad;     /* the smallest such element index; UINT64_MAX: none */
  uint64_t bytes;         /* of the delivered elements together, whatever data_cap was */
  uint64_t data_avail;    /* len - consumed */
} BrotliAmdUndlbaResult;

/* n segments in DEVICE memory: the lengths and bytes in the src_lens[i] bytes at d_src[i]; the first caps[i] elements' offsets go to
 * d_offsets[i] on top of offset_bases[i] (NULL: all 0) and their bytes to d_data[i], at most data_caps[i] of them, by flags[i] (NULL: all 0);
 * results[i] says what segment i held.  d_offsets and d_data, or single entries of them, may be NULL (data_caps too, where d_data is): that
 * destination is not written.  The launches run on hip_stream, and the call waits on that stream.  n == 0 returns 0.  A negative value, and a
 * BrotliAmdLastError text that names the segment and what was wrong, for a NULL batch, a NULL array (but those named) with n != 0 and
 * everything in the list above: all checked on the host in front of everything else, so nothing is launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchUndlbaSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, const size_t* src_lens,
                                               void* const* d_offsets /* or NULL */, void* const* d_data /* or NULL */,
                                               const uint64_t* data_caps /* or NULL */, const uint64_t* caps, const uint8_t* flags /* or NULL */,
                                               const uint64_t* offset_bases /* or NULL */, BrotliAmdUndlbaResult* results, void* hip_stream);

/* The same for the DELIVERED bytes of every stream of the last decode call on the object, by BrotliAmdBatchUndbpOutputs' rules for the three
 * kinds of decode call.  A stream with BROTLI_AMD_UNDLBA_SKIP in flags[i] is skipped: none of its other parameters are looked at and its
 * result is zeros with first_bad UINT64_MAX.  caps == NULL counts every stream and nothing else.  A negative value, and a BrotliAmdLastError
 * text, as there. */
BROTLI_DEC_API int BrotliAmdBatchUndlbaOutputs(BrotliAmdBatch* batch, void* const* d_offsets /* or NULL */, void* const* d_data /* or NULL */,
                                              const uint64_t* data_caps /* or NULL */, const uint64_t* caps /* or NULL */,
                                              const uint8_t* flags /* or NULL */, const uint64_t* offset_bases /* or NULL */,
                                              BrotliAmdUndlbaResult* results);

/* Milliseconds the undlba kernels took in the last of the two calls above (HIP events around its launches together), */
BROTLI_DEC_API float BrotliAmdBatchLastUndlbaMs(BrotliAmdBatch* batch);
/* and those of phase 1 (the walk), 2 (the delta sums), 3 (their carries), 4 (the lengths), 5 (their carries), 6 (the offsets) or 7 (the
 * data) alone; another: 0. */
BROTLI_DEC_API float BrotliAmdBatchLastUndlbaPhaseMs(BrotliAmdBatch* batch, uint32_t phase);

/* Test hook (no device needed): all phases by the functions of csrc/brotli_undbp.h and csrc/brotli_undlba.h on the host.  Three buffers, each
 * placed at its skew (0..15) past a 16-byte boundary in a room of its own: the source, the offsets and the data.  Segment i is src_lens[i]
 * bytes at src_offs[i]; its offsets go to offsets_offs[i] and its bytes to data_offs[i] (UINT64_MAX: that destination is NULL).
 * item_deltas: the deltas of an item, a multiple of 32, 0 for the device's own.  order_seed != 0: the items are taken in orders shuffled by
 * it, in every phase (no result and no byte may depend on it).  0; -1 and a BrotliAmdLastError text for arguments that are refused or a
 * segment or destination outside its buffer; -2 where a byte outside the destinations named above changed. */
BROTLI_DEC_API int BrotliAmdDebugUndlbaHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* offsets, size_t offsets_size, uint8_t* data,
                                           size_t data_size, const uint64_t* src_offs, const uint64_t* src_lens, const uint64_t* offsets_offs,
                                           const uint64_t* data_offs, const uint64_t* data_caps, const uint64_t* caps,
                                           const uint64_t* offset_bases, const uint8_t* flags /* or NULL */, uint32_t src_skew,
                                           uint32_t offsets_skew, uint32_t data_skew, uint32_t item_deltas, uint32_t order_seed,
                                           BrotliAmdUndlbaResult* results);

/* ---- Undba on the device: DELTA_BYTE_ARRAY of outputs back into OFFSETS AND BYTES ----
 *
 * DELTA_BYTE_ARRAY is Parquet's front coding: element i is the first p_i bytes of element i - 1 and then s_i bytes of its own.  Writers choose
 * it for sorted strings and keys -- URLs, paths, ids --, and it is parquet-mr's default for BYTE_ARRAY under the V2 encodings.  These calls
 * turn such a page body into an Arrow string column -- (offsets, data) -- in one call; the chain of prefix copies through the whole page is
 * resolved on the device, by a local phase an item, a carry over the items' last elements, and a fill.
 *
 * THE SEGMENT AND ITS PARAMETERS.  A segment is src[0, len) in device memory, at any alignment, three parts directly behind one another: a
 * DELTA_BINARY_PACKED stream P of N prefix lengths; a DELTA_BINARY_PACKED stream S of suffix lengths, from consumed_p on; the suffix bytes,
 * back to back, from consumed_p + consumed_s on.  S and the bytes together are exactly a DELTA_LENGTH_BYTE_ARRAY body.  Per segment, as in
 * undlba: a capacity cap in ELEMENTS, flags, offset_base, the destinations d_offsets and d_data, and data_cap in bytes.
 *
 * LENGTHS.  Both streams are read by undbp's grammar EXACTLY.  The result carries undbp's seven fields for P (.._p) and for S (.._s), S being
 * read from src + consumed_p over len - consumed_p bytes -- consumed_s counts from there --, each with the meaning and the status codes of
 * BrotliAmdUndbpResult for the same bytes and the same cap.  S is read from P's consumed whatever P's status is.  m = min(count_p, count_s,
 * cap).  p_i and s_i are the low 32 bits of the values as signed int32.
 *
 * BAD ELEMENTS.  D_i = p_i + s_i in 64 bits, D_-1 = 0.  Element i < m breaks the rules where p_i < 0 (BROTLI_AMD_UNDBA_BAD_PREFIX_NEGATIVE),
 * s_i < 0 (.._SUFFIX_NEGATIVE) or p_i > D_(i-1) (.._PREFIX_LONG): the first element's prefix is 0.  first_bad is the smallest such i
 * (UINT64_MAX: none) and bad_kind the first of the three rules, in that order, that it broke.  Elements i >= first_bad are EMPTY: L_i = 0.
 * Elements i < first_bad have L_i = D_i.  A bad prefix poisons everything behind it -- Arrow's decoder throws there --, unlike undlba's
 * "empty and go on".  The upper 32 bits of a value are not looked at.
 *
 * OFFSETS.  Exactly undlba's rule over these L_i: offsets[i] = offset_base + the sum of L_j over j < i, i = 0 .. m, of 4 bytes or of 8 with
 * BROTLI_AMD_UNDBA_OFFSETS64, truncated; with BROTLI_AMD_UNDBA_ENDS_ONLY offsets[0] is not written and d_offsets points at offsets[1]; with
 * cap != 0, a d_offsets and no ENDS_ONLY, offsets[0] is written even where m == 0.
 *
 * DATA.  bytes = the sum of L_i over i < m; suffix_bytes = the sum of s_i over i < min(m, first_bad); data_avail = len - consumed_p -
 * consumed_s.  Byte k of element i is byte k of element i - 1 where k < p_i, and otherwise suffix byte (the sum of s_j over j < i) + k - p_i.
 * A suffix byte at or behind src + len reads as 0 and is never loaded.  Delivered is d_data[0, min(bytes, data_cap)), cut exactly to the
 * byte: every copy's source lies in front of its destination, so a cut output is a prefix of the uncut one.  data_status is a set of bits:
 * BROTLI_AMD_UNDBA_DATA_SHORT where suffix_bytes > data_avail, .._DATA_BAD where first_bad is set, .._DATA_COUNTS_DIFFER where count_p !=
 * count_s with both walks OK.  Nothing in the result depends on data_cap or on how the work was shared out.
 *
 * KINDS OF CALL.  cap == 0 only COUNTS and is the two walks alone: the fourteen undbp fields and data_avail are filled (and COUNTS_DIFFER);
 * bytes and suffix_bytes are 0 and first_bad is UINT64_MAX.  cap != 0 with neither destination only MEASURES: the same launches with every
 * store off.  BROTLI_AMD_UNDBA_SKIP is for BrotliAmdBatchUndbaOutputs alone: the stream's result is zeros with first_bad UINT64_MAX.
 *
 * Examples (bytes: elements; offsets; other results):
 *   80 01 04 01 00 | 80 01 04 01 06 | 78 79 7a: "xyz"; 0 3; consumed_p 5, consumed_s 5, bytes 3, suffix_bytes 3, data_avail 3
 *   80 01 04 02 00 04 00 00 00 00 | 80 01 04 02 06 03 00 00 00 00 | 61 62 63 64: prefixes 0 2, suffix lengths 3 1: "abc", "abd"; 0 3 6;
 *     data abcabd, bytes 6, suffix_bytes 4
 *   the same with prefixes 0 4 (.. 02 00 08 00 ..): first_bad 1, PREFIX_LONG, DATA_BAD; 0 3 3; data abc, bytes 3, suffix_bytes 3
 *   the second without its last byte: DATA_SHORT; 0 3 6; data abcab\0, data_avail 3
 *   80 01 04 02 00 01 00 00 00 00 | 80 01 04 02 02 01 00 00 00 00 | 61: prefixes 0 -1: first_bad 1, PREFIX_NEGATIVE; 0 1 1; data a
 *   80 01 04 01 02 | 80 01 04 01 02 | 61: a first prefix of 1: first_bad 0, PREFIX_LONG; 0 0; no data byte written
 *   80 01 04 00 00 | 80 01 04 00 00: none (N = 0 in both); offset_base alone
 *
 * LOADS AND STORES.  No byte is written outside [d_data, d_data + min(bytes, data_cap)) and outside the offsets named above; nothing is read
 * outside the 16-byte-aligned span around [src, src + len) and the call's own destinations.  OUT OF PLACE ONLY: stated, not checked.
 *
 * REFUSED ON THE HOST, in front of everything that touches the device, with a BrotliAmdLastError text ("undba segment i: ..") that names the
 * segment: undlba's list -- unknown flag bits; BROTLI_AMD_UNDBA_SKIP in the Segments call; cap > 2^56; data_cap != 0 with a NULL d_data; a
 * NULL array with n != 0, but those named as optional.
 *
 * A call is nine launches in stream order, and no block ever waits for another: no spins, no flags, no atomics on offsets or data.  1. THE
 * WALKS, undbp's as it is, one wave a segment, P and then S from P's consumed: the result's fourteen fields, data_avail, both first values,
 * both streams' checkpoints, and -- derived on the device -- both streams as undbp segments for the items.  2. THE DELTA SUMS of both streams,
 * undbp's item function and group sum, one wave an item.  3. UNDELTA'S CARRY LAUNCH over both streams' records at once.  4. THE LENGTHS, one
 * wave an item: the lanes redo their 32 values of both streams on top of the carry-ins and test every element against the one in front of
 * it; the item's sums of L and of s up to ITS first bad element are two more tile records, and that element goes to the result with one
 * atomic minimum.  5. THE CARRY LAUNCH again, over those.  6. THE OFFSETS as undlba stores them; an item behind first_bad takes the bytes in
 * front of first_bad for its carry-in; the item of first_bad writes bad_kind, the last item bytes, suffix_bytes and data_status.  7. PHASE A,
 * one wave an item, items in any order: with r_e = min(p_first .. p_e) inside the item, every element's suffix bytes [p_e, L_e) and its bytes
 * [r_e, p_e), which element e - 1 of the same item has; the running string is kept in LDS up to BROTLI_AMD_UNDBA_LDS_STRING bytes, and a byte
 * beyond that is found by walking back through the item's elements to the suffix that holds it.  The item's last element is recorded.
 * 8. PHASE B, one wave a segment, its items one after the other: the LAST element of item j gets its bytes [0, r_last) from the last element
 * of item j - 1, complete by then; the carried string is kept in LDS up to BROTLI_AMD_UNDBA_LDS_CARRY bytes, and a byte beyond that is read
 * from the item whose phase A wrote it.  9. PHASE C, one wave an item, items in any order: every other element of an item j >= 1 gets its bytes
 * [0, r_e) from the last element of item j - 1, the bytes of 64 elements spread evenly over the lanes (csrc/brotli_undba.h,
 * csrc/brotli_undba_kernels.hip).
 *
 * OUT OF SCOPE: FIXED_LEN_BYTE_ARRAY under this encoding; nullable string columns in one call; page framing; a parallel walk of one long
 * segment; a parallel carry over one segment's items (phase B is serial in a segment's items); lengths wider than INT32. */
#define BROTLI_AMD_UNDBA_OFFSETS64 2u    /* offsets of 8 bytes */
#define BROTLI_AMD_UNDBA_ENDS_ONLY 4u    /* offsets[0] is not written, and d_offsets points at offsets[1] */
#define BROTLI_AMD_UNDBA_SKIP 8u         /* BrotliAmdBatchUndbaOutputs: the stream is skipped */
#define BROTLI_AMD_UNDBA_DATA_OK 0u
#define BROTLI_AMD_UNDBA_DATA_SHORT 1u          /* bits of data_status */
#define BROTLI_AMD_UNDBA_DATA_BAD 2u
#define BROTLI_AMD_UNDBA_DATA_COUNTS_DIFFER 4u
#define BROTLI_AMD_UNDBA_BAD_NONE 0u
#define BROTLI_AMD_UNDBA_BAD_PREFIX_NEGATIVE 1u
#define BROTLI_AMD_UNDBA_BAD_SUFFIX_NEGATIVE 2u
#define BROTLI_AMD_UNDBA_BAD_PREFIX_LONG 3u
#define BROTLI_AMD_UNDBA_LDS_STRING 4096u  /* phase A's running string in LDS */
#define BROTLI_AMD_UNDBA_LDS_CARRY 32768u  /* phase B's carried string in LDS */

typedef struct BrotliAmdUndbaResult {
  uint64_t count_p;         /* prefix lengths decoded, whatever cap was */
  uint64_t consumed_p;      /* undbp's: where S begins */
  uint64_t declared_p;      /* N of P */
  uint64_t blocks_p;
  uint32_t status_p;        /* BROTLI_AMD_UNDBP_* */
  uint32_t block_values_p;
  uint32_t miniblocks_p;
  uint32_t data_status;     /* BROTLI_AMD_UNDBA_DATA_* bits */
  uint64_t count_s;         /* suffix lengths decoded, whatever cap was */
  uint64_t consumed_s;      /* undbp's, counted from src + consumed_p: where the suffix bytes begin */
  uint64_t declared_s;
  uint64_t blocks_s;
  uint32_t status_s;
  uint32_t block_values_s;
  uint32_t miniblocks_s;
  uint32_t bad_kind;        /* BROTLI_AMD_UNDBA_BAD_*: the rule that element first_bad broke */
  uint64_t first_bad;       /* the smallest element index that broke a rule; UINT64_MAX: none */
  uint64_t bytes;           /* of the delivered elements together, whatever data_cap was */
  uint64_t suffix_bytes;    /* of their suffixes together */
  uint64_t data_avail;      /* len - consumed_p - consumed_s */
} BrotliAmdUndbaResult;

/* n segments in DEVICE memory, with the arguments of BrotliAmdBatchUndlbaSegments and their rules. */
BROTLI_DEC_API int BrotliAmdBatchUndbaSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_src, const size_t* src_lens,
                                              void* const* d_offsets /* or NULL */, void* const* d_data /* or NULL */,
                                              const uint64_t* data_caps /* or NULL */, const uint64_t* caps, const uint8_t* flags /* or NULL */,
                                              const uint64_t* offset_bases /* or NULL */, BrotliAmdUndbaResult* results, void* hip_stream);

/* The same for the DELIVERED bytes of every stream of the last decode call on the object, by BrotliAmdBatchUndbpOutputs' rules for the three
 * kinds of decode call.  A stream with BROTLI_AMD_UNDBA_SKIP in flags[i] is skipped: none of its other parameters are looked at and its
 * result is zeros with first_bad UINT64_MAX.  caps == NULL counts every stream and nothing else. */
BROTLI_DEC_API int BrotliAmdBatchUndbaOutputs(BrotliAmdBatch* batch, void* const* d_offsets /* or NULL */, void* const* d_data /* or NULL */,
                                             const uint64_t* data_caps /* or NULL */, const uint64_t* caps /* or NULL */,
                                             const uint8_t* flags /* or NULL */, const uint64_t* offset_bases /* or NULL */,
                                             BrotliAmdUndbaResult* results);

/* Milliseconds the undba kernels took in the last of the two calls above (HIP events around its launches together), */
BROTLI_DEC_API float BrotliAmdBatchLastUndbaMs(BrotliAmdBatch* batch);
/* and those of phase 1 (the walks), 2 (the delta sums), 3 (their carries), 4 (the lengths), 5 (their carries), 6 (the offsets), 7 (phase A),
 * 8 (phase B) or 9 (phase C) alone; another: 0. */
BROTLI_DEC_API float BrotliAmdBatchLastUndbaPhaseMs(BrotliAmdBatch* batch, uint32_t phase);

/* Test hook (no device needed): all phases by the functions of csrc/brotli_undbp.h and csrc/brotli_undba.h on the host, with the arguments of
 * BrotliAmdDebugUndlbaHost and its return values.  order_seed != 0: the items are taken in shuffled orders in every phase where the order is
 * free -- all but phase B, which takes a segment's items one after the other and the segments in a shuffled order. */
BROTLI_DEC_API int BrotliAmdDebugUndbaHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* offsets, size_t offsets_size, uint8_t* data,
                                          size_t data_size, const uint64_t* src_offs, const uint64_t* src_lens, const uint64_t* offsets_offs,
                                          const uint64_t* data_offs, const uint64_t* data_caps, const uint64_t* caps,
                                          const uint64_t* offset_bases, const uint8_t* flags /* or NULL */, uint32_t src_skew,
                                          uint32_t offsets_skew, uint32_t data_skew, uint32_t item_deltas, uint32_t order_seed,
                                          BrotliAmdUndbaResult* results);

/* ---- Unnull on the device: dense values spread over nulls by definition levels ----
 *
 * Every decoder above writes a DENSE array of the values that are there, and almost every real column is nullable: a Parquet writer puts
 * DEFINITION LEVELS -- unrle's runs of k-bit fields -- in front of the values of every nullable field, even where no value is null, and only
 * the slots whose level is the maximum have a value.  These calls take the levels and the dense values and write what a framework wants: one
 * slot a row, 0 where the row is null, and Arrow's validity bitmap.  The levels never reach memory as an array.
 *
 * THE SEGMENT AND ITS PARAMETERS.
 *   levels   the bytes src[0, len), read by unrle's grammar EXACTLY: headers, the two payload kinds, k == 0, an RLE run's value not masked,
 *            every stop, and count, consumed, runs, status and bits of the result.  The field width `bits` = k is 0 .. 32; there is no width
 *            byte.
 *   level    a uint32: slot i is PRESENT iff level_i == level, compared unmasked; it is NULL otherwise, for levels below and above alike.
 *   values   values_count = V dense elements of w bytes (w in {1, 2, 4, 8}) at `values`, any alignment.
 *   cap      the capacity in slots; dst, any alignment; valid, a byte pointer of any alignment, or NULL for no bitmap.
 *
 * SLOTS.  With m = min(count, cap), slot i < m gets the value of RANK r_i, the number of present slots in front of i, where it is present and
 * r_i < V, and 0 otherwise.  A present slot with r_i >= V is MISSING: its value is 0, nothing is read through that rank, and it is counted --
 * the rank goes through undict's bounds-checked entry load as the index.  VALIDITY follows the levels alone, so a missing slot's bit is still
 * 1.  It is Arrow's layout: bit i & 7 of byte i >> 3, LSB-first; exactly ceil(m / 8) bytes are written, and the bits at and above m in the
 * last byte are 0.
 *
 * LOADS AND STORES.  No byte outside [dst, dst + m w) and [valid, valid + ceil(m / 8)) is written, and all of the first range is.  Reads stay
 * inside the 16-byte-aligned spans around the levels and around [values, values + V w).  OUT OF PLACE ONLY: no destination or bitmap overlaps
 * a source, the values or another destination or bitmap.  This is stated, not checked.
 *
 * FLAGS.  BROTLI_AMD_UNNULL_LENGTH_PREFIX: the segment is the front of a v1 data page -- its first four bytes are the little-endian length L,
 * and the runs are src[4, 4 + L), judged as unrle judges a segment of that length.  consumed counts from the segment's first byte, so OK gives
 * 4 + L.  len < 4 or L > len - 4 is the status BROTLI_AMD_UNNULL_BAD_LENGTH: count 0, consumed 0.
 * BROTLI_AMD_UNNULL_VALUES_FOLLOW (refused without LENGTH_PREFIX): the values are what lies behind the runs in the same segment --
 * values = src + consumed and V = floor((len - consumed) / w) where the status is OK, V = 0 elsewhere.  The values and values_count arguments
 * are not looked at.
 *
 * RESULT.  BrotliAmdUnnullResult, 56 bytes: unrle's five fields with unrle's meaning, independent of cap and of how the work was shared
 * out; then present, the delivered slots whose level is `level`; missing, the delivered present slots of rank >= V; and values, the V that
 * was used.  present and missing depend on cap, like undict's bad: a call that only counts gives 0 for both.  A skipped stream's result is
 * zeros.
 *
 * Examples (k, level, levels; values; slots; validity; present, missing):
 *   1, 1, 03 A5; {10, 20, 30, 40} as uint16; 10 0 20 0 0 30 0 40; A5; 4, 0.
 *   3, 5, 10 05 (8 x 5); {1 .. 8} as uint8; 1 2 3 4 5 6 7 8; FF; 8, 0.
 *   3, 5, 10 05; {1 .. 6}: a MISSING value; 1 2 3 4 5 6 0 0; FF; 8, 2.
 *   3, 2, 03 88 C6 FA (0 .. 7); {9} as uint32; 0 0 9 0 0 0 0 0; 04; 1, 0.
 *   9, 300, 06 2C 01 (3 x 300, not masked); {7, 8, 9} as uint8; 7 8 9; 07; 3, 0.  With level 44: 0 0 0; 00; 0, 0.
 *   0, 0, 07 (24 x 0), cap 10; {1 .. 10} as uint8; 1 .. 10; FF 03; count 24, 10, 0.
 *   LENGTH_PREFIX | VALUES_FOLLOW, 1, 1, w = 2: the segment 02 00 00 00 03 A5 0A 00 14 00 1E 00 28 00 -- L = 2, consumed 6, V = 4 --;
 *     10 0 20 0 0 30 0 40; A5; 4, 0.  The same segment cut to 3 bytes, or with a first byte of 0B: BAD_LENGTH.
 *
 * REFUSED ON THE HOST, in front of everything that touches the device, with a text that names the segment: a width outside {1, 2, 4, 8};
 * unknown flag bits; VALUES_FOLLOW without LENGTH_PREFIX; bits > 32; cap > 2^56; values_count > 2^56; a NULL dst with cap != 0; a NULL
 * values with V != 0, cap != 0 and no VALUES_FOLLOW.
 *
 * A call is four launches in stream order, on undbp's shape, and no block ever waits for another -- no look-back, no flags, no spins, no
 * grid barrier, no atomics on the bitmap.  1. THE WALK, one wave a segment: the four bytes of the prefix where there is one, then unrle's
 * walk: the result, the checkpoints of unrle's items, the prefix entry.  2. THE COUNTS, one wave an item over the items of all segments: the
 * runs that cover the item, a lane's present mask of its 16 neighbouring slots -- inside an RLE run one compare --, and the wave's popcount
 * as an undelta tile record.  3. undelta's CARRY launch as it is: every item's present slots in front of it.  4. THE EXPANSION, the same item
 * function: a scan of the lanes' popcounts on top of the carry gives a lane its first rank; its present slots have consecutive ranks, so
 * neighbouring lanes read neighbouring values; slots go out as aligned 16-byte stores with single ones at the edges, and the lanes' two
 * validity bytes are gathered into aligned 16-byte stores.  The item that holds a segment's last delivered slot writes present and missing:
 * its carry-in and its own popcount are all of them, and the ranks at or above V are the missing ones.  A call that only counts is the first
 * launch alone (csrc/brotli_unnull.h, csrc/brotli_unnull_kernels.hip).
 *
 * OUT OF SCOPE: repetition levels and nested columns; a bit offset into the bitmap; a fill value other than 0; byte-array values (those of a
 * required dictionary column are the undict-bytes calls' above); thrift framing; a fused undict + unnull -- a nullable dictionary column is
 * two calls, and a counting call with LENGTH_PREFIX tells the caller where a v1 dictionary-index body begins --; a parallel walk of one long
 * segment. */
#define BROTLI_AMD_UNNULL_LENGTH_PREFIX 1u
#define BROTLI_AMD_UNNULL_VALUES_FOLLOW 2u
#define BROTLI_AMD_UNNULL_BAD_LENGTH 5u   /* a status behind BROTLI_AMD_UNRLE_*: the length prefix is cut, or says more than there is */

typedef struct BrotliAmdUnnullResult {
  uint64_t count;     /* levels in all runs, whatever cap was */
  uint64_t consumed;  /* unrle's table, from the segment's first byte */
  uint64_t runs;      /* runs that gave at least one level */
  uint32_t status;    /* BROTLI_AMD_UNRLE_*, or BROTLI_AMD_UNNULL_BAD_LENGTH */
  uint32_t bits;      /* the k that was used */
  uint64_t present;   /* delivered slots whose level is `level` */
  uint64_t missing;   /* delivered present slots of rank >= values */
  uint64_t values;    /* the V that was used */
} BrotliAmdUnnullResult;

/* n segments in DEVICE memory -- the level_lens[i] bytes at d_levels[i] are the levels, of fields of bits[i] bits, compared with levels[i];
 * the value_counts[i] dense values of widths[i] bytes at d_values[i] go to the first caps[i] slots at d_dst[i], and their validity bits to
 * d_valid[i] (NULL, or d_valid == NULL: no bitmap), by flags[i] (flags == NULL: all 0); results[i] says what segment i held; any alignment,
 * any length, 0 included; n is not bound by the batch object's max_streams --: the launches run on hip_stream, and the call waits on that
 * stream.  caps[i] == 0 only counts -- the walk alone --: d_dst[i], d_values[i] and value_counts[i] are not looked at but for the refusals
 * above, and d_dst, d_values and value_counts themselves may be NULL where every capacity is 0.  n == 0 returns 0.  A negative value, and a
 * BrotliAmdLastError text that names the segment and what was wrong, for a NULL batch, a NULL array (but flags, d_valid and the three just
 * named) with n != 0, and everything in the list above: all of these are checked on the host in front of everything else, so nothing is
 * launched and no byte is written. */
BROTLI_DEC_API int BrotliAmdBatchUnnullSegments(BrotliAmdBatch* batch, uint32_t n, const void* const* d_levels, const size_t* level_lens,
                                               const void* const* d_values, const uint64_t* value_counts, void* const* d_dst,
                                               void* const* d_valid /* or NULL */, const uint64_t* caps, const uint8_t* bits, const uint32_t* levels,
                                               const uint8_t* widths, const uint8_t* flags /* n entries, or NULL: all 0 */,
                                               BrotliAmdUnnullResult* results, void* hip_stream);

/* The same for the DELIVERED bytes of every stream of the last decode call on the object, by BrotliAmdBatchUnrleOutputs' rules for the three
 * kinds of decode call, for skipped streams (d_dst[i] == NULL: none of the stream's parameters are looked at, its result is zeros) and for
 * counting (d_dst == NULL or caps == NULL).  In two forms, stream by stream.  Where d_levels is NULL or d_levels[i] is NULL, stream i is a V1
 * BODY -- prefix, levels, values --, with both flags implied.  Where d_levels[i] is set, this is the V2 case: the levels are the caller's
 * uncompressed device bytes d_levels[i] of level_lens[i], with no flags, and the values are the whole of stream i's delivered bytes,
 * V = floor(decoded_size / widths[i]).  A negative value, and a BrotliAmdLastError text, for a NULL batch, bits, levels, widths or results, a
 * d_levels without level_lens, a refusal (nothing is launched), an object without a decode call, a last decode call that failed behind its
 * argument checks (one of no streams returns 0), and a launch that BrotliAmdBatchWait has not been called for. */
BROTLI_DEC_API int BrotliAmdBatchUnnullOutputs(BrotliAmdBatch* batch, void* const* d_dst /* or NULL */, void* const* d_valid /* or NULL */,
                                              const uint64_t* caps /* or NULL */, const uint8_t* bits, const uint32_t* levels, const uint8_t* widths,
                                              const void* const* d_levels /* or NULL */, const size_t* level_lens /* or NULL */,
                                              BrotliAmdUnnullResult* results);

/* Milliseconds the unnull kernels took in the last of the two calls above (HIP events around its launches together), */
BROTLI_DEC_API float BrotliAmdBatchLastUnnullMs(BrotliAmdBatch* batch);
/* and those of phase 1 (the walk), 2 (the counts), 3 (the carries) or 4 (the expansion) alone; another phase: 0. */
BROTLI_DEC_API float BrotliAmdBatchLastUnnullPhaseMs(BrotliAmdBatch* batch, uint32_t phase);

/* Test hook (no device needed): the four phases by the functions of csrc/brotli_unrle.h and csrc/brotli_unnull.h on the host.  It has
 * BrotliAmdDebugUndictHost's shape, with a values buffer values[0, values_size) and a validity buffer valid[0, valid_size), each placed at
 * its skew (0..15) past a 16-byte boundary in a room of its own: segment i's values are value_counts[i] elements of widths[i] bytes at
 * value_offs[i] (not looked at with VALUES_FOLLOW), and its bitmap lies at valid_offs[i] (UINT64_MAX: it has none).  item_elems: the slots of
 * an item, a multiple of 8, so that items own whole validity bytes (0: the device's, BrotliAmdDebugUnrleItemElems()); any other value is
 * refused.  The items are taken in an order shuffled by order_seed, in the counting phase and again in the expansion (no result may depend on
 * it).  0, results[0..n) filled, the slots' bytes of dst and the bitmaps' bytes of valid written; -1, a BrotliAmdLastError text and untouched
 * buffers for a refusal, a skew > 15 or a segment, values or bitmap outside its buffer; -2 where a byte outside the slots and the bitmap
 * bytes changed. */
BROTLI_DEC_API int BrotliAmdDebugUnnullHost(uint32_t n, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_size, const uint8_t* values,
                                           size_t values_size, uint8_t* valid, size_t valid_size, const uint64_t* src_offs, const uint64_t* src_lens,
                                           const uint64_t* dst_offs, const uint64_t* caps, const uint64_t* value_offs, const uint64_t* value_counts,
                                           const uint64_t* valid_offs, const uint32_t* levels, const uint8_t* bits, const uint8_t* widths,
                                           const uint8_t* flags /* or NULL */, uint32_t src_skew, uint32_t dst_skew, uint32_t values_skew,
                                           uint32_t valid_skew, uint32_t item_elems, uint32_t order_seed, BrotliAmdUnnullResult* results);

/* Milliseconds the last launch spent in the decode kernel (HIP events on the launch stream). */
BROTLI_DEC_API float BrotliAmdBatchLastKernelMs(BrotliAmdBatch* batch);

/* Host milliseconds the last BrotliAmdBatchDecodeDevice / DecodeHost call spent in the probe launch and its wait (0: no probe). */
BROTLI_DEC_API float BrotliAmdBatchLastProbeMs(BrotliAmdBatch* batch);

/* Streams the last BrotliAmdBatchWait had to continue in a second launch with a larger LDS arena (0 in the common case). */
BROTLI_DEC_API uint32_t BrotliAmdBatchLastSecondPassCount(BrotliAmdBatch* batch);

/* Blocks (CUs) that worked on each stream of the last launch: 1 as a rule; 2, 4, 8 or 16 where the batch had fewer streams than half the
 * device's CUs, at least one of them 64 KiB of compressed data or more, and each stream was given a gang of blocks (csrc/brotli_path_engine.h, path_engine<false, true>; BROTLI_AMD_GANG=0 turns that off). */
BROTLI_DEC_API uint32_t BrotliAmdBatchLastGang(BrotliAmdBatch* batch);

/* 1 where the last launch was a POOL: more than 32 streams, at most as many as CUs, of very different sizes (the largest more than twice the median) --
 * every block that has no stream of its own, at once or when its stream is done, joins the largest stream still being decoded
 * (BROTLI_AMD_POOL=0 turns that off).  BrotliAmdBatchLastGang says 1 for such a launch: a stream's helpers come and go. */
BROTLI_DEC_API uint32_t BrotliAmdBatchLastPool(BrotliAmdBatch* batch);

/* Test hook (no device needed): what a launch of n streams of these compressed sizes gets on a device of `cus` compute units -- 0 one block a
 * stream, 2 / 4 / 8 / 16 gangs of that many blocks a stream, 0x108 a pool -- and its number of blocks in *grid.  gang_env / pool_env: the values of
 * BROTLI_AMD_GANG / BROTLI_AMD_POOL, -1 where unset. */
BROTLI_DEC_API uint32_t BrotliAmdDebugPlanGangs(uint32_t n, uint32_t cus, const size_t* in_sizes, int gang_env, int pool_env, uint32_t* grid);

/* Test hooks (no device needed): the launch planner (csrc/brotli_launch_plan.h, which defines the four structs: plain words, for tests) -- the
 * shape it gives the first launch of n streams of these compressed sizes on the device and with the knobs described, kinds being what the
 * probe said of every stream or NULL where the device has not been asked (a plan with want_probe set is the probe launch's own); and the
 * shape of the pass after one of `level` blocks per CU and arena `cur_arena`, for m streams that came back.  Both return 0, or -1 for a NULL
 * among dev, knobs, in_sizes and the result, n == 0 or a device without compute units. */
struct BrotliAmdPlanDevice;
struct BrotliAmdPlanKnobs;
struct BrotliAmdLaunchPlan;
struct BrotliAmdLaterPass;
BROTLI_DEC_API int BrotliAmdDebugPlanLaunch(const struct BrotliAmdPlanDevice* dev, const struct BrotliAmdPlanKnobs* knobs, uint32_t per_cu_cap,
                                           uint32_t n, const size_t* in_sizes, const uint8_t* kinds, struct BrotliAmdLaunchPlan* plan);
BROTLI_DEC_API int BrotliAmdDebugPlanLaterPass(const struct BrotliAmdPlanDevice* dev, const struct BrotliAmdPlanKnobs* knobs, uint32_t per_cu_cap,
                                              uint32_t level, uint32_t cur_arena, uint32_t m, int deferred, struct BrotliAmdLaterPass* pass);

/* Streaming (BrotliDecoderDecompressStream, decode.h): the commands the device has decoded for this stream in all the launches
 * of its calls together.  A call is a launch from the last command boundary reached, so this stays close to the stream's own
 * number of commands however the input is cut up; a test asserts that instead of timing calls. */
struct BrotliDecoderStateStruct;
BROTLI_DEC_API uint64_t BrotliAmdDecoderDeviceCommands(const struct BrotliDecoderStateStruct* state);

/* Streaming with a custom dictionary (reference: BrotliState::new_with_custom_dictionary, src/state.rs:400-411; the adapters'
 * new_with_custom_dict, src/reader.rs:103-162, src/writer.rs:115-171): attaches ONE dictionary to an instance made by
 * BrotliDecoderCreateInstance, before it has decoded anything.  The bytes are copied (the caller's buffer may go); at most the last
 * (1 << 30) - 16 of them are kept, which is all any window reaches.  Every launch of BrotliDecoderDecompressStream then decodes with it.
 * Returns 1 on a fresh instance; size == 0 is a no-op that returns 1.  Returns 0 for a NULL state, NULL data with size != 0, a second
 * dictionary, and once BrotliDecoderIsUsed is true.  The one-shot functions of decode.h have no dictionary, as in src/ffi/mod.rs:120. */
BROTLI_DEC_API int BrotliAmdDecoderAttachDictionary(struct BrotliDecoderStateStruct* state, const uint8_t* data, size_t size);

/* ---- Stream sets: many streaming decoders advanced by one launch ----
 *
 * BrotliDecoderDecompressStream (decode.h) gives every state a batch object of one stream: a call is one blocking copy of its chunk to the
 * device, one launch of one stream, one wait and one blocking copy back.  A server with hundreds of open streams, each handed a few KiB at a
 * time, pays that per stream per round.  A stream set steps n states in ONE call:
 *
 *   BrotliAmdStreamSetDecompress(set, n, states, available_in, next_in, available_out, next_out, total_out, results)
 *
 * THE CONTRACT: for every i, states[i], the i-th entries of the five arrays and results[i] end up exactly as ONE
 *   results[i] = BrotliDecoderDecompressStream(states[i], &available_in[i], &next_in[i], &available_out[i], &next_out[i],
 *                                              total_out ? &total_out[i] : NULL)
 * would have left them: the result and the bytes consumed; the bytes written, and which; the latched error code and the error string;
 * BrotliDecoderIsFinished / IsUsed / HasMoreOutput / TakeOutput afterwards; trailing input handed back behind the end of a stream; an attached
 * custom dictionary; the state's own allocator callbacks for its host memory.  A state may be stepped through a set in one call and alone in
 * the next: the sequence behaves as one sequence of solo calls.  The states of a call are independent: an error in one changes nothing for
 * the others.
 *
 * How a call runs:
 *  1. per state, on the host: the argument and slice checks, the latched-error return and the owed-output rule of the solo function.  States
 *     that end there never reach the device: finished ones, ones with a latched error, ones given no input, ones whose owed output did not fit.
 *  2. the chunks of all remaining states are packed into one pinned staging buffer and go to the device in ONE transfer; one ragged-copy launch
 *     (csrc/brotli_copy_kernels.hip) appends each chunk to its state's input buffer.
 *  3. ONE launch over the set's own batch object of max_states streams decodes all of them -- fresh and resumed states, with and without a
 *     dictionary, mixed; block shapes, gangs and pools are the batch planner's for that many streams.
 *  4. states whose device output buffer was full go through the solo function's trim-and-grow rule and are launched again -- they alone.
 *  5. one ragged-copy launch gathers every state's new output into staging, ONE transfer brings it back, the host appends each part to its
 *     state's queue, and the solo function's tail (what fits is handed over, the result follows) runs per state.
 * If no state needs the device, nothing is launched or copied.  Staging is bounded (64 MiB in each direction): a chunk or an output part larger
 * than that travels by a copy of its own, and parts that add up to more go in several transfers.
 *
 * Everything runs on the null stream, as the solo path does.  The set binds to the HIP device that is current at its first call that needs
 * one, as a state does; a state first used through a set is bound to the set's device and gets no batch object of its own until it is first
 * stepped alone.  One thread at a time per set, and per state.
 *
 * The call as a whole fails -- a negative value, and nothing is touched -- for a NULL set, NULL states, NULL results or a NULL one among the four
 * in/out arrays, a NULL entry in states, n > max_states, the same state twice, and a state already bound to another device than the set's.
 * n == 0 returns 0.  Otherwise it returns 0, whatever the states' results: without a usable device the states that needed one end as the solo
 * call ends them -- BROTLI_DECODER_RESULT_ERROR, BROTLI_DECODER_ERROR_UNREACHABLE and the same error text. */
typedef struct BrotliAmdStreamSet BrotliAmdStreamSet;
/* needs no device; NULL only when out of memory (max_states == 0 counts as 1) */
BROTLI_DEC_API BrotliAmdStreamSet* BrotliAmdStreamSetCreate(uint32_t max_states);
/* the states stay the caller's: they are not destroyed, and may be stepped alone or through another set of the same device afterwards */
BROTLI_DEC_API void BrotliAmdStreamSetDestroy(BrotliAmdStreamSet* set);
BROTLI_DEC_API int BrotliAmdStreamSetDecompress(BrotliAmdStreamSet* set, uint32_t n, struct BrotliDecoderStateStruct* const* states,
                                               size_t* available_in, const uint8_t** next_in, size_t* available_out, uint8_t** next_out,
                                               size_t* total_out /* n entries or NULL */, BrotliDecoderResult* results /* n entries */);
/* decode launches of the last BrotliAmdStreamSetDecompress: 0 where no state needed the device, 1 as a rule, more where states had to grow
 * their device output buffer (step 4) */
BROTLI_DEC_API uint32_t BrotliAmdStreamSetLastLaunches(BrotliAmdStreamSet* set);
/* host <-> device copies of payload bytes (chunks in, output back) in it: at most 2 where one launch did and everything fitted the staging;
 * a dictionary's upload at a state's first step is not counted */
BROTLI_DEC_API uint32_t BrotliAmdStreamSetLastTransfers(BrotliAmdStreamSet* set);

/* Test hook: the ragged copy kernel alone (csrc/brotli_copy_kernels.hip).  Host arrays of n DEVICE pointers and n lengths: segment i is
 * lens[i] bytes from d_src[i] to d_dst[i], any alignment, any length, 0 included; the segments do not overlap each other.  One launch on the
 * null stream, and a wait.  No byte outside [d_dst[i], d_dst[i] + lens[i]) is written; nothing outside the 16-byte-aligned span around
 * [d_src[i], d_src[i] + lens[i]) is read.  Returns 0 on success. */
BROTLI_DEC_API int BrotliAmdDebugRaggedCopy(uint32_t n, const void* const* d_src, void* const* d_dst, const size_t* lens);
/* ... and the bytes of destination in one of its tiles (the unit in which the blocks of a launch share the work) */
BROTLI_DEC_API uint32_t BrotliAmdDebugRaggedCopyTile(void);

/* Text of the last HIP/runtime failure on this thread ("" if none). */
BROTLI_DEC_API const char* BrotliAmdLastError(void);

/* What the last call on this thread did differently without failing ("" if nothing): a device that refused blocks of sixteen
 * waves makes its batch context go on with blocks of eight (slower on batches of one stream a CU), and this says so. */
BROTLI_DEC_API const char* BrotliAmdLastNote(void);

/* Test hook, not part of the decode path: builds the device's prefix-code table for alphabet_size code lengths (0 = unused symbol;
 * a complete code, as src/huffman/mod.rs:273-386 is given them) and decodes every fifteen-bit value v through it the way the
 * kernel's symbol reader does: decoded[v] = symbol << 4 | code length (32768 entries).  table_entries = the table's size.
 * Returns 0 on success. */
BROTLI_DEC_API int BrotliAmdDebugBuildTree(const uint8_t* code_lengths, uint32_t alphabet_size, uint16_t* decoded, uint32_t* table_entries);

#if defined(__cplusplus)
} /* extern "C" */
#endif
#endif /* BROTLI_AMD_BATCH_H_ */
