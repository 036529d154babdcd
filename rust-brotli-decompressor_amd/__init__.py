"""MI355X-native Brotli decode path: thin Python binding of libbrotli_decompressor.so (ctypes).

The product is the shared library (HIP kernels + the reference's C ABI, see include/brotli/decode.h and
include/brotli/batch.h).  This module only loads it and gives tests and bench.py a convenient handle; it
contains no decoder and no CPU fallback -- if the library is missing or no HIP device is usable, calls fail.

Names follow the reference: `Decompressor` is the pull adapter of src/reader.rs (io::Read), `DecompressorWriter`
the push adapter of src/writer.rs (io::Write), `brotli_decode` the one-shot helper of src/lib.rs:447-468.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BROTLI_AMD_LIB") or os.path.join(_HERE, "libbrotli_decompressor.so")

RESULT_ERROR, RESULT_SUCCESS, RESULT_NEEDS_MORE_INPUT, RESULT_NEEDS_MORE_OUTPUT = 0, 1, 2, 3
FLAG_LARGE_WINDOW, FLAG_NO_CANNY = 1, 2
FLAG_SPILL_IN_PLACE = 16  # BROTLI_AMD_BATCH_SPILL_IN_PLACE: no second launch with a larger LDS arena
FLAG_EAGER_OUTPUT_LIMIT = 64  # BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT: NEEDS_MORE_OUTPUT where the buffer ends, no second look (batch.h)
PARAM_DISABLE_RING_BUFFER_REALLOCATION, PARAM_LARGE_WINDOW = 0, 1

# every symbol include/brotli/decode.h and include/brotli/batch.h declare
DECODE_H_SYMBOLS = [
    "BrotliDecoderSetParameter", "BrotliDecoderCreateInstance", "BrotliDecoderDestroyInstance", "BrotliDecoderDecompress",
    "BrotliDecoderDecompressWithReturnInfo", "BrotliDecoderDecompressPrealloc", "BrotliDecoderDecompressStream",
    "BrotliDecoderDecompressStreaming", "BrotliDecoderHasMoreOutput", "BrotliDecoderTakeOutput", "BrotliDecoderIsUsed",
    "BrotliDecoderIsFinished", "BrotliDecoderGetErrorCode", "BrotliDecoderGetErrorString", "BrotliDecoderErrorString",
    "BrotliDecoderVersion", "BrotliDecoderMallocU8", "BrotliDecoderFreeU8", "BrotliDecoderMallocUsize", "BrotliDecoderFreeUsize",
]
BATCH_H_SYMBOLS = [
    "BrotliAmdBatchCreate", "BrotliAmdBatchDestroy", "BrotliAmdBatchDecodeDevice", "BrotliAmdBatchRelaunch", "BrotliAmdBatchWait",
    "BrotliAmdBatchDecodeHost", "BrotliAmdBatchLastKernelMs", "BrotliAmdBatchLastSecondPassCount", "BrotliAmdBatchLastGang", "BrotliAmdBatchLastPool", "BrotliAmdBatchLastProbeMs", "BrotliAmdDebugPlanGangs", "BrotliAmdDebugPlanLaunch", "BrotliAmdDebugPlanLaterPass", "BrotliAmdLastError", "BrotliAmdLastNote", "BrotliAmdDebugBuildTree", "BrotliAmdDecoderDeviceCommands",
    "BrotliAmdBatchDecodeDeviceDict", "BrotliAmdBatchDecodeHostDict", "BrotliAmdDecoderAttachDictionary",
    "BrotliAmdStreamSetCreate", "BrotliAmdStreamSetDestroy", "BrotliAmdStreamSetDecompress", "BrotliAmdStreamSetLastLaunches",
    "BrotliAmdStreamSetLastTransfers", "BrotliAmdDebugRaggedCopy", "BrotliAmdDebugRaggedCopyTile",
    "BrotliAmdBatchSizeHints", "BrotliAmdDebugSizeWalk", "BrotliAmdBatchDecodeDevicePacked", "BrotliAmdBatchPackedOutput",
    "BrotliAmdBatchPackedFetch", "BrotliAmdBatchDecodeHostPacked", "BrotliAmdBatchLastPackedLaunches", "BrotliAmdBatchLastPackedCopies",
    "BrotliAmdBatchDigestSegments", "BrotliAmdBatchDigestOutputs", "BrotliAmdBatchLastDigestMs", "BrotliAmdDebugDigestTile",
    "BrotliAmdDebugDigestHost", "BrotliAmdDebugDigestShift",
    "BrotliAmdBatchUnshuffleSegments", "BrotliAmdBatchUnshuffleOutputs", "BrotliAmdBatchLastUnshuffleMs", "BrotliAmdDebugUnshuffleTile",
    "BrotliAmdDebugUnshuffleHost",
    "BrotliAmdBatchUndeltaSegments", "BrotliAmdBatchUndeltaOutputs", "BrotliAmdBatchLastUndeltaMs", "BrotliAmdBatchLastUndeltaPhaseMs",
    "BrotliAmdDebugUndeltaTile", "BrotliAmdDebugUndeltaCarrySpan", "BrotliAmdDebugUndeltaHost",
    "BrotliAmdBatchBitUnshuffleSegments", "BrotliAmdBatchBitUnshuffleOutputs", "BrotliAmdBatchLastBitUnshuffleMs", "BrotliAmdDebugBitUnshuffleTile",
    "BrotliAmdDebugBitUnshuffleHost",
    "BrotliAmdBatchBitUnpackSegments", "BrotliAmdBatchBitUnpackOutputs", "BrotliAmdBatchLastBitUnpackMs", "BrotliAmdDebugBitUnpackTile",
    "BrotliAmdDebugBitUnpackHost",
    "BrotliAmdBatchUnvarintSegments", "BrotliAmdBatchUnvarintOutputs", "BrotliAmdBatchLastUnvarintMs", "BrotliAmdBatchLastUnvarintPhaseMs",
    "BrotliAmdDebugUnvarintTile", "BrotliAmdDebugUnvarintHost",
    "BrotliAmdBatchUnrleSegments", "BrotliAmdBatchUnrleOutputs", "BrotliAmdBatchLastUnrleMs", "BrotliAmdBatchLastUnrlePhaseMs",
    "BrotliAmdDebugUnrleItemElems", "BrotliAmdDebugUnrleWalkChunk", "BrotliAmdDebugUnrleHost",
    "BrotliAmdBatchUndbpSegments", "BrotliAmdBatchUndbpOutputs", "BrotliAmdBatchLastUndbpMs", "BrotliAmdBatchLastUndbpPhaseMs",
    "BrotliAmdDebugUndbpItemDeltas", "BrotliAmdDebugUndbpWalkChunk", "BrotliAmdDebugUndbpHost",
    "BrotliAmdBatchUndictSegments", "BrotliAmdBatchUndictOutputs", "BrotliAmdBatchLastUndictMs", "BrotliAmdBatchLastUndictPhaseMs",
    "BrotliAmdDebugUndictHost",
    "BrotliAmdBatchUnnullSegments", "BrotliAmdBatchUnnullOutputs", "BrotliAmdBatchLastUnnullMs", "BrotliAmdBatchLastUnnullPhaseMs",
    "BrotliAmdDebugUnnullHost",
    "BrotliAmdBatchUndictBytesSegments", "BrotliAmdBatchUndictBytesOutputs", "BrotliAmdBatchLastUndictBytesMs", "BrotliAmdBatchLastUndictBytesPhaseMs",
    "BrotliAmdDebugUndictBytesHost",
    "BrotliAmdBatchUndlbaSegments", "BrotliAmdBatchUndlbaOutputs", "BrotliAmdBatchLastUndlbaMs", "BrotliAmdBatchLastUndlbaPhaseMs",
    "BrotliAmdDebugUndlbaHost",
    "BrotliAmdBatchUndbaSegments", "BrotliAmdBatchUndbaOutputs", "BrotliAmdBatchLastUndbaMs", "BrotliAmdBatchLastUndbaPhaseMs",
    "BrotliAmdDebugUndbaHost",
]


class ReturnInfo(ctypes.Structure):  # BrotliDecoderReturnInfo, reference src/lib.rs:336-342
    _fields_ = [("decoded_size", ctypes.c_size_t), ("error", ctypes.c_char * 256), ("result", ctypes.c_int), ("code", ctypes.c_int)]


class BatchResult(ctypes.Structure):  # BrotliAmdResult
    _fields_ = [("result", ctypes.c_int32), ("error_code", ctypes.c_int32), ("decoded_size", ctypes.c_uint64),
                ("consumed", ctypes.c_uint64), ("produced", ctypes.c_uint64), ("num_metablocks", ctypes.c_uint32),
                ("spilled_metablocks", ctypes.c_uint32), ("num_commands", ctypes.c_uint64),
                ("engine_commands", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class SizeHint(ctypes.Structure):  # BrotliAmdSizeHint: what a stream's headers say of its decoded size (batch.h)
    _fields_ = [("bytes", ctypes.c_uint64), ("walked_in", ctypes.c_uint64), ("exact", ctypes.c_uint32), ("status", ctypes.c_uint32)]

    def astuple(self):
        return (self.bytes, self.walked_in, self.exact, self.status)


SIZE_OK, SIZE_TRUNCATED, SIZE_REJECTED = 0, 1, 2  # SizeHint.status
DIGEST_CRC32, DIGEST_CRC32C = 1, 2  # BROTLI_AMD_DIGEST_*: zlib's polynomial, Castagnoli's
BITUNPACK_MSB_FIRST, BITUNPACK_SIGNED = 1, 2  # BROTLI_AMD_BITUNPACK_*: the first bit of a field is the value's highest; sign-extended
UNVARINT_ZIGZAG = 1  # BROTLI_AMD_UNVARINT_ZIGZAG: (v >> 1) ^ -(v & 1)


class UnvarintResult(ctypes.Structure):  # BrotliAmdUnvarintResult: what a segment of varints held (batch.h)
    _fields_ = [("count", ctypes.c_uint64), ("consumed", ctypes.c_uint64), ("overlong", ctypes.c_uint64)]

    def astuple(self):
        return (self.count, self.consumed, self.overlong)


UNRLE_WIDTH_BYTE = 1  # BROTLI_AMD_UNRLE_WIDTH_BYTE: the segment's first byte is the field width
UNRLE_OK, UNRLE_BAD_HEADER, UNRLE_ZERO_RUN, UNRLE_TRUNCATED, UNRLE_BAD_WIDTH = 0, 1, 2, 3, 4  # UnrleResult.status


class UnrleResult(ctypes.Structure):  # BrotliAmdUnrleResult: what a segment of RLE / bit-packed hybrid runs held (batch.h)
    _fields_ = [("count", ctypes.c_uint64), ("consumed", ctypes.c_uint64), ("runs", ctypes.c_uint64), ("status", ctypes.c_uint32), ("bits", ctypes.c_uint32)]

    def astuple(self):
        return (self.count, self.consumed, self.runs, self.status, self.bits)


UNDBP_OK, UNDBP_BAD_HEADER, UNDBP_BAD_WIDTH, UNDBP_TRUNCATED = 0, 1, 2, 3  # UndbpResult.status


class UndbpResult(ctypes.Structure):  # BrotliAmdUndbpResult: what a segment of DELTA_BINARY_PACKED blocks held (batch.h)
    _fields_ = [("count", ctypes.c_uint64), ("consumed", ctypes.c_uint64), ("declared", ctypes.c_uint64), ("blocks", ctypes.c_uint64),
                ("status", ctypes.c_uint32), ("block_values", ctypes.c_uint32), ("miniblocks", ctypes.c_uint32)]

    def astuple(self):
        return (self.count, self.consumed, self.declared, self.blocks, self.status, self.block_values, self.miniblocks)


UNDICT_WIDTH_BYTE = 1  # BROTLI_AMD_UNDICT_WIDTH_BYTE: the segment's first byte is the field width (UNRLE_WIDTH_BYTE's meaning)
UNDICT_NO_STREAM = 0xFFFFFFFF  # BROTLI_AMD_UNDICT_NO_STREAM: a stream's dictionary is a pointer of the caller's, not a stream of the decode call
UNDICT_NONE = (1 << 64) - 1  # UndictResult.first_bad where no element was bad


class UndictResult(ctypes.Structure):  # BrotliAmdUndictResult: what a segment of dictionary-index runs held, and its indices outside the dictionary (batch.h)
    _fields_ = [("count", ctypes.c_uint64), ("consumed", ctypes.c_uint64), ("runs", ctypes.c_uint64), ("status", ctypes.c_uint32), ("bits", ctypes.c_uint32),
                ("bad", ctypes.c_uint64), ("first_bad", ctypes.c_uint64)]

    def astuple(self):
        return (self.count, self.consumed, self.runs, self.status, self.bits, self.bad, self.first_bad)


UNDICT_BYTES_WIDTH_BYTE, UNDICT_BYTES_OFFSETS64, UNDICT_BYTES_ENDS_ONLY, UNDICT_BYTES_SKIP = 1, 2, 4, 8  # BROTLI_AMD_UNDICT_BYTES_*: a segment's flags
UNDICT_BYTES_ALL = (1 << 64) - 1  # BROTLI_AMD_UNDICT_BYTES_ALL: as many dictionary entries as the bytes hold
UNDICT_BYTES_DICT_OK, UNDICT_BYTES_DICT_CUT = 0, 1  # UndictBytesResult.dict_status
UNDICT_BYTES_NO_DESTINATION = (1 << 64) - 1  # undict_bytes_host: a segment's offsets or data offset where it has no such destination


class UndictBytesResult(ctypes.Structure):  # BrotliAmdUndictBytesResult: undict's seven fields, the elements' bytes and what the dictionary's walk found (batch.h)
    _fields_ = [("count", ctypes.c_uint64), ("consumed", ctypes.c_uint64), ("runs", ctypes.c_uint64), ("status", ctypes.c_uint32), ("bits", ctypes.c_uint32),
                ("bad", ctypes.c_uint64), ("first_bad", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("dict_entries", ctypes.c_uint64),
                ("dict_consumed", ctypes.c_uint64), ("dict_status", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def astuple(self):
        return (self.count, self.consumed, self.runs, self.status, self.bits, self.bad, self.first_bad, self.bytes, self.dict_entries, self.dict_consumed,
                self.dict_status)


UNDLBA_OFFSETS64, UNDLBA_ENDS_ONLY, UNDLBA_SKIP = 2, 4, 8  # BROTLI_AMD_UNDLBA_*: a segment's flags
UNDLBA_DATA_OK, UNDLBA_DATA_SHORT = 0, 1  # UndlbaResult.data_status
UNDLBA_NONE = (1 << 64) - 1  # UndlbaResult.first_bad where no length was negative
UNDLBA_NO_DESTINATION = (1 << 64) - 1  # undlba_host: a segment's offsets or data offset where it has no such destination


class UndlbaResult(ctypes.Structure):  # BrotliAmdUndlbaResult: undbp's seven fields, what became of the data, the negative lengths and the bytes (batch.h)
    _fields_ = [("count", ctypes.c_uint64), ("consumed", ctypes.c_uint64), ("declared", ctypes.c_uint64), ("blocks", ctypes.c_uint64),
                ("status", ctypes.c_uint32), ("block_values", ctypes.c_uint32), ("miniblocks", ctypes.c_uint32), ("data_status", ctypes.c_uint32),
                ("bad", ctypes.c_uint64), ("first_bad", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("data_avail", ctypes.c_uint64)]

    def astuple(self):
        return (self.count, self.consumed, self.declared, self.blocks, self.status, self.block_values, self.miniblocks, self.data_status, self.bad,
                self.first_bad, self.bytes, self.data_avail)


UNDBA_OFFSETS64, UNDBA_ENDS_ONLY, UNDBA_SKIP = 2, 4, 8  # BROTLI_AMD_UNDBA_*: a segment's flags
UNDBA_DATA_OK, UNDBA_DATA_SHORT, UNDBA_DATA_BAD, UNDBA_DATA_COUNTS_DIFFER = 0, 1, 2, 4  # UndbaResult.data_status: bits
UNDBA_BAD_NONE, UNDBA_BAD_PREFIX_NEGATIVE, UNDBA_BAD_SUFFIX_NEGATIVE, UNDBA_BAD_PREFIX_LONG = 0, 1, 2, 3  # UndbaResult.bad_kind
UNDBA_BAD_KINDS = ("no rule", "a negative prefix length", "a negative suffix length", "a prefix longer than the element in front of it")
UNDBA_NONE = (1 << 64) - 1  # UndbaResult.first_bad where no element broke a rule
UNDBA_NO_DESTINATION = (1 << 64) - 1  # undba_host: a segment's offsets or data offset where it has no such destination
UNDBA_LDS_STRING, UNDBA_LDS_CARRY = 4096, 32768  # BROTLI_AMD_UNDBA_LDS_*: the bytes of a running string that phases A and B keep in LDS


class UndbaResult(ctypes.Structure):  # BrotliAmdUndbaResult: undbp's seven fields of both streams, the first bad element, the bytes (batch.h)
    _fields_ = [("count_p", ctypes.c_uint64), ("consumed_p", ctypes.c_uint64), ("declared_p", ctypes.c_uint64), ("blocks_p", ctypes.c_uint64),
                ("status_p", ctypes.c_uint32), ("block_values_p", ctypes.c_uint32), ("miniblocks_p", ctypes.c_uint32), ("data_status", ctypes.c_uint32),
                ("count_s", ctypes.c_uint64), ("consumed_s", ctypes.c_uint64), ("declared_s", ctypes.c_uint64), ("blocks_s", ctypes.c_uint64),
                ("status_s", ctypes.c_uint32), ("block_values_s", ctypes.c_uint32), ("miniblocks_s", ctypes.c_uint32), ("bad_kind", ctypes.c_uint32),
                ("first_bad", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("suffix_bytes", ctypes.c_uint64), ("data_avail", ctypes.c_uint64)]

    def astuple(self):
        return tuple(getattr(self, name) for name, _ in self._fields_)


UNNULL_LENGTH_PREFIX, UNNULL_VALUES_FOLLOW = 1, 2  # BROTLI_AMD_UNNULL_*: a v1 data page's 4-byte length in front of the levels; the values lie behind them
UNNULL_BAD_LENGTH = 5  # UnnullResult.status behind UNRLE_*: the length prefix is cut, or says more than there is
UNNULL_NO_BITMAP = (1 << 64) - 1  # unnull_host: a segment's validity offset where it has no bitmap


class UnnullResult(ctypes.Structure):  # BrotliAmdUnnullResult: what a segment of definition levels held, its present and missing slots and the values used (batch.h)
    _fields_ = [("count", ctypes.c_uint64), ("consumed", ctypes.c_uint64), ("runs", ctypes.c_uint64), ("status", ctypes.c_uint32), ("bits", ctypes.c_uint32),
                ("present", ctypes.c_uint64), ("missing", ctypes.c_uint64), ("values", ctypes.c_uint64)]

    def astuple(self):
        return (self.count, self.consumed, self.runs, self.status, self.bits, self.present, self.missing, self.values)


def build(force=False):
    """Compile the HIP kernels for gfx950 and link the C-ABI library in-tree."""
    if force:
        subprocess.check_call(["make", "-s", "-C", _HERE, "clean"])
    subprocess.check_call(["make", "-s", "-C", _HERE])


_lib = None


def load_library():
    """The HIP extension.  Raises if it has not been built -- there is nothing to fall back to."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    L.BrotliDecoderCreateInstance.restype = vp
    L.BrotliDecoderCreateInstance.argtypes = [vp, vp, vp]
    L.BrotliDecoderDestroyInstance.argtypes = [vp]
    L.BrotliDecoderSetParameter.argtypes = [vp, ctypes.c_int, u32]
    L.BrotliDecoderDecompress.argtypes = [sz, vp, ctypes.POINTER(sz), vp]
    L.BrotliDecoderDecompressWithReturnInfo.restype = ReturnInfo
    L.BrotliDecoderDecompressWithReturnInfo.argtypes = [sz, vp, sz, vp]
    L.BrotliDecoderDecompressPrealloc.restype = ReturnInfo
    L.BrotliDecoderDecompressPrealloc.argtypes = [sz, vp, sz, vp, sz, vp, sz, vp, sz, vp]
    L.BrotliDecoderDecompressStream.argtypes = [vp, ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp),
                                                ctypes.POINTER(sz)]
    L.BrotliDecoderDecompressStreaming.argtypes = [vp, ctypes.POINTER(sz), vp, ctypes.POINTER(sz), vp]
    for name in ("BrotliDecoderHasMoreOutput", "BrotliDecoderIsUsed", "BrotliDecoderIsFinished", "BrotliDecoderGetErrorCode"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = ctypes.c_int
    L.BrotliDecoderTakeOutput.restype = vp
    L.BrotliDecoderTakeOutput.argtypes = [vp, ctypes.POINTER(sz)]
    L.BrotliDecoderGetErrorString.restype = ctypes.c_char_p
    L.BrotliDecoderGetErrorString.argtypes = [vp]
    L.BrotliDecoderErrorString.restype = ctypes.c_char_p
    L.BrotliDecoderErrorString.argtypes = [ctypes.c_int]
    L.BrotliDecoderVersion.restype = u32
    L.BrotliDecoderMallocU8.restype = vp
    L.BrotliDecoderMallocU8.argtypes = [vp, sz]
    L.BrotliDecoderFreeU8.argtypes = [vp, vp, sz]
    L.BrotliDecoderMallocUsize.restype = vp
    L.BrotliDecoderMallocUsize.argtypes = [vp, sz]
    L.BrotliDecoderFreeUsize.argtypes = [vp, vp, sz]
    L.BrotliAmdBatchCreate.restype = vp
    L.BrotliAmdBatchCreate.argtypes = [u32, u32, u32]
    L.BrotliAmdBatchDestroy.argtypes = [vp]
    L.BrotliAmdBatchDecodeDevice.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp]
    L.BrotliAmdBatchRelaunch.argtypes = [vp, vp]
    L.BrotliAmdBatchWait.argtypes = [vp, vp]
    L.BrotliAmdBatchDecodeHost.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp]
    if hasattr(L, "BrotliAmdBatchDecodeDeviceDict"):   # (custom dictionaries: an older build of the library, loaded for an A/B, has none)
        L.BrotliAmdBatchDecodeDeviceDict.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, u32, vp]
        L.BrotliAmdBatchDecodeHostDict.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, u32, vp]
        L.BrotliAmdDecoderAttachDictionary.argtypes = [vp, vp, sz]
        L.BrotliAmdDecoderAttachDictionary.restype = ctypes.c_int
    if hasattr(L, "BrotliAmdStreamSetCreate"):   # (stream sets and the ragged copy: an older build of the library, loaded for an A/B, has none)
        L.BrotliAmdStreamSetCreate.restype = vp
        L.BrotliAmdStreamSetCreate.argtypes = [u32]
        L.BrotliAmdStreamSetDestroy.argtypes = [vp]
        L.BrotliAmdStreamSetDecompress.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp]
        for name in ("BrotliAmdStreamSetLastLaunches", "BrotliAmdStreamSetLastTransfers"):
            getattr(L, name).restype = u32
            getattr(L, name).argtypes = [vp]
        L.BrotliAmdDebugRaggedCopy.argtypes = [u32, vp, vp, vp]
        L.BrotliAmdDebugRaggedCopyTile.restype = u32
    if hasattr(L, "BrotliAmdBatchSizeHints"):   # (size hints and the packed decode: an older build of the library, loaded for an A/B, has none)
        L.BrotliAmdBatchSizeHints.argtypes = [vp, u32, vp, vp, u32, vp, vp]
        L.BrotliAmdDebugSizeWalk.argtypes = [vp, sz, u32, vp]
        L.BrotliAmdBatchDecodeDevicePacked.argtypes = [vp, u32, vp, vp, vp, vp, ctypes.c_uint64, u32, vp, vp]
        L.BrotliAmdBatchDecodeHostPacked.argtypes = [vp, u32, vp, vp, vp, vp, ctypes.c_uint64, u32, vp]
        L.BrotliAmdBatchPackedOutput.restype = vp
        L.BrotliAmdBatchPackedOutput.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint64))]
        L.BrotliAmdBatchPackedFetch.argtypes = [vp, vp]
        for name in ("BrotliAmdBatchLastPackedLaunches", "BrotliAmdBatchLastPackedCopies"):
            getattr(L, name).restype = u32
            getattr(L, name).argtypes = [vp]
    if hasattr(L, "BrotliAmdBatchDigestSegments"):   # (digests: an older build of the library, loaded for an A/B, has none)
        L.BrotliAmdBatchDigestSegments.argtypes = [vp, u32, u32, vp, vp, vp, vp]
        L.BrotliAmdBatchDigestOutputs.argtypes = [vp, u32, vp]
        L.BrotliAmdBatchLastDigestMs.restype = ctypes.c_float
        L.BrotliAmdBatchLastDigestMs.argtypes = [vp]
        L.BrotliAmdDebugDigestTile.restype = u32
        L.BrotliAmdDebugDigestHost.restype = u32
        L.BrotliAmdDebugDigestHost.argtypes = [u32, vp, sz, u32, u32]
        L.BrotliAmdDebugDigestShift.restype = u32
        L.BrotliAmdDebugDigestShift.argtypes = [u32, u32, ctypes.c_uint64]
    # the element filters, name -> (restype, argtypes), None where ctypes' default stands.  A filter is there or not as a whole: an older build of
    # the library, loaded for an A/B, has those of its time
    f32, u64 = ctypes.c_float, ctypes.c_uint64
    for protos in (
            {"BrotliAmdBatchUnshuffleSegments": (None, [vp, u32, vp, vp, vp, vp, vp]), "BrotliAmdBatchUnshuffleOutputs": (None, [vp, vp, vp]),
             "BrotliAmdBatchLastUnshuffleMs": (f32, [vp]), "BrotliAmdDebugUnshuffleTile": (u32, None),
             "BrotliAmdDebugUnshuffleHost": (None, [u32, vp, sz, vp, u32, u32])},
            {"BrotliAmdBatchUndeltaSegments": (None, [vp, u32, vp, vp, vp, vp, vp]), "BrotliAmdBatchUndeltaOutputs": (None, [vp, vp, vp]),
             "BrotliAmdBatchLastUndeltaMs": (f32, [vp]), "BrotliAmdBatchLastUndeltaPhaseMs": (f32, [vp, u32]), "BrotliAmdDebugUndeltaTile": (u32, None),
             "BrotliAmdDebugUndeltaCarrySpan": (u32, None),
             "BrotliAmdDebugUndeltaHost": (None, [u32, vp, sz, vp, sz, vp, vp, vp, vp, u32, u32, u32, u32, ctypes.c_int])},
            {"BrotliAmdBatchBitUnshuffleSegments": (None, [vp, u32, vp, vp, vp, vp, vp, vp]), "BrotliAmdBatchBitUnshuffleOutputs": (None, [vp, vp, vp, vp]),
             "BrotliAmdBatchLastBitUnshuffleMs": (f32, [vp]), "BrotliAmdDebugBitUnshuffleTile": (u32, None),
             "BrotliAmdDebugBitUnshuffleHost": (None, [u32, u32, vp, sz, vp, u32, u32, vp])},
            {"BrotliAmdBatchBitUnpackSegments": (None, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]), "BrotliAmdBatchBitUnpackOutputs": (None, [vp, vp, vp, vp, vp, vp]),
             "BrotliAmdBatchLastBitUnpackMs": (f32, [vp]), "BrotliAmdDebugBitUnpackTile": (u32, None),
             "BrotliAmdDebugBitUnpackHost": (None, [u32, u32, u32, vp, sz, u64, vp, u32, u32, vp])},
            {"BrotliAmdBatchUnvarintSegments": (None, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]), "BrotliAmdBatchUnvarintOutputs": (None, [vp, vp, vp, vp, vp, vp]),
             "BrotliAmdBatchLastUnvarintMs": (f32, [vp]), "BrotliAmdBatchLastUnvarintPhaseMs": (f32, [vp, u32]), "BrotliAmdDebugUnvarintTile": (u32, None),
             "BrotliAmdDebugUnvarintHost": (None, [u32, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, vp])},
            {"BrotliAmdBatchUnrleSegments": (None, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]), "BrotliAmdBatchUnrleOutputs": (None, [vp, vp, vp, vp, vp, vp, vp]),
             "BrotliAmdBatchLastUnrleMs": (f32, [vp]), "BrotliAmdBatchLastUnrlePhaseMs": (f32, [vp, u32]), "BrotliAmdDebugUnrleItemElems": (u32, None),
             "BrotliAmdDebugUnrleWalkChunk": (u32, None),
             "BrotliAmdDebugUnrleHost": (None, [u32, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, vp])},
            {"BrotliAmdBatchUndbpSegments": (None, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]), "BrotliAmdBatchUndbpOutputs": (None, [vp, vp, vp, vp, vp, vp]),
             "BrotliAmdBatchLastUndbpMs": (f32, [vp]), "BrotliAmdBatchLastUndbpPhaseMs": (f32, [vp, u32]), "BrotliAmdDebugUndbpItemDeltas": (u32, None),
             "BrotliAmdDebugUndbpWalkChunk": (u32, None),
             "BrotliAmdDebugUndbpHost": (None, [u32, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, vp])},
            {"BrotliAmdBatchUndictSegments": (None, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
             "BrotliAmdBatchUndictOutputs": (None, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
             "BrotliAmdBatchLastUndictMs": (f32, [vp]), "BrotliAmdBatchLastUndictPhaseMs": (f32, [vp, u32]),
             "BrotliAmdDebugUndictHost": (None, [u32, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, u32, vp])},
            {"BrotliAmdBatchUnnullSegments": (None, [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
             "BrotliAmdBatchUnnullOutputs": (None, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
             "BrotliAmdBatchLastUnnullMs": (f32, [vp]), "BrotliAmdBatchLastUnnullPhaseMs": (f32, [vp, u32]),
             "BrotliAmdDebugUnnullHost": (None, [u32, vp, sz, vp, sz, vp, sz, vp, sz] + [vp] * 11 + [u32] * 6 + [vp])},
            {"BrotliAmdBatchUndictBytesSegments": (None, [vp, u32] + [vp] * 14), "BrotliAmdBatchUndictBytesOutputs": (None, [vp] * 13),
             "BrotliAmdBatchLastUndictBytesMs": (f32, [vp]), "BrotliAmdBatchLastUndictBytesPhaseMs": (f32, [vp, u32]),
             "BrotliAmdDebugUndictBytesHost": (None, [u32, vp, sz, vp, sz, vp, sz, vp, sz] + [vp] * 12 + [u32] * 7 + [vp, vp])},
            {"BrotliAmdBatchUndlbaSegments": (None, [vp, u32] + [vp] * 10), "BrotliAmdBatchUndlbaOutputs": (None, [vp] * 8),
             "BrotliAmdBatchLastUndlbaMs": (f32, [vp]), "BrotliAmdBatchLastUndlbaPhaseMs": (f32, [vp, u32]),
             "BrotliAmdDebugUndlbaHost": (None, [u32, vp, sz, vp, sz, vp, sz] + [vp] * 8 + [u32] * 5 + [vp])},
            {"BrotliAmdBatchUndbaSegments": (None, [vp, u32] + [vp] * 10), "BrotliAmdBatchUndbaOutputs": (None, [vp] * 8),
             "BrotliAmdBatchLastUndbaMs": (f32, [vp]), "BrotliAmdBatchLastUndbaPhaseMs": (f32, [vp, u32]),
             "BrotliAmdDebugUndbaHost": (None, [u32, vp, sz, vp, sz, vp, sz] + [vp] * 8 + [u32] * 5 + [vp])}):
        if hasattr(L, next(iter(protos))):
            for name, (restype, argtypes) in protos.items():
                if restype is not None:
                    getattr(L, name).restype = restype
                if argtypes is not None:
                    getattr(L, name).argtypes = argtypes
    if hasattr(L, "BrotliAmdDebugSegWalkParts"):   # (the segment walk's host model: an older build of the library, loaded for an A/B, has none)
        L.BrotliAmdDebugSegWalkParts.restype = ctypes.c_uint64
        L.BrotliAmdDebugSegWalkParts.argtypes = [u32, vp, u32, u32, vp, ctypes.c_uint64]
    L.BrotliAmdBatchLastKernelMs.restype = ctypes.c_float
    L.BrotliAmdBatchLastKernelMs.argtypes = [vp]
    L.BrotliAmdBatchLastSecondPassCount.restype = ctypes.c_uint32
    L.BrotliAmdBatchLastSecondPassCount.argtypes = [vp]
    if hasattr(L, "BrotliAmdBatchLastGang"):   # (libraries of earlier rounds, for A/B runs: tools/ab.sh)
        L.BrotliAmdBatchLastGang.restype = ctypes.c_uint32
        L.BrotliAmdBatchLastGang.argtypes = [vp]
    if hasattr(L, "BrotliAmdBatchLastProbeMs"):
        L.BrotliAmdBatchLastProbeMs.restype = ctypes.c_float
        L.BrotliAmdBatchLastProbeMs.argtypes = [vp]
    if hasattr(L, "BrotliAmdBatchLastPool"):
        L.BrotliAmdBatchLastPool.restype = ctypes.c_uint32
        L.BrotliAmdBatchLastPool.argtypes = [vp]
    L.BrotliAmdLastError.restype = ctypes.c_char_p
    if hasattr(L, "BrotliAmdLastNote"):   # (an older build of the library, loaded through BROTLI_AMD_LIB for an A/B, has no such symbol)
        L.BrotliAmdLastNote.restype = ctypes.c_char_p
    _lib = L
    return L


def last_error():
    return load_library().BrotliAmdLastError().decode()


# ------------------------------------------------------------------ one-shot (src/lib.rs:447-468)
def brotli_decode(data: bytes, out_cap: int):
    """-> (ReturnInfo, delivered bytes).  Large-window streams accepted, like the reference's brotli_decode."""
    L = load_library()
    out = ctypes.create_string_buffer(max(1, out_cap))
    src = ctypes.create_string_buffer(bytes(data), max(1, len(data)))
    info = L.BrotliDecoderDecompressWithReturnInfo(len(data), ctypes.addressof(src), out_cap, ctypes.addressof(out))
    return info, out.raw[:info.decoded_size]


def size_walk(data: bytes, flags=FLAG_LARGE_WINDOW):
    """BrotliAmdDebugSizeWalk: the size walk on the host (no device needed) -> SizeHint"""
    L = load_library()
    data = bytes(data)
    buf = ctypes.create_string_buffer(data, max(1, len(data)))
    hint = SizeHint()
    if L.BrotliAmdDebugSizeWalk(ctypes.addressof(buf), len(data), flags, ctypes.byref(hint)) != 0:
        raise RuntimeError("BrotliAmdDebugSizeWalk failed")
    return hint


def digest_host(data: bytes, kind=DIGEST_CRC32, skew=0, run_units=0):
    """BrotliAmdDebugDigestHost: the digest of `data` by the device's functions on the host (no device needed), the bytes placed `skew` past a
    16-byte boundary and cut into pieces of run_units 16-byte units (0: the kernel's own number)"""
    L = load_library()
    data = bytes(data)
    buf = ctypes.create_string_buffer(data, max(1, len(data)))
    return int(L.BrotliAmdDebugDigestHost(kind, ctypes.addressof(buf), len(data), skew, run_units))


def digest_shift(crc, nbytes, kind=DIGEST_CRC32):
    """BrotliAmdDebugDigestShift: crc x^(8 nbytes) mod the kind's polynomial -- crc(A + B) == digest_shift(crc(A), len(B)) ^ crc(B)"""
    return int(load_library().BrotliAmdDebugDigestShift(kind, crc, nbytes))


def unshuffle_host(data: bytes, width, src_skew=0, dst_skew=0):
    """BrotliAmdDebugUnshuffleHost: the byte planes in `data` back into elements of `width` bytes by the device's unit function on the host (no
    device needed), source and destination placed at their skews past a 16-byte boundary -> bytes"""
    L = load_library()
    data = bytes(data)
    src = ctypes.create_string_buffer(data, max(1, len(data)))
    dst = ctypes.create_string_buffer(max(1, len(data)))
    if L.BrotliAmdDebugUnshuffleHost(width, ctypes.addressof(src), len(data), ctypes.addressof(dst), src_skew, dst_skew) != 0:
        raise RuntimeError("BrotliAmdDebugUnshuffleHost failed: " + last_error())
    return dst.raw[:len(data)]


def unshuffle_tile():
    """BrotliAmdDebugUnshuffleTile: the bytes of destination in one tile of an unshuffle launch"""
    return int(load_library().BrotliAmdDebugUnshuffleTile())


def bitunshuffle_host(data: bytes, width, block=0, src_skew=0, dst_skew=0):
    """BrotliAmdDebugBitUnshuffleHost: the bit planes in `data` back into elements of `width` bytes, in blocks of `block` elements (0: one block),
    by the device's functions on the host (no device needed), source and destination placed at their skews past a 16-byte boundary
    -> (bytes, the runs of 32 elements that went the fast way)"""
    L = load_library()
    data = bytes(data)
    src = ctypes.create_string_buffer(data, max(1, len(data)))
    dst = ctypes.create_string_buffer(max(1, len(data)))
    fast = ctypes.c_uint64(0)
    if L.BrotliAmdDebugBitUnshuffleHost(width, block, ctypes.addressof(src), len(data), ctypes.addressof(dst), src_skew, dst_skew, ctypes.byref(fast)) != 0:
        raise RuntimeError("BrotliAmdDebugBitUnshuffleHost failed: " + last_error())
    return dst.raw[:len(data)], int(fast.value)


def bitunpack_host(data: bytes, count, bits, width, flags=0, src_skew=0, dst_skew=0):
    """BrotliAmdDebugBitUnpackHost: the first `count` fields of `bits` bits in `data` back into elements of `width` bytes (flags: BITUNPACK_*),
    by the device's functions on the host (no device needed), source and destination placed at their skews past a 16-byte boundary
    -> (bytes, the runs of 32 elements that went the fast way)"""
    L = load_library()
    data = bytes(data)
    room = count * width if 0 <= count <= (1 << 40) and 0 < width <= 8 else 0   # (what is refused writes nothing)
    src = ctypes.create_string_buffer(data, max(1, len(data)))
    dst = ctypes.create_string_buffer(max(1, room))
    fast = ctypes.c_uint64(0)
    clip = lambda v, top: v if 0 <= v <= top else top   # (what no C type of the call holds is refused as its largest value is)
    if L.BrotliAmdDebugBitUnpackHost(clip(bits, 0xFFFFFFFF), clip(width, 0xFFFFFFFF), clip(flags, 0xFFFFFFFF), ctypes.addressof(src), len(data),
                                     clip(count, (1 << 64) - 1), ctypes.addressof(dst), clip(src_skew, 0xFFFFFFFF), clip(dst_skew, 0xFFFFFFFF),
                                     ctypes.byref(fast)) != 0:
        raise RuntimeError("BrotliAmdDebugBitUnpackHost failed: " + last_error())
    return dst.raw[:room], int(fast.value)


def bitunpack_tile():
    """BrotliAmdDebugBitUnpackTile: the bytes of destination in one tile of a bit-unpack launch"""
    return int(load_library().BrotliAmdDebugBitUnpackTile())


def bitunshuffle_tile():
    """BrotliAmdDebugBitUnshuffleTile: the bytes of destination in one tile of a bit-unshuffle launch"""
    return int(load_library().BrotliAmdDebugBitUnshuffleTile())


def undelta_host(src: bytes, segs, dst_size=None, src_skew=0, dst_skew=0, tile_units=0, order_seed=0, in_place=False, fill=0):
    """BrotliAmdDebugUndeltaHost: the deltas in `src` back into values by the device's unit and tile functions on the host (no device needed).
    segs: [(source offset, destination offset, length, width)]; the destination has dst_size bytes (default: as many as the source), all
    `fill` in front of the call; the buffers are placed at their skews past a 16-byte boundary; tile_units: the 16-byte units of a tile (0: the
    kernel's); order_seed != 0 shuffles the order in which the tiles are taken; in_place: the segments' sources are their destinations, in one
    buffer that starts as `src`.  -> the destination's bytes (in place: what no segment covers is `fill`)"""
    L = load_library()
    src = bytes(src)
    dst_size = len(src) if dst_size is None else dst_size
    n = len(segs)
    s_buf = ctypes.create_string_buffer(src, max(1, len(src)))
    d_buf = ctypes.create_string_buffer(bytes([fill]) * dst_size, max(1, dst_size))
    a_s = (ctypes.c_uint64 * max(1, n))(*[s[0] for s in segs])
    a_d = (ctypes.c_uint64 * max(1, n))(*[s[1] for s in segs])
    a_l = (ctypes.c_uint64 * max(1, n))(*[s[2] for s in segs])
    a_w = (ctypes.c_uint8 * max(1, n))(*[s[3] if 0 <= s[3] <= 255 else 0 for s in segs])
    if L.BrotliAmdDebugUndeltaHost(n, ctypes.addressof(s_buf), len(src), ctypes.addressof(d_buf), dst_size, a_s, a_d, a_l, a_w, src_skew, dst_skew,
                                   tile_units, order_seed, 1 if in_place else 0) != 0:
        raise RuntimeError("BrotliAmdDebugUndeltaHost failed: " + last_error())
    return d_buf.raw[:dst_size]


def _counted_host(fn_name, Result, src, segs, dst_size, columns, src_skew, dst_skew, knob, order_seed, fill):
    """what the hooks of the filters with a result per segment share.  segs: [(source offset, source length, destination offset, capacity, ...)];
    columns: [(index in a segment's tuple, what stands in for a value no byte holds)], the byte columns in the call's order; knob: the tile or item
    size.  -> (the destination's bytes, [a result's tuple per segment])"""
    L = load_library()
    src = bytes(src)
    n = len(segs)
    before = bytes(fill) if isinstance(fill, (bytes, bytearray)) else bytes([fill]) * dst_size
    if len(before) != dst_size:
        raise ValueError("fill: %d bytes for a destination of %d" % (len(before), dst_size))
    s_buf = ctypes.create_string_buffer(src, max(1, len(src)))
    d_buf = ctypes.create_string_buffer(before, max(1, dst_size))
    u64s = [(ctypes.c_uint64 * max(1, n))(*[s[k] if 0 <= s[k] < (1 << 64) else (1 << 64) - 1 for s in segs]) for k in range(4)]
    u8s = [(ctypes.c_uint8 * max(1, n))(*[s[k] if 0 <= s[k] <= 255 else bad for s in segs]) for k, bad in columns]
    res = (Result * max(1, n))()
    if getattr(L, fn_name)(n, ctypes.addressof(s_buf), len(src), ctypes.addressof(d_buf), dst_size, *u64s, *u8s, src_skew, dst_skew, knob, order_seed, res) != 0:
        raise RuntimeError(fn_name + " failed: " + last_error())
    return d_buf.raw[:dst_size], [res[i].astuple() for i in range(n)]


def unvarint_host(src: bytes, segs, dst_size, src_skew=0, dst_skew=0, tile_units=0, order_seed=0, fill=0):
    """BrotliAmdDebugUnvarintHost: the LEB128 varints in `src` back into elements by the device's unit and tile functions on the host (no device
    needed).  segs: [(source offset, source length, destination offset, capacity in elements, width, flags)]; the destination has dst_size bytes,
    all `fill` in front of the call (or, where `fill` is bytes of that size, those); the buffers are placed at their skews past a 16-byte
    boundary; tile_units: the 16-byte units of SOURCE in a tile (0: the kernel's); order_seed != 0 shuffles the order in which the tiles are
    taken.  -> (the destination's bytes, [(count, consumed, overlong)])"""
    return _counted_host("BrotliAmdDebugUnvarintHost", UnvarintResult, src, segs, dst_size, [(4, 0), (5, 255)], src_skew, dst_skew, tile_units, order_seed, fill)


def unrle_host(src: bytes, segs, dst_size, src_skew=0, dst_skew=0, item_elems=0, order_seed=0, fill=0):
    """BrotliAmdDebugUnrleHost: the RLE / bit-packed hybrid runs in `src` back into elements by the device's walk and item functions on the host
    (no device needed).  segs: [(source offset, source length, destination offset, capacity in elements, bits, width, flags)]; the destination
    has dst_size bytes, all `fill` in front of the call (or, where `fill` is bytes of that size, those); the buffers are placed at their skews
    past a 16-byte boundary; item_elems: the elements of an item (0: the device's); order_seed != 0 shuffles the order in which the items are
    taken.  -> (the destination's bytes, [(count, consumed, runs, status, bits)])"""
    return _counted_host("BrotliAmdDebugUnrleHost", UnrleResult, src, segs, dst_size, [(4, 255), (5, 0), (6, 255)], src_skew, dst_skew, item_elems, order_seed, fill)


def undbp_host(src: bytes, segs, dst_size, src_skew=0, dst_skew=0, item_deltas=0, order_seed=0, fill=0):
    """BrotliAmdDebugUndbpHost: the DELTA_BINARY_PACKED streams in `src` back into elements by the device's walk, block, group and item functions on
    the host (no device needed).  segs: [(source offset, source length, destination offset, capacity in elements, width)] -- a sixth entry is the
    segment's flags, which are all refused --; the destination has dst_size bytes, all `fill` in front of the call (or, where `fill` is bytes of
    that size, those); the buffers are placed at their skews past a 16-byte boundary; item_deltas: the deltas of an item, a multiple of 32 (0: the
    device's); order_seed != 0 shuffles the order in which the items are taken.
    -> (the destination's bytes, [(count, consumed, declared, blocks, status, block_values, miniblocks)])"""
    segs = [tuple(s) if len(s) > 5 else tuple(s) + (0,) for s in segs]
    return _counted_host("BrotliAmdDebugUndbpHost", UndbpResult, src, segs, dst_size, [(4, 0), (5, 255)], src_skew, dst_skew, item_deltas, order_seed, fill)


def undict_host(src: bytes, dictionary: bytes, segs, dst_size, src_skew=0, dst_skew=0, dict_skew=0, item_elems=0, order_seed=0, fill=0):
    """BrotliAmdDebugUndictHost: the dictionary-index runs in `src` back into the values they name in `dictionary`, by unrle's walk and the item
    and lookup functions of csrc/brotli_undict.h on the host (no device needed).  segs: [(source offset, source length, destination offset,
    capacity in elements, bits, width, flags, dictionary offset, dictionary entries)]; the destination has dst_size bytes, all `fill` in front
    of the call (or, where `fill` is bytes of that size, those); the three buffers are placed at their skews past a 16-byte boundary;
    item_elems: the elements of an item (0: the device's, unrle_item_elems()); order_seed != 0 shuffles the order in which the items are taken.
    -> (the destination's bytes, [(count, consumed, runs, status, bits, bad, first_bad)])"""
    L = load_library()
    src, dictionary, n = bytes(src), bytes(dictionary), len(segs)
    before = bytes(fill) if isinstance(fill, (bytes, bytearray)) else bytes([fill]) * dst_size
    if len(before) != dst_size:
        raise ValueError("fill: %d bytes for a destination of %d" % (len(before), dst_size))
    s_buf = ctypes.create_string_buffer(src, max(1, len(src)))
    d_buf = ctypes.create_string_buffer(before, max(1, dst_size))
    t_buf = ctypes.create_string_buffer(dictionary, max(1, len(dictionary)))
    u64s = [(ctypes.c_uint64 * max(1, n))(*[s[k] if 0 <= s[k] < (1 << 64) else (1 << 64) - 1 for s in segs]) for k in (0, 1, 2, 3, 7, 8)]
    u8s = [(ctypes.c_uint8 * max(1, n))(*[s[k] if 0 <= s[k] <= 255 else bad for s in segs]) for k, bad in [(4, 255), (5, 0), (6, 255)]]
    res = (UndictResult * max(1, n))()
    if L.BrotliAmdDebugUndictHost(n, ctypes.addressof(s_buf), len(src), ctypes.addressof(d_buf), dst_size, ctypes.addressof(t_buf), len(dictionary),
                                  *u64s, *u8s, src_skew, dst_skew, dict_skew, item_elems, order_seed, res) != 0:
        raise RuntimeError("BrotliAmdDebugUndictHost failed: " + last_error())
    return d_buf.raw[:dst_size], [res[i].astuple() for i in range(n)]


def undict_bytes_host(src: bytes, dictionary: bytes, segs, offsets_size, data_size, src_skew=0, offsets_skew=0, data_skew=0, dict_skew=0, item_elems=0, order_seed=0,
                      word_seed=0, offsets_fill=0, data_fill=0):
    """BrotliAmdDebugUndictBytesHost: the dictionary-index runs in `src` and the PLAIN byte arrays in `dictionary` back into offsets and bytes, by
    unrle's walk and the functions of csrc/brotli_undict_bytes.h on the host (no device needed).  segs: [(source offset, source length, offsets
    offset or UNDICT_BYTES_NO_DESTINATION, data offset or UNDICT_BYTES_NO_DESTINATION, data capacity in bytes, capacity in elements, offset
    base, dictionary offset, dictionary length, dictionary entries or UNDICT_BYTES_ALL, bits, flags)]; the two destinations have offsets_size
    and data_size bytes, all `offsets_fill` and `data_fill` in front of the call (or, where those are bytes of that size, those); the four
    buffers are placed at their skews past a 16-byte boundary; item_elems: the elements of an item (0: the device's, unrle_item_elems());
    order_seed != 0 shuffles the order in which the items are taken, word_seed != 0 that of an item's destination words.
    -> (the offsets' bytes, the data's bytes, [(count, consumed, runs, status, bits, bad, first_bad, bytes, dict_entries, dict_consumed,
    dict_status)], the dictionaries that were walked)"""
    L = load_library()
    src, dictionary, n = bytes(src), bytes(dictionary), len(segs)
    rooms = []
    for fill, size, what in ((offsets_fill, offsets_size, "offsets_fill"), (data_fill, data_size, "data_fill")):
        before = bytes(fill) if isinstance(fill, (bytes, bytearray)) else bytes([fill]) * size
        if len(before) != size:
            raise ValueError("%s: %d bytes for a destination of %d" % (what, len(before), size))
        rooms.append(ctypes.create_string_buffer(before, max(1, size)))
    s_buf = ctypes.create_string_buffer(src, max(1, len(src)))
    t_buf = ctypes.create_string_buffer(dictionary, max(1, len(dictionary)))
    # the call's order: source, offsets, data, data capacity, capacity, base, dictionary offset, length, entries
    u64s = [(ctypes.c_uint64 * max(1, n))(*[s[k] if 0 <= s[k] < (1 << 64) else (1 << 64) - 1 for s in segs]) for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)]
    u8s = [(ctypes.c_uint8 * max(1, n))(*[s[k] if 0 <= s[k] <= 255 else 255 for s in segs]) for k in (10, 11)]
    res = (UndictBytesResult * max(1, n))()
    walks = ctypes.c_uint64(0)
    if L.BrotliAmdDebugUndictBytesHost(n, ctypes.addressof(s_buf), len(src), ctypes.addressof(rooms[0]), offsets_size, ctypes.addressof(rooms[1]), data_size,
                                       ctypes.addressof(t_buf), len(dictionary), *u64s, *u8s, src_skew, offsets_skew, data_skew, dict_skew, item_elems, order_seed,
                                       word_seed, res, ctypes.byref(walks)) != 0:
        raise RuntimeError("BrotliAmdDebugUndictBytesHost failed: " + last_error())
    return rooms[0].raw[:offsets_size], rooms[1].raw[:data_size], [res[i].astuple() for i in range(n)], walks.value


def undlba_host(src: bytes, segs, offsets_size, data_size, src_skew=0, offsets_skew=0, data_skew=0, item_deltas=0, order_seed=0, offsets_fill=0, data_fill=0):
    """BrotliAmdDebugUndlbaHost: the DELTA_LENGTH_BYTE_ARRAY bodies in `src` back into offsets and bytes, by undbp's walk and items and the
    functions of csrc/brotli_undlba.h on the host (no device needed).  segs: [(source offset, source length, offsets offset or
    UNDLBA_NO_DESTINATION, data offset or UNDLBA_NO_DESTINATION, data capacity in bytes, capacity in elements, offset base, flags)]; the two
    destinations have offsets_size and data_size bytes, all `offsets_fill` and `data_fill` in front of the call (or, where those are bytes of
    that size, those); the three buffers are placed at their skews past a 16-byte boundary; item_deltas: the deltas of an item, a multiple of
    32 (0: the device's, undbp_item_deltas()); order_seed != 0 shuffles the order in which the items are taken, in every phase.
    -> (the offsets' bytes, the data's bytes, [(count, consumed, declared, blocks, status, block_values, miniblocks, data_status, bad,
    first_bad, bytes, data_avail)])"""
    L = load_library()
    src, n = bytes(src), len(segs)
    rooms = []
    for fill, size, what in ((offsets_fill, offsets_size, "offsets_fill"), (data_fill, data_size, "data_fill")):
        before = bytes(fill) if isinstance(fill, (bytes, bytearray)) else bytes([fill]) * size
        if len(before) != size:
            raise ValueError("%s: %d bytes for a destination of %d" % (what, len(before), size))
        rooms.append(ctypes.create_string_buffer(before, max(1, size)))
    s_buf = ctypes.create_string_buffer(src, max(1, len(src)))
    # the call's order: source, length, offsets, data, data capacity, capacity, base
    u64s = [(ctypes.c_uint64 * max(1, n))(*[s[k] if 0 <= s[k] < (1 << 64) else (1 << 64) - 1 for s in segs]) for k in range(7)]
    flags = (ctypes.c_uint8 * max(1, n))(*[s[7] if 0 <= s[7] <= 255 else 255 for s in segs])
    res = (UndlbaResult * max(1, n))()
    if L.BrotliAmdDebugUndlbaHost(n, ctypes.addressof(s_buf), len(src), ctypes.addressof(rooms[0]), offsets_size, ctypes.addressof(rooms[1]), data_size, *u64s, flags,
                                  src_skew, offsets_skew, data_skew, item_deltas, order_seed, res) != 0:
        raise RuntimeError("BrotliAmdDebugUndlbaHost failed: " + last_error())
    return rooms[0].raw[:offsets_size], rooms[1].raw[:data_size], [res[i].astuple() for i in range(n)]


def undba_host(src: bytes, segs, offsets_size, data_size, src_skew=0, offsets_skew=0, data_skew=0, item_deltas=0, order_seed=0, offsets_fill=0, data_fill=0):
    """BrotliAmdDebugUndbaHost: the DELTA_BYTE_ARRAY bodies in `src` back into offsets and bytes, by undbp's walk and items and the functions
    of csrc/brotli_undba.h on the host (no device needed), with undlba_host's arguments: segs: [(source offset, source length, offsets offset
    or UNDBA_NO_DESTINATION, data offset or UNDBA_NO_DESTINATION, data capacity in bytes, capacity in elements, offset base, flags)];
    order_seed != 0 shuffles the order in which the items are taken in every phase where it is free.
    -> (the offsets' bytes, the data's bytes, [UndbaResult's twenty fields in their order])"""
    L = load_library()
    src, n = bytes(src), len(segs)
    rooms = []
    for fill, size, what in ((offsets_fill, offsets_size, "offsets_fill"), (data_fill, data_size, "data_fill")):
        before = bytes(fill) if isinstance(fill, (bytes, bytearray)) else bytes([fill]) * size
        if len(before) != size:
            raise ValueError("%s: %d bytes for a destination of %d" % (what, len(before), size))
        rooms.append(ctypes.create_string_buffer(before, max(1, size)))
    s_buf = ctypes.create_string_buffer(src, max(1, len(src)))
    # the call's order: source, length, offsets, data, data capacity, capacity, base
    u64s = [(ctypes.c_uint64 * max(1, n))(*[s[k] if 0 <= s[k] < (1 << 64) else (1 << 64) - 1 for s in segs]) for k in range(7)]
    flags = (ctypes.c_uint8 * max(1, n))(*[s[7] if 0 <= s[7] <= 255 else 255 for s in segs])
    res = (UndbaResult * max(1, n))()
    if L.BrotliAmdDebugUndbaHost(n, ctypes.addressof(s_buf), len(src), ctypes.addressof(rooms[0]), offsets_size, ctypes.addressof(rooms[1]), data_size, *u64s, flags,
                                 src_skew, offsets_skew, data_skew, item_deltas, order_seed, res) != 0:
        raise RuntimeError("BrotliAmdDebugUndbaHost failed: " + last_error())
    return rooms[0].raw[:offsets_size], rooms[1].raw[:data_size], [res[i].astuple() for i in range(n)]


def unnull_host(src: bytes, values: bytes, segs, dst_size, valid_size, src_skew=0, dst_skew=0, values_skew=0, valid_skew=0, item_elems=0, order_seed=0, fill=0,
                valid_fill=0):
    """BrotliAmdDebugUnnullHost: the dense `values` spread over nulls by the definition levels in `src`, by unrle's walk and the prefix, mask,
    rank and validity functions of csrc/brotli_unnull.h on the host (no device needed).  segs: [(source offset, source length, destination
    offset, capacity in slots, bits, width, flags, level, values offset, values count, validity offset or UNNULL_NO_BITMAP)]; the destination
    has dst_size bytes and the bitmaps' buffer valid_size, all `fill` and `valid_fill` in front of the call (or, where those are bytes of that
    size, those); the four buffers are placed at their skews past a 16-byte boundary; item_elems: the slots of an item, a multiple of 8 (0:
    the device's, unrle_item_elems()); order_seed != 0 shuffles the order in which the items are taken, in both phases.
    -> (the destination's bytes, the bitmaps' bytes, [(count, consumed, runs, status, bits, present, missing, values)])"""
    L = load_library()
    src, values, n = bytes(src), bytes(values), len(segs)

    def before(f, size):
        b = bytes(f) if isinstance(f, (bytes, bytearray)) else bytes([f]) * size
        if len(b) != size:
            raise ValueError("fill: %d bytes for a buffer of %d" % (len(b), size))
        return b
    s_buf = ctypes.create_string_buffer(src, max(1, len(src)))
    d_buf = ctypes.create_string_buffer(before(fill, dst_size), max(1, dst_size))
    v_buf = ctypes.create_string_buffer(values, max(1, len(values)))
    b_buf = ctypes.create_string_buffer(before(valid_fill, valid_size), max(1, valid_size))
    u64s = [(ctypes.c_uint64 * max(1, n))(*[s[k] if 0 <= s[k] < (1 << 64) else (1 << 64) - 1 for s in segs]) for k in (0, 1, 2, 3, 8, 9, 10)]
    lv = (ctypes.c_uint32 * max(1, n))(*[s[7] for s in segs])
    u8s = [(ctypes.c_uint8 * max(1, n))(*[s[k] if 0 <= s[k] <= 255 else bad for s in segs]) for k, bad in [(4, 255), (5, 0), (6, 255)]]
    res = (UnnullResult * max(1, n))()
    if L.BrotliAmdDebugUnnullHost(n, ctypes.addressof(s_buf), len(src), ctypes.addressof(d_buf), dst_size, ctypes.addressof(v_buf), len(values),
                                  ctypes.addressof(b_buf), valid_size, *u64s, lv, *u8s, src_skew, dst_skew, values_skew, valid_skew, item_elems, order_seed, res) != 0:
        raise RuntimeError("BrotliAmdDebugUnnullHost failed: " + last_error())
    return d_buf.raw[:dst_size], b_buf.raw[:valid_size], [res[i].astuple() for i in range(n)]


def undbp_item_deltas():
    """BrotliAmdDebugUndbpItemDeltas: the deltas of one item of an undbp call"""
    return int(load_library().BrotliAmdDebugUndbpItemDeltas())


def undbp_walk_chunk():
    """BrotliAmdDebugUndbpWalkChunk: the source bytes that the walk of an undbp call stages at a time"""
    return int(load_library().BrotliAmdDebugUndbpWalkChunk())


def unrle_item_elems():
    """BrotliAmdDebugUnrleItemElems: the elements of one item of an unrle call's expansion"""
    return int(load_library().BrotliAmdDebugUnrleItemElems())


def unrle_walk_chunk():
    """BrotliAmdDebugUnrleWalkChunk: the source bytes that the walk of an unrle call stages at a time"""
    return int(load_library().BrotliAmdDebugUnrleWalkChunk())


def unvarint_tile():
    """BrotliAmdDebugUnvarintTile: the bytes of SOURCE in one tile of an unvarint call"""
    return int(load_library().BrotliAmdDebugUnvarintTile())


def undelta_tile():
    """BrotliAmdDebugUndeltaTile: the bytes of destination in one tile of an undelta call"""
    return int(load_library().BrotliAmdDebugUndeltaTile())


def undelta_carry_span():
    """BrotliAmdDebugUndeltaCarrySpan: the tiles the carry launch's one block takes in one pass of its loop"""
    return int(load_library().BrotliAmdDebugUndeltaCarrySpan())


def seg_walk_parts(units, tile_units, grid):
    """BrotliAmdDebugSegWalkParts: the segment walk of csrc/brotli_seg_walk.h on the host (no device needed) over segments of units[i] 16-byte
    units each, with tiles of tile_units and `grid` blocks -> [(block, tile, lo, hi)], every part of every block's tiles, block by block"""
    L = load_library()
    n = len(units)
    a_u = (ctypes.c_uint64 * max(1, n))(*units)
    count = int(L.BrotliAmdDebugSegWalkParts(n, a_u, tile_units, grid, None, 0))
    out = (ctypes.c_uint64 * max(1, 4 * count))()
    if int(L.BrotliAmdDebugSegWalkParts(n, a_u, tile_units, grid, out, count)) != count:
        raise RuntimeError("BrotliAmdDebugSegWalkParts: two runs disagree")
    return [tuple(out[4 * k:4 * k + 4]) for k in range(count)]


# ------------------------------------------------------------------ batch (include/brotli/batch.h)
class Batch:
    """Owns one BrotliAmdBatch on the current HIP device."""

    def __init__(self, max_streams, lds_arena_bytes=0, grid_blocks=0):
        self._L = load_library()
        self._h = self._L.BrotliAmdBatchCreate(max_streams, lds_arena_bytes, grid_blocks)
        if not self._h:
            raise RuntimeError("BrotliAmdBatchCreate failed: " + last_error())
        self.max_streams = max_streams
        self.n = 0
        self.out_n = 0   # streams of the last decode call, a packed one included (digest_outputs)
        self.out_sizes = None   # their delivered bytes (None: no call yet, or a launch nobody has waited for): tensors.outputs_as_tensors
        self._caps = []

    def close(self):
        if self._h:
            self._L.BrotliAmdBatchDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_device(self, in_ptrs, in_sizes, out_ptrs, out_caps, flags=FLAG_LARGE_WINDOW, stream=None, dict_ptrs=None, dict_sizes=None):
        """Device pointers in, asynchronous launch on `stream` (a hipStream_t handle as int, None = default).
        dict_ptrs / dict_sizes: per stream the device address and size of its custom dictionary (None or 0: none) --
        BrotliAmdBatchDecodeDeviceDict; the dictionaries stay where they are until wait() has returned."""
        n = len(in_ptrs)
        a_in = (ctypes.c_void_p * n)(*in_ptrs)
        a_is = (ctypes.c_size_t * n)(*in_sizes)
        a_out = (ctypes.c_void_p * n)(*out_ptrs)
        a_oc = (ctypes.c_size_t * n)(*out_caps)
        if dict_ptrs is not None or dict_sizes is not None:
            if dict_ptrs is None or dict_sizes is None or len(dict_ptrs) != n or len(dict_sizes) != n:
                raise ValueError("dict_ptrs and dict_sizes: one entry per stream each")
            a_dp = (ctypes.c_void_p * n)(*[p or None for p in dict_ptrs])
            a_ds = (ctypes.c_size_t * n)(*[int(v or 0) for v in dict_sizes])
            if self._L.BrotliAmdBatchDecodeDeviceDict(self._h, n, a_in, a_is, a_out, a_oc, a_dp, a_ds, flags, stream) != 0:
                raise RuntimeError("BrotliAmdBatchDecodeDeviceDict failed: " + last_error())
        elif self._L.BrotliAmdBatchDecodeDevice(self._h, n, a_in, a_is, a_out, a_oc, flags, stream) != 0:
            raise RuntimeError("BrotliAmdBatchDecodeDevice failed: " + last_error())
        self.n = self.out_n = n
        self.out_sizes, self._caps = None, list(out_caps)

    def relaunch(self, stream=None):
        if self._L.BrotliAmdBatchRelaunch(self._h, stream) != 0:
            raise RuntimeError("BrotliAmdBatchRelaunch failed: " + last_error())

    def wait(self):
        res = (BatchResult * max(1, self.n))()
        if self._L.BrotliAmdBatchWait(self._h, res) != 0:
            raise RuntimeError("BrotliAmdBatchWait failed: " + last_error())
        if self.n and self.out_n == self.n:
            self.out_sizes = [min(res[i].decoded_size, self._caps[i]) for i in range(self.n)]
        return list(res)[:self.n]

    def last_kernel_ms(self):
        return float(self._L.BrotliAmdBatchLastKernelMs(self._h))

    def last_second_pass_count(self):
        return int(self._L.BrotliAmdBatchLastSecondPassCount(self._h))

    def last_gang(self):
        """blocks (CUs) a stream of the last launch: 1, or 2 / 4 / 8 where each stream had a gang of blocks"""
        return int(self._L.BrotliAmdBatchLastGang(self._h)) if hasattr(self._L, "BrotliAmdBatchLastGang") else 1

    def last_probe_ms(self):
        """host milliseconds the last decode call spent asking the device what kind the batch's streams are (batch.h; 0: no probe)"""
        return float(self._L.BrotliAmdBatchLastProbeMs(self._h)) if hasattr(self._L, "BrotliAmdBatchLastProbeMs") else 0.0

    def last_pool(self):
        """whether the last launch was a pool: blocks without a stream of their own help the largest stream still being decoded"""
        return bool(self._L.BrotliAmdBatchLastPool(self._h)) if hasattr(self._L, "BrotliAmdBatchLastPool") else False

    def decode_host(self, datas, out_caps, flags=FLAG_LARGE_WINDOW, dicts=None):
        """Host bytes in, (results, outputs) out: upload, decode, download.
        dicts: per stream its custom dictionary (bytes; None or b"": none) -- BrotliAmdBatchDecodeHostDict.  Streams that are
        given the same bytes object share one upload."""
        n = len(datas)
        ins = [ctypes.create_string_buffer(bytes(d), max(1, len(d))) for d in datas]
        outs = [ctypes.create_string_buffer(max(1, c)) for c in out_caps]
        a_in = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in ins])
        a_is = (ctypes.c_size_t * n)(*[len(d) for d in datas])
        a_out = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in outs])
        a_oc = (ctypes.c_size_t * n)(*out_caps)
        res = (BatchResult * max(1, n))()
        if dicts is not None:
            if len(dicts) != n:
                raise ValueError("dicts: one entry per stream")
            held = {}  # id of the caller's object -> its buffer: one (pointer, size) pair per distinct dictionary
            for d in dicts:
                if d and id(d) not in held:
                    held[id(d)] = ctypes.create_string_buffer(bytes(d), len(d))
            a_dp = (ctypes.c_void_p * n)(*[ctypes.addressof(held[id(d)]) if d else None for d in dicts])
            a_ds = (ctypes.c_size_t * n)(*[len(d) if d else 0 for d in dicts])
            if self._L.BrotliAmdBatchDecodeHostDict(self._h, n, a_in, a_is, a_out, a_oc, a_dp, a_ds, flags, res) != 0:
                raise RuntimeError("BrotliAmdBatchDecodeHostDict failed: " + last_error())
        elif self._L.BrotliAmdBatchDecodeHost(self._h, n, a_in, a_is, a_out, a_oc, flags, res) != 0:
            raise RuntimeError("BrotliAmdBatchDecodeHost failed: " + last_error())
        self.n = self.out_n = n
        results = list(res)[:n]
        self.out_sizes = [min(results[i].decoded_size, out_caps[i]) for i in range(n)]
        return results, [outs[i].raw[:min(results[i].decoded_size, out_caps[i])] for i in range(n)]

    def size_hints(self, in_ptrs, in_sizes, flags=FLAG_LARGE_WINDOW, stream=None):
        """BrotliAmdBatchSizeHints: device pointers in -> [SizeHint], one launch of one lane a stream and a wait on `stream`"""
        n = len(in_ptrs)
        a_in = (ctypes.c_void_p * max(1, n))(*in_ptrs)
        a_is = (ctypes.c_size_t * max(1, n))(*in_sizes)
        hints = (SizeHint * max(1, n))()
        if self._L.BrotliAmdBatchSizeHints(self._h, n, a_in, a_is, flags, hints, stream) != 0:
            raise RuntimeError("BrotliAmdBatchSizeHints failed: " + last_error())
        return list(hints)[:n]

    def _packed_view(self, n):
        offs = ctypes.POINTER(ctypes.c_uint64)()
        ptr = self._L.BrotliAmdBatchPackedOutput(self._h, ctypes.byref(offs))
        if not offs:
            raise RuntimeError("no packed output: the last decode call on this object was not a packed call that succeeded")
        return ptr or 0, [int(offs[i]) for i in range(n + 1)]

    def decode_device_packed(self, in_ptrs, in_sizes, dict_ptrs=None, dict_sizes=None, max_out=0, flags=FLAG_LARGE_WINDOW, stream=None):
        """BrotliAmdBatchDecodeDevicePacked: device pointers in, NO output buffers and no sizes -> (results, device pointer, offsets).
        Synchronous.  Stream i's bytes are [offsets[i], offsets[i + 1]) of the library's buffer at the device pointer (0 where the
        batch delivered nothing), valid until the next decode call on this object; packed_fetch() copies them to the host."""
        n = len(in_ptrs)
        a_in = (ctypes.c_void_p * max(1, n))(*in_ptrs)
        a_is = (ctypes.c_size_t * max(1, n))(*in_sizes)
        a_dp = a_ds = None
        if dict_ptrs is not None or dict_sizes is not None:
            if dict_ptrs is None or dict_sizes is None or len(dict_ptrs) != n or len(dict_sizes) != n:
                raise ValueError("dict_ptrs and dict_sizes: one entry per stream each")
            a_dp = (ctypes.c_void_p * max(1, n))(*[p or None for p in dict_ptrs])
            a_ds = (ctypes.c_size_t * max(1, n))(*[int(v or 0) for v in dict_sizes])
        res = (BatchResult * max(1, n))()
        if self._L.BrotliAmdBatchDecodeDevicePacked(self._h, n, a_in, a_is, a_dp, a_ds, max_out, flags, stream, res) != 0:
            raise RuntimeError("BrotliAmdBatchDecodeDevicePacked failed: " + last_error())
        self.n, self.out_n = 0, n
        ptr, offsets = self._packed_view(n)
        self.out_sizes = [offsets[i + 1] - offsets[i] for i in range(n)]
        return list(res)[:n], ptr, offsets

    def packed_fetch(self, total):
        """BrotliAmdBatchPackedFetch: the whole packed output of the last packed call (total = offsets[-1] bytes) as bytes"""
        buf = ctypes.create_string_buffer(max(1, total))
        if self._L.BrotliAmdBatchPackedFetch(self._h, ctypes.addressof(buf)) != 0:
            raise RuntimeError("BrotliAmdBatchPackedFetch failed: " + last_error())
        return buf.raw[:total]

    def decode_packed(self, datas, dicts=None, max_out=0, flags=FLAG_LARGE_WINDOW):
        """Host bytes in, (results, [bytes]) out without any sizes from the caller: BrotliAmdBatchDecodeHostPacked, then a fetch.
        dicts: as in decode_host."""
        n = len(datas)
        ins = [ctypes.create_string_buffer(bytes(d), max(1, len(d))) for d in datas]
        a_in = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(b) for b in ins])
        a_is = (ctypes.c_size_t * max(1, n))(*[len(d) for d in datas])
        a_dp = a_ds = None
        if dicts is not None:
            if len(dicts) != n:
                raise ValueError("dicts: one entry per stream")
            held = {}
            for d in dicts:
                if d and id(d) not in held:
                    held[id(d)] = ctypes.create_string_buffer(bytes(d), len(d))
            a_dp = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(held[id(d)]) if d else None for d in dicts])
            a_ds = (ctypes.c_size_t * max(1, n))(*[len(d) if d else 0 for d in dicts])
        res = (BatchResult * max(1, n))()
        if self._L.BrotliAmdBatchDecodeHostPacked(self._h, n, a_in, a_is, a_dp, a_ds, max_out, flags, res) != 0:
            raise RuntimeError("BrotliAmdBatchDecodeHostPacked failed: " + last_error())
        self.n, self.out_n = 0, n
        _, offsets = self._packed_view(n)
        self.out_sizes = [offsets[i + 1] - offsets[i] for i in range(n)]
        blob = self.packed_fetch(offsets[n])
        return list(res)[:n], [blob[offsets[i]:offsets[i + 1]] for i in range(n)]

    def last_packed_launches(self):
        """decode launches of the last packed call: 1 where no stream had to grow"""
        return int(self._L.BrotliAmdBatchLastPackedLaunches(self._h))

    def last_packed_copies(self):
        """ragged-copy launches of the last packed call: 0 where its first allocation was the packed output"""
        return int(self._L.BrotliAmdBatchLastPackedCopies(self._h))

    def digest_segments(self, ptrs, lens, kind=DIGEST_CRC32, stream=None):
        """BrotliAmdBatchDigestSegments: the CRC-32 / CRC-32C of lens[i] bytes at the device address ptrs[i] (any alignment, any length) ->
        [int], one launch and a wait on `stream`"""
        n = len(ptrs)
        if len(lens) != n:
            raise ValueError("ptrs and lens: one entry per segment each")
        a_p = (ctypes.c_void_p * max(1, n))(*ptrs)
        a_l = (ctypes.c_size_t * max(1, n))(*lens)
        out = (ctypes.c_uint32 * max(1, n))()
        if self._L.BrotliAmdBatchDigestSegments(self._h, kind, n, a_p, a_l, out, stream) != 0:
            raise RuntimeError("BrotliAmdBatchDigestSegments failed: " + last_error())
        return list(out)[:n]

    def digest_outputs(self, kind=DIGEST_CRC32):
        """BrotliAmdBatchDigestOutputs: the digests of the delivered bytes of every stream of the last decode call on this object (after
        decode_device: once wait() has returned) -> [int]"""
        n = self.out_n
        out = (ctypes.c_uint32 * max(1, n))()
        if self._L.BrotliAmdBatchDigestOutputs(self._h, kind, out) != 0:
            raise RuntimeError("BrotliAmdBatchDigestOutputs failed: " + last_error())
        return list(out)[:n]

    def last_digest_ms(self):
        """milliseconds the digest kernel took in the last digest_segments / digest_outputs"""
        return float(self._L.BrotliAmdBatchLastDigestMs(self._h))

    @staticmethod
    def _column(ctype, values, n, bad=None, what=None):
        """one of a filter call's parallel arrays: n values of a ctypes type, or None where the call takes NULL for "all 0".  what: the ValueError
        text for a column that has not n entries.  bad: what stands in for a value the C type cannot hold -- a value the call refuses, or,
        where there is none, the type's largest, so that it is refused as that is"""
        if values is None:
            return None
        if what is not None and len(values) != n:
            raise ValueError(what)
        if bad is not None:
            top = (1 << 8 * ctypes.sizeof(ctype)) - 1
            values = [v if 0 <= v <= top else bad for v in values]
        return (ctype * max(1, n))(*values)

    def _filter_call(self, name, *args):
        if getattr(self._L, name)(self._h, *args) != 0:
            raise RuntimeError(name + " failed: " + last_error())

    def _width_segments(self, name, src_ptrs, dst_ptrs, lens, widths, stream, *blocks):
        """BrotliAmdBatch<name>Segments over the caller's segments (blocks: bit-unshuffle's one more column)"""
        n, col = len(src_ptrs), self._column
        if len(dst_ptrs) != n or len(lens) != n or len(widths) != n:
            raise ValueError("src_ptrs, dst_ptrs, lens and widths: one entry per segment each")
        self._filter_call(name, n, col(ctypes.c_void_p, src_ptrs, n), col(ctypes.c_void_p, dst_ptrs, n), col(ctypes.c_size_t, lens, n),
                          col(ctypes.c_uint8, widths, n, 0), *[self._block_column(b, n) for b in blocks], stream)

    def _width_outputs(self, name, dst_ptrs, widths, *blocks):
        """BrotliAmdBatch<name>Outputs over the streams of the last decode call"""
        n, col = self.out_n, self._column
        if len(dst_ptrs) != n or len(widths) != n:
            raise ValueError("dst_ptrs and widths: one entry per stream of the last decode call each")
        self._filter_call(name, col(ctypes.c_void_p, [p or None for p in dst_ptrs], n), col(ctypes.c_uint8, widths, n, 0),
                          *[self._block_column(b, n) for b in blocks])

    def _counted_segments(self, name, Result, src_ptrs, src_lens, dst_ptrs, caps, columns, stream, more=()):
        """BrotliAmdBatch<name>Segments of a filter with a capacity and a result per segment.  columns: its byte columns in the call's order, each
        (values, its name, what stands in for a value no byte holds); more: the arrays it has behind them (undict's dictionaries), each
        (C type, values or None, its name).  -> [a result's tuple per segment]"""
        n, col = len(src_ptrs), self._column
        if len(src_lens) != n or (dst_ptrs is not None and len(dst_ptrs) != n) or len(caps) != n:
            raise ValueError("src_ptrs, src_lens, dst_ptrs and caps: one entry per segment each")
        a_d = None if dst_ptrs is None else col(ctypes.c_void_p, [p or None for p in dst_ptrs], n)
        res = (Result * max(1, n))()
        self._filter_call(name, n, col(ctypes.c_void_p, src_ptrs, n), col(ctypes.c_size_t, src_lens, n), a_d, col(ctypes.c_uint64, caps, n, (1 << 64) - 1),
                          *[self._byte_column(v, n, what, bad) for v, what, bad in columns], *self._more_columns(more, n), res, stream)
        return [res[i].astuple() for i in range(n)]

    def _more_columns(self, more, n):
        """the arrays of a counted call behind its byte columns: None stays NULL, a pointer that is None or 0 is NULL, a number its type cannot hold
        becomes the type's largest -- which the call refuses or takes for what it is"""
        out = []
        for ctype, values, what in more:
            if values is not None and len(values) != n:
                raise ValueError("%s: one entry per segment or stream" % what)
            if values is not None and ctype is ctypes.c_void_p:
                values = [p or None for p in values]
            out.append(self._column(ctype, values, n, None if ctype is ctypes.c_void_p else (1 << 8 * ctypes.sizeof(ctype)) - 1))
        return out

    def _counted_outputs(self, name, Result, dst_ptrs, caps, columns, more=()):
        """BrotliAmdBatch<name>Outputs of such a filter over the streams of the last decode call -> [a result's tuple per stream]"""
        n, col = self.out_n, self._column
        if (dst_ptrs is not None and len(dst_ptrs) != n) or (caps is not None and len(caps) != n):
            raise ValueError("dst_ptrs and caps: one entry per stream of the last decode call each")
        a_d = None if dst_ptrs is None else col(ctypes.c_void_p, [p or None for p in dst_ptrs], n)
        res = (Result * max(1, n))()
        self._filter_call(name, a_d, col(ctypes.c_uint64, caps, n, (1 << 64) - 1), *[self._byte_column(v, n, what, bad) for v, what, bad in columns],
                          *self._more_columns(more, n), res)
        return [res[i].astuple() for i in range(n)]

    def _last_ms(self, stem, phase):
        """BrotliAmdBatchLast<stem>Ms, or BrotliAmdBatchLast<stem>PhaseMs of one launch"""
        if phase is None:
            return float(getattr(self._L, "BrotliAmdBatchLast%sMs" % stem)(self._h))
        return float(getattr(self._L, "BrotliAmdBatchLast%sPhaseMs" % stem)(self._h, phase))

    def unshuffle_segments(self, src_ptrs, dst_ptrs, lens, widths, stream=None):
        """BrotliAmdBatchUnshuffleSegments: lens[i] bytes of byte planes at the device address src_ptrs[i] become elements of widths[i] bytes
        (1, 2, 4, 8) at dst_ptrs[i]; any alignment, any length; out of place.  One launch and a wait on `stream`."""
        self._width_segments("BrotliAmdBatchUnshuffleSegments", src_ptrs, dst_ptrs, lens, widths, stream)

    def unshuffle_outputs(self, dst_ptrs, widths):
        """BrotliAmdBatchUnshuffleOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device:
        once wait() has returned), taken as byte planes of widths[i], become elements at the device address dst_ptrs[i] (None or 0: the stream
        is skipped).  One launch on that call's stream, and a wait."""
        self._width_outputs("BrotliAmdBatchUnshuffleOutputs", dst_ptrs, widths)

    def last_unshuffle_ms(self):
        """milliseconds the unshuffle kernel took in the last unshuffle_segments / unshuffle_outputs"""
        return float(self._L.BrotliAmdBatchLastUnshuffleMs(self._h))

    def undelta_segments(self, src_ptrs, dst_ptrs, lens, widths, stream=None):
        """BrotliAmdBatchUndeltaSegments: lens[i] bytes of deltas at the device address src_ptrs[i] become the running sums of their elements of
        widths[i] bytes (1, 2, 4, 8; little-endian, wrapping) at dst_ptrs[i]; any alignment, any length; out of place, or in place
        (dst_ptrs[i] == src_ptrs[i]) at a multiple of the width.  Three launches and a wait on `stream`."""
        self._width_segments("BrotliAmdBatchUndeltaSegments", src_ptrs, dst_ptrs, lens, widths, stream)

    def undelta_outputs(self, dst_ptrs, widths):
        """BrotliAmdBatchUndeltaOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device: once
        wait() has returned), taken as deltas of widths[i], become values at the device address dst_ptrs[i] (None or 0: the stream is skipped).
        Three launches on that call's stream, and a wait."""
        self._width_outputs("BrotliAmdBatchUndeltaOutputs", dst_ptrs, widths)

    def last_undelta_ms(self, phase=None):
        """milliseconds the undelta kernels took in the last undelta_segments / undelta_outputs: all launches together, or phase 1, 2 or 3"""
        return self._last_ms("Undelta", phase)

    def _block_column(self, blocks, n):
        """block sizes as the C calls take them: None (all 0), or n of them"""
        return self._column(ctypes.c_uint32, blocks, n, 1, "blocks: one entry per segment or stream, or None")   # (1: no multiple of 8, so it is refused)

    def bitunshuffle_segments(self, src_ptrs, dst_ptrs, lens, widths, blocks=None, stream=None):
        """BrotliAmdBatchBitUnshuffleSegments: lens[i] bytes of bit planes at the device address src_ptrs[i] become elements of widths[i] bytes
        (1, 2, 4, 8), in blocks of blocks[i] elements (0: one block; None: all 0), at dst_ptrs[i]; any alignment, any length; out of place.
        One launch and a wait on `stream`."""
        self._width_segments("BrotliAmdBatchBitUnshuffleSegments", src_ptrs, dst_ptrs, lens, widths, stream, blocks)

    def bitunshuffle_outputs(self, dst_ptrs, widths, blocks=None):
        """BrotliAmdBatchBitUnshuffleOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device:
        once wait() has returned), taken as bit planes of widths[i] in blocks of blocks[i] elements, become elements at the device address
        dst_ptrs[i] (None or 0: the stream is skipped).  One launch on that call's stream, and a wait."""
        self._width_outputs("BrotliAmdBatchBitUnshuffleOutputs", dst_ptrs, widths, blocks)

    def _byte_column(self, values, n, what, bad=255):
        """small parameters as the C calls take them: n bytes; what no byte holds becomes `bad`, which the call refuses"""
        return self._column(ctypes.c_uint8, values, n, bad, what + ": one entry per segment or stream")

    def bitunpack_segments(self, src_ptrs, src_lens, dst_ptrs, counts, bits, widths, flags=None, stream=None):
        """BrotliAmdBatchBitUnpackSegments: the first counts[i] fields of bits[i] bits (1 .. 8 widths[i]) of the src_lens[i] bytes at the device
        address src_ptrs[i] become counts[i] elements of widths[i] bytes (1, 2, 4, 8) at dst_ptrs[i], by flags[i] (BITUNPACK_MSB_FIRST,
        BITUNPACK_SIGNED; None: all 0); any alignment, any count; out of place.  One launch and a wait on `stream`."""
        n, col = len(src_ptrs), self._column
        if len(src_lens) != n or len(dst_ptrs) != n or len(counts) != n:
            raise ValueError("src_ptrs, src_lens, dst_ptrs and counts: one entry per segment each")
        a_s, a_l, a_d = col(ctypes.c_void_p, src_ptrs, n), col(ctypes.c_size_t, src_lens, n), col(ctypes.c_void_p, dst_ptrs, n)
        a_c, a_f = col(ctypes.c_uint64, counts, n, (1 << 64) - 1), self._byte_column(flags, n, "flags")
        self._filter_call("BrotliAmdBatchBitUnpackSegments", n, a_s, a_l, a_d, a_c, self._byte_column(bits, n, "bits"), self._byte_column(widths, n, "widths", 0),
                          a_f, stream)

    def bitunpack_outputs(self, dst_ptrs, bits, widths, counts=None, flags=None):
        """BrotliAmdBatchBitUnpackOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device: once
        wait() has returned), taken as fields of bits[i] bits, become counts[i] elements of widths[i] bytes at the device address dst_ptrs[i]
        (None or 0: the stream is skipped); counts=None: as many whole fields as were delivered.  One launch on that call's stream, and a wait."""
        n, col = self.out_n, self._column
        if len(dst_ptrs) != n or (counts is not None and len(counts) != n):
            raise ValueError("dst_ptrs and counts: one entry per stream of the last decode call each")
        a_d, a_c = col(ctypes.c_void_p, [p or None for p in dst_ptrs], n), col(ctypes.c_uint64, counts, n, (1 << 64) - 1)
        a_f = self._byte_column(flags, n, "flags")
        self._filter_call("BrotliAmdBatchBitUnpackOutputs", a_d, a_c, self._byte_column(bits, n, "bits"), self._byte_column(widths, n, "widths", 0), a_f)

    def unvarint_segments(self, src_ptrs, src_lens, dst_ptrs, caps, widths, flags=None, stream=None):
        """BrotliAmdBatchUnvarintSegments: the LEB128 varints in the src_lens[i] bytes at the device address src_ptrs[i] become elements of
        widths[i] bytes (1, 2, 4, 8) at dst_ptrs[i], the first caps[i] of them, by flags[i] (UNVARINT_ZIGZAG; None: all 0); any alignment, any
        length; out of place; caps[i] == 0 needs no destination (dst_ptrs[i] may be None; dst_ptrs=None: none has one).  Three launches and a
        wait on `stream`.  -> [(count, consumed, overlong)]: what each segment held, whatever its capacity was"""
        return self._counted_segments("BrotliAmdBatchUnvarintSegments", UnvarintResult, src_ptrs, src_lens, dst_ptrs, caps, [(widths, "widths", 0), (flags, "flags", 255)], stream)

    def unvarint_outputs(self, dst_ptrs, caps, widths, flags=None):
        """BrotliAmdBatchUnvarintOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device: once
        wait() has returned), taken as LEB128 varints, become elements of widths[i] bytes at the device address dst_ptrs[i], the first caps[i]
        of them (None or 0: the stream is skipped, and its result is zeros).  dst_ptrs=None or caps=None: every stream is counted and nothing is
        written.  Three launches on that call's stream, and a wait.  -> [(count, consumed, overlong)], one per stream"""
        return self._counted_outputs("BrotliAmdBatchUnvarintOutputs", UnvarintResult, dst_ptrs, caps, [(widths, "widths", 0), (flags, "flags", 255)])

    def count_varints_outputs(self):
        """unvarint_outputs without destinations: how many varints every stream of the last decode call holds, the bytes they take and the
        overlong ones among them -> [(count, consumed, overlong)]; the way to size the destinations of the call that writes"""
        return self.unvarint_outputs(None, None, [1] * self.out_n)

    def last_unvarint_ms(self, phase=None):
        """milliseconds the unvarint kernels took in the last unvarint_segments / unvarint_outputs: all launches together, or phase 1, 2 or 3"""
        return self._last_ms("Unvarint", phase)

    def unrle_segments(self, src_ptrs, src_lens, dst_ptrs, caps, bits, widths, flags=None, stream=None):
        """BrotliAmdBatchUnrleSegments: the RLE / bit-packed hybrid runs in the src_lens[i] bytes at the device address src_ptrs[i], of fields of
        bits[i] bits (0 .. 32), become elements of widths[i] bytes (1, 2, 4, 8) at dst_ptrs[i], the first caps[i] of them, by flags[i]
        (UNRLE_WIDTH_BYTE; None: all 0); any alignment, any length; out of place; caps[i] == 0 needs no destination (dst_ptrs[i] may be None;
        dst_ptrs=None: none has one).  Two launches and a wait on `stream`.  -> [(count, consumed, runs, status, bits)]: what each segment
        held, whatever its capacity was"""
        return self._counted_segments("BrotliAmdBatchUnrleSegments", UnrleResult, src_ptrs, src_lens, dst_ptrs, caps, [(bits, "bits", 255), (widths, "widths", 0), (flags, "flags", 255)], stream)

    def unrle_outputs(self, dst_ptrs, caps, bits, widths, flags=None):
        """BrotliAmdBatchUnrleOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device: once
        wait() has returned), taken as RLE / bit-packed hybrid runs of fields of bits[i] bits, become elements of widths[i] bytes at the device
        address dst_ptrs[i], the first caps[i] of them (None or 0: the stream is skipped, and its result is zeros).  dst_ptrs=None or caps=None:
        every stream is counted and nothing is written.  Two launches on that call's stream, and a wait.
        -> [(count, consumed, runs, status, bits)], one per stream"""
        return self._counted_outputs("BrotliAmdBatchUnrleOutputs", UnrleResult, dst_ptrs, caps, [(bits, "bits", 255), (widths, "widths", 0), (flags, "flags", 255)])

    def count_rle_outputs(self, bits=None):
        """unrle_outputs without destinations: how many values the runs of every stream of the last decode call hold -> [(count, consumed, runs,
        status, bits)]; bits: every stream's field width, or None: every stream's first byte says it (UNRLE_WIDTH_BYTE).  The way to size the
        destinations of the call that writes"""
        n = self.out_n
        if bits is None:
            return self.unrle_outputs(None, None, [0] * n, [4] * n, [UNRLE_WIDTH_BYTE] * n)
        return self.unrle_outputs(None, None, bits, [4] * n)

    def last_unrle_ms(self, phase=None):
        """milliseconds the unrle kernels took in the last unrle_segments / unrle_outputs: both launches together, or phase 1 (the walk) or 2
        (the expansion)"""
        return self._last_ms("Unrle", phase)

    def undict_segments(self, src_ptrs, src_lens, dst_ptrs, caps, bits, widths, flags, dict_ptrs, dict_entries, stream=None):
        """BrotliAmdBatchUndictSegments: the RLE / bit-packed hybrid runs in the src_lens[i] bytes at the device address src_ptrs[i], of fields of
        bits[i] bits (0 .. 32, whatever the width), are INDICES into the dict_entries[i] entries of widths[i] bytes at the device address
        dict_ptrs[i]; the first caps[i] of the entries they name go to dst_ptrs[i], by flags[i] (UNDICT_WIDTH_BYTE; None: all 0); any alignment,
        any length; out of place.  An index at or above dict_entries[i] gives 0 and is counted.  caps[i] == 0 only counts (dst_ptrs, dict_ptrs
        and dict_entries may then be None).  Two launches and a wait on `stream`.  -> [(count, consumed, runs, status, bits, bad, first_bad)]"""
        return self._counted_segments("BrotliAmdBatchUndictSegments", UndictResult, src_ptrs, src_lens, dst_ptrs, caps,
                                      [(bits, "bits", 255), (widths, "widths", 0), (flags, "flags", 255)], stream,
                                      [(ctypes.c_void_p, dict_ptrs, "dict_ptrs"), (ctypes.c_uint64, dict_entries, "dict_entries")])

    def undict_outputs(self, dst_ptrs, caps, bits, widths, flags=None, dict_streams=None, dict_ptrs=None, dict_entries=None):
        """BrotliAmdBatchUndictOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device: once
        wait() has returned), taken as dictionary-index runs, become the values they name at dst_ptrs[i] (None or 0: the stream is skipped).
        dict_streams[i]: the stream of the same decode call whose delivered bytes are stream i's dictionary, or UNDICT_NO_STREAM (and
        dict_streams None) for the dictionary at the device address dict_ptrs[i] with dict_entries[i] entries.  dst_ptrs None or caps None:
        every stream is counted and nothing is written.  -> [(count, consumed, runs, status, bits, bad, first_bad)]"""
        return self._counted_outputs("BrotliAmdBatchUndictOutputs", UndictResult, dst_ptrs, caps, [(bits, "bits", 255), (widths, "widths", 0), (flags, "flags", 255)],
                                     [(ctypes.c_uint32, dict_streams, "dict_streams"), (ctypes.c_void_p, dict_ptrs, "dict_ptrs"),
                                      (ctypes.c_uint64, dict_entries, "dict_entries")])

    def last_undict_ms(self, phase=None):
        """milliseconds the undict kernels took in the last undict_segments / undict_outputs: both launches together, or phase 1 (the walk) or 2
        (the expansion with the lookup)"""
        return self._last_ms("Undict", phase)

    def undict_bytes_segments(self, src_ptrs, src_lens, offsets_ptrs, data_ptrs, data_caps, caps, bits, flags, offset_bases, dict_ptrs, dict_lens, dict_entries=None,
                              stream=None):
        """BrotliAmdBatchUndictBytesSegments: the RLE / bit-packed hybrid runs in the src_lens[i] bytes at the device address src_ptrs[i], of fields
        of bits[i] bits (0 .. 32), are INDICES into the PLAIN byte arrays -- a 4-byte length, then the bytes -- of the dict_lens[i] bytes at
        dict_ptrs[i], at most dict_entries[i] of them (None: as many as the bytes hold).  The first caps[i] elements become an Arrow string
        column: offsets on top of offset_bases[i] (None: 0) at offsets_ptrs[i] -- int32, or int64 with UNDICT_BYTES_OFFSETS64; with
        UNDICT_BYTES_ENDS_ONLY without offsets[0] --, and the bytes at data_ptrs[i], at most data_caps[i] of them.  A destination that is None
        is not written: with neither the call MEASURES, and `bytes` of the result sizes the data.  An index at or above the dictionary's
        entries gives an empty element and is counted.  caps[i] == 0 only counts.  Five launches and a wait on `stream`.
        -> [(count, consumed, runs, status, bits, bad, first_bad, bytes, dict_entries, dict_consumed, dict_status)]"""
        n, col = len(src_ptrs), self._column
        if len(src_lens) != n or len(caps) != n:
            raise ValueError("src_ptrs, src_lens and caps: one entry per segment each")
        res = (UndictBytesResult * max(1, n))()
        big = (1 << 64) - 1
        self._filter_call("BrotliAmdBatchUndictBytesSegments", n, col(ctypes.c_void_p, src_ptrs, n), col(ctypes.c_size_t, src_lens, n),
                          self._ptr_column(offsets_ptrs, n, "offsets_ptrs"), self._ptr_column(data_ptrs, n, "data_ptrs"),
                          col(ctypes.c_uint64, data_caps, n, big, "data_caps: one entry per segment"), col(ctypes.c_uint64, caps, n, big),
                          self._byte_column(bits, n, "bits"), self._byte_column(flags, n, "flags"), col(ctypes.c_uint64, offset_bases, n, None, "offset_bases: one entry per segment"),
                          self._ptr_column(dict_ptrs, n, "dict_ptrs"), col(ctypes.c_uint64, dict_lens, n, big, "dict_lens: one entry per segment"),
                          col(ctypes.c_uint64, dict_entries, n, big, "dict_entries: one entry per segment"), res, stream)
        return [res[i].astuple() for i in range(n)]

    def undict_bytes_outputs(self, offsets_ptrs, data_ptrs, data_caps, caps, bits, flags=None, offset_bases=None, dict_streams=None, dict_ptrs=None, dict_lens=None,
                             dict_entries=None):
        """BrotliAmdBatchUndictBytesOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device:
        once wait() has returned), taken as dictionary-index runs, become offsets at offsets_ptrs[i] and bytes at data_ptrs[i] as in
        undict_bytes_segments.  A stream with UNDICT_BYTES_SKIP in flags[i] is skipped -- the dictionary pages of the batch -- and its result is
        zeros.  dict_streams[i]: the stream of the same decode call whose delivered bytes are stream i's dictionary, or UNDICT_NO_STREAM (and
        dict_streams None) for the dict_lens[i] bytes at the device address dict_ptrs[i]; dict_entries[i] bounds either kind (None: all the
        bytes hold).  caps None: every stream is counted and nothing else.
        -> [(count, consumed, runs, status, bits, bad, first_bad, bytes, dict_entries, dict_consumed, dict_status)], one per stream"""
        n, col = self.out_n, self._column
        if caps is not None and len(caps) != n:
            raise ValueError("caps: one entry per stream of the last decode call")
        res = (UndictBytesResult * max(1, n))()
        big = (1 << 64) - 1
        self._filter_call("BrotliAmdBatchUndictBytesOutputs", self._ptr_column(offsets_ptrs, n, "offsets_ptrs"), self._ptr_column(data_ptrs, n, "data_ptrs"),
                          col(ctypes.c_uint64, data_caps, n, big, "data_caps: one entry per stream"), col(ctypes.c_uint64, caps, n, big), self._byte_column(bits, n, "bits"),
                          self._byte_column(flags, n, "flags"), col(ctypes.c_uint64, offset_bases, n, None, "offset_bases: one entry per stream"),
                          col(ctypes.c_uint32, dict_streams, n, None, "dict_streams: one entry per stream"), self._ptr_column(dict_ptrs, n, "dict_ptrs"),
                          col(ctypes.c_uint64, dict_lens, n, big, "dict_lens: one entry per stream"),
                          col(ctypes.c_uint64, dict_entries, n, big, "dict_entries: one entry per stream"), res)
        return [res[i].astuple() for i in range(n)]

    def measure_dict_bytes_outputs(self, caps, bits, dict_streams=None, dict_ptrs=None, dict_lens=None, dict_entries=None, flags=None):
        """undict_bytes_outputs without destinations: what the first caps[i] elements of every stream of the last decode call take -- `bytes`
        of the result -- and what its dictionary holds; caps[i] None skips the stream (UNDICT_BYTES_SKIP).  The way to size the data of the
        call that writes: the rows are in the page header, the bytes are not."""
        n = self.out_n
        if len(caps) != n:
            raise ValueError("caps: one entry per stream of the last decode call")
        flags = [(flags[i] if flags is not None else 0) | (UNDICT_BYTES_SKIP if caps[i] is None else 0) for i in range(n)]
        return self.undict_bytes_outputs(None, None, None, [c or 0 for c in caps], bits, flags, None, dict_streams, dict_ptrs, dict_lens, dict_entries)

    def last_undict_bytes_ms(self, phase=None):
        """milliseconds the undict-bytes kernels took in the last undict_bytes_segments / undict_bytes_outputs: all launches together, or phase 1
        (the dictionary walk), 2 (the RLE walk), 3 (the lengths), 4 (the carries) or 5 (the expansion)"""
        return self._last_ms("UndictBytes", phase)

    def undlba_segments(self, src_ptrs, src_lens, offsets_ptrs, data_ptrs, data_caps, caps, flags=None, offset_bases=None, stream=None):
        """BrotliAmdBatchUndlbaSegments: the src_lens[i] bytes at the device address src_ptrs[i] are a DELTA_LENGTH_BYTE_ARRAY body -- a
        DELTA_BINARY_PACKED stream of lengths and, directly behind it, the values' bytes.  The first caps[i] elements become an Arrow string
        column: offsets on top of offset_bases[i] (None: 0) at offsets_ptrs[i] -- int32, or int64 with UNDLBA_OFFSETS64; with UNDLBA_ENDS_ONLY
        without offsets[0] --, and the bytes at data_ptrs[i], at most data_caps[i] of them.  A destination that is None is not written: with
        neither the call MEASURES.  A negative length gives an empty element and is counted.  caps[i] == 0 only counts: `data_avail` of the
        result sizes the data.  Seven launches and a wait on `stream`.
        -> [(count, consumed, declared, blocks, status, block_values, miniblocks, data_status, bad, first_bad, bytes, data_avail)]"""
        n, col = len(src_ptrs), self._column
        if len(src_lens) != n or len(caps) != n:
            raise ValueError("src_ptrs, src_lens and caps: one entry per segment each")
        res = (UndlbaResult * max(1, n))()
        big = (1 << 64) - 1
        self._filter_call("BrotliAmdBatchUndlbaSegments", n, col(ctypes.c_void_p, src_ptrs, n), col(ctypes.c_size_t, src_lens, n),
                          self._ptr_column(offsets_ptrs, n, "offsets_ptrs"), self._ptr_column(data_ptrs, n, "data_ptrs"),
                          col(ctypes.c_uint64, data_caps, n, big, "data_caps: one entry per segment"), col(ctypes.c_uint64, caps, n, big),
                          self._byte_column(flags, n, "flags"), col(ctypes.c_uint64, offset_bases, n, None, "offset_bases: one entry per segment"), res, stream)
        return [res[i].astuple() for i in range(n)]

    def undlba_outputs(self, offsets_ptrs, data_ptrs, data_caps, caps, flags=None, offset_bases=None):
        """BrotliAmdBatchUndlbaOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device: once
        wait() has returned), taken as DELTA_LENGTH_BYTE_ARRAY bodies, become offsets at offsets_ptrs[i] and bytes at data_ptrs[i] as in
        undlba_segments.  A stream with UNDLBA_SKIP in flags[i] is skipped, and its result is zeros.  caps None: every stream is counted and
        nothing else.
        -> [(count, consumed, declared, blocks, status, block_values, miniblocks, data_status, bad, first_bad, bytes, data_avail)], one per stream"""
        n, col = self.out_n, self._column
        if caps is not None and len(caps) != n:
            raise ValueError("caps: one entry per stream of the last decode call")
        res = (UndlbaResult * max(1, n))()
        big = (1 << 64) - 1
        self._filter_call("BrotliAmdBatchUndlbaOutputs", self._ptr_column(offsets_ptrs, n, "offsets_ptrs"), self._ptr_column(data_ptrs, n, "data_ptrs"),
                          col(ctypes.c_uint64, data_caps, n, big, "data_caps: one entry per stream"), col(ctypes.c_uint64, caps, n, big),
                          self._byte_column(flags, n, "flags"), col(ctypes.c_uint64, offset_bases, n, None, "offset_bases: one entry per stream"), res)
        return [res[i].astuple() for i in range(n)]

    def count_dlba_outputs(self, flags=None):
        """undlba_outputs without capacities: how many lengths the DELTA_LENGTH_BYTE_ARRAY body of every stream of the last decode call holds,
        where its bytes begin (`consumed`) and how many there are (`data_avail`); a stream with UNDLBA_SKIP in flags[i] is skipped.  The way to
        size the destinations of the call that writes: a well-formed page has bytes == data_avail"""
        return self.undlba_outputs(None, None, None, None, flags)

    def measure_dlba_outputs(self, caps, flags=None):
        """undlba_outputs without destinations: what the first caps[i] elements of every stream of the last decode call take -- `bytes` of the
        result -- and which lengths are negative; caps[i] None skips the stream (UNDLBA_SKIP)"""
        n = self.out_n
        if len(caps) != n:
            raise ValueError("caps: one entry per stream of the last decode call")
        flags = [(flags[i] if flags is not None else 0) | (UNDLBA_SKIP if caps[i] is None else 0) for i in range(n)]
        return self.undlba_outputs(None, None, None, [c or 0 for c in caps], flags)

    def last_undlba_ms(self, phase=None):
        """milliseconds the undlba kernels took in the last undlba_segments / undlba_outputs: all launches together, or phase 1 (the walk), 2
        (the delta sums), 3 (their carries), 4 (the lengths), 5 (their carries), 6 (the offsets) or 7 (the data)"""
        return self._last_ms("Undlba", phase)

    def undba_segments(self, src_ptrs, src_lens, offsets_ptrs, data_ptrs, data_caps, caps, flags=None, offset_bases=None, stream=None):
        """BrotliAmdBatchUndbaSegments: the src_lens[i] bytes at the device address src_ptrs[i] are a DELTA_BYTE_ARRAY body -- a
        DELTA_BINARY_PACKED stream of prefix lengths, one of suffix lengths and the suffix bytes, directly behind one another.  The first
        caps[i] elements become an Arrow string column with undlba_segments' arguments and flags (UNDBA_*).  The first element that breaks a
        rule, and every one behind it, is empty.  caps[i] == 0 only counts; with neither destination the call MEASURES: `bytes` of the
        result sizes the data.  Nine launches and a wait on `stream`.
        -> [UndbaResult's twenty fields in their order]"""
        n, col = len(src_ptrs), self._column
        if len(src_lens) != n or len(caps) != n:
            raise ValueError("src_ptrs, src_lens and caps: one entry per segment each")
        res = (UndbaResult * max(1, n))()
        big = (1 << 64) - 1
        self._filter_call("BrotliAmdBatchUndbaSegments", n, col(ctypes.c_void_p, src_ptrs, n), col(ctypes.c_size_t, src_lens, n),
                          self._ptr_column(offsets_ptrs, n, "offsets_ptrs"), self._ptr_column(data_ptrs, n, "data_ptrs"),
                          col(ctypes.c_uint64, data_caps, n, big, "data_caps: one entry per segment"), col(ctypes.c_uint64, caps, n, big),
                          self._byte_column(flags, n, "flags"), col(ctypes.c_uint64, offset_bases, n, None, "offset_bases: one entry per segment"), res, stream)
        return [res[i].astuple() for i in range(n)]

    def undba_outputs(self, offsets_ptrs, data_ptrs, data_caps, caps, flags=None, offset_bases=None):
        """BrotliAmdBatchUndbaOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device: once
        wait() has returned), taken as DELTA_BYTE_ARRAY bodies, become offsets at offsets_ptrs[i] and bytes at data_ptrs[i] as in
        undba_segments.  A stream with UNDBA_SKIP in flags[i] is skipped, and its result is zeros.  caps None: every stream is counted and
        nothing else.  -> [UndbaResult's twenty fields in their order], one per stream"""
        n, col = self.out_n, self._column
        if caps is not None and len(caps) != n:
            raise ValueError("caps: one entry per stream of the last decode call")
        res = (UndbaResult * max(1, n))()
        big = (1 << 64) - 1
        self._filter_call("BrotliAmdBatchUndbaOutputs", self._ptr_column(offsets_ptrs, n, "offsets_ptrs"), self._ptr_column(data_ptrs, n, "data_ptrs"),
                          col(ctypes.c_uint64, data_caps, n, big, "data_caps: one entry per stream"), col(ctypes.c_uint64, caps, n, big),
                          self._byte_column(flags, n, "flags"), col(ctypes.c_uint64, offset_bases, n, None, "offset_bases: one entry per stream"), res)
        return [res[i].astuple() for i in range(n)]

    def count_dba_outputs(self, flags=None):
        """undba_outputs without capacities: the two walks of every stream of the last decode call alone -- how many prefix and suffix lengths
        its DELTA_BYTE_ARRAY body holds and how many suffix bytes are there (`data_avail`); a stream with UNDBA_SKIP in flags[i] is skipped"""
        return self.undba_outputs(None, None, None, None, flags)

    def measure_dba_outputs(self, caps, flags=None):
        """undba_outputs without destinations: what the first caps[i] elements of every stream of the last decode call take -- `bytes` of the
        result, which sizes the data --, and the first element that breaks a rule; caps[i] None skips the stream (UNDBA_SKIP)"""
        n = self.out_n
        if len(caps) != n:
            raise ValueError("caps: one entry per stream of the last decode call")
        flags = [(flags[i] if flags is not None else 0) | (UNDBA_SKIP if caps[i] is None else 0) for i in range(n)]
        return self.undba_outputs(None, None, None, [c or 0 for c in caps], flags)

    def last_undba_ms(self, phase=None):
        """milliseconds the undba kernels took in the last undba_segments / undba_outputs: all launches together, or phase 1 (the walks), 2
        (the delta sums), 3 (their carries), 4 (the lengths), 5 (their carries), 6 (the offsets), 7 (phase A), 8 (phase B) or 9 (phase C)"""
        return self._last_ms("Undba", phase)

    def _ptr_column(self, ptrs, n, what):
        """device addresses as the C calls take them: None stays NULL, and so does an entry that is None or 0"""
        return self._column(ctypes.c_void_p, None if ptrs is None else [p or None for p in ptrs], n, None, what + ": one entry per segment or stream")

    def unnull_segments(self, level_ptrs, level_lens, value_ptrs, value_counts, dst_ptrs, valid_ptrs, caps, bits, levels, widths, flags=None, stream=None):
        """BrotliAmdBatchUnnullSegments: the level_lens[i] bytes at the device address level_ptrs[i] are DEFINITION LEVELS, unrle runs of fields of
        bits[i] bits (0 .. 32); slot j of the first caps[i] is present where its level equals levels[i], and the present slots get the
        value_counts[i] dense values of widths[i] bytes at value_ptrs[i] in order, every other slot 0, at dst_ptrs[i]; bit j & 7 of byte j >> 3
        at valid_ptrs[i] (None: no bitmap; valid_ptrs=None: none has one) says whether slot j is present.  flags[i]: UNNULL_LENGTH_PREFIX,
        UNNULL_VALUES_FOLLOW (None: all 0).  Any alignment, any length; out of place.  caps[i] == 0 only counts (dst_ptrs, value_ptrs and
        value_counts may then be None).  Four launches and a wait on `stream`.
        -> [(count, consumed, runs, status, bits, present, missing, values)]"""
        n, col = len(level_ptrs), self._column
        if len(level_lens) != n or len(caps) != n or len(levels) != n:
            raise ValueError("level_ptrs, level_lens, caps and levels: one entry per segment each")
        res = (UnnullResult * max(1, n))()
        self._filter_call("BrotliAmdBatchUnnullSegments", n, col(ctypes.c_void_p, level_ptrs, n), col(ctypes.c_size_t, level_lens, n),
                          self._ptr_column(value_ptrs, n, "value_ptrs"), col(ctypes.c_uint64, value_counts, n, (1 << 64) - 1, "value_counts: one entry per segment"),
                          self._ptr_column(dst_ptrs, n, "dst_ptrs"), self._ptr_column(valid_ptrs, n, "valid_ptrs"), col(ctypes.c_uint64, caps, n, (1 << 64) - 1),
                          self._byte_column(bits, n, "bits"), col(ctypes.c_uint32, levels, n, (1 << 32) - 1), self._byte_column(widths, n, "widths", 0),
                          self._byte_column(flags, n, "flags"), res, stream)
        return [res[i].astuple() for i in range(n)]

    def unnull_outputs(self, dst_ptrs, valid_ptrs, caps, bits, levels, widths, level_ptrs=None, level_lens=None):
        """BrotliAmdBatchUnnullOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device: once
        wait() has returned), spread over nulls into the slots at dst_ptrs[i] (None or 0: the stream is skipped) and the bitmap at
        valid_ptrs[i] (None: no bitmap).  Without level_ptrs, or where level_ptrs[i] is None, stream i is a V1 BODY: a 4-byte length, the
        levels, the values.  Where level_ptrs[i] is set -- the V2 case -- the levels are the level_lens[i] uncompressed bytes at that device
        address, and the stream's delivered bytes are the values.  dst_ptrs None or caps None: every stream is counted and nothing is written.
        -> [(count, consumed, runs, status, bits, present, missing, values)], one per stream"""
        n, col = self.out_n, self._column
        if len(levels) != n or (caps is not None and len(caps) != n):
            raise ValueError("caps and levels: one entry per stream of the last decode call each")
        res = (UnnullResult * max(1, n))()
        self._filter_call("BrotliAmdBatchUnnullOutputs", self._ptr_column(dst_ptrs, n, "dst_ptrs"), self._ptr_column(valid_ptrs, n, "valid_ptrs"),
                          col(ctypes.c_uint64, caps, n, (1 << 64) - 1), self._byte_column(bits, n, "bits"), col(ctypes.c_uint32, levels, n, (1 << 32) - 1),
                          self._byte_column(widths, n, "widths", 0), self._ptr_column(level_ptrs, n, "level_ptrs"),
                          col(ctypes.c_size_t, level_lens, n, None, "level_lens: one entry per stream"), res)
        return [res[i].astuple() for i in range(n)]

    def count_levels_outputs(self, bits, level_ptrs=None, level_lens=None):
        """unnull_outputs without destinations: how many levels every stream of the last decode call holds -- a v1 body behind its 4-byte
        length, or the levels at level_ptrs[i] -- and where they end -> [(count, consumed, runs, status, bits, 0, 0, values)].  The way to size the
        destinations of the call that writes; `consumed` of a v1 body is where its values -- or its dictionary-index body -- begin"""
        n = self.out_n
        return self.unnull_outputs(None, None, None, bits, [0] * n, [1] * n, level_ptrs, level_lens)

    def last_unnull_ms(self, phase=None):
        """milliseconds the unnull kernels took in the last unnull_segments / unnull_outputs: all launches together, or phase 1 (the walk), 2
        (the counts), 3 (the carries) or 4 (the expansion)"""
        return self._last_ms("Unnull", phase)

    def undbp_segments(self, src_ptrs, src_lens, dst_ptrs, caps, widths, flags=None, stream=None):
        """BrotliAmdBatchUndbpSegments: the DELTA_BINARY_PACKED stream in the src_lens[i] bytes at the device address src_ptrs[i] becomes elements
        of widths[i] bytes (1, 2, 4, 8) at dst_ptrs[i], the first caps[i] of them; flags: None or all 0; any alignment, any length; out of place;
        caps[i] == 0 needs no destination (dst_ptrs[i] may be None; dst_ptrs=None: none has one).  Four launches and a wait on `stream`.
        -> [(count, consumed, declared, blocks, status, block_values, miniblocks)]: what each segment held, whatever its capacity was"""
        return self._counted_segments("BrotliAmdBatchUndbpSegments", UndbpResult, src_ptrs, src_lens, dst_ptrs, caps, [(widths, "widths", 0), (flags, "flags", 255)], stream)

    def undbp_outputs(self, dst_ptrs, caps, widths, flags=None):
        """BrotliAmdBatchUndbpOutputs: the delivered bytes of every stream of the last decode call on this object (after decode_device: once
        wait() has returned), taken as DELTA_BINARY_PACKED streams, become elements of widths[i] bytes at the device address dst_ptrs[i], the
        first caps[i] of them (None or 0: the stream is skipped, and its result is zeros).  dst_ptrs=None or caps=None: every stream is counted
        and nothing is written.  Four launches on that call's stream, and a wait.
        -> [(count, consumed, declared, blocks, status, block_values, miniblocks)], one per stream"""
        return self._counted_outputs("BrotliAmdBatchUndbpOutputs", UndbpResult, dst_ptrs, caps, [(widths, "widths", 0), (flags, "flags", 255)])

    def count_dbp_outputs(self):
        """undbp_outputs without destinations: how many values the DELTA_BINARY_PACKED stream of every stream of the last decode call holds, and
        where it ends -> [(count, consumed, declared, blocks, status, block_values, miniblocks)].  The way to size the destinations of the call
        that writes"""
        return self.undbp_outputs(None, None, [8] * self.out_n)

    def last_undbp_ms(self, phase=None):
        """milliseconds the undbp kernels took in the last undbp_segments / undbp_outputs: all launches together, or phase 1 (the walk), 2 (the
        items' sums), 3 (the carries) or 4 (the expansion)"""
        return self._last_ms("Undbp", phase)

    def last_bitunpack_ms(self):
        """milliseconds the bit-unpack kernel took in the last bitunpack_segments / bitunpack_outputs"""
        return float(self._L.BrotliAmdBatchLastBitUnpackMs(self._h))

    def last_bitunshuffle_ms(self):
        """milliseconds the bit-unshuffle kernel took in the last bitunshuffle_segments / bitunshuffle_outputs"""
        return float(self._L.BrotliAmdBatchLastBitUnshuffleMs(self._h))

    def decode_host_raw(self, in_ptrs, in_sizes, out_ptrs, out_caps, flags=FLAG_LARGE_WINDOW):
        """BrotliAmdBatchDecodeHost on buffers the caller owns (host addresses as integers): nothing is copied on the Python side"""
        n = len(in_ptrs)
        a_in = (ctypes.c_void_p * n)(*in_ptrs)
        a_is = (ctypes.c_size_t * n)(*in_sizes)
        a_out = (ctypes.c_void_p * n)(*out_ptrs)
        a_oc = (ctypes.c_size_t * n)(*out_caps)
        res = (BatchResult * max(1, n))()
        if self._L.BrotliAmdBatchDecodeHost(self._h, n, a_in, a_is, a_out, a_oc, flags, res) != 0:
            raise RuntimeError("BrotliAmdBatchDecodeHost failed: " + last_error())
        self.n = self.out_n = n
        self.out_sizes = [min(res[i].decoded_size, out_caps[i]) for i in range(n)]
        return list(res)[:n]


# ------------------------------------------------------------------ streaming state (src/ffi/mod.rs:390-463)
class DecoderState:
    """BrotliDecoderState through the C ABI."""

    def __init__(self, large_window=False, dictionary=None):
        self._L = load_library()
        self._h = self._L.BrotliDecoderCreateInstance(None, None, None)
        if not self._h:
            raise MemoryError("BrotliDecoderCreateInstance")
        if large_window:
            self._L.BrotliDecoderSetParameter(self._h, PARAM_LARGE_WINDOW, 1)
        if dictionary and not self.attach_dictionary(dictionary):  # BrotliState::new_with_custom_dictionary (state.rs:400-411)
            raise RuntimeError("BrotliAmdDecoderAttachDictionary refused the dictionary")

    def attach_dictionary(self, data):
        """BrotliAmdDecoderAttachDictionary (batch.h): one custom dictionary, before anything is decoded; the bytes are copied."""
        data = bytes(data)
        buf = ctypes.create_string_buffer(data, max(1, len(data)))
        return bool(self._L.BrotliAmdDecoderAttachDictionary(self._h, ctypes.addressof(buf), len(data)))

    def close(self):
        if self._h:
            self._L.BrotliDecoderDestroyInstance(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decompress_stream(self, data: bytes, out_cap: int):
        """One BrotliDecoderDecompressStream call -> (result, bytes consumed, output bytes)."""
        L = self._L
        src = ctypes.create_string_buffer(bytes(data), max(1, len(data)))
        out = ctypes.create_string_buffer(max(1, out_cap))
        avail_in, avail_out = ctypes.c_size_t(len(data)), ctypes.c_size_t(out_cap)
        next_in, next_out = ctypes.c_void_p(ctypes.addressof(src)), ctypes.c_void_p(ctypes.addressof(out))
        total = ctypes.c_size_t(0)
        r = L.BrotliDecoderDecompressStream(self._h, ctypes.byref(avail_in), ctypes.byref(next_in), ctypes.byref(avail_out),
                                            ctypes.byref(next_out), ctypes.byref(total))
        return r, len(data) - avail_in.value, out.raw[:out_cap - avail_out.value]

    def error_code(self):
        return self._L.BrotliDecoderGetErrorCode(self._h)

    def error_string(self):
        return self._L.BrotliDecoderGetErrorString(self._h).decode()

    def is_finished(self):
        return bool(self._L.BrotliDecoderIsFinished(self._h))

    def is_used(self):
        return bool(self._L.BrotliDecoderIsUsed(self._h))

    def device_commands(self):
        """commands the device has decoded for this stream in all launches together (batch.h: BrotliAmdDecoderDeviceCommands)"""
        self._L.BrotliAmdDecoderDeviceCommands.restype = ctypes.c_uint64
        self._L.BrotliAmdDecoderDeviceCommands.argtypes = [ctypes.c_void_p]
        return int(self._L.BrotliAmdDecoderDeviceCommands(self._h))

    def has_more_output(self):
        return bool(self._L.BrotliDecoderHasMoreOutput(self._h))


class StreamSet:
    """BrotliAmdStreamSet (batch.h): steps many DecoderStates in one call -- one transfer in, one launch, one transfer back."""

    def __init__(self, max_states):
        self._L = load_library()
        self._h = self._L.BrotliAmdStreamSetCreate(max_states)
        if not self._h:
            raise MemoryError("BrotliAmdStreamSetCreate")
        self.max_states = max_states

    def close(self):
        if self._h:
            self._L.BrotliAmdStreamSetDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decompress(self, states, datas, out_caps):
        """One BrotliAmdStreamSetDecompress call: states[i] (a DecoderState) is given datas[i] and room for out_caps[i] bytes.
        -> [(result, bytes consumed, output bytes), ...], each what states[i].decompress_stream(datas[i], out_caps[i]) returns."""
        n = len(states)
        if len(datas) != n or len(out_caps) != n:
            raise ValueError("datas and out_caps: one entry per state")
        srcs = [ctypes.create_string_buffer(bytes(d), max(1, len(d))) for d in datas]
        outs = [ctypes.create_string_buffer(max(1, c)) for c in out_caps]
        a_st = (ctypes.c_void_p * max(1, n))(*[s._h for s in states])
        a_ai = (ctypes.c_size_t * max(1, n))(*[len(d) for d in datas])
        a_ni = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(b) for b in srcs])
        a_ao = (ctypes.c_size_t * max(1, n))(*out_caps)
        a_no = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(b) for b in outs])
        a_tot = (ctypes.c_size_t * max(1, n))()
        a_res = (ctypes.c_int * max(1, n))()
        if self._L.BrotliAmdStreamSetDecompress(self._h, n, a_st, a_ai, a_ni, a_ao, a_no, a_tot, a_res) != 0:
            raise RuntimeError("BrotliAmdStreamSetDecompress failed: " + last_error())
        return [(a_res[i], len(datas[i]) - a_ai[i], outs[i].raw[:out_caps[i] - a_ao[i]]) for i in range(n)]

    def last_launches(self):
        """decode launches of the last decompress(): 0 where no state needed the device, 1 as a rule"""
        return int(self._L.BrotliAmdStreamSetLastLaunches(self._h))

    def last_transfers(self):
        """host <-> device copies of payload bytes in the last decompress()"""
        return int(self._L.BrotliAmdStreamSetLastTransfers(self._h))


class Decompressor:
    """Pull adapter, reference src/reader.rs:91-182 (`Decompressor<R>: io::Read`): wraps a readable object that
    yields compressed bytes; read(n) returns decompressed bytes, b'' at the end of the stream.  A failure of the
    decoder, or input that ends before the stream does, raises ValueError (io::ErrorKind::InvalidData /
    UnexpectedEof in the reference, reader.rs:335-346)."""

    def __init__(self, reader, buffer_size=4096, large_window=True, dictionary=None):
        self._r = reader
        self._bufsize = max(1, buffer_size)
        # native constructors default to large_window (state.rs:394); dictionary: Decompressor::new_with_custom_dict (reader.rs:103-162)
        self._st = DecoderState(large_window=large_window, dictionary=dictionary)
        self._pending = b""
        self._done = False
        self._eof = False

    def read(self, n=-1):
        if n is None or n < 0:
            chunks = []
            while True:
                c = self.read(65536)
                if not c:
                    return b"".join(chunks)
                chunks.append(c)
        out = b""
        while not out and not self._done:
            if not self._pending and not self._eof:
                self._pending = self._r.read(self._bufsize) or b""  # an exception from the reader passes through
                if not self._pending:
                    self._eof = True
            r, used, out = self._st.decompress_stream(self._pending, n)
            self._pending = self._pending[used:]
            if r == RESULT_ERROR:
                raise ValueError("Invalid Data: " + self._st.error_string())
            if r == RESULT_SUCCESS:
                self._done = True
            elif r == RESULT_NEEDS_MORE_INPUT and self._eof and not out:
                raise ValueError("Unexpected EOF")
        return out

    def into_inner(self):
        return self._r


class DecompressorWriter:
    """Push adapter, reference src/writer.rs:104-199 (`DecompressorWriter<W>: io::Write`): write() takes compressed
    bytes and forwards decompressed bytes to the wrapped writer; close() drains and fails if the stream is
    incomplete (writer.rs:257-289)."""

    def __init__(self, writer, buffer_size=4096, large_window=True, dictionary=None):
        self._w = writer
        self._bufsize = max(1, buffer_size)
        self._st = DecoderState(large_window=large_window, dictionary=dictionary)  # DecompressorWriter::new_with_custom_dictionary (writer.rs:115-171)
        self._done = False

    def write(self, data: bytes):
        data = bytes(data)
        off = 0
        while True:
            r, used, out = self._st.decompress_stream(data[off:], self._bufsize)
            off += used
            if out:
                self._w.write(out)
            if r == RESULT_ERROR:
                raise ValueError("Invalid Data: " + self._st.error_string())
            if r == RESULT_SUCCESS:
                self._done = True
                return off  # bytes after the end of the stream are not consumed (writer.rs:383-398)
            if r == RESULT_NEEDS_MORE_INPUT:
                return len(data)

    def close(self):
        while not self._done:
            r, _, out = self._st.decompress_stream(b"", self._bufsize)
            if out:
                self._w.write(out)
            if r == RESULT_ERROR:
                raise ValueError("Invalid Data: " + self._st.error_string())
            if r == RESULT_SUCCESS:
                self._done = True
            elif r == RESULT_NEEDS_MORE_INPUT:
                raise ValueError("Unexpected EOF")
        return self._w
