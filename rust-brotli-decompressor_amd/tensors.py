"""Decoded outputs as typed tensors: the byte planes of a decode call's outputs back into elements, on the device, in one launch.

    results, ptr, offsets = batch.decode_device_packed(in_ptrs, in_sizes)
    weights = tensors.outputs_as_tensors(batch, [(torch.bfloat16, (4096, 11008)), (torch.float32, (4096,)), None])

Two launches in all: the decode and the unshuffle (Batch.unshuffle_outputs).  The streams hold arrays SHUFFLED into byte planes (Parquet's
BYTE_STREAM_SPLIT, the shuffle filter of Blosc and HDF5, the byte grouping of checkpoint compressors); the element width is the dtype's.
A stream whose array was stored as DELTAS (sorted timestamps, offsets, index arrays), with or without the shuffle, says so in its spec and
is summed up again by one more call (Batch.undelta_segments / Batch.undelta_outputs).  A stream whose array went through BITSHUFFLE (the bit
transpose of the bitshuffle library and HDF5 filter 32008, the bit-shuffle mode of Blosc-style containers) says so in its spec too, with the
block size where there is one, and its bit planes are turned back by one call for all such streams (Batch.bitunshuffle_outputs).  A stream
whose array was BIT-PACKED -- fields of k bits back to back: Parquet's bit-packed runs, Arrow's validity bitmaps, 4-bit weights,
numpy.packbits -- names k in its spec; it is the one stream whose slot is larger than its delivered bytes, and one call unpacks all such
streams into their slots (Batch.bitunpack_outputs).  A stream whose array was stored as VARINTS -- LEB128, protobuf's base-128 integers, plain or
zigzag: packed repeated fields, postings lists, offset tables -- says so in its spec; its size depends on its values, so one call decodes all such
streams into their slots and says how many integers each held (Batch.unvarint_outputs), and a stream that held another number than its shape
says, unfinished bytes or an integer of more than ten bytes is refused.  A stream whose array was stored as RUNS -- Parquet's RLE / bit-packed
hybrid: dictionary indices, definition and repetition levels, booleans -- says so in its spec, with its field width k or, where the stream's
first byte holds k, without; one call decodes all such streams into their slots (Batch.unrle_outputs), and a stream whose runs did not end
well or held fewer values than its shape says is refused.  A stream whose array was stored as DELTA BLOCKS -- Parquet's DELTA_BINARY_PACKED:
INT32 and INT64 pages, the lengths of byte arrays -- says "dbp"; one call decodes all such streams into their slots (Batch.undbp_outputs), and
a stream that did not end well or held another number of values than its shape says is refused; bytes behind its last block are not judged.
A stream that is a DICTIONARY-INDEX PAGE BODY -- Parquet's RLE_DICTIONARY: a width byte and then runs of indices -- names its dictionary, another
stream of the same call or a tensor, and one call turns all such streams into their VALUES (Batch.undict_outputs): the indices never reach
memory, and a stream with an index outside its dictionary is refused.  A stream that is the body of a NULLABLE column's data page -- definition
levels and the dense values that are there -- says ("nulls", level): one call spreads the values of all such streams over their nulls
(Batch.unnull_outputs), and the stream's entry is the pair (tensor, validity bitmap).  A STRING column -- the index page body over a
dictionary of byte arrays -- has no slot size before it is decoded, so it has a function of its own: outputs_as_strings."""
import collections

import torch

SLOT_ALIGN = 64   # every returned tensor starts at a multiple of this many bytes of one buffer


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


FILTERS = ("shuffle", "delta", "bitshuffle", "bitpack", "varint", "rle", "dbp", "dict", "nulls")
BITPACK_OPTIONS = {"big": 1, "signed": 2}   # BITUNPACK_MSB_FIRST, BITUNPACK_SIGNED
VARINT_OPTIONS = {"zigzag": 1}              # UNVARINT_ZIGZAG
RLE_WIDTH_BYTE = 1                          # UNRLE_WIDTH_BYTE, UNDICT_WIDTH_BYTE
DICT_NO_STREAM = 0xFFFFFFFF                 # UNDICT_NO_STREAM
DBP_STATUS = ("ok", "a header that is none", "a miniblock of more than 64 bits", "blocks that the stream's end cuts")
RLE_STATUS = ("ok", "a header of more than five bytes", "a run of no values", "runs that the stream's end cuts", "a width byte that is none",
              "a length in front of the levels that is cut or says more than there is")


# What a wanted stream's spec says: the slot's bytes, the tensor's dtype and shape, the element width, the names of its filters, bitshuffle's block
# and bitpack's (k, flags) -- (1, 0) where the stream is not packed, as for a stream that is not wanted --, varint's flags, rle's (k, flags) --
# (0, 0) where the stream has no runs --, dict's dictionary: a stream's number or a tensor (None where the stream has none), nulls' (level, the
# levels' tensor or None: they lie in the stream) (None where the stream has no levels)
_Stream = collections.namedtuple("_Stream", "want dtype shape item filters block pack varint rle dict nulls")


def _parse_spec(i, spec, size):
    """spec of stream i, which delivered `size` bytes -> _Stream; ValueError, naming the stream, for what outputs_as_tensors refuses"""
    dtype, shape = spec[0], spec[1]
    flt, block, pack, varint, rle, dictionary, nulls = [], 0, None, 0, None, None, None
    for name in (tuple(spec[2]) if len(spec) > 2 else ("shuffle",)):
        if isinstance(name, (tuple, list)) and len(name) == 2 and name[0] == "bitshuffle":   # ("bitshuffle", block_elems)
            name, block = name[0], int(name[1])
            if block < 0 or block % 8 != 0:
                raise ValueError("stream %d: a bitshuffle block of %d elements is neither 0 nor a multiple of 8" % (i, block))
        if isinstance(name, (tuple, list)) and len(name) >= 1 and name[0] == "bitpack":   # ("bitpack", k, options...)
            if len(name) < 2:
                raise ValueError("stream %d: \"bitpack\" without its field width: (\"bitpack\", k)" % i)
            for opt in name[2:]:
                if opt not in BITPACK_OPTIONS:
                    raise ValueError("stream %d: unknown bitpack option %r (known: %s)" % (i, opt, ", ".join(BITPACK_OPTIONS)))
            name, pack = name[0], (int(name[1]), sum({BITPACK_OPTIONS[opt] for opt in name[2:]}))
        elif name == "bitpack":
            raise ValueError("stream %d: \"bitpack\" without its field width: (\"bitpack\", k)" % i)
        if isinstance(name, (tuple, list)) and len(name) >= 1 and name[0] == "varint":   # ("varint", options...)
            for opt in name[1:]:
                if opt not in VARINT_OPTIONS:
                    raise ValueError("stream %d: unknown varint option %r (known: %s)" % (i, opt, ", ".join(VARINT_OPTIONS)))
            name, varint = name[0], sum({VARINT_OPTIONS[opt] for opt in name[1:]})
        if isinstance(name, (tuple, list)) and len(name) >= 1 and name[0] == "rle":   # ("rle", k)
            if len(name) != 2:
                raise ValueError("stream %d: (\"rle\", k) names the field width and nothing else; \"rle\" alone: the stream's first byte holds it" % i)
            name, rle = name[0], (int(name[1]), 0)
        elif name == "rle":
            rle = (0, RLE_WIDTH_BYTE)
        if isinstance(name, (tuple, list)) and len(name) >= 1 and name[0] == "dict":   # ("dict", j) or ("dict", tensor)
            if len(name) != 2 or isinstance(name[1], bool) or not isinstance(name[1], (int, torch.Tensor)):
                raise ValueError("stream %d: (\"dict\", j) names the stream that holds the dictionary, (\"dict\", tensor) the dictionary itself, and nothing else" % i)
            name, dictionary = name[0], name[1]
        elif name == "dict":
            raise ValueError("stream %d: \"dict\" without its dictionary: (\"dict\", j) or (\"dict\", tensor)" % i)
        if isinstance(name, (tuple, list)) and len(name) >= 1 and name[0] == "nulls":   # ("nulls", level) or ("nulls", level, levels_tensor)
            if len(name) not in (2, 3) or isinstance(name[1], bool) or not isinstance(name[1], int) or not 0 <= name[1] < (1 << 32) or \
                    (len(name) == 3 and not isinstance(name[2], torch.Tensor)):
                raise ValueError("stream %d: (\"nulls\", level) names the definition level of a value that is there, 0 .. 2^32 - 1, "
                                 "(\"nulls\", level, tensor) the levels' bytes as well, and nothing else" % i)
            name, nulls = name[0], (int(name[1]), name[2] if len(name) == 3 else None)
        elif name == "nulls":
            raise ValueError("stream %d: \"nulls\" without its level: (\"nulls\", level) or (\"nulls\", level, tensor)" % i)
        if name in VARINT_OPTIONS and flt and flt[-1] == "varint":   # ("varint", "zigzag") as the spec's filters: the option right behind its filter
            varint |= VARINT_OPTIONS[name]
            continue
        if name not in FILTERS:
            raise ValueError("stream %d: unknown filter %r (known: %s)" % (i, name, ", ".join(FILTERS)))
        flt.append(name)
    flt = tuple(flt)
    if "dict" in flt and len(flt) != 1:
        raise ValueError("stream %d: \"dict\" stands alone in a spec: the values come out of the dictionary as they are" % i)
    if "nulls" in flt and len(flt) != 1:
        raise ValueError("stream %d: \"nulls\" stands alone in a spec: the values go to their slots as they are" % i)
    if "shuffle" in flt and "bitshuffle" in flt:
        raise ValueError("stream %d: \"shuffle\" and \"bitshuffle\" in one spec: an array goes through one of them" % i)
    if pack is not None and ("shuffle" in flt or "bitshuffle" in flt):
        raise ValueError("stream %d: \"bitpack\" with \"shuffle\" or \"bitshuffle\" in one spec: packed fields have no byte or bit planes" % i)
    if "varint" in flt and ("shuffle" in flt or "bitshuffle" in flt or pack is not None):
        raise ValueError("stream %d: \"varint\" with \"shuffle\", \"bitshuffle\" or \"bitpack\" in one spec: integers of variable length have no planes and no fields" % i)
    if "rle" in flt and ("shuffle" in flt or "bitshuffle" in flt or pack is not None or "varint" in flt):
        raise ValueError("stream %d: \"rle\" with \"shuffle\", \"bitshuffle\", \"bitpack\" or \"varint\" in one spec: runs have no planes, and their fields and headers are their own" % i)
    if "dbp" in flt and len(flt) != 1 and flt != ("dbp", "delta"):
        raise ValueError("stream %d: \"dbp\" stands alone or in front of \"delta\": its blocks have no planes, and their fields and varints are their own" % i)
    shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    item = torch.empty(0, dtype=dtype).element_size()
    if item not in (1, 2, 4, 8):
        raise ValueError("stream %d: elements of %d bytes (%s) cannot be unshuffled" % (i, item, dtype))
    want = _numel(shape) * item
    if pack is not None:
        if not 1 <= pack[0] <= 8 * item:
            raise ValueError("stream %d: bitpack fields of %d bits, but %s takes 1 .. %d" % (i, pack[0], dtype, 8 * item))
        stored = (_numel(shape) * pack[0] + 7) // 8
        if size != stored:
            raise ValueError("stream %d: %d delivered bytes, but %d fields of %d bits (shape %s) are %d" % (i, size, _numel(shape), pack[0], shape, stored))
    elif "varint" in flt or "rle" in flt or "dbp" in flt or "dict" in flt or "nulls" in flt:
        pass   # (how many integers the delivered bytes hold is the call's to say: outputs_as_tensors checks its result)
    elif size != want:
        raise ValueError("stream %d: %d delivered bytes, but %s of shape %s is %d" % (i, size, dtype, shape, want))
    if rle is not None and not rle[1] and not 0 <= rle[0] <= min(32, 8 * item):
        raise ValueError("stream %d: rle fields of %d bits, but %s takes 0 .. %d" % (i, rle[0], dtype, min(32, 8 * item)))
    if isinstance(dictionary, torch.Tensor) and (dictionary.dtype != dtype or dictionary.dim() != 1 or not dictionary.is_contiguous() or not dictionary.is_cuda):
        raise ValueError("stream %d: its dictionary is a %s tensor of shape %s%s, not a contiguous 1-D device tensor of %s" %
                         (i, dictionary.dtype, tuple(dictionary.shape), "" if dictionary.is_cuda else " on the host", dtype))
    if nulls is not None and nulls[1] is not None and (nulls[1].dtype != torch.uint8 or nulls[1].dim() != 1 or not nulls[1].is_contiguous() or not nulls[1].is_cuda):
        raise ValueError("stream %d: its levels are a %s tensor of shape %s%s, not a contiguous 1-D device tensor of torch.uint8" %
                         (i, nulls[1].dtype, tuple(nulls[1].shape), "" if nulls[1].is_cuda else " on the host"))
    return _Stream(want, dtype, shape, item, flt, block, pack or (1, 0), varint, rle or (0, 0), dictionary, nulls)


def outputs_as_tensors(batch, specs):
    """specs[i]: (torch dtype, shape) of stream i of the last decode call on `batch` (after decode_device: once wait() has returned), or None
    for a stream that is not wanted.  -> a list of tensors (None where the spec was None), views of ONE torch.uint8 buffer on the batch
    object's device with 64-byte-aligned slots.  Raises ValueError, naming the stream, where a stream's delivered bytes are not
    numel x itemsize, and for an element size that is not 1, 2, 4 or 8.

    A spec may carry a third item, a tuple of the FILTERS the stream's array went through in front of the codec:
        (dtype, shape)                        ("shuffle",): the stream holds byte planes
        (dtype, shape, ("shuffle", "delta"))  byte planes of deltas: unshuffled as above, then Batch.undelta_segments in place over the slots
        (dtype, shape, ("delta",))            deltas: Batch.undelta_outputs straight into the slot
        (dtype, shape, ())                    the array's bytes as they are: a copy
        (dtype, shape, ("bitshuffle",))       bit planes, one block over the whole array (Blosc's rule): ONE Batch.bitunshuffle_outputs call
                                              for all such streams, into the slots
        (dtype, shape, (("bitshuffle", 2048),))  bit planes in blocks of 2048 elements -- an item of the tuple may be the pair
                                              ("bitshuffle", block_elems), a multiple of 8; HDF5's default is 8192 // itemsize
        (dtype, shape, ("bitshuffle", "delta"))  bit planes of deltas: that call, then Batch.undelta_segments in place over the slots
        (dtype, shape, (("bitpack", 12),))    numel fields of 12 bits, LSB-first, zero-extended into the dtype's elements (k = 1 ..
                                              8 x itemsize): ONE Batch.bitunpack_outputs call for all such streams, into the slots.  Such a
                                              stream must have delivered exactly ceil(numel k / 8) bytes; its slot is numel x itemsize
        (dtype, shape, (("bitpack", 4, "signed"),))  ... sign-extended from bit k - 1; "big" behind k: MSB-first (numpy.packbits, PNG); both may stand
        (dtype, shape, (("bitpack", 20), "delta"))  packed deltas (frame of reference): that call, then Batch.undelta_segments in place
        (dtype, shape, ("varint",))           numel LEB128 varints, each truncated to the dtype's elements: ONE Batch.unvarint_outputs call for
                                              all such streams, into the slots.  ValueError, naming the stream, where the delivered bytes hold
                                              another number of varints than numel, end in an unfinished one, or hold one of more than ten bytes
        (dtype, shape, (("varint", "zigzag"),))  ... zigzag: (v >> 1) ^ -(v & 1), the signed integers of protobuf's sint64 and Avro's long;
                                              ("varint", "zigzag") as the filters, the option right behind its filter, says the same
        (dtype, shape, ("varint", "delta"))   varints of deltas (sorted ids, postings): that call, then Batch.undelta_segments in place
        (dtype, shape, (("rle", 12),))        runs of Parquet's RLE / bit-packed hybrid with fields of 12 bits (k = 0 .. 32 and at most
                                              8 x itemsize), zero-extended into the dtype's elements: ONE Batch.unrle_outputs call for all such
                                              streams, into the slots, which are numel x itemsize.  ValueError, naming the stream and what was
                                              found, where the runs do not end well (a status that is not OK) or hold fewer values than numel;
                                              more values than numel are the last group's padding and are not judged
        (dtype, shape, ("rle",))              ... the stream's first byte holds k: a dictionary-index page body
        (dtype, shape, (("rle", 20), "delta"))  runs of deltas: that call, then Batch.undelta_segments in place
        (dtype, shape, ("dbp",))              a DELTA_BINARY_PACKED stream (Parquet's INT32 and INT64 pages, the lengths of its byte arrays), its
                                              values truncated to the dtype's elements: ONE Batch.undbp_outputs call for all such streams, into
                                              the slots.  ValueError, naming the stream and what was found, where the stream does not end well
                                              (a status that is not OK) or holds another number of values than numel; bytes behind its last
                                              block are not judged
        (dtype, shape, ("dbp", "delta"))      such a stream of deltas: that call, then Batch.undelta_segments in place; "dbp" with any other
                                              filter raises ValueError
        (dtype, shape, (("dict", j),))        a dictionary-index page body -- a width byte k, then runs of k-bit indices --, whose dictionary is
                                              what stream j of the same call delivered, taken as elements of the dtype (D = its bytes //
                                              itemsize; stream j's own spec may be None or one of its own): ONE Batch.undict_outputs call for
                                              all such streams, into the slots; the indices never reach memory.  ValueError, naming the stream
                                              and what was found, where the runs do not end well (a status that is not OK), hold fewer values
                                              than numel, or hold an index outside the dictionary (the text names the first one and D); more
                                              values than numel are the last group's padding and are not judged
        (dtype, shape, (("dict", tensor),))   ... whose dictionary is a 1-D contiguous device tensor of the dtype; "dict" with any other
                                              filter raises ValueError, and so does a j that is the stream itself or no stream of the call
        (dtype, shape, (("nulls", level),))   the body of a NULLABLE column's v1 data page: a 4-byte length, the definition levels -- runs of
                                              fields of level.bit_length() bits --, and behind them the dense values of the rows that are
                                              there, PLAIN.  ONE Batch.unnull_outputs call for all such streams spreads the values over the
                                              rows: a row whose level is `level` gets the next value, every other row 0.  The stream's entry
                                              in the result is the PAIR (tensor, valid), valid being a uint8 tensor of ceil(numel / 8) bytes,
                                              Arrow's validity bitmap (bit i & 7 of byte i >> 3).  ValueError, naming the stream and what was
                                              found, where the levels do not end well (a status that is not OK), hold another number of rows
                                              than numel, a row that is there has no value, or values are left over
        (dtype, shape, (("nulls", level, levels),))  ... of a v2 data page: the levels are the caller's, a contiguous 1-D uint8 device tensor
                                              (a v2 page keeps them outside the compressed body), and the stream holds the dense values
                                              alone; "nulls" with any other filter raises ValueError
    "varint" together with "shuffle", "bitshuffle" or "bitpack" in one spec raises ValueError, naming the stream; so does "rle" together with
    any of those four.
    "shuffle" together with "bitshuffle", and "bitpack" together with either, in one spec raises ValueError, naming the stream; so does a k outside
    1 .. 8 x itemsize and an unknown option.
    Delta is a wrapping running sum over the flattened array, on the dtype's BIT PATTERN taken as a little-endian unsigned integer of its
    width: meant for integer dtypes, allowed for any.  An unknown filter name raises ValueError, naming the stream."""
    sizes = batch.out_sizes
    if sizes is None:
        raise RuntimeError("no outputs: no decode call on this batch object yet, or its launch has not been waited for")
    if len(specs) != len(sizes):
        raise ValueError("specs: %d entries for the %d streams of the last decode call" % (len(specs), len(sizes)))
    streams = [None if spec is None else _parse_spec(i, spec, sizes[i]) for i, spec in enumerate(specs)]
    offs, total = [], 0   # every stream's slot in the buffer
    for st in streams:
        offs.append(total)
        if st is not None:
            total = (total + st.want + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN
            if st.nulls is not None:   # the bitmap has a slot of its own behind the rows'
                total = (total + (_numel(st.shape) + 7) // 8 + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN
    buf = torch.empty(total + SLOT_ALIGN, dtype=torch.uint8, device="cuda")
    skip = -buf.data_ptr() % SLOT_ALIGN   # (the allocator's blocks are aligned far beyond this; nothing here depends on it)
    buf = buf[skip:skip + total]
    base = buf.data_ptr()
    # (a slot of no bytes has a pointer too: a NULL one would mean "skip", which is the same here)
    at = [None if st is None else base + off for st, off in zip(streams, offs)]
    widths = [1 if st is None else st.item for st in streams]

    def only(which):
        """the slots of the streams in `which`, None for the others"""
        return [p if i in which else None for i, p in enumerate(at)]

    wanted = [i for i, st in enumerate(streams) if st is not None]
    bits = [i for i in wanted if "bitshuffle" in streams[i].filters]
    packed = [i for i in wanted if "bitpack" in streams[i].filters]
    varints = [i for i in wanted if "varint" in streams[i].filters]
    runs = [i for i in wanted if "rle" in streams[i].filters]
    blocks = [i for i in wanted if "dbp" in streams[i].filters]
    dicts = [i for i in wanted if "dict" in streams[i].filters]
    nullable = [i for i in wanted if "nulls" in streams[i].filters]
    for i in dicts:
        j = streams[i].dict
        if not isinstance(j, torch.Tensor) and (j == i or not 0 <= j < len(sizes)):
            raise ValueError("stream %d: its dictionary stream %d is %s" % (i, j, "the stream itself" if j == i else "none of the %d streams of the last decode call" % len(sizes)))
    # deltas only: every other wanted stream that is neither of bit planes nor of packed fields is the unshuffle call's; without "shuffle" it is
    # a copy -- width 1
    plain = [i for i in wanted if i not in bits and i not in packed and i not in varints and i not in runs and i not in blocks and i not in dicts and i not in nullable and "shuffle" not in streams[i].filters and "delta" in streams[i].filters]
    batch.unshuffle_outputs(only([i for i in wanted if i not in plain and i not in bits and i not in packed and i not in varints and i not in runs and i not in blocks and i not in dicts and i not in nullable]),
                            [st.item if st is not None and "shuffle" in st.filters else 1 for st in streams])
    if bits:    # bit planes: from the outputs straight into the slots
        batch.bitunshuffle_outputs(only(bits), widths, [0 if st is None else st.block for st in streams])
    if packed:  # packed fields: from the outputs straight into the slots, which are larger than the outputs
        batch.bitunpack_outputs(only(packed), [1 if st is None else st.pack[0] for st in streams], widths,
                                [0 if st is None else _numel(st.shape) for st in streams], [0 if st is None else st.pack[1] for st in streams])
    if varints:  # varints: from the outputs straight into the slots, numel elements each; what a stream held must be exactly that
        res = batch.unvarint_outputs(only(varints), [0 if st is None else _numel(st.shape) for st in streams], widths,
                                     [0 if st is None else st.varint for st in streams])
        for i in varints:
            count, consumed, overlong = res[i]
            if count != _numel(streams[i].shape):
                raise ValueError("stream %d: %d varints, but shape %s is %d elements" % (i, count, streams[i].shape, _numel(streams[i].shape)))
            if consumed != sizes[i]:
                raise ValueError("stream %d: %d delivered bytes, but its varints end after %d: an unfinished one trails them" % (i, sizes[i], consumed))
            if overlong != 0:
                raise ValueError("stream %d: %d varints of more than ten bytes" % (i, overlong))
    if runs:    # runs: from the outputs straight into the slots, numel elements each; a stream must have ended well and held at least that
        res = batch.unrle_outputs(only(runs), [0 if st is None else _numel(st.shape) for st in streams], [0 if st is None else st.rle[0] for st in streams], widths,
                                  [0 if st is None else st.rle[1] for st in streams])
        for i in runs:
            count, consumed, _, status, k = res[i]
            if status != 0:
                raise ValueError("stream %d: %s (status %d) after %d values in %d of its %d delivered bytes, fields of %d bits" %
                                 (i, RLE_STATUS[status] if status < len(RLE_STATUS) else "an unknown status", status, count, consumed, sizes[i], k))
            if count < _numel(streams[i].shape):
                raise ValueError("stream %d: %d values in its runs, but shape %s is %d elements" % (i, count, streams[i].shape, _numel(streams[i].shape)))
    if blocks:  # delta blocks: from the outputs straight into the slots; a stream must have ended well and held exactly numel values
        res = batch.undbp_outputs(only(blocks), [0 if st is None else _numel(st.shape) for st in streams], widths)
        for i in blocks:
            count, consumed, declared, _, status, _, _ = res[i]
            if status != 0:
                raise ValueError("stream %d: %s (status %d) after %d of %d declared values in %d of its %d delivered bytes" %
                                 (i, DBP_STATUS[status] if status < len(DBP_STATUS) else "an unknown status", status, count, declared, consumed, sizes[i]))
            if count != _numel(streams[i].shape):
                raise ValueError("stream %d: %d values in its blocks, but shape %s is %d elements" % (i, count, streams[i].shape, _numel(streams[i].shape)))
    if dicts:   # dictionary indices: the values from the outputs and the dictionaries straight into the slots; every index must lie inside
        by_tensor = {i: isinstance(streams[i].dict, torch.Tensor) for i in dicts}
        entries = {i: streams[i].dict.numel() if by_tensor[i] else sizes[streams[i].dict] // streams[i].item for i in dicts}
        res = batch.undict_outputs(only(dicts), [0 if st is None else _numel(st.shape) for st in streams], [0] * len(streams), widths,
                                   [RLE_WIDTH_BYTE if i in by_tensor else 0 for i in range(len(streams))],
                                   [streams[i].dict if i in by_tensor and not by_tensor[i] else DICT_NO_STREAM for i in range(len(streams))],
                                   [streams[i].dict.data_ptr() if by_tensor.get(i) else None for i in range(len(streams))],
                                   [entries[i] if by_tensor.get(i) else 0 for i in range(len(streams))])
        for i in dicts:
            count, consumed, _, status, k, bad, first_bad = res[i]
            if status != 0:
                raise ValueError("stream %d: %s (status %d) after %d values in %d of its %d delivered bytes, indices of %d bits" %
                                 (i, RLE_STATUS[status] if status < len(RLE_STATUS) else "an unknown status", status, count, consumed, sizes[i], k))
            if count < _numel(streams[i].shape):
                raise ValueError("stream %d: %d values in its runs, but shape %s is %d elements" % (i, count, streams[i].shape, _numel(streams[i].shape)))
            if bad != 0:
                raise ValueError("stream %d: %d of its %d values have an index outside its dictionary of %d entries, the first of them value %d" %
                                 (i, bad, _numel(streams[i].shape), entries[i], first_bad))
    valid_at = {i: offs[i] + (streams[i].want + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN for i in nullable}   # the bitmaps' slots
    if nullable:   # levels and dense values: the rows and their bitmaps from the outputs straight into the slots; every row that is there has a value
        n = len(streams)
        level_of = [streams[i].nulls[0] if i in valid_at else 0 for i in range(n)]
        lv = [streams[i].nulls[1] if i in valid_at else None for i in range(n)]
        res = batch.unnull_outputs(only(nullable), [base + valid_at[i] if i in valid_at else None for i in range(n)], [0 if st is None else _numel(st.shape) for st in streams],
                                   [v.bit_length() for v in level_of], level_of, widths,
                                   [None if t is None else t.data_ptr() or 1 for t in lv] if any(t is not None for t in lv) else None,
                                   [0 if t is None else t.numel() for t in lv] if any(t is not None for t in lv) else None)
        for i in nullable:
            count, consumed, _, status, k, present, missing, values = res[i]
            numel = _numel(streams[i].shape)
            if status != 0:
                raise ValueError("stream %d: %s (status %d) after %d levels in %d of their bytes, levels of %d bits" %
                                 (i, RLE_STATUS[status] if status < len(RLE_STATUS) else "an unknown status", status, count, consumed, k))
            if count != numel:
                raise ValueError("stream %d: %d levels, but shape %s is %d elements" % (i, count, streams[i].shape, numel))
            if missing != 0:
                raise ValueError("stream %d: %d of its %d rows that are there have no value: the stream holds %d values" % (i, missing, present, values))
            if present != values:
                raise ValueError("stream %d: %d values for the %d rows that are there: values are left over" % (i, values, present))
    if plain:   # deltas only: from the outputs straight into the slots
        batch.undelta_outputs(only(plain), widths)
    both = [i for i in wanted if i not in plain and "delta" in streams[i].filters]
    if both:    # in place over the slots, which are 64-byte aligned
        batch.undelta_segments([at[i] for i in both], [at[i] for i in both], [streams[i].want for i in both], [widths[i] for i in both])
    out = [None if st is None else buf[off:off + st.want].view(st.dtype).reshape(st.shape) for st, off in zip(streams, offs)]
    for i in nullable:
        out[i] = (out[i], buf[valid_at[i]:valid_at[i] + (_numel(streams[i].shape) + 7) // 8])
    return out


BYTES_OFFSETS64, BYTES_SKIP, BYTES_ALL = 2, 8, (1 << 64) - 1   # UNDICT_BYTES_OFFSETS64, UNDICT_BYTES_SKIP, UNDICT_BYTES_ALL
DLBA_OFFSETS64, DLBA_SKIP = 2, 8   # UNDLBA_OFFSETS64, UNDLBA_SKIP
DBA_OFFSETS64, DBA_SKIP = 2, 8   # UNDBA_OFFSETS64, UNDBA_SKIP
DBA_BAD_KINDS = ("no rule", "a negative prefix length", "a negative suffix length", "a prefix longer than the element in front of it")   # UndbaResult.bad_kind
INT32_MAX = (1 << 31) - 1


def outputs_as_strings(batch, specs):
    """The streams of the last decode call on `batch` that are DICTIONARY-INDEX PAGE BODIES of string columns -- a width byte k, then runs of
    k-bit indices into a dictionary of PLAIN byte arrays (Parquet's RLE_DICTIONARY over BYTE_ARRAY) -- as Arrow string columns.  specs[i]:
    None for a stream that is not wanted (a dictionary page among them), (rows, j) for a body of `rows` rows whose dictionary is what stream j of
    the same call delivered, or (rows, tensor) with the dictionary page's bytes as a contiguous 1-D uint8 device tensor; a third item "large"
    asks for int64 offsets.  -> a list of (offsets, data) pairs (None where the spec was None): offsets has rows + 1 entries, int32 or int64,
    data is uint8, and both are views of ONE buffer with 64-byte-aligned slots.  One measuring call (Batch.measure_dict_bytes_outputs: the
    rows are in the page header, the bytes are not), one allocation and one writing call (Batch.undict_bytes_outputs); the indices never
    reach memory.  ValueError, naming the stream and what was found, where the runs do not end well (a status that is not OK), hold fewer
    values than rows (more are the last group's padding and are not judged), the dictionary is cut, an index lies outside the dictionary (the
    text names the first one and D), the bytes are more than 2^31 - 1 without "large", or j is the stream itself or no stream of the call.
    specs[i] may also be ("dlba", rows) or ("dlba", rows, "large") for a DELTA_LENGTH_BYTE_ARRAY page body of a required column -- the lengths
    as DELTA_BINARY_PACKED, then the bytes --: one counting call (Batch.count_dlba_outputs gives the bytes there are), the same allocation, one
    writing call (Batch.undlba_outputs).  ValueError for such a stream where the lengths do not end well, their number is not `rows` exactly
    (the encoding states it: there is no padding to forgive), a length is negative (the text names the first one), or the lengths' sum is not
    the bytes that are there (the text says which is larger).  Both kinds may stand in one call: two pairs of library calls into one buffer.
    specs[i] may also be ("dba", rows) or ("dba", rows, "large") for a DELTA_BYTE_ARRAY page body of a required column -- prefix lengths and
    suffix lengths as DELTA_BINARY_PACKED, then the suffix bytes --: one measuring call (Batch.measure_dba_outputs gives the bytes the strings
    take), the same allocation, one writing call (Batch.undba_outputs).  ValueError for such a stream where either stream of lengths does not
    end well, the two hold different numbers of lengths, their number is not `rows` exactly, an element breaks a rule (the text names the first
    one and the rule), or the suffix lengths' sum is not the bytes that are there (the data is short, or bytes are left over)."""
    sizes = batch.out_sizes
    if sizes is None:
        raise RuntimeError("no outputs: no decode call on this batch object yet, or its launch has not been waited for")
    n = len(sizes)
    if len(specs) != n:
        raise ValueError("specs: %d entries for the %d streams of the last decode call" % (len(specs), n))
    rows, large, dict_streams, dict_ptrs, dict_lens = [None] * n, [False] * n, [DICT_NO_STREAM] * n, [None] * n, [0] * n
    dlba = {}   # the streams that are DELTA_LENGTH_BYTE_ARRAY bodies: their rows
    dba = {}    # the streams that are DELTA_BYTE_ARRAY bodies: their rows
    for i, spec in enumerate(specs):
        if spec is None:
            continue
        if len(spec) >= 1 and isinstance(spec[0], str) and spec[0] == "dlba":
            if len(spec) not in (2, 3) or (len(spec) == 3 and spec[2] != "large") or isinstance(spec[1], bool) or not isinstance(spec[1], int) or spec[1] < 0:
                raise ValueError("stream %d: a \"dlba\" spec is (\"dlba\", rows) or (\"dlba\", rows, \"large\")" % i)
            dlba[i], large[i] = int(spec[1]), len(spec) == 3
            continue
        if len(spec) >= 1 and isinstance(spec[0], str) and spec[0] == "dba":
            if len(spec) not in (2, 3) or (len(spec) == 3 and spec[2] != "large") or isinstance(spec[1], bool) or not isinstance(spec[1], int) or spec[1] < 0:
                raise ValueError("stream %d: a \"dba\" spec is (\"dba\", rows) or (\"dba\", rows, \"large\")" % i)
            dba[i], large[i] = int(spec[1]), len(spec) == 3
            continue
        if len(spec) not in (2, 3) or (len(spec) == 3 and spec[2] != "large") or isinstance(spec[0], bool) or not isinstance(spec[0], int) or spec[0] < 0:
            raise ValueError("stream %d: a spec is (rows, j), (rows, tensor) or either with \"large\" behind it" % i)
        rows[i], large[i], j = int(spec[0]), len(spec) == 3, spec[1]
        if isinstance(j, torch.Tensor):
            if j.dtype != torch.uint8 or j.dim() != 1 or not j.is_contiguous() or not j.is_cuda:
                raise ValueError("stream %d: its dictionary is a %s tensor of shape %s%s, not a contiguous 1-D device tensor of torch.uint8" %
                                 (i, j.dtype, tuple(j.shape), "" if j.is_cuda else " on the host"))
            dict_ptrs[i], dict_lens[i] = j.data_ptr(), j.numel()
        elif isinstance(j, bool) or not isinstance(j, int):
            raise ValueError("stream %d: (rows, j) names the stream that holds the dictionary, (rows, tensor) the dictionary's bytes, and nothing else" % i)
        elif j == i or not 0 <= j < n:
            raise ValueError("stream %d: its dictionary stream %d is %s" % (i, j, "the stream itself" if j == i else "none of the %d streams of the last decode call" % n))
        else:
            dict_streams[i] = j
    wanted = [i for i in range(n) if rows[i] is not None]
    flags = [1 | (BYTES_OFFSETS64 if large[i] else 0) if rows[i] is not None else BYTES_SKIP for i in range(n)]
    # a column of no rows is still measured and written: a capacity of 0 would only count, and offsets[0] would stay unwritten
    caps = [None if r is None else max(r, 1) for r in rows]
    res = batch.measure_dict_bytes_outputs(caps, [0] * n, dict_streams, dict_ptrs, dict_lens, None, [f & ~BYTES_SKIP for f in flags])
    kept = {}
    for i in wanted:
        count, consumed, _, status, k, bad, first_bad, nbytes, D, dict_consumed, dict_status = res[i]
        if status != 0:
            raise ValueError("stream %d: %s (status %d) after %d values in %d of its %d delivered bytes, indices of %d bits" %
                             (i, RLE_STATUS[status] if status < len(RLE_STATUS) else "an unknown status", status, count, consumed, sizes[i], k))
        if count < rows[i]:
            raise ValueError("stream %d: %d values in its runs, but the column has %d rows" % (i, count, rows[i]))
        if dict_status != 0:
            raise ValueError("stream %d: its dictionary is cut: %d whole entries in %d of its bytes" % (i, D, dict_consumed))
        if rows[i] == 0:   # (the one element that was measured is not the column's)
            bad, nbytes = 0, 0
        if bad != 0:
            raise ValueError("stream %d: %d of its %d values have an index outside its dictionary of %d entries, the first of them value %d" % (i, bad, rows[i], D, first_bad))
        if nbytes > INT32_MAX and not large[i]:
            raise ValueError("stream %d: %d bytes of strings, more than int32 offsets hold: ask for \"large\"" % (i, nbytes))
        kept[i] = nbytes
    dlba_flags = [(DLBA_OFFSETS64 if large[i] else 0) if i in dlba else DLBA_SKIP for i in range(n)]
    if dlba:   # the lengths state the rows, and the bytes that are there are the data's size
        counted = batch.count_dlba_outputs(dlba_flags)
        for i in sorted(dlba):
            count, consumed, declared, _, status, _, _, _, _, _, _, avail = counted[i]
            if status != 0:
                raise ValueError("stream %d: %s (status %d) after %d lengths in %d of its %d delivered bytes, of %d declared" %
                                 (i, DBP_STATUS[status] if status < len(DBP_STATUS) else "an unknown status", status, count, consumed, sizes[i], declared))
            if count != dlba[i]:
                raise ValueError("stream %d: %d lengths in its stream, but the column has %d rows" % (i, count, dlba[i]))
            if avail > INT32_MAX and not large[i]:
                raise ValueError("stream %d: %d bytes of strings, more than int32 offsets hold: ask for \"large\"" % (i, avail))
            rows[i], kept[i] = dlba[i], avail
        wanted = sorted(wanted + list(dlba))
    dba_flags = [(DBA_OFFSETS64 if large[i] else 0) if i in dba else DBA_SKIP for i in range(n)]
    if dba:   # everything is judged by the measuring call: nothing in a result depends on the data's capacity
        measured = batch.measure_dba_outputs([max(dba[i], 1) if i in dba else None for i in range(n)], [f & ~DBA_SKIP for f in dba_flags])
        for i in sorted(dba):
            r = measured[i]
            for what, (count, consumed, declared, _, status) in (("prefix", r[0:5]), ("suffix", r[8:13])):
                if status != 0:
                    raise ValueError("stream %d: its %s lengths: %s (status %d) after %d lengths in %d bytes, of %d declared" %
                                     (i, what, DBP_STATUS[status] if status < len(DBP_STATUS) else "an unknown status", status, count, consumed, declared))
            count_p, count_s, kind, first_bad, nbytes, suffix_bytes, avail = r[0], r[8], r[15], r[16], r[17], r[18], r[19]
            if count_p != count_s:
                raise ValueError("stream %d: %d prefix lengths and %d suffix lengths" % (i, count_p, count_s))
            if count_p != dba[i]:
                raise ValueError("stream %d: %d lengths in its streams, but the column has %d rows" % (i, count_p, dba[i]))
            if dba[i] != 0 and first_bad != (1 << 64) - 1:
                raise ValueError("stream %d: element %d of its %d has %s" % (i, first_bad, dba[i], DBA_BAD_KINDS[kind] if kind < len(DBA_BAD_KINDS) else "an unknown fault"))
            if suffix_bytes != avail:
                raise ValueError("stream %d: its suffix lengths add up to %d bytes and %d are there: %s" %
                                 (i, suffix_bytes, avail, "bytes are left over" if avail > suffix_bytes else "the data is short"))
            if nbytes > INT32_MAX and not large[i]:
                raise ValueError("stream %d: %d bytes of strings, more than int32 offsets hold: ask for \"large\"" % (i, nbytes))
            rows[i], kept[i] = dba[i], nbytes
        wanted = sorted(wanted + list(dba))
    up = lambda v: (v + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN
    o_at, d_at, total = {}, {}, 0
    for i in wanted:
        o_at[i], total = total, up(total + (rows[i] + 1) * (8 if large[i] else 4))
        d_at[i], total = total, up(total + kept[i])
    buf = torch.empty(total + SLOT_ALIGN, dtype=torch.uint8, device="cuda")
    skip = -buf.data_ptr() % SLOT_ALIGN
    buf = buf[skip:skip + total]
    base = buf.data_ptr()
    if len(wanted) > len(dlba) + len(dba):
        # rows of 0: a capacity of 1 with a data capacity of 0 writes offsets[0] and offsets[1], and offsets[1]'s slot is the padding's
        of_dict = lambda at: [base + at[i] if i in at and i not in dlba and i not in dba else None for i in range(n)]
        batch.undict_bytes_outputs(of_dict(o_at), of_dict(d_at), [0 if i in dlba or i in dba else kept.get(i, 0) for i in range(n)], [0 if c is None else c for c in caps], [0] * n, flags,
                                   None, dict_streams, dict_ptrs, dict_lens)
    if dlba:
        # (rows of 0: the stream has no lengths, as was counted, so a capacity of 1 writes offsets[0] alone)
        written = batch.undlba_outputs([base + o_at[i] if i in dlba else None for i in range(n)], [base + d_at[i] if i in dlba else None for i in range(n)],
                                       [kept[i] if i in dlba else 0 for i in range(n)], [max(dlba[i], 1) if i in dlba else 0 for i in range(n)], dlba_flags)
        for i in sorted(dlba):
            bad, first_bad, nbytes, avail = written[i][8:12]
            if bad != 0:
                raise ValueError("stream %d: %d of its %d lengths are negative, the first of them value %d" % (i, bad, dlba[i], first_bad))
            if nbytes != avail:
                raise ValueError("stream %d: its lengths add up to %d bytes and %d are there: %s" %
                                 (i, nbytes, avail, "bytes are left over" if avail > nbytes else "the data is short"))
    if dba:
        # (rows of 0: the streams have no lengths, as was measured, so a capacity of 1 writes offsets[0] alone)
        batch.undba_outputs([base + o_at[i] if i in dba else None for i in range(n)], [base + d_at[i] if i in dba else None for i in range(n)],
                            [kept[i] if i in dba else 0 for i in range(n)], [max(dba[i], 1) if i in dba else 0 for i in range(n)], dba_flags)
    out = [None] * n
    for i in wanted:
        offsets = buf[o_at[i]:o_at[i] + (rows[i] + 1) * (8 if large[i] else 4)].view(torch.int64 if large[i] else torch.int32)
        out[i] = (offsets, buf[d_at[i]:d_at[i] + kept[i]])
    return out
