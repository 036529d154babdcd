"""Decoded outputs as typed tensors: the byte planes of a decode call's outputs back into elements, on the device, in one launch.

    results, ptr, offsets = batch.decode_device_packed(in_ptrs, in_sizes)
    weights = tensors.outputs_as_tensors(batch, [(torch.bfloat16, (4096, 11008)), (torch.float32, (4096,)), None])

Two launches in all: the decode and the unshuffle (Batch.unshuffle_outputs).  The streams hold arrays SHUFFLED into byte planes (Parquet's
BYTE_STREAM_SPLIT, the shuffle filter of Blosc and HDF5, the byte grouping of checkpoint compressors); the element width is the dtype's.
A stream whose array was stored as DELTAS (sorted timestamps, offsets, index arrays), with or without the shuffle, says so in its spec and
is summed up again by one more call (Batch.undelta_segments / Batch.undelta_outputs)."""
import torch

SLOT_ALIGN = 64   # every returned tensor starts at a multiple of this many bytes of one buffer


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


FILTERS = ("shuffle", "delta")


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
    Delta is a wrapping running sum over the flattened array, on the dtype's BIT PATTERN taken as a little-endian unsigned integer of its
    width: meant for integer dtypes, allowed for any.  An unknown filter name raises ValueError, naming the stream."""
    sizes = batch.out_sizes
    if sizes is None:
        raise RuntimeError("no outputs: no decode call on this batch object yet, or its launch has not been waited for")
    if len(specs) != len(sizes):
        raise ValueError("specs: %d entries for the %d streams of the last decode call" % (len(specs), len(sizes)))
    slots, widths, filters, total = [], [], [], 0
    for i, spec in enumerate(specs):
        if spec is None:
            slots.append(None); widths.append(1); filters.append(())
            continue
        dtype, shape = spec[0], spec[1]
        flt = tuple(spec[2]) if len(spec) > 2 else ("shuffle",)
        for name in flt:
            if name not in FILTERS:
                raise ValueError("stream %d: unknown filter %r (known: %s)" % (i, name, ", ".join(FILTERS)))
        shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty(0, dtype=dtype).element_size()
        if item not in (1, 2, 4, 8):
            raise ValueError("stream %d: elements of %d bytes (%s) cannot be unshuffled" % (i, item, dtype))
        want = _numel(shape) * item
        if sizes[i] != want:
            raise ValueError("stream %d: %d delivered bytes, but %s of shape %s is %d" % (i, sizes[i], dtype, shape, want))
        slots.append((total, want, dtype, shape)); widths.append(item); filters.append(flt)
        total = (total + want + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN
    buf = torch.empty(total + SLOT_ALIGN, dtype=torch.uint8, device="cuda")
    skip = -buf.data_ptr() % SLOT_ALIGN   # (the allocator's blocks are aligned far beyond this; nothing here depends on it)
    buf = buf[skip:skip + total]
    base = buf.data_ptr()
    # (a slot of no bytes has a pointer too: a NULL one would mean "skip", which is the same here)
    at = [None if s is None else base + s[0] for s in slots]
    # the unshuffle call: every wanted stream but those that are deltas only; without "shuffle" it is a copy -- width 1
    plain = [i for i, s in enumerate(slots) if s is not None and "shuffle" not in filters[i] and "delta" in filters[i]]
    batch.unshuffle_outputs([None if i in plain else p for i, p in enumerate(at)], [w if "shuffle" in f else 1 for w, f in zip(widths, filters)])
    if plain:   # deltas only: from the outputs straight into the slots
        batch.undelta_outputs([p if i in plain else None for i, p in enumerate(at)], widths)
    both = [i for i, s in enumerate(slots) if s is not None and "shuffle" in filters[i] and "delta" in filters[i]]
    if both:    # in place over the slots, which are 64-byte aligned
        batch.undelta_segments([at[i] for i in both], [at[i] for i in both], [slots[i][1] for i in both], [widths[i] for i in both])
    return [None if s is None else buf[s[0]:s[0] + s[1]].view(s[2]).reshape(s[3]) for s in slots]
