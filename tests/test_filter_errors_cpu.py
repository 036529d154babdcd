"""The refusals of the four element filters (unshuffle, undelta, bit-unshuffle, bit-unpack) that need no device, each with the literal text it
leaves in last_error(): the host hooks with a bad width, block, bits, flags, count, source length or skew, and the *Segments / *Outputs entry
points with a NULL batch and with NULL arrays."""
import ctypes

import pytest

SRC = bytes(range(64))


def _refused(pkg, rc, text):
    assert rc < 0, rc
    assert pkg.last_error() == text


def _bufs(n=64):
    return ctypes.create_string_buffer(SRC, 64), ctypes.create_string_buffer(b"\x77" * n, n)


@pytest.mark.parametrize("width", [0, 3, 5, 16, 255])
def test_unshuffle_hook_width(pkg, width):
    src, dst = _bufs()
    _refused(pkg, pkg.load_library().BrotliAmdDebugUnshuffleHost(width, ctypes.addressof(src), 64, ctypes.addressof(dst), 0, 0),
             "unshuffle width is not 1, 2, 4 or 8")
    assert dst.raw == b"\x77" * 64


def test_unshuffle_hook_arguments(pkg):
    L = pkg.load_library()
    src, dst = _bufs()
    for args in ((4, ctypes.addressof(src), 64, ctypes.addressof(dst), 16, 0), (4, ctypes.addressof(src), 64, ctypes.addressof(dst), 0, 16),
                 (4, None, 64, ctypes.addressof(dst), 0, 0), (4, ctypes.addressof(src), 64, None, 0, 0)):
        _refused(pkg, L.BrotliAmdDebugUnshuffleHost(*args), "invalid unshuffle arguments")
    assert dst.raw == b"\x77" * 64
    # the width is looked at first
    _refused(pkg, L.BrotliAmdDebugUnshuffleHost(3, None, 64, None, 16, 16), "unshuffle width is not 1, 2, 4 or 8")


def _undelta(pkg, segs, src_size=64, dst_size=64, ss=0, ds=0, in_place=0, arrays=True, src=True, dst=True):
    L = pkg.load_library()
    s, d = _bufs()
    n = len(segs)
    cols = [(ctypes.c_uint64 * max(1, n))(*[sg[c] for sg in segs]) for c in range(3)]
    a_w = (ctypes.c_uint8 * max(1, n))(*[sg[3] for sg in segs])
    rc = L.BrotliAmdDebugUndeltaHost(n, ctypes.addressof(s) if src else None, src_size, ctypes.addressof(d) if dst else None, dst_size,
                                     cols[0] if arrays else None, cols[1], cols[2], a_w, ss, ds, 0, 0, in_place)
    assert rc == 0 or d.raw == b"\x77" * 64
    return rc


def test_undelta_hook(pkg):
    assert _undelta(pkg, [(0, 0, 64, 4)]) == 0
    for width in (0, 3, 5, 16, 255):
        _refused(pkg, _undelta(pkg, [(0, 0, 64, 4), (0, 0, 8, width)]), "undelta width is not 1, 2, 4 or 8")
    for kw in (dict(ss=16), dict(ds=16), dict(arrays=False), dict(src=False), dict(dst=False), dict(in_place=1, src_size=32)):
        _refused(pkg, _undelta(pkg, [(0, 0, 8, 4)], **kw), "invalid undelta arguments")
    for seg in ((0, 0, 65, 1), (0, 60, 8, 1), (60, 0, 8, 1)):
        _refused(pkg, _undelta(pkg, [seg]), "invalid undelta arguments: a segment outside its buffer")
    _refused(pkg, _undelta(pkg, [(0, 2, 8, 4)], in_place=1), "undelta in place at an address that is not a multiple of the width")
    _refused(pkg, _undelta(pkg, [(0, 0, 8, 4)], ds=1, in_place=1), "undelta in place at an address that is not a multiple of the width")


def test_bitunshuffle_hook(pkg):
    L = pkg.load_library()
    src, dst = _bufs()
    a_s, a_d = ctypes.addressof(src), ctypes.addressof(dst)
    assert L.BrotliAmdDebugBitUnshuffleHost(4, 0, a_s, 64, a_d, 0, 0, None) == 0
    src, dst = _bufs()
    a_s, a_d = ctypes.addressof(src), ctypes.addressof(dst)
    for width in (0, 3, 5, 16, 255):
        _refused(pkg, L.BrotliAmdDebugBitUnshuffleHost(width, 0, a_s, 64, a_d, 0, 0, None), "bit-unshuffle width is not 1, 2, 4 or 8")
    for block in (1, 7, 9, 12, (1 << 32) - 1):
        _refused(pkg, L.BrotliAmdDebugBitUnshuffleHost(4, block, a_s, 64, a_d, 0, 0, None), "bit-unshuffle block_elems is neither 0 nor a multiple of 8")
    # the width is looked at in front of the block, both in front of the rest
    _refused(pkg, L.BrotliAmdDebugBitUnshuffleHost(3, 1, None, 64, None, 16, 16, None), "bit-unshuffle width is not 1, 2, 4 or 8")
    _refused(pkg, L.BrotliAmdDebugBitUnshuffleHost(4, 1, None, 64, None, 16, 16, None), "bit-unshuffle block_elems is neither 0 nor a multiple of 8")
    for args in ((4, 8, a_s, 64, a_d, 16, 0), (4, 8, a_s, 64, a_d, 0, 16), (4, 8, None, 64, a_d, 0, 0), (4, 8, a_s, 64, None, 0, 0)):
        _refused(pkg, L.BrotliAmdDebugBitUnshuffleHost(*args, None), "invalid bit-unshuffle arguments")
    assert dst.raw == b"\x77" * 64


def _bitunpack(pkg, bits, width, flags, count, src_len=64, ss=0, ds=0, src=True, dst=True):
    s, d = _bufs(1024)
    rc = pkg.load_library().BrotliAmdDebugBitUnpackHost(bits, width, flags, ctypes.addressof(s) if src else None, src_len, count,
                                                        ctypes.addressof(d) if dst else None, ss, ds, None)
    assert rc == 0 or d.raw == b"\x77" * 1024
    return rc


def test_bitunpack_hook_shape(pkg):
    assert _bitunpack(pkg, 3, 1, 0, 8) == 0
    shape = "bit-unpack segment 0: %s (bits %d, width %d, flags %d)"
    for width in (0, 3, 5, 16, 255):
        _refused(pkg, _bitunpack(pkg, 1, width, 0, 8), shape % ("width is not 1, 2, 4 or 8", 1, width, 0))
    for width in (1, 8):
        _refused(pkg, _bitunpack(pkg, 0, width, 0, 8), shape % ("field of 0 bits", 0, width, 0))
    for bits, width in ((9, 1), (17, 2), (33, 4), (65, 8), (255, 8)):
        _refused(pkg, _bitunpack(pkg, bits, width, 0, 8), shape % ("field is wider than the element", bits, width, 0))
    for flags in (4, 8, 128, 255, 1 << 31):
        _refused(pkg, _bitunpack(pkg, 3, 1, flags, 8), shape % ("unknown flag bits", 3, 1, flags))
    # in this order: width, bits, flags
    _refused(pkg, _bitunpack(pkg, 0, 3, 4, 8), shape % ("width is not 1, 2, 4 or 8", 0, 3, 4))
    _refused(pkg, _bitunpack(pkg, 0, 1, 4, 8), shape % ("field of 0 bits", 0, 1, 4))


def test_bitunpack_hook_count_and_source(pkg):
    for count in ((1 << 56) + 1, 1 << 63, (1 << 64) - 1):
        _refused(pkg, _bitunpack(pkg, 1, 1, 0, count), "bit-unpack segment 0: a count of %d elements is above 2^56" % count)
    assert _bitunpack(pkg, 3, 1, 0, 170) == 0   # 64 bytes hold 170 fields of 3 bits
    _refused(pkg, _bitunpack(pkg, 3, 1, 0, 171), "bit-unpack segment 0: 171 fields of 3 bits need 65 source bytes, and there are 64")
    _refused(pkg, _bitunpack(pkg, 8, 1, 0, 1, src_len=0), "bit-unpack segment 0: 1 fields of 8 bits need 1 source bytes, and there are 0")
    _refused(pkg, _bitunpack(pkg, 64, 8, 0, 1 << 56, src_len=1 << 59), "bit-unpack on the host: more than 2^40 destination bytes")
    # the shape and the count are looked at in front of the rest
    _refused(pkg, _bitunpack(pkg, 3, 1, 0, 171, ss=16, src=False), "bit-unpack segment 0: 171 fields of 3 bits need 65 source bytes, and there are 64")


def test_bitunpack_hook_arguments(pkg):
    for kw in (dict(ss=16), dict(ds=16), dict(ss=255, ds=3), dict(src=False), dict(dst=False)):
        _refused(pkg, _bitunpack(pkg, 3, 1, 0, 8, **kw), "invalid bit-unpack arguments")


def _arrays():
    """one segment's columns, none of which is looked at by a call that is refused"""
    return dict(ptr=(ctypes.c_void_p * 1)(16), size=(ctypes.c_size_t * 1)(0), u8=(ctypes.c_uint8 * 1)(4), u32=(ctypes.c_uint32 * 1)(0),
                u64=(ctypes.c_uint64 * 1)(0))


@pytest.mark.parametrize("name,text", [("Unshuffle", "invalid unshuffle arguments"), ("Undelta", "invalid undelta arguments")])
def test_width_entry_points(pkg, name, text):
    L, a = pkg.load_library(), _arrays()
    segments, outputs = getattr(L, "BrotliAmdBatch%sSegments" % name), getattr(L, "BrotliAmdBatch%sOutputs" % name)
    _refused(pkg, segments(None, 1, a["ptr"], a["ptr"], a["size"], a["u8"], None), text)
    _refused(pkg, segments(None, 0, None, None, None, None, None), text)
    _refused(pkg, outputs(None, a["ptr"], a["u8"]), text)
    _refused(pkg, outputs(None, None, None), text)
    assert getattr(L, "BrotliAmdBatchLast%sMs" % name)(None) == 0.0


def test_bitunshuffle_entry_points(pkg):
    L, a, text = pkg.load_library(), _arrays(), "invalid bit-unshuffle arguments"
    _refused(pkg, L.BrotliAmdBatchBitUnshuffleSegments(None, 1, a["ptr"], a["ptr"], a["size"], a["u8"], a["u32"], None), text)
    _refused(pkg, L.BrotliAmdBatchBitUnshuffleSegments(None, 0, None, None, None, None, None, None), text)
    _refused(pkg, L.BrotliAmdBatchBitUnshuffleOutputs(None, a["ptr"], a["u8"], a["u32"]), text)
    _refused(pkg, L.BrotliAmdBatchBitUnshuffleOutputs(None, None, None, None), text)
    assert L.BrotliAmdBatchLastBitUnshuffleMs(None) == 0.0


def test_bitunpack_entry_points(pkg):
    L, a, text = pkg.load_library(), _arrays(), "invalid bit-unpack arguments"
    _refused(pkg, L.BrotliAmdBatchBitUnpackSegments(None, 1, a["ptr"], a["size"], a["ptr"], a["u64"], a["u8"], a["u8"], None, None), text)
    _refused(pkg, L.BrotliAmdBatchBitUnpackSegments(None, 0, None, None, None, None, None, None, None, None), text)
    _refused(pkg, L.BrotliAmdBatchBitUnpackOutputs(None, a["ptr"], None, a["u8"], a["u8"], None), text)
    _refused(pkg, L.BrotliAmdBatchBitUnpackOutputs(None, None, None, None, None, None), text)
    assert L.BrotliAmdBatchLastBitUnpackMs(None) == 0.0
    assert L.BrotliAmdBatchLastUndeltaPhaseMs(None, 1) == 0.0
