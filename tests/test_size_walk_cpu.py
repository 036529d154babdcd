"""The size walk on the host (BrotliAmdDebugSizeWalk: csrc/brotli_size_walk.h, the function the device runs a lane a stream) against the CPU
oracle, and the new names of batch.h.  A hint's contract (batch.h): `bytes` is a lower bound for every stream that decodes, the exact
size where exact == 1 and status == 0, and status == 2 only where the decoder reports an error."""
import os
import re

import pytest

import oracle_lib as oracle
import size_streams as ss
import san_program
from conftest import ROOT

E = ss.E
NEW_SYMBOLS = ["BrotliAmdBatchSizeHints", "BrotliAmdDebugSizeWalk", "BrotliAmdBatchDecodeDevicePacked", "BrotliAmdBatchPackedOutput",
               "BrotliAmdBatchPackedFetch", "BrotliAmdBatchDecodeHostPacked", "BrotliAmdBatchLastPackedLaunches", "BrotliAmdBatchLastPackedCopies"]

_oracle = {}


def _expected(data, cap):
    """the oracle's (result, decoded_size) with room for the whole stream, once per stream: `cap` is where it starts, and grows while the
    oracle asks for more output"""
    key = (bytes(data), cap)
    if key not in _oracle:
        info, _ = oracle.decode(data, cap, oracle.FLAG_LARGE_WINDOW)
        while info.result == oracle.RESULT_NEEDS_MORE_OUTPUT:
            cap *= 4
            info, _ = oracle.decode(data, cap, oracle.FLAG_LARGE_WINDOW)
        _oracle[key] = (info.result, info.decoded_size)
    return _oracle[key]


def _holds(h, data, cap, what):
    """the bounds of a hint against the oracle's decode into `cap` bytes (enough for the whole stream) -> whether the stream was sized exactly"""
    result, size = _expected(data, cap)
    assert result != oracle.RESULT_NEEDS_MORE_OUTPUT
    assert h.walked_in <= len(data) and h.status in (0, 1, 2) and h.exact in (0, 1), (what, h.astuple())
    if result == oracle.RESULT_SUCCESS:
        assert h.bytes <= size, (what, h.astuple(), size)
        if h.exact == 1 and h.status == 0:
            assert h.bytes == size, (what, h.astuple(), size)
    if h.status == 2:
        assert result == oracle.RESULT_ERROR, (what, h.astuple(), result)
    return result == oracle.RESULT_SUCCESS and h.exact == 1 and h.status == 0


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "brotli", "batch.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"BROTLI_DEC_API\s+[^;()]*\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
        assert name in pkg.BATCH_H_SYMBOLS, name
    assert "typedef struct BrotliAmdSizeHint" in header
    import ctypes
    assert ctypes.sizeof(pkg.SizeHint) == 24


def test_golden_corpus(pkg):
    exact = {}
    for which in ("testdata", "emitter", "param_corpus"):
        exact[which] = 0
        for name, data, size in ss.corpus(which):
            h = pkg.size_walk(data)
            exact[which] += _holds(h, data, (size if size is not None else 1 << 20) + 64, (which, name))
    print("streams sized exactly:", exact)
    assert exact["testdata"] >= 40, exact


def test_empty_input(pkg):
    assert pkg.size_walk(b"").astuple() == (0, 0, 0, 1)


def test_long_walk(pkg):
    stream, raw, at = ss.long_walk_stream()
    assert _expected(stream, len(raw) + 64) == (oracle.RESULT_SUCCESS, len(raw))
    h = pkg.size_walk(stream)
    assert h.astuple() == (len(raw), at, 1, 0), (h.astuple(), len(raw), at)


def test_prefixes(pkg):
    """every prefix: the input ended inside the walk, or the bounds hold for the prefix as a stream of its own"""
    long_stream, raw, _ = ss.long_walk_stream()
    for what, stream, cap in [("long", long_stream, len(raw) + 64)] + [(n, ss.golden(n), 4096) for n in ss.SHORT_GOLDEN]:
        assert what == "long" or len(stream) < 100
        for n in range(len(stream) + 1):
            h = pkg.size_walk(stream[:n])
            assert h.walked_in <= n, (what, n, h.astuple())
            if h.status != 1:
                _holds(h, stream[:n], cap, (what, n))
        assert pkg.size_walk(stream).status == 0


def _header(bits):
    """a stream of the given header bits [(value, nbits)] and an empty last metablock"""
    w = E.BitWriter()
    for v, k in bits:
        w.put(v, k)
    E.emit_last_empty(w)
    return w.finish()


def test_every_wbits_encoding(pkg):
    cases = []
    for wbits in range(10, 25):
        w = E.BitWriter(); E.write_stream_header(w, wbits); E.emit_last_empty(w)
        cases.append(("standard %d" % wbits, w.finish()))
    for wbits in range(0, 64):   # the large-window form: 0010001, a zero, six bits (10 .. 30 are valid)
        cases.append(("large %d" % wbits, _header([(1, 1), (0, 3), (1, 3), (0, 1), (wbits, 6)])))
    cases.append(("reserved", _header([(1, 1), (0, 3), (1, 3), (1, 1), (20, 6)])))   # ... with a one behind it: reserved
    seen = set()
    for flags in (oracle.FLAG_LARGE_WINDOW, 0):
        for what, stream in cases:
            info, _ = oracle.decode(stream, 64, flags)
            h = pkg.size_walk(stream, flags)
            assert (h.status == 2) == (info.result == oracle.RESULT_ERROR), (what, flags, h.astuple(), info.result, info.error_code)
            if info.result == oracle.RESULT_SUCCESS:
                assert h.astuple() == (0, len(stream), 1, 0), (what, flags, h.astuple())
            seen.add((what.split()[0], flags, h.status))
    # valid and rejected forms of each kind were among them
    assert {("standard", 1, 0), ("standard", 0, 0), ("large", 1, 0), ("large", 1, 2), ("large", 0, 2), ("reserved", 1, 2), ("reserved", 0, 2)} <= seen, seen


def test_walk_under_sanitizers(pkg, tmp_path):
    """tests/tools/size_walk_san.cpp: every prefix of the streams from an exactly-sized heap block, under ASan and UBSan, as a program of its own"""
    files = []
    for k, stream in enumerate([ss.long_walk_stream()[0]] + [ss.golden(n) for n in ss.SHORT_GOLDEN] + [ss.golden("empty.compressed.17")[:3000]]):
        files.append(str(tmp_path / ("s%d.br" % k)))
        open(files[-1], "wb").write(stream)
    r = san_program.run("size_walk_san", tmp_path, files)
    assert "walks" in r.stdout
