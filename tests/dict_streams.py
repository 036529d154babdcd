"""Streams made for a custom (LZ77 prefix) dictionary, and the check of the device's decode of them against the CPU oracle
(brotli_oracle_decode_dict: BrotliState::new_with_custom_dictionary, src/state.rs:400-411).  Shared by test_custom_dict_cpu.py
and test_gpu_custom_dict.py; the generators (tools/dict_gen.py) are seeded and use the repository's own emitter (tools/brotli_emit.py)."""
import ctypes
import json
import os
import random
import sys

import oracle_lib as oracle
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
from dict_gen import context_plan, emit, related, stream_for, text  # noqa: E402,F401  (the generators: shared with tools/dict_batch.py)

GOLD = os.path.join(ROOT, "tests", "golden")


def oracle_decode_dict(data, out_cap, flags, dictionary):
    """-> (OracleInfo, bytes delivered) of the oracle's decode with `dictionary` (None or b"": none)"""
    L = oracle.lib()
    L.brotli_oracle_decode_dict.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                            ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(oracle.OracleInfo)]
    L.brotli_oracle_decode_dict.restype = ctypes.c_int
    out = ctypes.create_string_buffer(max(1, out_cap))
    info = oracle.OracleInfo()
    d = bytes(dictionary) if dictionary else None
    L.brotli_oracle_decode_dict(bytes(data), len(data), out, out_cap, flags, d, len(d) if d else 0, ctypes.byref(info))
    return info, out.raw[:info.decoded_size]


def vectors():
    """the reference's two known-answer vectors (src/test.rs:438-520): [(name, compressed, dictionary, expected)]"""
    return [(v["name"], bytes.fromhex(v["compressed"]), bytes.fromhex(v["dictionary"]), bytes.fromhex(v["expected"]))
            for v in json.load(open(os.path.join(GOLD, "custom_dict_vectors.json")))]


def reaching(cmds_data, dictionary_size):
    """how many of a command list's copies start in front of output position 0"""
    pos, n = 0, 0
    for ins, clen, dist in cmds_data:
        pos += len(ins)
        if clen and dist > pos:
            n += 1
        pos += clen
    return n


def variants(rnd, c, n, damaged=6):
    """a valid stream with exact, short and roomy output buffers, truncated and bit-flipped copies of it
    (test_gpu_engine._variants) -> (datas, caps)"""
    datas, caps = [], []
    for cap in (n, n - 1, n // 2, n + 1000):
        datas.append(c); caps.append(max(0, cap))
    for _ in range(damaged):
        d = bytearray(c)
        if rnd.random() < 0.4:
            d = d[:rnd.randrange(1, len(d))]
        else:
            for _ in range(rnd.choice([1, 1, 2])):
                d[rnd.randrange(0, len(d))] ^= 1 << rnd.randrange(8)
        datas.append(bytes(d)); caps.append(n + 4096)
    return datas, caps


_expected = {}


def expected(data, cap, flags=0, dictionary=None):
    """the oracle's answer, computed once per (stream, capacity, the oracle's two flags, dictionary) -- answers of more than 4 MiB are
    not kept.  The one cache of the suites: brotli_oracle_decode is brotli_oracle_decode_dict without a dictionary."""
    flags &= oracle.FLAG_LARGE_WINDOW | oracle.FLAG_NO_CANNY   # (what else a batch's flags hold is the device's)
    key = (bytes(data), cap, flags, bytes(dictionary) if dictionary else b"")
    if key in _expected:
        return _expected[key]
    got = oracle_decode_dict(data, cap, flags, dictionary)
    if len(got[1]) <= 1 << 22:
        _expected[key] = got
    return got


def first_difference(out, exp):
    """the first byte at which two outputs differ; None: one is the other's beginning"""
    n = min(len(out), len(exp))
    return None if out[:n] == exp[:n] else next(k for k in range(n) if out[k] != exp[k])


def compare(results, outs, datas, caps, dicts, flags, what="", entries=None, where=None):
    """result, error code, decoded_size and every output byte against the oracle; on success consumed, num_commands and
    num_metablocks too (test_gpu_engine._check_against_oracle with dictionaries) -> the mismatches, each with its first differing
    byte; `entries`: the manifest entry of each stream, which names it, and where(entry, byte) what the byte belongs to"""
    bad = []
    for i, (d, cap) in enumerate(zip(datas, caps)):
        info, exp = expected(d, cap, flags, dicts[i] if dicts else None)
        r = results[i]
        ok = (r.result, r.error_code, r.decoded_size, outs[i]) == (info.result, info.error_code, info.decoded_size, exp)
        if ok and info.result == 1:
            ok = r.consumed == info.consumed and r.num_commands == info.num_commands and r.num_metablocks == info.num_metablocks
        if not ok:
            first = first_difference(outs[i], exp)
            e = entries[i] if entries else None
            bad.append((i, what, e and e["label"], (r.result, r.error_code, r.decoded_size), (info.result, info.error_code, info.decoded_size),
                        r.consumed, info.consumed, r.num_commands, info.num_commands, len(d), cap, len(dicts[i]) if dicts and dicts[i] else 0, first,
                        e and where and where(e, first)))
    return bad


def check(pkg, datas, caps, dicts, flags=1, what="", batch=None, entries=None, where=None):
    """decodes the streams in one batch (the caller's, or one of its own) with their dictionaries and compares with the oracle;
    -> the results"""
    b = batch or pkg.Batch(len(datas))
    try:
        results, outs = b.decode_host(datas, caps, flags, dicts=dicts)
    finally:
        if batch is None:
            b.close()
    bad = compare(results, outs, datas, caps, dicts, flags, what, entries, where)
    assert not bad, (len(bad), bad[:8])
    return results
