"""Streams for the tests of the size walk and the packed decode (test_size_walk_cpu.py, test_gpu_packed.py): the golden corpora as
(label, bytes, decoded size or None), and emitter streams made for the walk (tools/brotli_emit.py, seeded)."""
import json
import os
import random
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SHORT_GOLDEN = ("10x10y.compressed", "quickfox.compressed", "ukkonooa.compressed")   # three streams of under 100 bytes

_cache = {}


def corpus(which):
    """every stream file of tests/golden/<which> -> [(name, bytes, the manifest's decoded size or None)]"""
    if which not in _cache:
        d = os.path.join(GOLD, which)
        sizes = {e.get("name") or e.get("file"): e.get("size") for e in json.load(open(os.path.join(GOLD, "manifest.json" if which == "testdata" else which + "/manifest.json")))}
        _cache[which] = [(n, open(os.path.join(d, n), "rb").read(), sizes.get(n)) for n in sorted(os.listdir(d)) if not n.endswith(".json")]
    return _cache[which]


def golden(name):
    return next(d for n, d, _ in corpus("testdata") if n == name)


def long_walk_stream():
    """70 stored metablocks of 1 .. 300 bytes between metadata blocks (empty ones among them), then a compressed last metablock
    -> (stream, raw bytes, byte offset of the compressed metablock's header)"""
    if "long" not in _cache:
        rnd = random.Random(70)
        w = E.BitWriter(); E.write_stream_header(w, 18)
        raw = bytearray()
        for k in range(70):
            for _ in range(rnd.randrange(0, 3)):
                E.emit_metadata(w, bytes(rnd.randrange(256) for _ in range(rnd.choice([0, 0, 1, 2, 17, 255, 256, 300]))))
            part = bytes(rnd.randrange(256) for _ in range(1 + (k * 37 + rnd.randrange(300)) % 300))
            E.emit_stored(w, part); raw += part
        E.emit_metadata(w, b"")
        at = len(w.out)   # (the header begins in the byte that is not yet written out)
        tail = (b"the quick brown fox jumps over the lazy dog, " * 40)[:1500]
        got = E.emit_compressed(w, E.greedy_commands(tail, max_dist=1000, history=b""), E.Plan(), True, prev=bytes(raw))
        assert got == tail
        raw += tail
        _cache["long"] = (w.finish(), bytes(raw), at)
    return _cache["long"]


def growing_stream():
    """three compressed metablocks of about 200 KiB each of repeated data: a few hundred compressed bytes, so that a first guess of
    six times the input is the 64 KiB floor -> (stream, raw bytes)"""
    if "grow" not in _cache:
        w = E.BitWriter(); E.write_stream_header(w, 22)
        raw = b""
        for k in range(3):
            unit = bytes([65 + k]) + b"0123456789abcdef" * 4
            n = (200 << 10) + 1000 * k + 7
            # literals of one unit, then copies of at most 2000 bytes at the unit's distance
            cmds, left = [(unit, min(2000, n - len(unit)), len(unit))], n - len(unit) - min(2000, n - len(unit))
            while left:
                c = min(2000, left) if left - min(2000, left) != 1 else 1999   # (no copy of one byte)
                cmds.append((b"", c, len(unit))); left -= c
            raw += E.emit_compressed(w, cmds, E.Plan(), k == 2, prev=raw)
        _cache["grow"] = (w.finish(), raw)
    return _cache["grow"]
