"""tests/golden/emitter_words/ (tools/make_word_vectors.py): the committed streams and the oracle's answers for them.
Shared by test_emitter_words_cpu.py and test_gpu_words.py."""
import json
import random
import os

import oracle_lib as oracle
from conftest import ROOT

DIR = os.path.join(ROOT, "tests", "golden", "emitter_words")


def load():
    """[(manifest entry, stream)] in the manifest's order"""
    out = []
    for e in json.load(open(os.path.join(DIR, "manifest.json"))):
        if "hex" in e:
            comp = bytes.fromhex(e["hex"])
        else:  # (a stream of more than 64 KiB lies in parts)
            comp = b"".join(open(os.path.join(DIR, name), "rb").read() for name in e.get("files", [e.get("file")]))
        assert len(comp) == e["csize"], e["label"]
        out.append((e, comp))
    return out


_expected = {}


def expected(data, cap, flags=0):
    """the oracle's answer, computed once per (stream, capacity, flags)"""
    key = (data, cap, flags)
    if key not in _expected:
        _expected[key] = oracle.decode(data, cap, flags)
    return _expected[key]


def leg_set():
    """the streams that go through every command path of the device (test_gpu_words.py): every valid vector whole, every
    stream that is invalid on purpose, some of the tiny ones, and short / truncated / damaged copies of a few -> [(label, stream,
    capacity)].  Positions 0 and 30 hold the long stream, so that each half of the set, decoded as a batch of its own, is one
    that gets gangs of blocks."""
    rnd = random.Random(60)
    by = {e["label"]: (e, c) for e, c in load()}
    out = []

    def take(label, cap=None, damage=None):
        e, c = by[label]
        n = e["size"]
        if damage == "cut":
            c = c[:rnd.randrange(len(c) // 2, len(c))]
        elif damage == "flip":
            d = bytearray(c); d[rnd.randrange(len(d) // 3, len(d))] ^= 1 << rnd.randrange(8); c = bytes(d)
        cap = {None: n if e["valid"] and not damage else n + 64, "short": n - 1, "half": n // 2, "random": rnd.randrange(1, max(2, n)), "roomy": n + 1000}.get(cap, cap)
        out.append((label + ("" if cap == n and not damage else "/%s/%s" % (cap, damage)), c, cap))

    take("C2-text-long-cf")
    for label in ("A1-matrix", "A2-multibyte", "B-matrix-w10", "B-matrix-w16", "C-text", "D-chains", "F-boundary", "G-utf8-upper", "H-small"):
        take(label + "-cf"); take(label + "-ctx")
    take("C-text-cf4")
    for label in ("E-p0-code0", "E-p3-code1", "E-p12-code3", "E-code8-beyond1", "E-code15-beyond1", "E-p0-code0-len2", "E-p4-code9-len25"):
        take(label + ("-cf" if len(out) & 1 else "-ctx"))
    take("F-t121-cf"); take("F-t121-ctx"); take("F-tmax-cf")
    assert len(out) == 30, len(out)
    take("C2-text-long-cf", "short")
    take("F-tmax-ctx")
    for label in ("F-len3", "F-len25", "F-ring-zero", "F-ring-minus2", "F-mlen-plus1", "F-mlen-plus1-ring-end"):
        take(label + "-cf"); take(label + "-ctx")
    take("C-text-cf", "short"); take("C-text-ctx", "half"); take("C-text-cf4", "random"); take("A1-matrix-cf", "half"); take("B-matrix-w16-ctx", "short")
    take("D-chains-cf", "random"); take("A2-multibyte-ctx", "roomy"); take("E2-ring-words-deep-cf"); take("E2-ring-words-deep-ctx")
    take("C-text-cf", damage="cut"); take("C-text-ctx", damage="flip"); take("C-text-cf4", damage="flip"); take("C2-text-long-cf", damage="flip")
    take("A1-matrix-cf", damage="flip"); take("B-matrix-w10-cf", damage="cut"); take("D-chains-ctx", damage="flip"); take("B-matrix-w16-cf", damage="flip")
    assert len(out) <= 62, len(out)
    return out
