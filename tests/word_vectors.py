"""tests/golden/emitter_words/ (tools/make_word_vectors.py): the committed streams and the oracle's answers for them.
Shared by test_emitter_words_cpu.py and test_gpu_words.py."""
import os
import random

import path_harness as H
from conftest import ROOT
from path_harness import expected  # noqa: F401  ((stream, capacity, flags=0) -> the oracle's answer, computed once)

DIR = os.path.join(ROOT, "tests", "golden", "emitter_words")


def load():
    """[(manifest entry, stream)] in the manifest's order"""
    return H.store.load(DIR)


SPLIT = 30  # (leg_set: the second batch starts here)


def leg_set():
    """the streams that go through every command path of the device (test_gpu_words.py): every valid vector whole, every
    stream that is invalid on purpose, some of the tiny ones, and short / truncated / damaged copies of a few -> [(label, stream,
    capacity, 0, None)].  Positions 0 and SPLIT hold the long stream, so that each half of the set, decoded as a batch of its own, is
    one that gets gangs of blocks."""
    out = []
    take = H.take({e["label"]: (e, c) for e, c in load()}, random.Random(60), out, random_cap=True)
    take("C2-text-long-cf")
    for label in ("A1-matrix", "A2-multibyte", "B-matrix-w10", "B-matrix-w16", "C-text", "D-chains", "F-boundary", "G-utf8-upper", "H-small"):
        take(label + "-cf"); take(label + "-ctx")
    take("C-text-cf4")
    for label in ("E-p0-code0", "E-p3-code1", "E-p12-code3", "E-code8-beyond1", "E-code15-beyond1", "E-p0-code0-len2", "E-p4-code9-len25"):
        take(label + ("-cf" if len(out) & 1 else "-ctx"))
    take("F-t121-cf"); take("F-t121-ctx"); take("F-tmax-cf")
    assert len(out) == SPLIT, len(out)
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
