"""tests/golden/emitter_copies/ (tools/make_copy_vectors.py): the committed streams and the oracle's answers for them.
Shared by test_emitter_copies_cpu.py and test_gpu_copies.py."""
import os
import random

import path_harness as H
from conftest import ROOT
from path_harness import expected  # noqa: F401  ((stream, capacity, flags=0) -> the oracle's answer, computed once -- answers of more than 4 MiB are not kept)

DIR = os.path.join(ROOT, "tests", "golden", "emitter_copies")
MAX_FILE, MAX_PARTS = H.store.MAX_FILE, H.store.MAX_PARTS


def load():
    """[(manifest entry, stream)] in the manifest's order"""
    return H.store.load(DIR)


SPLIT = 26  # (leg_set: the second batch starts here)


def wide_set():
    """the streams of window 24 -- S2 and D under (0, 0) and (3, 120), 17 to 22 MB of output each -- which go through three of the
    paths in a test of their own -> [(label, stream, capacity, 0, None)]"""
    by = {e["label"]: (e, c) for e, c in load()}
    out = [(label, by[label][1], by[label][0]["size"], 0, None) for label in ("S2-wide-fields-cf", "S2-wide-fields-ctx", "D-p0-d0-cf", "D-p0-d0-ctx", "D-p3-d120-cf", "D-p3-d120-ctx")]
    return out + [("S2-wide-fields-cf/half", by["S2-wide-fields-cf"][1], by["S2-wide-fields-cf"][0]["size"] // 2, 0, None)]


def leg_set():
    """the streams that go through every command path of the device (test_gpu_copies.py): S1, M in both orders, T under its
    three plans, H and W whole, D for the seven parameter pairs of window 18, and short / half / cut / flipped copies of a few
    (wide_set has S2 and the other two pairs) -> [(label, stream, capacity, 0, None)].  Positions 0 and SPLIT hold T's long form, so that
    each part of the set, decoded as a batch of its own, is one that gets gangs of blocks."""
    out = []
    take = H.take({e["label"]: (e, c) for e, c in load()}, random.Random(61), out)
    take("T2-text-long-cf")
    for label in ("S1a-symbols", "S1b-symbols", "M-rows-w22", "M-mixed-w22", "T-text", "H-chains", "W-edge-w10", "W-edge-w11", "W-edge-w16"):
        take(label + "-cf"); take(label + "-ctx")
    take("T-text-cf4"); take("M-rows-w16-cf"); take("M-mixed-w16-ctx")
    for k, label in enumerate(("D-p0-d15", "D-p1-d0", "D-p1-d2", "D-p1-d30")):
        take(label + ("-ctx" if k & 1 else "-cf"))
    assert len(out) == SPLIT, len(out)
    take("T2-text-long-cf", "short")
    for k, label in enumerate(("D-p2-d4", "D-p2-d60", "D-p3-d8")):
        take(label + ("-ctx" if k & 1 else "-cf"))
    take("M-rows-w16-ctx"); take("M-mixed-w16-cf"); take("L-n64-d64-cf"); take("L-n1025-d5000-ctx"); take("L-n3000-d1-cf")
    take("T-text-cf", "short"); take("T-text-ctx", "half"); take("M-mixed-w22-cf", "half"); take("H-chains-cf", "short"); take("S1b-symbols-ctx", "half")
    take("S1a-symbols-cf", damage="cut"); take("M-rows-w22-ctx", damage="flip"); take("T-text-cf4", damage="flip"); take("H-chains-ctx", damage="flip")
    take("W-edge-w16-cf", damage="cut"); take("D-p2-d60-cf", damage="flip"); take("T2-text-long-cf", damage="flip")
    assert len(out) <= 62, len(out)
    return out
