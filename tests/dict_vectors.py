"""tests/golden/emitter_dict/ (tools/make_dict_vectors.py): the committed streams, their dictionaries -- made again from the seed the
manifest holds -- and the oracle's answers for them.  Shared by test_emitter_dict_cpu.py and test_gpu_dict_paths.py."""
import hashlib
import os
import random

import path_harness as H
from conftest import ROOT

import dict_gen  # noqa: I100  (tools/, which path_harness has put on the path)

DIR = os.path.join(ROOT, "tests", "golden", "emitter_dict")
MAX_FILE, MAX_PARTS = H.store.MAX_FILE, H.store.MAX_PARTS
ALPHABET = "etaoinshrdlucmfwypvbgkqjxz ,.0123456789"   # (tools/make_dict_vectors.py ALPHABET)

_dicts = {}


def dictionary(seed, size):
    """tools/make_dict_vectors.dictionary, stated again: one object per (seed, size), so that a batch uploads a shared one once"""
    if (seed, size) not in _dicts:
        _dicts[(seed, size)] = dict_gen.text(random.Random(seed), size + 8, ALPHABET, 400)[:size]
    return _dicts[(seed, size)]


_loaded = []


def load():
    """[(manifest entry, stream, dictionary)] in the manifest's order"""
    if not _loaded:
        shas = {(x["seed"], x["size"]): x["sha256"] for x in H.store.manifest(DIR)["dictionaries"]}
        for e, comp in H.store.load(DIR):
            d = dictionary(*e["dict"])
            assert len(d) == e["dict"][1] and hashlib.sha256(d).hexdigest() == shas[tuple(e["dict"])], e["label"]
            _loaded.append((e, comp, d))
    return list(_loaded)


def expected(data, cap, dictionary, flags=0):
    """the oracle's answer with the dictionary, computed once (path_harness.expected)"""
    return H.expected(data, cap, flags, dictionary)


SPLIT = 32  # (leg_set: the second batch starts here; 32 streams a batch: more, and a launch's gangs are of four blocks)
CARRIERS = ("F-T-cf", "F-T-ctx", "F-T-cf4", "F-C-cf", "F-C-ctx", "F-T2-long-cf", "F-S-cf", "F-S-ctx", "F-W-cf", "F-W-ctx")


def leg_set():
    """the streams that go through every command path of the device (test_gpu_dict_paths.py): the carriers F, the matrices of A for
    eight dictionary sizes, B, C, D, E and G in samples, invalid ones, and short / half / cut / flipped copies of a few
    -> [(label, stream, capacity, 0, dictionary)].  Positions 0 and SPLIT hold F's long form, so that each part of the set, decoded as
    a batch of its own, is one that gets gangs of blocks."""
    out = []
    take = H.take({e["label"]: (e, c, d) for e, c, d in load()}, random.Random(62), out, named_tag=True)
    take("F-T2-long-cf")
    for label in CARRIERS[:5]:
        take(label)
    for size in (1, 15, 16, 17, 300, 70000):
        take("A-matrix-D%d-cf" % size); take("A-matrix-D%d-ctx" % size)
    for label in ("C-regimes-cf", "C-regimes-ctx", "C-run-cf", "C-last-words-ctx", "C-edge-w22-D300-cf", "C-edge-w10-D2500-ctx", "B-w16-D60000-cf", "B-w16-D60000-ctx",
                  "G-n2-b1-cf", "G-n40-b17-ctx", "G-n300-b64-cf", "G-n3000-b1025-ctx", "E-mode0-ctx", "E-mode3-ctx"):
        take(label)
    assert len(out) == SPLIT, len(out)
    take("F-T2-long-cf", "short")
    for label in ("E-mode1-ctx", "E-mode2-ctx", "A-matrix-D1026-cf", "A-matrix-D1037-ctx", "A-overrun-w22-cf", "A-overrun-w10-cross-ctx", "C-transform-n11-cf",
                  "C-dictionary-n25-regime2-cf"):
        take(label)
    small = [e["label"] for e, _, _ in load() if e["label"].startswith(("B-D", "D-w"))]
    for label in small[::14][:12]:   # (twelve of B's and D's small streams)
        take(label)
    take("F-S-cf"); take("F-S-ctx"); take("F-W-cf"); take("F-W-ctx")
    take("F-T-cf", "short"); take("F-T-ctx", "half"); take("F-C-cf", "half")
    take("F-T-cf", damage="cut"); take("F-C-ctx", damage="flip"); take("F-T-cf4", damage="flip"); take("F-T2-long-cf", damage="flip")
    assert len(out) == 2 * SPLIT, len(out)
    return out
