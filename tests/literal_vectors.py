"""tests/golden/emitter_literals/ (tools/make_literal_vectors.py): the committed streams and the oracle's answers for them.
Shared by test_emitter_literals_cpu.py and test_gpu_literals.py."""
import os
import random

import oracle_lib as oracle
import path_harness as H
from conftest import ROOT
from path_harness import expected  # noqa: F401  ((stream, capacity, flags=0) -> the oracle's answer, computed once)

DIR = os.path.join(ROOT, "tests", "golden", "emitter_literals")
MAX_FILE, MAX_PARTS = H.store.MAX_FILE, H.store.MAX_PARTS
FLAG_LARGE_WINDOW = oracle.FLAG_LARGE_WINDOW


_loaded = []


def load():
    """[(manifest entry, stream)] in the manifest's order.  An entry as the manifest has it names what cannot be derived; here it
    gets "family" (the label's first letter), "window" (22 unless named), "valid" (every vector of this family is) and "oracle"
    filled in.  Streams of less than 256 bytes lie end to end in small.N.bin, at offset "at"."""
    if not _loaded:
        for e, comp in H.store.load(DIR):
            _loaded.append((dict(e, family=e["label"][0], window=e.get("window", 22), large=False, valid=True, oracle=[1, 1, e["size"]]), comp))
    return list(_loaded)


def by_label():
    return {e["label"]: (e, c) for e, c in load()}


def cap_of(e):
    """room for everything a vector puts out"""
    return e["size"]


def where(e, k):
    """what the output byte k of a vector belongs to, out of the manifest: a probe with its cell, or a literal run with the byte's
    number in it; None for anything else (a copy, a word, a literal of a short run)"""
    if k is None:
        return None
    probes = e.get("probes", [])
    for i in range(0, len(probes), 2):
        if probes[i] == k:
            return "probe %s at %d" % (e["cells"][probes[i + 1]], k)
    runs = e.get("runs", [])
    for i in range(0, len(runs), 2):
        if runs[i] <= k < runs[i] + runs[i + 1]:
            return "literal %d of the run of %d at %d" % (k - runs[i], runs[i + 1], runs[i])
    return None


SPLIT = 31  # (leg_set: the second batch starts here)


def leg_set():
    """the streams that go through every command path of the device (test_gpu_literals.py): every shape of S with the sweep in front
    and at the end -- the end vectors' first command is a run of PE_RUN_MIN literals, which a gang declines --, every X vector, E's
    long runs, and short / half / cut / flipped copies of a few -> [(label, stream, capacity, 0, None)].  Positions 0 and SPLIT hold
    streams of more than 64 KiB (the size from which a launch forms gangs), most of it the runs of 40 000 and 2 x PE_RUN_MIN + 1
    literals: the staircase's front vector, and the staircase's long runs behind a first command of PE_RUN_MIN literals (built here by
    the generator, not committed)."""
    by = by_label()
    out = []
    take = H.take(by, random.Random(63), out)
    shapes = ["simple1", "simple2", "simple3", "simple4a", "simple4b", "flat8", "stair", "deep9", "deep10", "deep11", "deep12", "grid"]
    take("S-stair-front")
    for s in shapes:
        if s not in ("stair", "grid"):
            take("S-%s-front" % s)
    for s in shapes:
        take("S-%s-end" % s)
    for label in ("X-lut-mode0", "X-lut-mode1", "X-every-tree", "X-source", "X-words", "X-maps", "X-boundary", "X-words-start"):
        take(label)
    assert len(out) == SPLIT and len(out[0][1]) > 65536, (len(out), len(out[0][1]))
    import make_literal_vectors   # (tools/: the one stream of the set that is not committed, 0.3 s to build)
    b = make_literal_vectors.s_vector("stair", "first", 1099)
    by["S-stair-first"] = ({"label": "S-stair-first", "size": len(b.out), "runs": b.runs, "valid": True}, b.w.finish())
    assert [r["insert"] for r in b.clog][0] >= make_literal_vectors.PE_RUN_MIN
    take("S-stair-first")
    assert len(out[SPLIT][1]) > 65536
    take("S-grid-front")
    for label in ("X-lut-mode2", "X-lut-mode3", "E-stair-block-6100-767-5999", "E-flat8-block-6100-768-6000", "E-stair-block-800-768", "E-flat8-block-800-767",
                  "E-stair-cap-6000", "E-flat8-cap-6000", "E-stair-cap-768", "E-flat8-cap-768", "E-stair-two-800-800", "E-flat8-two-800-800", "E-stair-window10-0",
                  "E-flat8-window10-3", "E-stair-last-130", "E-flat8-last-64", "E-stair-block-130-64", "E-flat8-block-130-17"):
        take(label)
    take("S-stair-front", "short"); take("S-deep12-front", "half"); take("X-source", "short"); take("X-maps", "half"); take("E-stair-cap-6000", "half")
    take("S-grid-end", damage="cut"); take("S-deep11-front", damage="cut"); take("X-every-tree", damage="flip"); take("S-flat8-front", damage="flip")
    take("X-words", damage="flip"); take("S-grid-front", damage="flip")
    assert len(out) <= 62, len(out)
    return out
