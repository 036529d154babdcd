"""tests/golden/emitter_headers/ (tools/make_header_vectors.py): the committed streams and the oracle's answers for them.
Shared by test_emitter_headers_cpu.py and test_gpu_headers.py."""
import os
import random

import oracle_lib as oracle
import path_harness as H
from conftest import ROOT
from path_harness import expected  # noqa: F401  ((stream, capacity, flags=0) -> the oracle's answer, computed once -- answers of more than 4 MiB are not kept)

DIR = os.path.join(ROOT, "tests", "golden", "emitter_headers")
MAX_FILE, MAX_PARTS = H.store.MAX_FILE, H.store.MAX_PARTS
FLAG_LARGE_WINDOW = oracle.FLAG_LARGE_WINDOW


_loaded = []


def load():
    """[(manifest entry, stream)] in the manifest's order.  An entry as the manifest has it names what cannot be derived; here it
    gets "family" (the label's first letter), "window" (22 unless named), "large", "valid" (no "oracle" triple: the answer is
    (1, 1, size)) and "oracle" filled in.  Streams of less than 256 bytes lie end to end in small.N.bin, at offset "at"."""
    if not _loaded:
        for e, comp in H.store.load(DIR):
            e = dict(e, family=e["label"][0], window=e.get("window", 22), large=e.get("large", False), valid="oracle" not in e)
            e.setdefault("oracle", [1, 1, e["size"]])
            _loaded.append((e, comp))
    return list(_loaded)


def flags_of(e):
    """the flags under which the manifest's answer holds: a large-window stream needs the flag, the others decode alike with it"""
    return FLAG_LARGE_WINDOW if e["large"] else 0


def big(e):
    """the one vector of 16 MiB of output (M: MLEN = 2^24)"""
    return e["size"] > 1 << 22


def cap_of(e):
    """room for everything a vector puts out (an invalid one delivers at most what lies in front of its fault)"""
    return e["size"] if e["valid"] else e["size"] + 64


SPLIT = 30  # (leg_set: the second batch starts here)


def leg_set():
    """the streams that go through every command path of the device (test_gpu_headers.py): B's long form and its every-length-code
    streams, the mixed trivial / non-trivial maps, the 256-type vectors, P and C vectors of every kind, valid and not, and short /
    cut / flipped copies of a few -> [(label, stream, capacity, flags, None)].  Positions 0 and SPLIT hold a stream of more than 64 KiB
    (M's metadata block of 65 537 bytes: the size from which a launch forms gangs)."""
    out = []
    take = H.take({e["label"]: (e, c) for e, c in load()}, random.Random(62), out, flags_of)
    take("M-metadata-65537")
    for label in ("B-long", "B-lit-every-length-code", "B-cmd-every-length-code", "B-dist-every-length-code", "C-some-types-trivial", "C-all-trivial-and-different",
                  "B-lit-n256-ring", "B-cmd-n256-ring", "B-dist-n256-direct", "B-lit-n255-direct", "B-ones-all", "C-lit-n256-r16", "C-dist-n256-r16", "C-runs-1-8",
                  "C-run-c13-ones", "C-imtf-big-r9", "C-imtf-every-tree-r0", "C-code-repeats", "C-dist-each-context-its-tree", "P-lit-one-16", "P-lit-one-8",
                  "P-cmd-depth-sixteens", "P-lit-depth-plain", "P-cmd-16chain-k5-e3", "P-cmd-17chain-k4-e0", "P-lit-sweep00", "P-cmd-sweep01", "P-dlw-sweep02",
                  "P-d520-end-at-max-symbol"):
        take(label)
    assert len(out) == SPLIT, len(out)
    take("M-metadata-65537", "short")
    for label in ("P-lit-V-seventeens-21", "P-cmd-V-seventeens-16", "P-lit-V-repeat-one-beyond", "P-dlw-V-repeat-one-beyond", "P-cmd-V-space-over-by-a-repeat",
                  "P-lit-V-cl-space-left", "P-lit-zeros-behind-the-end", "P-d64-V-simple-same-24", "C-V-run-one-beyond", "C-V-run-c16-ones", "M-V-stored-padding",
                  "M-metadata-run-200x1", "B-lit-last-block-exact-inner", "B-cmd-last-block-exact-inner", "B-dist-last-block-one-short-inner"):
        take(label)
    take("B-long", "short"); take("B-long", "half"); take("C-some-types-trivial", "short"); take("B-cmd-n256-ring", "half")
    take("B-long", damage="cut"); take("B-long", damage="flip"); take("C-imtf-big-r9", damage="flip"); take("B-lit-n256-ring", damage="flip")
    take("C-runs-1-8", damage="cut"); take("B-dist-every-length-code", damage="flip"); take("M-metadata-65537", damage="flip")
    assert len(out) <= 62, len(out)
    return out
