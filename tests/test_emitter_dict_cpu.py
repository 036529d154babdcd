"""tests/golden/emitter_dict/ on the CPU: the generator (tools/make_dict_vectors.py) writes the committed bytes again, the oracle's
answer with the dictionary is the manifest's, the emitter's idea of the output equals the oracle's, a stream that reaches its
dictionary does not decode to the same bytes without it, and the emitter's command log shows that the vectors hold what they are
for -- every cell of A .. E and G is looked up in the log (`pos`, `distance`, `max_distance`, `copy_len`, `word`, coding, ring code)
and the sets reached are compared with the sets asked for.  The log is the emitter's; no decoder is asked what a stream contains.
Nothing here skips."""
import collections
import hashlib
import os
import sys

import pytest

import dict_streams
import dict_vectors
import oracle_lib as oracle
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import make_dict_vectors as M  # noqa: E402


@pytest.fixture(scope="module")
def made():
    """{label: vector} as the generator makes them now"""
    return {v["label"]: v for v in M.vectors()}


@pytest.fixture(scope="module")
def committed():
    return dict_vectors.load()


def _copies(log):
    """the log's copies out of the dictionary: they start in front of position 0"""
    return [r for r in log if r["coding"] != "tail" and not r["word"] and r["distance"] > r["pos"]]


def _before(r):
    return r["distance"] - r["pos"]


def test_generator_writes_the_committed_bytes_again(made, committed):
    assert [e["label"] for e, _, _ in committed] == list(made)
    for e, comp, d in committed:
        v = made[e["label"]]
        assert comp == v["comp"], e["label"]
        assert (e["window"], e["kind"], e["valid"], e["dict"]) == (v["window"], v["kind"], v["valid"], [v["dseed"], v["dsize"]]), e["label"]
        assert d == M.dictionary(v["dseed"], v["dsize"]), e["label"]   # (its SHA-256 is the manifest's: dict_vectors.load)
        assert e == M.entry(v, dict_streams.oracle_decode_dict) | {k: e[k] for k in ("hex", "file", "files") if k in e}, e["label"]
        parts = e.get("files", [0])
        assert len(parts) <= dict_vectors.MAX_PARTS and len(comp) <= dict_vectors.MAX_FILE * len(parts), e["label"]
        assert ("hex" in e) == (len(comp) < 256)
    names = {n for e, _, _ in committed for n in e.get("files", [e.get("file")]) if n} | {"manifest.json"}
    assert set(os.listdir(dict_vectors.DIR)) == names
    for name in names:
        assert os.path.getsize(os.path.join(dict_vectors.DIR, name)) <= dict_vectors.MAX_FILE or name == "manifest.json", name
    assert os.path.getsize(os.path.join(dict_vectors.DIR, "manifest.json")) < 1 << 20


def test_the_oracle_the_emitter_and_the_manifest_agree(made, committed):
    """the oracle's answer with the dictionary is the manifest's; for a valid vector its bytes are those the emitter expected (exact-fit
    capacity); a valid vector that reaches its dictionary gives other bytes, or no success, without it"""
    reaching = 0
    for e, comp, d in committed:
        v = made[e["label"]]
        info, out = dict_streams.oracle_decode_dict(comp, e["size"] + 64, 0, d)
        assert [info.result, info.error_code, info.decoded_size] == e["oracle"] and hashlib.sha256(out).hexdigest() == e["sha256"], e["label"]
        if not e["valid"]:
            assert info.result == 0 and info.error_code < 0 and "success" not in e, e["label"]
            continue
        info, out = dict_streams.oracle_decode_dict(comp, e["size"], 0, d)
        assert (info.result, info.error_code, info.decoded_size) == (1, 1, e["size"]) and out == v["raw"], e["label"]
        assert [info.consumed, info.num_commands, info.num_metablocks] == e["success"] and info.consumed == len(comp) and info.num_commands == len(v["log"]), e["label"]
        if _copies(v["log"]):
            reaching += 1
            bare, got = oracle.decode(comp, e["size"], 0)
            assert bare.result != 1 or got != v["raw"], e["label"]
    assert reaching >= 350 and len(committed) >= 500, (reaching, len(committed))


# ------------------------------------------------------------------ A
def test_coverage_of_the_copy_shapes(made):
    """A: per dictionary size every `before` of A_BEFORE in reach and D - 1, D; per `before` a copy that ends in front of position 0, on
    it, one byte behind it and further on; every length of A_LEN; sixteen destination alignments; sixteen residues of the dictionary's
    size; as the first command at every P of A_POS (P = 0 without a literal), where copies repeat themselves at distances below, at
    and above 16; as a metablock's last command with MLEN used up and as the stream's last; MLEN overrun with both error codes"""
    assert {s % 16 for s in M.A_SIZES} == set(range(16)) and {1, 15, 16, 17, 300, 70000} <= set(M.A_SIZES)
    lens, aligns = set(), set()
    for size in M.A_SIZES:
        for kind in ("cf", "ctx"):
            v = made["A-matrix-D%d-%s" % (size, kind)]
            cells = _copies(v["log"])
            assert len(cells) == len(v["log"]) - 1 == len(M.a_cells(size)) + 1 and v["dsize"] == size
            assert all(r["max_distance"] == r["pos"] + size and r["coding"] == "explicit" and r["total"] == r["copy_len"] for r in cells)
            want = ({b for b in M.A_BEFORE if b <= size} | {size - 1, size}) - {0}
            assert {_before(r) for r in cells} == want, size
            assert collections.Counter((_before(r), r["copy_len"]) for r in cells[1:]) == collections.Counter(M.a_cells(size))
            for b in want:
                ns = {r["copy_len"] for r in cells if _before(r) == b}
                assert b + 1 in ns and (b < 2 or b in ns) and (b <= 2 or any(n < b for n in ns)) and (b + 1 >= 3000 or any(n > b + 1 for n in ns)), (size, b, ns)
            assert {r["copy_len"] for r in cells} >= set(M.A_LEN)
            lens |= {r["copy_len"] for r in cells}
            aligns |= {r["pos"] % 16 for r in cells}
            assert len(cells) < 40 or {r["pos"] % 16 for r in cells} == set(range(16)), size
    assert aligns == set(range(16)) and {70000, 70001} <= lens
    # the first command
    first = {l: v for l, v in made.items() if l.startswith("A-first-") and l.endswith("-cf")}
    seen = collections.defaultdict(set)
    forms = collections.Counter()
    for label, v in first.items():
        r = v["log"][0]
        assert r["insert"] == r["pos"] and r in _copies(v["log"]) and v["dsize"] == 300 and ((label[:-2] + "ctx" in made) == ("-lits-" in label))
        seen[(r["pos"], r["distance"])].add(r["copy_len"])
        form = label.split("-")[-2]
        forms[form] += 1
        if form == "last":
            assert len(v["log"]) == 1 and r["pos"] + r["copy_len"] == len(v["raw"])
        elif form == "mbend":
            assert len(v["log"]) == 3 and v["log"][1]["pos"] == r["pos"] + r["copy_len"] + 4   # (another metablock follows: see the manifest's count below)
        else:
            assert v["log"][1]["coding"] == "tail" and v["log"][1]["insert"] == 3 and made[label[:-2] + "ctx"]["raw"] == v["raw"]
    assert set(seen) == {(p, d) for p in M.A_POS for d in [p + 1, p + 2] + [x for x in M.A_FIRST_DIST if x > p + 2]}
    for (p, d), ns in seen.items():
        assert ns == {2, d, d + 1, 65, 1040} - {1}, (p, d, ns)
    repeating = {r["distance"] for v in first.values() for r in v["log"][:1] if r["copy_len"] > r["distance"]}
    assert any(d < 16 for d in repeating) and 16 in repeating and any(d > 16 for d in repeating)
    assert min(forms.values()) >= 30, forms
    mbend = [e for e, _, _ in dict_vectors.load() if "-mbend-" in e["label"]]
    assert mbend and all(e["success"][2] == 2 for e in mbend)
    # invalid on purpose
    codes = {}
    for e, _, _ in dict_vectors.load():
        if e["label"].startswith("A-overrun-"):
            v = made[e["label"]]
            r = v["log"][-1]
            assert not e["valid"] and r in _copies(v["log"]) and e["oracle"][0] == 0
            codes[e["label"]] = e["oracle"][1]
    assert set(codes.values()) == {-9, -10}, codes   # (ERROR_FORMAT_BLOCK_LENGTH_1 and _2)
    assert codes["A-overrun-w10-cross-cf"] == -9 and codes["A-overrun-w22-cf"] == -10 and len(codes) == 6


# ------------------------------------------------------------------ B
def test_coverage_of_the_window_regimes(made):
    """B: for every dictionary size of B_SIZES and every position round the regimes' borders, a copy at the largest distance and the
    word one beyond it, at exactly that position; the three regimes; a dictionary longer than the window keeps its tail; at least
    three windows of output, as one metablock and as several; one form at window 16"""
    mb = M.mb_of(M.B_WBITS)
    seen, regimes = set(), collections.defaultdict(set)
    for label, v in made.items():
        if v["meta"].get("family") != "B":
            continue
        size, target, what = v["dsize"], v["meta"]["target"], v["meta"]["what"]
        r = next(r for r in v["log"] if r["pos"] == target and r["coding"] == "explicit" and r["copy_len"])
        reach = min(target + size, mb)
        assert r["max_distance"] == reach and v["window"] == M.B_WBITS
        if what == "copy":
            assert r["distance"] == reach and not r["word"]
            assert (r["distance"] > r["pos"]) == (target < mb)   # (in the third regime nothing of the dictionary is in reach)
        else:
            assert r["distance"] == reach + 1 and r["word"] and (r["word_idx"], r["transform"]) == (0, 0) and 4 <= r["copy_len"] <= 24
        seen.add((size, target, what))
        regimes[M.regime(target, size, M.B_WBITS)].add((size, what))
        assert len(v["raw"]) >= 3 << M.B_WBITS
    assert seen == {(s, t, w) for s in M.B_SIZES for t in M.b_targets(s) for w in ("copy", "word")}
    assert M.b_targets(600) == [mb - 601, mb - 600, mb - 599, mb - 1, mb, mb + 1] and M.b_targets(1007) == [0, 1, 2, mb - 1, mb, mb + 1] and M.b_targets(2500)[:2] == [0, 1]
    assert regimes[1] == {(600, "copy"), (600, "word"), (1007, "copy"), (1007, "word")}   # (a dictionary that fills the window leaves no first regime)
    assert regimes[2] == regimes[3] == {(s, w) for s in M.B_SIZES for w in ("copy", "word")}
    deep = [r for v in made.values() if v["meta"].get("family") == "B" and v["dsize"] == 2500 for r in _copies(v["log"]) if r["distance"] == mb]
    assert deep   # (the byte 1008 in front of position 0 of a dictionary of 2500)
    counts = {e["label"]: e["success"][2] for e, _, _ in dict_vectors.load() if e["label"].startswith("B-D")}
    assert set(counts.values()) == {1, 3} and counts["B-D600-p%d-copy-ctx" % (mb - 600)] == 3
    v = made["B-w16-D60000-cf"]
    mb16 = M.mb_of(16)
    at = {r["pos"]: r for r in v["log"] if r["coding"] == "explicit" and r["distance"] == r["max_distance"]}
    assert {mb16 - 60001, mb16 - 59999, mb16 - 1, mb16 + 1} <= set(at) and len(v["raw"]) >= 3 << 16
    assert at[mb16 - 60001]["distance"] == mb16 - 1 and at[mb16 - 59999]["distance"] == mb16 == at[mb16 + 1]["distance"]
    assert {M.regime(p, 60000, 16) for p in at} == {1, 2, 3} and sum(1 for r in v["log"] if r["word"]) == 2


# ------------------------------------------------------------------ C
def test_coverage_of_the_far_edge(made):
    """C: distance = reach is a copy of the dictionary's first byte in reach and reach + 1 word 0 under transform 0, for every word
    length; the largest word number; one beyond it, and lengths 2, 3, 25 beyond reach, are the errors the format names; the ring
    forms; three kinds of transform for every length in every regime; 80 dictionary copies in a row"""
    for wbits, size in M.C_EDGE:
        v = made["C-edge-w%d-D%d-cf" % (wbits, size)]
        reach = lambda r: min(r["pos"] + size, M.mb_of(wbits))
        assert {r["copy_len"] for r in _copies(v["log"]) if r["distance"] == r["max_distance"] == reach(r)} == set(range(4, 25))
        assert {r["copy_len"] for r in v["log"] if r["word"] and r["distance"] == reach(r) + 1 and (r["word_idx"], r["transform"]) == (0, 0)} == set(range(4, 25))
    words = [r for r in made["C-last-words-cf"]["log"] if r["word"]]
    assert [(r["copy_len"], r["word_idx"], r["transform"]) for r in words] == [(n, (1 << E.tables()["size_bits"][n]) - 1, 120) for n in range(4, 25)]
    assert all(r["distance"] == r["pos"] + 300 + (121 << E.tables()["size_bits"][r["copy_len"]]) for r in words)
    by = {e["label"]: e for e, _, _ in dict_vectors.load()}
    got = collections.Counter()
    for label, wbits, size, cmds in M.c_invalid():
        e, v = by[label + "-cf"], made[label + "-cf"]
        r = v["log"][-1]
        assert r.get("invalid") and not e["valid"] and r["max_distance"] == min(r["pos"] + size, M.mb_of(wbits))
        if "transform" in label:
            assert r["distance"] == r["max_distance"] + 1 + (121 << E.tables()["size_bits"][r["copy_len"]]) and e["oracle"][:2] == [0, -11], label   # (ERROR_FORMAT_TRANSFORM)
            assert v["log"][-2]["word"] and v["log"][-2]["transform"] == 120 and v["log"][-2]["distance"] - v["log"][-2]["max_distance"] == r["distance"] - r["max_distance"] - 1
            got["transform"] += 1
        else:
            assert r["distance"] == r["max_distance"] + 1 and r["copy_len"] in (2, 3, 25) and e["oracle"][:2] == [0, -12], label   # (ERROR_FORMAT_DICTIONARY)
            got[(r["copy_len"], M.regime(r["pos"], size, wbits))] += 1
    assert got == collections.Counter({"transform": 3, **{(n, g): 1 for n in (2, 3, 25) for g in (1, 2, 3)}})
    ring = [v for v in made.values() if v["meta"].get("family") == "C-ring"]
    assert len(ring) >= 20 and sum(1 for v in ring if not v["valid"]) == 9
    for v in ring:
        r = v["log"][0]
        assert r["coding"] == "ring" and r["word"] and r["max_distance"] == r["pos"] + 1 and v["dsize"] == 1
        assert v["valid"] or (r.get("invalid") and by[v["label"]]["oracle"][:2] == [0, -12])
    assert {v["log"][0]["code"] for v in ring} == set(range(16)) - {8}   # (code 8 on the initial ring is distance 1: in reach of any dictionary)
    v = made["C-regimes-cf"]
    seen = set()
    for r in v["log"]:
        if r["word"]:
            kind = "same" if r["total"] == r["copy_len"] else "more" if r["total"] > r["copy_len"] else "less"
            seen.add((M.regime(r["pos"], M.C_REG_SIZE, M.C_REG_WBITS), r["copy_len"], kind))
            assert r["max_distance"] == min(r["pos"] + M.C_REG_SIZE, M.mb_of(M.C_REG_WBITS)) and r["total"] > 0
    assert seen == {(g, n, k) for g in (1, 2, 3) for n in range(4, 25) for k in ("same", "more", "less")}
    assert {M.regime(r["pos"], M.C_REG_SIZE, M.C_REG_WBITS) for r in _copies(v["log"])} == {1, 2}
    log = made["C-run-cf"]["log"]
    assert len(_copies(log)) == len(log) - 1 >= 80 and all(r["insert"] <= 2 for r in log[:-1])


# ------------------------------------------------------------------ D
def _ring_walk(log):
    """-> per command the ring in front of it (section 4: code 0, the implicit distance and words do not push)"""
    ring, out = list(E.RING_INIT), []
    for r in log:
        out.append(tuple(ring))
        if r["coding"] in ("explicit", "ring") and r["code"] != 0 and not r["word"]:
            ring = [r["distance"]] + ring[:3]
    return out


def test_coverage_of_the_ring(made):
    """D: the ring holds four distances that reached into the dictionary; a short code (or the implicit distance) on one of them gives
    a distance that is still into the dictionary, inside the output, on either side of position 0, and on either side of reach --
    where it names a word, which pushes nothing.  A distance is at most the reach of its own position and reach never shrinks, so
    reach + 1 takes a code that adds, and reach one that does not subtract; in the first regime reach grows with P, and only the codes
    that add 2 or 3 to the last distance get there (codes 7 and 9)."""
    seen = collections.defaultdict(set)
    for v in made.values():
        if v["meta"].get("family") != "D":
            continue
        code, scen, log = v["meta"]["code"], v["meta"]["scenario"], v["log"]
        rings = _ring_walk(log)
        assert all(r in _copies(log) and r["coding"] == "explicit" for r in log[:4])   # (the ring's four entries reached into the dictionary)
        r = log[4]
        e, delta = M.code_parts(code)
        assert (r["coding"], r["code"]) == (("implicit", None) if code is None else ("ring", code)) and r["distance"] == rings[4][e] + delta == log[3 - e]["distance"] + delta
        off = r["distance"] - r["pos"]
        reach = min(r["pos"] + v["dsize"], M.mb_of(v["window"]))
        assert r["max_distance"] == reach
        ok = {"into": off == 5, "inside": off == -3, "zero": off == 0, "zero+1": off == 1, "reach": r["distance"] == reach and off > 0, "reach+1": r["distance"] == reach + 1}[scen]
        assert ok and r["word"] == (scen == "reach+1"), v["label"]
        pushed = not r["word"] and code not in (None, 0)
        assert log[5]["coding"] == "implicit" and log[5]["distance"] == (r["distance"] if pushed else rings[4][0])
        assert log[6]["code"] == 1 and log[6]["distance"] == (rings[4][0] if pushed else rings[4][1])
        seen[(v["window"], scen)].add(code)
    every = set(range(16)) | {None}
    adds = {c for c in range(4, 16) if c & 1}
    for scen in ("into", "inside", "zero", "zero+1"):
        assert seen[(22, scen)] == seen[(10, scen)] == every, scen
    assert seen[(10, "reach")] == {None, 0, 1, 2, 3} | adds and seen[(10, "reach+1")] == adds
    assert seen[(22, "reach")] == {7, 9} and seen[(22, "reach+1")] == {9}


# ------------------------------------------------------------------ E
def test_coverage_of_the_literal_context(made):
    """E: under each of the four context modes a probe (a literal that decodes to another byte or length under every wrong context
    make_literal_vectors.alternatives names: Build.cell refuses a cell in which one of them is no real one) and the literal behind
    it, directly behind a copy at P = 0, a copy of two bytes that lie in the dictionary, and a copy whose last two bytes straddle
    position 0"""
    for mode in range(4):
        v = made["E-mode%d-ctx" % mode]
        m = v["meta"]
        assert m["mode"] == mode and set(m["cells"]) == {c + s for c in ("copy-p0", "copy-dict2", "copy-straddle") for s in ("", "+1")}
        end_of = {r["pos"] + r["copy_len"]: r for r in _copies(v["log"])}
        lit = {r["pos"]: r for r in m["llog"]}
        count = collections.Counter()
        for pos, cell in zip(m["probes"][0::2], m["probes"][1::2]):
            name = m["cells"][cell]
            second = name.endswith("+1")
            r = end_of[pos - second]
            l = lit[pos]
            assert (l["p1"], l["p2"]) == (v["raw"][pos - 1], v["raw"][pos - 2]) and l["mode"] == mode and l["context"] == E.literal_context(mode, l["p1"], l["p2"])
            assert l["tree"] == l["context"]   # (64 trees under the identity map)
            if name.startswith("copy-p0"):
                assert r["pos"] == 0 and r["insert"] == 0
            elif name.startswith("copy-dict2"):
                assert r["copy_len"] == 2 and _before(r) >= 2 and r["pos"] > 0
            else:
                assert _before(r) == r["copy_len"] - 1 and r["pos"] > 0 and v["raw"][pos - second - 1] == v["raw"][0]
            count[name] += 1
        assert count["copy-p0"] == count["copy-p0+1"] == 1 and count["copy-dict2"] == 6 and count["copy-straddle"] == 4 and {r["copy_len"] for r in _copies(v["log"]) if _before(r) == r["copy_len"] - 1} >= {2, 3, 9, 40}


# ------------------------------------------------------------------ F
def test_coverage_of_the_carriers(made):
    """F: the text-like streams of make_copy_vectors and make_word_vectors with one command in twenty a cell (the streams' own
    copies reach into the dictionary as well while P is below their distances): dictionary copies
    with every `before` and every short and long length, the copy at reach and the word beyond it, every ring code behind a
    dictionary copy; the long form is of the size from which a launch forms gangs"""
    for label, least in (("F-T-cf", 6000), ("F-T-ctx", 6000), ("F-T-cf4", 6000), ("F-C-cf", 6000), ("F-C-ctx", 6000), ("F-T2-long-cf", 16000)):
        v = made[label]
        log = v["log"]
        cells = _copies(log)
        assert len(log) >= least and 0.04 * len(log) <= len(cells) <= 0.25 * len(log), (label, len(cells), len(log))
        assert {_before(r) for r in cells} >= set(M._F_BEFORE) and {r["copy_len"] for r in cells} >= set(M._F_LEN) | set(M._F_LONG)
        assert {r["copy_len"] for r in cells if r["distance"] == r["max_distance"]} >= set(range(4, 25))
        assert {r["copy_len"] for r in log if r["word"] and r["distance"] == r["max_distance"] + 1 and r["transform"] == 0} >= set(range(4, 25))
        behind = {log[i + 1]["code"] for i, r in enumerate(log[:-1]) if r in cells[:400] and log[i + 1]["coding"] == "ring"}
        assert behind == set(range(16)), (label, behind)
        assert v["dsize"] == M.F_SIZE and all(r["max_distance"] == r["pos"] + M.F_SIZE for r in log if r["coding"] != "tail")
    # F-S: C's make-up, a cell every 300 commands and no other distance beyond P -- regions of words and plain copies for the path engine
    for label in ("F-S-cf", "F-S-ctx"):
        log = made[label]["log"]
        cells = [i for i, r in enumerate(log) if r["coding"] != "tail" and r["distance"] > r["pos"] and (not r["word"] or r["transform"] == 0 and r["word_idx"] == 0)]
        words = [r for r in log if r["word"]]
        assert len(log) == 6001 and len(_copies(log)) >= 15 and len(words) >= 500 and all(r["max_distance"] == r["pos"] + M.F_SIZE for r in words)
        assert {r["copy_len"] for r in words} == set(range(4, 25)) and len({r["transform"] for r in words}) >= 100
        assert {i % M.F_SPARSE for i, r in enumerate(log) if r in _copies(log)} <= set(range(7, 14))   # (the cells, and the ring codes and implicit distances behind them)
        gaps = [b - a for a, b in zip(cells, cells[1:])]
        assert max(gaps) <= M.F_SPARSE and sum(1 for g in gaps if g >= 250) >= 15   # (stretches of 250 commands and more without a dictionary copy)
    # F-W: window 16, a dictionary of 600 bytes: dictionary copies while it is in reach, then two thirds of the commands behind the window
    for label in ("F-W-cf", "F-W-ctx"):
        v = made[label]
        mb = M.mb_of(16)
        late = [r for r in v["log"] if r["pos"] >= mb]
        assert (v["window"], v["dsize"]) == M.F_W == (16, 600) and len(v["log"]) == 6001 and len(late) >= 3500 and sum(1 for r in late if r["word"]) >= 300
        assert all(r["max_distance"] == mb for r in late if r["coding"] != "tail") and not _copies(late)
        assert len(_copies(v["log"])) >= 8 and all(r["pos"] < mb for r in _copies(v["log"]))
    assert len(made["F-T2-long-cf"]["comp"]) > 65536
    assert sum(1 for r in made["F-C-cf"]["log"] if r["word"]) >= 500 and made["F-T-cf"]["raw"] == made["F-T-ctx"]["raw"] == made["F-T-cf4"]["raw"]


# ------------------------------------------------------------------ G
def test_the_limit_streams_end_in_their_copy(made):
    """G: 300 text-like commands and one final copy out of the dictionary, `before` inside n"""
    got = []
    for label, v in made.items():
        if v["meta"].get("family") == "G" and label.endswith("-cf"):
            r = v["log"][-1]
            assert (r["copy_len"], _before(r)) == tuple(v["meta"]["final"]) and _before(r) < r["copy_len"] <= r["distance"] and r["coding"] == "explicit"
            assert r["pos"] + r["copy_len"] == len(v["raw"]) and made[label[:-2] + "ctx"]["raw"] == v["raw"] and len(v["log"]) == 301
            got.append(tuple(v["meta"]["final"]))
    assert got == M.G_SHAPES and [n for n, _ in got] == [2, 40, 300, 3000]
