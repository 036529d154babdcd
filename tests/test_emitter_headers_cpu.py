"""tests/golden/emitter_headers/ on the CPU: the generator (tools/make_header_vectors.py) writes the committed bytes again; the
emitter's idea of every stream equals the oracle's and libbrotlidec's; and the emitter's header log -- one record per prefix
code with a chosen wire form, per context map and per category's block switches, with bit positions -- shows that the vectors
hold every form they are for.  The log is the emitter's; no decoder is asked what a stream contains.  Nothing here skips."""
import collections
import hashlib
import os
import sys

import pytest

import header_vectors
import libbrotli_ref as ref
import oracle_lib as oracle
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import make_header_vectors as H  # noqa: E402

E_NIBBLE, E_RESERVED, E_META_NIBBLE, E_SIMPLE_ALPHABET, E_SIMPLE_SAME, E_CL_SPACE, E_HUFFMAN_SPACE, E_MAP_REPEAT = -1, -2, -3, -4, -5, -6, -7, -8
E_WINDOW_BITS, E_PADDING_1, E_PADDING_2 = -13, -14, -15


@pytest.fixture(scope="module")
def made():
    """{label: vector} as the generator makes them now"""
    return {v["label"]: v for v in H.vectors()}


@pytest.fixture(scope="module")
def committed():
    return header_vectors.load()


@pytest.fixture(scope="module")
def verdict(committed):
    """{label: the oracle's error code, 1 for a success} out of the manifest (pinned against the oracle below)"""
    return {e["label"]: e["oracle"][1] for e, _ in committed}


def test_generator_writes_the_committed_bytes_again(made, committed):
    assert [e["label"] for e, _ in committed] == list(made)
    for e, comp in committed:
        v = made[e["label"]]
        assert comp == v["stream"], e["label"]
        assert (e["family"], e["window"], e["large"], e["valid"], e["size"], e["first_command"]) == \
               (v["family"], v["window"], v["large"], v["valid"], len(v["output"]), v["first_command"]), e["label"]
        assert not e["valid"] or e["sha"] == hashlib.sha256(v["output"]).hexdigest()[:16], e["label"]
        parts = e.get("files", [0])
        assert len(parts) <= header_vectors.MAX_PARTS and len(comp) <= header_vectors.MAX_FILE * len(parts), e["label"]
        assert ("at" in e) == (len(comp) < 256)
    for name in os.listdir(header_vectors.DIR):
        assert os.path.getsize(os.path.join(header_vectors.DIR, name)) <= header_vectors.MAX_FILE or name == "manifest.json", name
    assert os.path.getsize(os.path.join(header_vectors.DIR, "manifest.json")) < 1 << 20
    assert len(committed) >= 700


def test_three_opinions_on_every_vector(made, committed):
    """valid vectors: the emitter's output, the oracle's and libbrotlidec's are the same bytes, the whole stream consumed.  The
    others -- headers no decoder accepts, and unchecked ones whose words run on behind their code's end -- : the manifest's triple
    is the oracle's, it is no success, the oracle and libbrotlidec agree on failure and on the bytes they deliver (one a prefix of
    the other, the rule of test_emitter_words_cpu.py), and those are a prefix of what the emitter put out in front."""
    n = 0
    for e, comp in committed:
        v = made[e["label"]]
        raw, flags = v["output"], header_vectors.flags_of(e)
        cap = header_vectors.cap_of(e)
        info, out = oracle.decode(comp, cap, flags)
        assert [info.result, info.error_code, info.decoded_size] == e["oracle"], e["label"]
        if e["valid"]:
            assert (info.result, info.error_code, info.decoded_size, info.consumed) == (1, 1, len(raw), len(comp)) and out == raw, e["label"]
            assert [info.num_metablocks, info.num_commands] == e["counts"], e["label"]
            if not v["large"]:   # (a stream of a standard window decodes alike under the flag)
                assert oracle.decode(comp, cap, header_vectors.FLAG_LARGE_WINDOW)[1] == raw, e["label"]
        else:
            assert info.result != 1 and out == raw[:len(out)], (e["label"], info.result, info.error_code)
            n += 1
        if ref.available():
            res, code, rout, used = ref.decode(comp, cap, bool(flags))
            if e["valid"]:
                assert res == 1 and rout == raw and used == len(comp), e["label"]
            else:
                assert res != 1 and (res == 0) == (info.result == 0), (e["label"], res, code, info.result, info.error_code)
                assert out == rout[:len(out)] or rout == out[:len(rout)], e["label"]
    assert n >= 150, n
    # a large-window stream without the flag is no stream at all
    for e, comp in committed:
        if e["large"]:
            info, out = oracle.decode(comp, e["size"] + 64, 0)
            assert (info.result, info.error_code, out) == (0, E_WINDOW_BITS, b""), e["label"]


def test_the_data_shows_the_code_under_test(made):
    """every valid P vector's literals, commands or distances use one of the shallowest and one of the deepest symbols of the code
    under test (a wrong length changes bytes, not only a verdict) -- but for the distance codes whose every symbol is a distance
    that a small stream cannot reach: there the verdict is what shows, and they are few"""
    hidden = [l for l, v in made.items() if v["family"] == "P" and v["valid"] and not v["extremes"]]
    assert all(v["slot"].startswith("d") for v in (made[l] for l in hidden)), hidden
    assert len(hidden) <= 12, hidden
    assert sum(1 for v in made.values() if v["family"] == "P" and v["valid"] and v["extremes"]) >= 380


# ------------------------------------------------------------------ P
def _codes(made, slot=None, form=None):
    """[(label, the log record of the code under test)] of the P vectors"""
    out = []
    for label, v in made.items():
        if v["family"] == "P" and (slot is None or v["slot"] == slot) and (form is None or v["form"] == form):
            recs = [r for r in v["hlog"] if r["kind"] == H.SLOTS[v["slot"]][0] + "0"]
            out.append((label, recs[-1]))
    return out


def _read(rec):
    return [w for w in rec.get("words", []) if w["read"]]


def test_p_every_bit_phase(made):
    """the code starts at every bit phase 0 .. 31 of the stream, as the literal, the command and a distance code; under four windows"""
    for slot in ("lit", "cmd", "d64"):
        recs = _codes(made, slot, "phase")
        assert {r["start"] % 32 for _, r in recs} == set(range(32)), slot
        assert len({r["words_start"] % 64 for _, r in recs}) >= 16, slot   # (where the first step starts)
    assert {made[l]["window"] for l, _ in _codes(made, "lit", "phase")} == {10, 16, 17, 22}


def _step_ends(rec):
    """{(kind, bits of the word's code, bits of the word in front of bit 64 of its step)} of the words that end on or straddle it"""
    out = set()
    for w in _read(rec):
        bits = w["end"] - w["start"]
        if w["at"] < 64 <= w["at"] + bits:
            out.add(("len" if w["word"] < 16 else w["word"], w["mid"] - w["start"], 64 - w["at"]))
    return out


def test_p_words_on_every_side_of_a_step(made):
    """a reader that takes 64 stream bits a step: for a length, a 16 and a 17, with a code of one to five bits, a word that ends
    exactly on bit 64 of its step, and one that straddles it at every offset -- inside the code, between the code and the extra
    bits, inside the extra bits.  A word that starts on bit 64 is the first of the next step: behind every exact end there is one."""
    want = {(kind, n, o) for kind, more in (("len", 0), (16, 2), (17, 3)) for n in range(1, 6) for o in range(1, n + more + 1)}
    seen = collections.defaultdict(set)
    starts = set()
    for label, rec in _codes(made):
        if rec["form"] == "complex" and rec["cl_symbols"] > 1:
            seen[made[label]["slot"]] |= _step_ends(rec)
            words = _read(rec)
            for a, b in zip(words, words[1:]):
                if b["step"] == a["step"] + 1 and a["at"] + a["end"] - a["start"] == 64:
                    starts.add(("len" if b["word"] < 16 else b["word"]))
    for slot in H.SLOTS:   # (every place in every code: what seeded codes of 64 and 74 symbols do not reach, the generator builds)
        assert seen[slot] >= want, (slot, sorted(want - seen[slot], key=str))
    assert starts == {"len", 16, 17}
    assert max(w["step"] for _, rec in _codes(made) for w in rec.get("words", [])) >= 3


def test_p_repeat_runs(made):
    for slot, (pslot, alphabet, max_symbol, *_rest) in H.SLOTS.items():
        recs = dict(_codes(made, slot))
        words = {label: _read(rec) for label, rec in recs.items() if rec["form"] == "complex"}
        # a 16 as the first word repeats the initial 8; with every extra value
        first = {w[0]["extra"]: w[0] for label, w in words.items() if w and w[0]["word"] == 16}
        assert set(first) == {0, 1, 2, 3} and all(w["value"] == 8 and w["run"] == 3 + e for e, w in first.items()), slot
        # a 16 behind zeros repeats the last length that was not zero
        assert any(a["word"] == 0 and b["word"] == 16 and b["value"] not in (0, 8) for w in words.values() for a, b in zip(w, w[1:])), slot
        # chains as written: sixteens of 1 .. 6 links with every extra value at the last link, seventeens of 1 .. 4 links.  As read: a
        # decoder stops at the link that passes the alphabet's end (a chain of k sixteens names at least 3, 7, 23, 87, 343, 1367
        # symbols, of k seventeens 3, 11, 75, 587), so the depth that is reached is the alphabet's
        last16, last17 = set(), set()
        for label, rec in recs.items():
            w = rec.get("words", [])
            for i, a in enumerate(w):
                if a["word"] >= 16 and (i + 1 == len(w) or w[i + 1]["word"] != a["word"]):
                    k = 1
                    while i - k >= 0 and w[i - k]["word"] == a["word"]:
                        k += 1
                    (last16 if a["word"] == 16 else last17).add((k, a["extra"]))
        assert last16 >= {(k, e) for k in range(1, 7) for e in range(4)}, (slot, sorted(last16))
        assert {k for k, _ in last17} >= {1, 2, 3, 4}, (slot, last17)
        reach16 = max(x["chain"] for w in words.values() for x in w if x["word"] == 16)
        reach17 = max(x["chain"] for w in words.values() for x in w if x["word"] == 17 and recs)
        assert reach16 == {"lit": 5, "cmd": 6, "d64": 4, "d520": 6, "dlw": 4}[slot], (slot, reach16)
        assert reach17 >= {"lit": 3, "cmd": 4, "d64": 2, "d520": 4, "dlw": 3}[slot], (slot, reach17)
        # the run of a chain is the number its extra values spell, in base four or eight
        for w in words.values():
            total = 0
            for x in w:
                if x["chain"]:
                    total = x["run"] if x["chain"] == 1 else total + x["run"]
                    nbits = x["word"] - 14
                    assert x["chain"] == 1 or total == ((before - 2) << nbits) + x["extra"] + 3
                    before = total
        # 16 behind 17 and 17 behind 16: the run starts again; so does a 16 behind a literal length equal to the repeated one
        pairs = {(a["word"], b["word"]) for w in words.values() for a, b in zip(w, w[1:]) if b["chain"] == 1}
        assert {(16, 17), (17, 16)} <= pairs, slot
        assert any(a["word"] == 16 and b["word"] == a["value"] and c["word"] == 16 and c["chain"] == 1 and c["value"] == a["value"]
                   for w in words.values() for a, b, c in zip(w, w[1:], w[2:])), slot
        # a run that goes on across a step's end (the first word of a step has chain depth 2 or more), for both repeat words; and a
        # step that starts with the other repeat word than the one before ended with (the run does not go on)
        heads = [(a, b) for w in words.values() for a, b in zip(w, w[1:]) if b["step"] == a["step"] + 1]
        assert {b["word"] for a, b in heads if b["chain"] and b["chain"] >= 2} == {16, 17}, slot
        assert {(a["word"], b["word"]) for a, b in heads if b["chain"] == 1 and a["word"] >= 16} >= {(16, 17), (17, 16)}, slot
        for name in ("on-16", "on-17", "turn-16-17", "turn-17-16"):   # built for it: twelve words of five bits, a repeat word that ends on bit 64, the next one
            w = words["P-%s-step-%s" % (slot, name)]
            assert (w[12]["at"], w[12]["end"] - w[12]["start"], w[13]["step"], w[13]["at"]) == (60, 4, 1, 0) and w[13]["chain"] == (2 if "on" in name else 1), (slot, name)
    # A run that goes on across TWO steps' ends cannot be written: its chain would be more than 64 bits of repeat words, eight links
    # at the least, and a chain of seven links names more than 4^6 symbols.  The longest chains are V-seventeens-16 and -21 with their
    # four-bit words: they cross a step's end, and every decoder stops at the third link (test_p_verdicts).


def test_p_ends(made, verdict):
    for slot, (pslot, alphabet, max_symbol, *_rest) in H.SLOTS.items():
        recs = {l: r for l, r in _codes(made, slot) if r["form"] == "complex" and made[l]["valid"]}
        last = {l: _read(r)[-1] for l, r in recs.items() if _read(r)}
        assert any(w["word"] < 16 for w in last.values()) and any(w["word"] == 16 for w in last.values()), slot   # complete on a length; inside a repeat
        assert all(r["space"] == 0 for r in recs.values())
        at_end = [l for l, r in recs.items() if r["reached"] == max_symbol]
        assert len(at_end) >= 2 and {last[l]["word"] < 16 for l in at_end} == {True, False}, (slot, at_end)   # the last symbol completes it: a length, a repeat
        assert all(r["max_symbol"] == max_symbol and r["alphabet"] == alphabet for r in recs.values())
        # words behind the code's end, in an unchecked stream: not read; the stream is parsed on from there (no decoder succeeds)
        label = "P-%s-zeros-behind-the-end" % slot
        rec = dict(_codes(made, slot))[label]
        assert rec["space"] == 0 and rec["consumed"] == len(rec["words"]) - 3 and not made[label]["valid"] and verdict[label] != 1
        # HSKIP below what the zeros allow, and the three values
        assert {(r["hskip"], r["cl_lengths"][1] == 0 and r["cl_lengths"][2] == 0) for r in recs.values()} >= {(0, True), (2, True), (3, True), (0, False)}, slot
        assert any(r["hskip"] == 0 and r["cl_lengths"][1:4] == [0, 0, 0] for r in recs.values()) and any(r["hskip"] == 2 and r["cl_lengths"][1:4] == [0, 0, 0] for r in recs.values())
    assert H.SLOTS["dlw"][1:3] == (140, 74) and H.SLOTS["d520"][1] == 520 and H.SLOTS["d64"][1] == 64


_V = {"V-repeat-one-beyond": E_HUFFMAN_SPACE, "V-seventeens-16": E_HUFFMAN_SPACE, "V-seventeens-21": E_HUFFMAN_SPACE,
      "V-space-over-by-a-length": E_HUFFMAN_SPACE, "V-space-over-by-a-repeat": E_HUFFMAN_SPACE, "V-space-left-at-max-symbol": E_HUFFMAN_SPACE,
      "V-cl-space-left": E_CL_SPACE, "V-cl-space-over": E_CL_SPACE, "one-17": E_HUFFMAN_SPACE,
      "V-simple-same-12": E_SIMPLE_SAME, "V-simple-same-13": E_SIMPLE_SAME, "V-simple-same-23": E_SIMPLE_SAME, "V-simple-same-14": E_SIMPLE_SAME,
      "V-simple-same-24": E_SIMPLE_SAME, "V-simple-same-34": E_SIMPLE_SAME}


def test_p_verdicts(made, verdict):
    """each listed verdict, by name, in every place a code can stand; in front of each a valid compressed metablock"""
    for slot, (pslot, alphabet, max_symbol, *_rest) in H.SLOTS.items():
        recs = dict(_codes(made, slot))
        for form, code in _V.items():
            label = "P-%s-%s" % (slot, form)
            assert verdict[label] == code and not made[label]["valid"], (label, verdict[label])
            assert len([r for r in made[label]["hlog"] if r["kind"] == "metablock"]) == 2 and len(made[label]["output"]) == 53, label
        # a repeat that passes the alphabet's end (under large window: max_symbol, below the alphabet) by one
        r = recs["P-%s-V-repeat-one-beyond" % slot]
        w = _read(r)
        assert r["space"] is None and len(w) + 1 == max_symbol and w[-1]["word"] == 17 and w[-1]["run"] == 3   # (max_symbol - 2 symbols passed, three more)
        # chains of seventeens with a one-bit word: 3 and 4 links pass 256 symbols (704 take four links), 16 and 21 links pass any;
        # the 21 links pass 2^32 as well -- every decoder stops at the link that passes the alphabet
        for k in (3, 4, 16, 21):
            r = recs["P-%s-V-seventeens-%d" % (slot, k)]
            assert len(r["words"]) == k and all(x["word"] == 17 and x["end"] - x["start"] == 4 for x in r["words"]) and r["cl_lengths"][17] == 1
            stop = _read(r)
            if k >= 16 or max_symbol <= 586:
                assert verdict["P-%s-V-seventeens-%d" % (slot, k)] == E_HUFFMAN_SPACE
                total = sum(x["run"] for x in stop)
                if max_symbol == 74:   # (two links name exactly the 74 symbols a large-window distance code may have: no repeat passes the end, the space is left)
                    assert len(stop) == 2 and total == 74 == r["reached"] and r["space"] == 32768
                else:
                    assert r["space"] is None and len(stop) == (2 if max_symbol < 74 else 3 if max_symbol < 586 else 4) and total > max_symbol
        assert recs["P-%s-V-seventeens-21" % slot]["words"][-1]["end"] - recs["P-%s-V-seventeens-21" % slot]["words_start"] == 84   # (across a step's end)
        assert recs["P-%s-V-space-over-by-a-length" % slot]["space"] < 0 and recs["P-%s-V-space-over-by-a-repeat" % slot]["space"] < 0
        assert _read(recs["P-%s-V-space-over-by-a-repeat" % slot])[2]["word"] == 16
        assert recs["P-%s-V-space-left-at-max-symbol" % slot]["space"] > 0 and recs["P-%s-V-space-left-at-max-symbol" % slot]["reached"] == max_symbol
        assert (recs["P-%s-V-cl-space-left" % slot]["cl_symbols"], recs["P-%s-V-cl-space-left" % slot]["cl_space"] > 0) == (2, True)
        assert recs["P-%s-V-cl-space-over" % slot]["cl_space"] < 0
        for i, j in ((1, 2), (1, 3), (2, 3), (1, 4), (2, 4), (3, 4)):
            r = recs["P-%s-V-simple-same-%d%d" % (slot, i, j)]
            assert r["form"] == "simple" and r["symbols"][i - 1] == r["symbols"][j - 1] and len(set(r["symbols"])) == r["nsym"] - 1
    # a simple code's symbol at max_symbol and beyond: wherever the symbols' bits can say one (not with 256 and 64 symbols)
    for slot in ("cmd", "d520", "dlw"):
        label = "P-%s-V-simple-symbol-at-max-symbol" % slot
        assert verdict[label] == E_SIMPLE_ALPHABET and max(dict(_codes(made, slot))[label]["symbols"]) == H.SLOTS[slot][2], label
    assert verdict["P-dlw-V-simple-symbol-at-alphabet"] == E_SIMPLE_ALPHABET and dict(_codes(made, "dlw"))["P-dlw-V-simple-symbol-at-alphabet"]["symbols"][0] == 140
    assert not any(l.endswith("V-simple-symbol-at-max-symbol") for l, _ in _codes(made, "lit") + _codes(made, "d64"))


def test_p_simple_codes(made):
    """NSYM 1 .. 4, both tree-select values, symbols not in sorted order"""
    for slot in H.SLOTS:
        recs = [r for l, r in _codes(made, slot) if r["form"] == "simple" and made[l]["valid"]]
        assert {(r["nsym"], r["tree_select"]) for r in recs} == {(1, None), (2, None), (3, None), (4, 0), (4, 1)}, slot
        assert all(r["symbols"] != sorted(r["symbols"]) for r in recs if r["nsym"] > 1), slot


def test_p_the_serial_loop_and_the_depth(made, verdict):
    """code-length codes of one symbol (their words take no bits): only 16 -- four words with extra bits 2, 2, 2, 1 make 256 lengths
    of 8 --, only 8, only 17 (a verdict), only 1; lengths 1, 2 .. 15, 15 through the reader, plain and with repeat words"""
    for slot, (pslot, alphabet, max_symbol, *_rest) in H.SLOTS.items():
        recs = dict(_codes(made, slot))
        for name, sym in (("one-16", 16), ("one-8", 8), ("one-17", 17), ("one-1", 1)):
            r = recs["P-%s-%s" % (slot, name)]
            assert r["cl_symbols"] == 1 and r["cl_lengths"][sym] and all(w["mid"] == w["start"] for w in r["words"]), (slot, name)
        r = recs["P-%s-one-16" % slot]
        assert [w["extra"] for w in r["words"]] == [2, 2, 2, 1] and r["words_start"] + 8 == r["end"]   # (no bits but the extra ones: 21 bytes of stream as the literal code)
        ok = max_symbol >= 256
        assert made["P-%s-one-16" % slot]["valid"] == made["P-%s-one-8" % slot]["valid"] == ok and made["P-%s-one-1" % slot]["valid"]
        if ok:
            assert sum(w["run"] for w in _read(r)) == 256 and r["symbols"] == 256 and r["depth"] == 8 and recs["P-%s-one-8" % slot]["symbols"] == 256
        else:   # (64 and 74 symbols have no room for 256 lengths of 8: the reference's verdict)
            assert verdict["P-%s-one-16" % slot] == verdict["P-%s-one-8" % slot] == E_HUFFMAN_SPACE
        assert verdict["P-%s-one-17" % slot] == E_HUFFMAN_SPACE and recs["P-%s-one-1" % slot]["symbols"] == 2
        plain, rep = recs["P-%s-depth-plain" % slot], recs["P-%s-depth-sixteens" % slot]
        assert plain["depth"] == rep["depth"] == 15 and plain["symbols"] == 16 and rep["symbols"] == 20
        assert not any(w["word"] >= 16 for w in plain["words"]) and [w["run"] for w in rep["words"] if w["word"] == 16] == [3, 4]
        assert made["P-%s-depth-plain" % slot]["valid"] and made["P-%s-depth-sixteens" % slot]["valid"] and made["P-%s-depth-plain" % slot]["extremes"]


# ------------------------------------------------------------------ C
def _last_maps(made, kind):
    """[(label, the record of the map of `kind` in the vector's last metablock)]"""
    out = []
    for l, v in made.items():
        if v["family"] == "C":
            recs = [r for r in v["hlog"] if r["kind"] == kind]
            if recs[-1]["ntrees"] > 1:
                out.append((l, recs[-1]))
    return out


def test_c_sizes_and_run_codes(made, verdict):
    lit, dist = _last_maps(made, "lit_map"), _last_maps(made, "dist_map")
    assert {(r["ntrees"], r["rlemax"]) for _, r in lit} >= {(n, m) for n in (2, 3, 64, 65, 255, 256) for m in (0, 1, 5, 16)}
    assert {(r["ntrees"], r["rlemax"]) for _, r in dist} >= {(n, m) for n in (2, 4, 65, 256) for m in (0, 3, 16)}
    assert any(r["ntrees"] + r["rlemax"] == 272 for _, r in lit) and any(r["ntrees"] + r["rlemax"] == 272 for _, r in dist)
    # every run-length code 1 .. 16 with extra bits all zeros and all ones; 16384 entries for the wide ones; those that no map holds
    valid, beyond = set(), set()
    for l, r in lit:
        for code, extra, at in r["runs"]:
            if extra in (0, (1 << code) - 1):
                (valid if made[l]["valid"] else beyond).add((code, extra == 0))
    assert valid >= {(c, z) for c in range(1, 14) for z in (True, False)} | {(14, True)}, sorted(valid)
    assert beyond >= {(14, False), (15, True), (15, False), (16, True), (16, False)}
    for l, r in lit:
        if l.startswith("C-V-run-c"):
            assert verdict[l] == E_MAP_REPEAT and r["size"] == 16384 and r["filled"] > r["size"] and r["rlemax"] == 16, l
    # run ends: exactly at the map's end; one beyond it; a map that is one run of zeros behind NTREES >= 2
    for l, r in (x for x in lit + dist if made[x[0]]["valid"]):
        assert r["filled"] == r["size"] == len(r["map"]), l
    ends = [l for l, r in lit if made[l]["valid"] and r["items"][-1][0] == "run" and len(r["items"]) > 1]
    assert "C-run-ends-the-map" in ends and "C-run-c13-ones" in ends
    for label, kind in (("C-V-run-one-beyond", "lit_map"), ("C-dist-V-run-one-beyond", "dist_map")):
        r = dict(_last_maps(made, kind))[label]
        assert r["filled"] == r["size"] + 1 and r["items"][-1][0] == "run" and verdict[label] == E_MAP_REPEAT, label
    whole = [(l, r) for l, r in lit + dist if made[l]["valid"] and len(r["items"]) == 1]
    assert {l for l, _ in whole} == {"C-run-c14-zeros-whole-map", "C-one-run-n2", "C-dist-one-run-n3"} and all(r["ntrees"] >= 2 and not any(r["map"]) for _, r in whole)


def test_c_move_to_front(made):
    lit = dict(_last_maps(made, "lit_map"))
    for name in ("edges", "every-tree", "big"):
        for rlemax in (0, 9):
            r = lit["C-imtf-%s-r%d" % (name, rlemax)]
            assert r["imtf"] == 1 and set(r["indices"]) >= {0, 1, 63, 64, 65, 127, 128, 129, 255} and r["mtf_max"] == 255 and r["rlemax"] == rlemax
            values = [i[1] for i in r["items"] if i[0] == "v"]
            assert any(a == b == 0 for a, b in zip(values, values[1:])) or rlemax   # (repeats of 0: as symbols, or inside runs)
            assert E.forward_mtf(r["map"])[:len(H.MTF_SEQ)] == H.MTF_SEQ
            if name != "edges":   # 256 times the last of the list: every tree comes to the front once
                idx = E.forward_mtf(r["map"])
                assert idx[len(H.MTF_SEQ):len(H.MTF_SEQ) + 256] == [255] * 256 and len(set(r["map"][len(H.MTF_SEQ):len(H.MTF_SEQ) + 256])) == 256
            if name != "big":   # the same symbols without the transform
                p = lit["C-plain-%s-r%d" % (name, rlemax)]
                assert p["imtf"] == 0 and p["items"] == r["items"] and p["map"] != r["map"]
    assert lit["C-imtf-big-r9"]["size"] == lit["C-imtf-big-r0"]["size"] == 16384 and lit["C-imtf-big-r0"]["ntrees"] == 256
    assert any(r["imtf"] == 1 for _, r in _last_maps(made, "dist_map"))


def test_c_the_maps_own_code_and_what_the_maps_select(made):
    v = made["C-code-simple"]
    assert sum(1 for r in v["hlog"] if r["kind"] in ("lit_map", "dist_map") and 2 <= r["ntrees"] + r["rlemax"] <= 4) == 2   # (at most four symbols: PrefixCode writes them simple)
    rec = [r for r in made["C-code-repeats"]["hlog"] if r["kind"] == "lit_map_code"][-1]
    assert rec["form"] == "complex" and {16, 17} <= {w["word"] for w in rec["words"]} and rec["alphabet"] == 255 + 4 and made["C-code-repeats"]["valid"]
    lit = dict(_last_maps(made, "lit_map"))
    trivial = lambda r: [len(set(r["map"][t * 64:t * 64 + 64])) == 1 for t in range(r["size"] // 64)]
    mixed = trivial(lit["C-some-types-trivial"])
    assert True in mixed and False in mixed
    allt = lit["C-all-trivial-and-different"]
    assert all(trivial(allt)) and len({allt["map"][t * 64] for t in range(5)}) == 5 and allt["ntrees"] == 5
    # every literal block type of these maps is visited
    for label in ("C-some-types-trivial", "C-all-trivial-and-different"):
        sw = [r for r in made[label]["hlog"] if r["kind"] == "switches" and r["cat"] == 0][-1]
        assert sw["nbt"] == lit[label]["size"] // 64 and sum(sw["counts"][:-1]) < sw["symbols"]
    d = dict(_last_maps(made, "dist_map"))["C-dist-each-context-its-tree"]
    assert all(sorted(d["map"][t * 4:t * 4 + 4]) == [0, 1, 2, 3] for t in range(3)) and d["imtf"] == 1
    lens = {r["copy_len"] for r in made["C-dist-each-context-its-tree"]["clog"] if r["coding"] == "explicit"}
    assert {2, 3, 4} <= lens and max(lens) >= 5


# ------------------------------------------------------------------ B
def _switches(v, cat=None):
    return [r for r in v["hlog"] if r["kind"] == "switches" and (cat is None or r["cat"] == cat)]


def _types(rec):
    """the block types the type codes spell, as a decoder resolves them"""
    second, last, out = 1, 0, [0]
    for c in rec["type_codes"]:
        t = second if c == 0 else (last + 1) % rec["nbt"] if c == 1 else c - 2
        second, last = last, t
        out.append(t)
    return out


def test_b_block_lengths(made):
    """every block-length code 0 .. 25 with extra bits all zeros and all ones, in each category; code 25 also at 1 and with bit 16
    set; the codes up to 17 run out (a switch follows), the wider ones are a metablock's last block"""
    for cat, name in enumerate(("lit", "cmd", "dist")):
        recs = _switches(made["B-%s-every-length-code" % name], cat)
        seen = {(c, "zeros" if v == 0 else "ones" if v == (1 << nb) - 1 else v) for r in recs for c, v, nb in r["lengths"]}
        assert seen >= {(c, x) for c in range(26) for x in ("zeros", "ones")} | {(25, 1), (25, 65536 + 9)}, (name, sorted(seen))
        assert all(nb == E._BL_EXTRA[c] for r in recs for c, v, nb in r["lengths"])
        first = recs[0]
        ran_out = {c for c, _, _ in first["lengths"][:-1]}
        assert ran_out >= set(range(18)) and sum(first["counts"][:36]) <= first["symbols"]
        assert len(recs) == 1 + 18 and all(r["counts"][-1] > r["symbols"] for r in recs[1:])


def test_b_block_types(made):
    for cat, name in enumerate(("lit", "cmd", "dist")):
        for nbt in (2, 3, 255, 256):
            ring, direct = (_switches(made["B-%s-n%d-%s" % (name, nbt, how)], cat)[0] for how in ("ring", "direct"))
            assert ring["nbt"] == direct["nbt"] == nbt and _types(ring) == _types(direct)
            assert set(_types(ring)) == set(range(nbt))
            assert {min(c, 2) for c in ring["type_codes"]} >= ({0, 1, 2} if nbt > 2 else {0}) and all(c >= 2 for c in direct["type_codes"])
            if nbt > 2:   # last + 1 round the end
                types = _types(ring)
                assert any(c == 1 and a == nbt - 1 and b == 0 for c, a, b in zip(ring["type_codes"], types, types[1:]))
    simple = {r["simple"][0] for v in made.values() if v["family"] == "B" for r in _switches(v)}
    assert simple == {True, False}


def test_b_blocks_of_one_and_the_last_block(made):
    for label, cats in (("B-ones-lit", (0,)), ("B-ones-cmd", (1,)), ("B-ones-dist", (2,)), ("B-ones-all", (0, 1, 2))):
        recs = _switches(made[label])
        assert {r["cat"] for r in recs} == set(cats)
        assert all(set(r["counts"]) == {1} and len(r["counts"]) == r["symbols"] >= 40 for r in recs), label   # a switch in front of every symbol but the first
    for cat, name in enumerate(("lit", "cmd", "dist")):
        for last in ("last", "inner"):
            for end, off in (("exact", 0), ("one-short", -1), ("one-over", 1)):
                v = made["B-%s-last-block-%s-%s" % (name, end, last)]
                r = _switches(v, cat)[0]
                if off >= 0:
                    assert sum(r["counts"]) == r["symbols"] + off and len(r["counts"]) == 2
                else:
                    assert sum(r["counts"]) == r["symbols"] and r["counts"][-1] == 1 and len(r["counts"]) == 3
                assert len([x for x in v["hlog"] if x["kind"] == "metablock"]) == (1 if last == "last" else 2) and v["valid"]


def test_b_switch_positions_and_the_long_form(made):
    # a literal switch in front of the first, a middle and the last literal of an insert
    v = made["B-lit-switch-first-middle-last"]
    r = _switches(v, 0)[0]
    edges, at = set(), 0
    for c in r["counts"][:-1]:
        at += c; edges.add(at)
    where, at = set(), 0
    for c in v["clog"]:
        n = c["insert"]
        for k in range(n):
            if at + k in edges:
                where.add("first" if k == 0 else "last" if k == n - 1 else "middle")
        at += n
    assert where == {"first", "middle", "last"}
    # a command switch right behind a command with an implicit distance
    v = made["B-cmd-switch-behind-implicit"]
    r = _switches(v, 1)[0]
    assert v["clog"][r["counts"][0] - 1]["coding"] == "implicit"
    # a distance switch in front of ring code 0
    v = made["B-dist-switch-before-ring0"]
    r = _switches(v, 2)[0]
    with_dist = [c for c in v["clog"] if c["coding"] in ("explicit", "ring")]
    starts, at = [], 0
    for c in r["counts"][:-1]:
        at += c; starts.append(at)
    assert sum(1 for s in starts if with_dist[s]["coding"] == "ring" and with_dist[s]["code"] == 0) == 2
    # the long form
    v = made["B-long"]
    recs = _switches(v)
    assert [r["cat"] for r in recs] == [0, 1, 2] and len(v["clog"]) >= 4000
    for r in recs:
        assert set(r["counts"][:-1]) == set(range(1, 41)) and len(r["counts"]) >= 300 and r["nbt"] == 3 and set(r["type_codes"]) >= {0, 1}
    assert not any(x["kind"] in ("lit_map", "dist_map") and x["ntrees"] > 3 for x in v["hlog"])


# ------------------------------------------------------------------ M
def test_m_framing(made, verdict):
    m = {l: v for l, v in made.items() if v["family"] == "M"}
    # MNIBBLES 4, 5, 6 at their extremes; one nibble and two nibbles too many
    sizes = {(v["mlen"], v["nibbles"]): l for l, v in m.items() if "mlen" in v}
    for n, nib in ((1, 4), (65536, 4), (65537, 5), (1 << 20, 5), ((1 << 20) + 1, 6), (1 << 24, 6)):
        assert verdict[sizes[(n, nib)]] == 1 and len(m[sizes[(n, nib)]]["output"]) == n
    for n, nib in ((7, 5), (7, 6), (65537, 6)):
        assert verdict[sizes[(n, nib)]] == E_NIBBLE
    # metadata: MSKIPBYTES 0 .. 3 on both sides of 128 / 129 bytes, 256, 65536, 65537; too many bytes; the reserved bit; the padding
    assert {(v["metadata"], v["nbytes"]) for v in m.values() if "metadata" in v} == {(0, 0), (1, 1), (128, 1), (129, 1), (256, 1), (65536, 2), (65537, 3)}
    assert all(verdict[l] == 1 for l, v in m.items() if "metadata" in v)
    assert [verdict["M-V-metadata-exuberant-%s" % k] for k in ("2", "3", "3-of-1")] == [E_META_NIBBLE] * 3
    assert (m["M-V-metadata-exuberant-2"]["nbytes"], m["M-V-metadata-exuberant-2"]["payload"], m["M-V-metadata-exuberant-3"]["payload"]) == (2, 200, 300)
    assert verdict["M-V-metadata-reserved"] == E_RESERVED
    assert verdict["M-V-metadata-padding"] == verdict["M-V-stored-padding"] == verdict["M-V-final-padding"] == E_PADDING_2
    # runs of empty and one-byte metadata blocks in front of a compressed metablock, another behind it
    assert {v["run"] for v in m.values() if "run" in v} == {(c, s) for c in (1, 2, 200) for s in (0, 1)}
    assert all(verdict[l] == 1 and len([r for r in v["hlog"] if r["kind"] == "metablock"]) == 2 for l, v in m.items() if "run" in v)
    # ISLASTEMPTY behind a compressed metablock; every window code; the large-window form, valid and not
    assert verdict["M-last-empty-behind-compressed"] == 1
    assert {v["wbits"] for v in m.values() if "wbits" in v and not v["large"]} == set(range(10, 25))
    assert {v["wbits"] for v in m.values() if "wbits" in v and v["large"]} == {10, 22, 30}
    assert [verdict["M-V-large-window-%s" % k] for k in ("reserved-bit", "9", "31")] == [E_WINDOW_BITS] * 3
