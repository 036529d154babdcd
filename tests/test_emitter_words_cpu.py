"""tests/golden/emitter_words/ on the CPU: the emitter (tools/brotli_emit.py) writes the committed bytes again, its own idea of
the output -- words and transforms restated in plain Python -- equals the oracle's and libbrotlidec's, and its command log
shows that the vectors hold what they are for: every (copy length, transform) pair, every ring code behind every kind of
predecessor, the chains of words, the ring codes that name words.  The log is the emitter's; no decoder is asked what a
stream contains.  Needs no encoder library: nothing here skips."""
import collections
import ctypes
import hashlib
import os
import random
import sys

import pytest

import libbrotli_ref as ref
import oracle_lib as oracle
import word_vectors
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import make_word_vectors as M  # noqa: E402


@pytest.fixture(scope="module")
def made():
    """{label: (window, stream, output, log, valid)} as the generator makes them now"""
    return {label: rest for label, *rest in M.vectors()}


@pytest.fixture(scope="module")
def committed():
    return word_vectors.load()


def test_generator_writes_the_committed_bytes_again(made, committed):
    assert [e["label"] for e, _ in committed] == list(made)
    for e, comp in committed:
        wbits, again, raw, log, valid = made[e["label"]]
        assert comp == again, e["label"]
        assert (e["window"], e["valid"], e["size"], e["sha256"]) == (wbits, valid, len(raw), hashlib.sha256(raw).hexdigest()), e["label"]
        assert len(comp) <= 64466 * len(e.get("files", [0])), e["label"]  # (no file larger than the largest under tests/golden/emitter/)


def test_valid_vectors_decode_to_what_the_emitter_expects(made, committed):
    """three opinions: the emitter's output (exact-fit capacity), the oracle's, libbrotlidec's where the image has it"""
    n = 0
    for e, comp in committed:
        if not e["valid"]:
            continue
        raw, log = made[e["label"]][2], made[e["label"]][3]
        info, out = oracle.decode(comp, len(raw), 0)
        assert (info.result, info.error_code, info.decoded_size, info.consumed) == (1, 1, len(raw), len(comp)), e["label"]
        assert out == raw, e["label"]
        assert (info.num_commands, info.num_metablocks) == (e["commands"], e["metablocks"]) and info.num_commands == len(log), e["label"]
        if ref.available():
            r = ref.decode(comp, len(raw), False)
            assert r[0] == 1 and r[2] == raw and r[3] == len(comp), e["label"]
        n += 1
    assert n >= 70, n


def test_invalid_vectors_fail_the_same_way_everywhere(made, committed):
    """F and the invalid part of E: the manifest's triple is the oracle's; the oracle and libbrotlidec agree under the rule of
    test_oracle.py::test_differential_vs_libbrotlidec (codes equal, or the {-9, -10} pair; one output a prefix of the other);
    whatever comes out is a prefix of what the emitter had put out in front of the offending command"""
    n = 0
    for e, comp in committed:
        if e["valid"]:
            continue
        raw = made[e["label"]][2]
        cap = len(raw) + 64
        info, out = oracle.decode(comp, cap, 0)
        assert [info.result, info.error_code, info.decoded_size] == e["oracle"] and info.result == 0, e["label"]
        assert out == raw[:len(out)], e["label"]
        if ref.available():
            res, code, rout, _ = ref.decode(comp, cap, False)
            assert res == 0 and (code == info.error_code or {code, info.error_code} == {-9, -10}), (e["label"], code, info.error_code)
            assert out == rout[:len(out)] or rout == out[:len(rout)], e["label"]
            assert rout == raw[:len(rout)], e["label"]
        n += 1
    assert n >= 30, n
    codes = {e["label"].rsplit("-", 1)[0]: e["oracle"][1] for e, _ in committed if not e["valid"]}
    assert codes["F-t121"] == codes["F-tmax"] == -11 and codes["F-len3"] == codes["F-len25"] == -12
    assert codes["F-ring-zero"] == codes["F-ring-minus2"] == -16 and {codes["F-mlen-plus1"], codes["F-mlen-plus1-ring-end"]} <= {-9, -10}


def test_the_emitters_transforms_agree_with_the_oracles():
    """all 121 transforms on 200 seeded dictionary words and on the multi-byte ones of vector A: localises a disagreement"""
    L = oracle.lib()
    rnd = random.Random(121)
    words = [(length, rnd.randrange(M.nwords(length))) for length in (rnd.randrange(4, 25) for _ in range(200))] + M.multibyte_words()
    for length, idx in words:
        word = E.dictionary_word(length, idx)
        for t in range(E.NUM_TRANSFORMS):
            dst, src = ctypes.create_string_buffer(64), ctypes.create_string_buffer(word + b"\0" * 8)
            n = L.brotli_oracle_transform(dst, src, length, t)
            assert dst.raw[:n] == E.transform_word(word, t), (length, idx, t)


def _words(log):
    return [r for r in log if r["word"] and not r.get("invalid")]


def test_coverage_of_the_matrix(made):
    """A (and B, which repeats A's matrix): all 21 x 121 pairs; indices 0, last and others; the pairs of total 0; at least two
    literals behind every word; at least 40 multi-byte words through every transform built on the two uppercase ones"""
    for label in ("A1-matrix-cf", "A1-matrix-ctx", "B-matrix-w10-cf", "B-matrix-w16-ctx"):
        log = made[label][3]
        ws = _words(log)
        assert {(r["copy_len"], r["transform"]) for r in ws} == {(l, t) for l in range(4, 25) for t in range(121)}, label
        assert all(r["coding"] == "explicit" for r in ws)
        kinds = collections.Counter("first" if r["word_idx"] == 0 else "last" if r["word_idx"] == M.nwords(r["copy_len"]) - 1 else "other" for r in ws)
        assert min(kinds["first"], kinds["last"], kinds["other"]) >= 800, kinds
        assert sum(1 for r in ws if r["total"] == 0) >= 10 and sum(1 for r in ws if r["total"] == 1) >= 5, label
        if label.startswith("A1"):
            assert len(log) == 2541 + 1 and all(log[i + 1]["insert"] >= 2 for i, r in enumerate(log) if r["word"]), label
            assert all(r["max_distance"] == r["pos"] for r in ws), label  # (window 22 never fills: the word's number depends on P)
    log = made["A2-multibyte-cf"][3]
    upper = set(M.uppercase_transforms())
    assert len(upper) >= 30 and any(E.tables()["transforms"][t][0] and E.tables()["transforms"][t][2] for t in upper)
    by_word = collections.defaultdict(set)
    for r in _words(log):
        by_word[(r["copy_len"], r["word_idx"])].add(r["transform"])
    two = [k for k in by_word if any(0xC0 <= c < 0xE0 for c in E.dictionary_word(*k))]
    three = [k for k in by_word if any(c >= 0xE0 for c in E.dictionary_word(*k))]
    assert len(by_word) >= 40 and len(two) >= 20 and len(three) >= 20 and all(v == upper for v in by_word.values())
    assert all(log[i + 1]["insert"] >= 2 for i, r in enumerate(log) if r["word"])


def test_coverage_of_the_full_windows(made):
    """B: at window 10 the maximum distance is 1008 from the first few dozen commands on; at window 16 P passes 65520 inside
    a run of 140 one-word commands"""
    ws = _words(made["B-matrix-w10-cf"][3])
    assert sum(1 for r in ws if r["max_distance"] == 1008) >= len(ws) - 100 and ws[0]["max_distance"] == ws[0]["pos"] < 1008
    log = made["B-matrix-w16-cf"][3]
    run = [i for i, r in enumerate(log) if r["word"] and r["insert"] == 0]
    assert len(run) >= 139 and run[-1] - run[0] == len(run) - 1
    before = [i for i in run if log[i]["pos"] < 65520]
    assert 20 <= len(before) <= 120 and all(log[i]["max_distance"] == 65520 for i in run if i not in before)
    assert log[before[-1]]["pos"] + log[before[-1]]["total"] > 65520 or log[before[-1] + 1]["pos"] >= 65520


def test_coverage_of_the_text_like_vector(made):
    """C: a word every 8 commands or so; every ring code at least 20 times, at least once straight behind a word and once
    straight behind a code-0 command (the two predecessors that do not push); the implicit distance straight behind a word at
    least 20 times"""
    for label in ("C-text-cf", "C-text-ctx", "C-text-cf4"):
        log = made[label][3]
        assert len(log) >= 6000
        n_words = sum(1 for r in log if r["word"])
        assert len(log) / 12 <= n_words <= len(log) / 6, n_words
        plain = [r for r in log if not r["word"] and r["coding"] != "tail"]
        share = collections.Counter(r["coding"] for r in plain)
        assert 0.2 <= share["explicit"] / len(plain) <= 0.4 and 0.4 <= share["ring"] / len(plain) <= 0.6 and 0.1 <= share["implicit"] / len(plain) <= 0.3, share
        assert all(2 <= r["copy_len"] <= 70 for r in plain) and all(r["insert"] <= 12 for r in log[2:-1])
        assert {r["copy_len"] for r in plain} == set(range(2, 71))
        codes = collections.Counter(r["code"] for r in log if r["coding"] == "ring" and not r["word"])
        assert all(codes[k] >= 20 for k in range(16)), codes
        after_word = {r["code"] for p, r in zip(log, log[1:]) if p["word"] and r["coding"] == "ring" and not r["word"]}
        after_zero = {r["code"] for p, r in zip(log, log[1:]) if p["coding"] == "ring" and p["code"] == 0 and not p["word"] and r["coding"] == "ring" and not r["word"]}
        assert after_word == set(range(16)) and after_zero == set(range(16)), (after_word, after_zero)
        assert sum(1 for p, r in zip(log, log[1:]) if p["word"] and r["coding"] == "implicit" and not r["word"]) >= 20


def test_coverage_of_the_chains(made):
    """D: chains of 2, 8, 9, 20 and 64 one-word commands without literals; every word of index 0 or the last, with a
    transform whose neighbour on that side gives another total"""
    log = made["D-chains-cf"][3]
    chains, i = [], 0
    while i < len(log):
        if log[i]["word"]:
            j = i
            while j + 1 < len(log) and log[j + 1]["word"] and log[j + 1]["insert"] == 0:
                j += 1
            chains.append(log[i:j + 1]); i = j + 1
        else:
            i += 1
    assert sorted(len(c) for c in chains) == sorted([2, 8, 9, 20, 64] * 3)
    for c in chains:
        for r in c:
            last = M.nwords(r["copy_len"]) - 1
            assert r["word_idx"] in (0, last)
            nb = r["transform"] + (1 if r["word_idx"] == last else -1)
            assert 0 <= nb < 121 and len(E.transform_word(E.dictionary_word(r["copy_len"], 0), nb)) != r["total"] > 0
    assert {r["word_idx"] == 0 for c in chains for r in c} == {True, False}
    plain = [r for r in log if not r["word"]]
    assert sum(r["insert"] + r["total"] for r in plain) // len(chains) >= 300  # (300 bytes of plain commands between the chains)


def test_coverage_of_the_ring_codes_that_name_words(made):
    """E: codes 0 .. 3 against the initial ring at P = 0, 1, 2, 3, 5, 12 wherever the distance exceeds P; codes 4 .. 15 whose
    -+ 1 .. 3 lands on P + 1 .. P + 3; the same with copy lengths 2, 3 and 25, which no decoder may accept"""
    first = {label: v[3][0] for label, v in made.items() if label.startswith("E-")}
    valid = {label: r for label, r in first.items() if made[label][4]}
    assert all(r["coding"] == "ring" and r["word"] and r["distance"] > r["pos"] == r["max_distance"] for r in first.values())
    assert all(r["total"] >= 4 and r["transform"] == 0 for r in valid.values())
    for kind in ("cf", "ctx"):
        got = {(r["pos"], r["code"]) for label, r in valid.items() if label.endswith("-" + kind) and r["code"] < 4}
        assert got == {(p, k) for p in (0, 1, 2, 3, 5, 12) for k in range(4) if E.RING_INIT[k] > p}, got
        high = {r["code"]: r["distance"] - r["pos"] for label, r in valid.items() if label.endswith("-" + kind) and r["code"] >= 4}
        assert set(high) == set(range(4, 16)) and set(high.values()) == {1, 2, 3}, high
        bad = {(r["code"], r["copy_len"]) for label, r in first.items() if label.endswith("-" + kind) and not made[label][4]}
        assert len(bad) == 9 and {c for _, c in bad} == {2, 3, 25} and all(first[l].get("invalid") for l in first if not made[l][4])
    # behind such a word the ring is as it was: the implicit distance and code 1 are the initial 4 and 11
    for label in valid:
        log = made[label][3]
        assert (log[1]["coding"], log[1]["distance"], log[2]["code"], log[2]["distance"]) == ("implicit", 4, 1, 11) and not log[1]["word"] and not log[2]["word"]


def test_coverage_of_the_ring_codes_that_name_words_deep_in_a_stream(made):
    """E2: behind a copy at the maximum distance a ring code that adds 1 .. 3 names a word; 60 of them between commands of C's
    make-up, 12 before the window (16) is full and 48 after; codes 5, 7, 9 on the last and 11, 13, 15 on the second last
    distance; the implicit distance behind each is the copy's again"""
    for kind in ("cf", "ctx"):
        log = made["E2-ring-words-deep-" + kind][3]
        hits = [i for i, r in enumerate(log) if r["word"] and r["coding"] == "ring"]
        assert len(hits) == 60 and len(log) >= 3000
        assert sum(1 for i in hits if log[i]["max_distance"] == log[i]["pos"]) == 12 and sum(1 for i in hits if log[i]["max_distance"] == 65520) == 48
        assert {log[i]["code"] for i in hits} == {5, 7, 9, 11, 13, 15} and {log[i]["distance"] - log[i]["max_distance"] for i in hits} == {1, 2, 3}
        assert all(log[i]["total"] == log[i]["copy_len"] and log[i]["transform"] == 0 for i in hits) and min(hits) >= 300
        for i in hits:
            far = log[i - 1] if log[i]["code"] < 10 else log[i - 2]
            assert not far["word"] and far["coding"] == "explicit" and far["distance"] == far["max_distance"]
            assert log[i + 1]["coding"] == "implicit" and not log[i + 1]["word"] and log[i + 1]["distance"] == log[i - 1]["distance"]


def test_the_faults_lie_deep_in_their_streams(made):
    """F: at least 3000 valid commands of C's make-up in front of each fault; G: the last command is the word"""
    for label, (wbits, comp, raw, log, valid) in made.items():
        if label.startswith("F-"):
            assert len(log) > 3000 and sum(1 for r in log[:3000] if r["word"]) >= 250 and {r["code"] for r in log[:3000] if r["coding"] == "ring"} == set(range(16)), label
            if not valid and "mlen" not in label:
                assert log[-1].get("invalid") and not any(r.get("invalid") for r in log[:-1]), label
    assert made["F-t121-cf"][3][-1]["distance"] - made["F-t121-cf"][3][-1]["max_distance"] - 1 == 121 << 10
    b = made["F-boundary-cf"][3]
    assert (b[-3]["word"], b[-3]["word_idx"], b[-3]["transform"], b[-3]["copy_len"]) == (True, 0, 0, 4) and b[-3]["distance"] == b[-3]["max_distance"] + 1
    assert not b[-2]["word"] and b[-2]["distance"] == b[-2]["max_distance"] == b[-2]["pos"]
    assert made["F-mlen-plus1-ring-end-cf"][3][-1]["pos"] + made["F-mlen-plus1-ring-end-cf"][3][-1]["total"] == 131073
    for name, total in (("total1", 1), ("total2", 2)):
        assert made["G-%s-cf" % name][3][-1]["word"] and made["G-%s-cf" % name][3][-1]["total"] == total
    g = made["G-utf8-upper-cf"][3][-1]
    prefix, kind, suffix = E.tables()["transforms"][g["transform"]]
    assert g["word"] and kind == 11 and prefix and suffix and any(c >= 0xE0 for c in E.dictionary_word(g["copy_len"], g["word_idx"]))
    for kind in ("cf", "ctx"):
        log = made["H-small-" + kind][3]
        assert sum(1 for r in log if r["word"]) >= 30 and len(made["H-small-" + kind][2]) <= 600


def test_the_context_plan_has_many_trees_that_differ():
    """CTX: modes UTF8 and SIGNED on two literal block types, 64 contexts on at least 16 trees; the literal histograms of the
    trees differ (else a wrong p1 / p2 behind a word would go unnoticed)"""
    p = M.plan("ctx")
    assert p.modes == [2, 3] and len(set(p.lit_map)) >= 16 and {t for t, _ in p.lit_blocks} == {0, 1}
    real = M.realise(M.text_commands(random.Random(3), 1500) + [(4, 0, 0)], 22, 5)
    _, out, log, _ = M.emit(real, "ctx", 22)
    type_of = [t for t, c in p.lit_blocks[:200] for _ in range(c)]
    hist, k = collections.defaultdict(collections.Counter), 0
    for r, (ins, _, _) in zip(log, real):
        at = r["pos"] - len(ins)  # (the log's position is that of the copy part)
        for j, b in enumerate(ins):
            p1 = out[at + j - 1] if at + j >= 1 else 0; p2 = out[at + j - 2] if at + j >= 2 else 0
            t = type_of[k]; k += 1
            hist[p.lit_map[t * 64 + E.literal_context(p.modes[t], p1, p2)]][b] += 1
    assert len(hist) >= 16
    top = {tree: tuple(b for b, _ in h.most_common(3)) for tree, h in hist.items() if sum(h.values()) >= 50}
    assert len(top) >= 12 and len(set(top.values())) >= len(top) - 1, top
