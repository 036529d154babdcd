"""tests/golden/emitter_copies/ on the CPU: the generator (tools/make_copy_vectors.py) writes the committed bytes again, the
emitter's idea of the output equals the oracle's and libbrotlidec's, and the emitter's command log shows that the vectors hold
what they are for: all 704 command symbols with both extremes of their extra fields, every reachable distance symbol under
nine (NPOSTFIX, NDIRECT) pairs, every cell of the copy matrix at sixteen destination alignments, the chains, the window's edge.
The log is the emitter's; no decoder is asked what a stream contains.  Nothing here skips."""
import collections
import hashlib
import os
import sys

import pytest

import copy_vectors
import libbrotli_ref as ref
import oracle_lib as oracle
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import make_copy_vectors as C  # noqa: E402


@pytest.fixture(scope="module")
def made():
    """{label: (window, stream, output, log, notes)} as the generator makes them now"""
    return {label: rest for label, *rest in C.vectors()}


@pytest.fixture(scope="module")
def committed():
    return copy_vectors.load()


def test_generator_writes_the_committed_bytes_again(made, committed):
    assert [e["label"] for e, _ in committed] == list(made)
    for e, comp in committed:
        wbits, again, raw, log, meta = made[e["label"]]
        assert comp == again, e["label"]
        assert (e["window"], e["size"], e["sha256"], e["npostfix"], e["ndirect"]) == (wbits, len(raw), hashlib.sha256(raw).hexdigest(), meta["npostfix"], meta["ndirect"]), e["label"]
        parts = e.get("files", [0])
        assert len(parts) <= copy_vectors.MAX_PARTS and len(comp) <= copy_vectors.MAX_FILE * len(parts), e["label"]
        assert ("hex" in e) == (len(comp) < 256)
    for name in os.listdir(copy_vectors.DIR):
        assert os.path.getsize(os.path.join(copy_vectors.DIR, name)) <= copy_vectors.MAX_FILE or name == "manifest.json", name
    assert os.path.getsize(os.path.join(copy_vectors.DIR, "manifest.json")) < 1 << 20


def test_valid_vectors_decode_to_what_the_emitter_expects(made, committed):
    """three opinions: the emitter's output (exact-fit capacity), the oracle's, libbrotlidec's where the image has it"""
    for e, comp in committed:
        raw, log = made[e["label"]][2], made[e["label"]][3]
        info, out = oracle.decode(comp, len(raw), 0)
        assert (info.result, info.error_code, info.decoded_size, info.consumed) == (1, 1, len(raw), len(comp)), e["label"]
        assert out == raw, e["label"]
        assert (info.num_commands, info.num_metablocks) == (e["commands"], e["metablocks"]) and info.num_commands == len(log), e["label"]
        if ref.available():
            r = ref.decode(comp, len(raw), False)
            assert r[0] == 1 and r[2] == raw and r[3] == len(comp), e["label"]
        assert not any(r["word"] for r in log), e["label"]
    assert len(committed) >= 60


def _codes(r):
    ic = E._code_of(r["insert"], E._INS_BASE, E._INS_EXTRA)
    cc = E._code_of(r["copy_len"], E._COPY_BASE, E._COPY_EXTRA)
    return ic, cc


@pytest.mark.parametrize("kind", ["cf", "ctx"])
def test_coverage_of_the_command_symbols(made, kind):
    """S1a + S1b: all 704 symbols; every (insert code, copy code) pair with an explicit distance and the 8 x 16 pairs with the
    implicit one, each with both extra fields all zeros and with both all ones (a 24-bit field: 0, 1 and a value with bit 16 set).
    S2: insert code 22 / 23, copy code 22 / 23 and a distance of 20 / 22 extra bits in all eight zero / one patterns."""
    log = [r for label in ("S1a-symbols-", "S1b-symbols-") for r in made[label + kind][3] if r["coding"] != "tail"]
    cells = collections.defaultdict(set)
    for r in log:
        (ic, iv, ib), (cc, cv, cb) = _codes(r)
        cells[E.command_symbol(ic, cc, r["coding"] == "implicit")].add((iv, cv))
    assert set(cells) == set(range(704))
    for sym, seen in cells.items():
        cell, ic, cc = sym >> 6, (sym >> 3) & 7, sym & 7
        ic += 8 * (0, 0, 0, 0, 1, 1, 0, 2, 1, 2, 2)[cell]; cc += 8 * (0, 1, 0, 1, 0, 1, 2, 0, 2, 1, 2)[cell]
        ones = lambda bits: (1 << bits) - 1 if bits <= 14 else 1
        assert {(0, 0), (ones(E._INS_EXTRA[ic]), ones(E._COPY_EXTRA[cc]))} <= seen, (sym, ic, cc, seen)
    assert any(r["insert"] - E._INS_BASE[23] >= 1 << 16 for r in log) and any(r["copy_len"] - E._COPY_BASE[23] >= 1 << 16 for r in log)
    assert max(r["insert"] + r["copy_len"] for r in log) < 150000
    # S2
    s2 = made["S2-wide-fields-" + kind]
    wide = collections.defaultdict(set)
    gaps = set()
    for i, r in enumerate(s2[3]):
        if r["insert"] >= E._INS_BASE[22] and r["copy_len"] >= E._COPY_BASE[22]:
            (ic, iv, ib), (cc, cv, cb) = _codes(r)
            sym, dv, nb = E.distance_symbol(r["distance"], 0, 0)
            assert r["coding"] == "explicit" and nb >= 20
            wide[(ic, cc, nb)].add((iv == 0, cv == 0, dv == 0))
            assert dv in (0, (1 << nb) - 1) and (iv == 0 or iv & (iv + 1) == 0 or iv >> 16) and (cv == 0 or cv & (cv + 1) == 0)
            gaps.add(s2[3][i + 1]["insert"])
    assert set(wide) == {(ic, cc, nb) for ic in (22, 23) for cc in (22, 23) for nb in (20, 22)} and all(len(v) == 8 for v in wide.values())
    assert {0, 2} <= gaps and len(s2[3]) >= 200 and s2[0] == 24


def _ring_walk(log):
    """-> per command the ring in front of it (section 4: code 0, the implicit distance and words do not push)"""
    ring, out = list(E.RING_INIT), []
    for r in log:
        out.append(tuple(ring))
        if r["coding"] in ("explicit", "ring") and r["code"] != 0 and not r["word"]:
            ring = [r["distance"]] + ring[:3]
    return out


@pytest.mark.parametrize("kind", ["cf", "ctx"])
def test_coverage_of_the_distance_symbols(made, kind):
    """D: per (NPOSTFIX, NDIRECT) every direct code and every distance symbol whose first distance is at most the maximum
    distance, at its first distance and at its last one or the maximum distance; the maximum distance itself; explicit distances
    equal to each of the four ring entries with ring codes 1, 2, 3 behind them; copy lengths 2, 3, 4, 9, 17, 70; no words"""
    for npostfix, ndirect in C.PAIRS:
        wbits, comp, raw, log, meta = made["D-p%d-d%d-%s" % (npostfix, ndirect, kind)]
        assert wbits == (24 if (npostfix, ndirect) in ((0, 0), (3, 120)) else 18) and (meta["npostfix"], meta["ndirect"]) == (npostfix, ndirect)
        md = (1 << wbits) - 16
        body = [r for r in log if r["max_distance"] == md]
        seen = collections.defaultdict(set)
        for r in body:
            if r["coding"] == "explicit":
                sym, dv, nb = E.distance_symbol(r["distance"], npostfix, ndirect)
                seen[sym].add(r["distance"])
        want = 0
        for sym in range(16, 16 + ndirect + (48 << npostfix)):
            if sym < 16 + ndirect:
                assert seen[sym] == {sym - 15}, sym
                continue
            first, last, nb = C._dist_range(sym, npostfix, ndirect)
            if first <= md:
                top = last if last <= md else md - (md - first) % (1 << npostfix)   # (the symbol's last distance, or its last one within the maximum distance)
                assert {first, top} <= seen[sym] and all(first <= d <= last and (d - first) % (1 << npostfix) == 0 for d in seen[sym]), (npostfix, ndirect, sym)
                want += 1
            else:
                assert sym not in seen
        assert want >= (2 * (wbits - 3 - npostfix)) << npostfix, want   # (extra-bit widths 1 .. wbits - 3 - NPOSTFIX are reachable whole)
        assert any(r["distance"] == md for r in body) and {r["copy_len"] for r in body if r["coding"] != "tail"} == {2, 3, 4, 9, 17, 70}
        assert all(r["insert"] <= 3 for r in body) and not any(r["word"] for r in log)
        rings = _ring_walk(log)
        dup = collections.Counter()
        for i, r in enumerate(log[:-4]):
            if r["coding"] == "explicit" and [x["code"] for x in log[i + 1:i + 4]] == [1, 2, 3]:
                dup[rings[i].index(r["distance"])] += 1
        assert all(dup[k] == 3 for k in range(4)), dup


def test_coverage_of_the_copy_matrix(made):
    """M: every (distance, length) cell once, none dropped and none a word; per length all sixteen destination addresses modulo
    16; at window 16 (NPOSTFIX 3, NDIRECT 120) the three distances beyond 65520 are the maximum distance"""
    for label in ("M-rows-w22-cf", "M-mixed-w22-ctx", "M-rows-w16-ctx", "M-mixed-w16-cf"):
        wbits, comp, raw, log, meta = made[label]
        md = (1 << wbits) - 16
        cells = log[2:-1]
        assert len(cells) == len(C.M_DIST) * len(C.M_LEN) == 92 * 41
        assert collections.Counter((r["distance"], r["copy_len"]) for r in cells) == collections.Counter((min(d, md), n) for d in C.M_DIST for n in C.M_LEN)
        assert all(r["coding"] == "explicit" and not r["word"] and r["total"] == r["copy_len"] and r["insert"] <= 15 for r in cells)
        align = collections.defaultdict(set)
        for r in cells:
            align[r["copy_len"]].add(r["pos"] % 16)
        assert all(align[n] == set(range(16)) for n in C.M_LEN)
        for n in C.M_LEN:
            assert any(r["distance"] < n for r in cells if r["copy_len"] == n) and any(r["distance"] >= n for r in cells if r["copy_len"] == n)
        assert (meta["npostfix"], meta["ndirect"]) == ((3, 120) if wbits == 16 else (0, 0))
        rows = [(r["distance"], r["copy_len"]) for r in cells]
        assert (rows == [(min(d, md), n) for d in C.M_DIST for n in C.M_LEN]) == ("rows" in label)


def test_coverage_of_the_text_like_vector(made):
    """T: at least 6000 commands (the long form 16000 and more than 64 KiB); 0 .. 12 literals; copies of 2 .. 70 bytes, those of more
    than 63 rare; explicit, ring and implicit distances; lengths 15 .. 17, lengths 62 .. 64 and distances below the copy length
    at least 5 % of the commands each"""
    for label in ("T-text-cf", "T-text-ctx", "T-text-cf4", "T2-text-long-cf"):
        log = made[label][3]
        plain = [r for r in log if r["coding"] != "tail"]
        assert len(plain) >= (16000 if label.startswith("T2") else 6000)
        share = collections.Counter(r["coding"] for r in plain)
        assert 0.2 <= share["explicit"] / len(plain) <= 0.4 and 0.4 <= share["ring"] / len(plain) <= 0.6 and 0.1 <= share["implicit"] / len(plain) <= 0.3, share
        assert all(2 <= r["copy_len"] <= 70 for r in plain) and all(r["insert"] <= 12 for r in log[2:-1])
        assert sum(1 for r in plain if r["copy_len"] > 63) <= 0.05 * len(plain)
        assert {r["copy_len"] for r in plain if r["copy_len"] <= 63} >= {n for n in C.M_LEN if n <= 63}
        for what in (lambda r: 15 <= r["copy_len"] <= 17, lambda r: 62 <= r["copy_len"] <= 64, lambda r: r["distance"] < r["copy_len"]):
            assert sum(1 for r in plain if what(r)) >= 0.05 * len(plain)
        assert {r["code"] for r in plain if r["coding"] == "ring"} == set(range(16))
    assert len(made["T2-text-long-cf"][1]) > 65536


def test_coverage_of_the_chains(made):
    """H: chains of every depth x unit x (no literal, one literal), each link's source range the destination range of the link
    before; chains that touch in one byte; sources that straddle P - 300 at 400 consecutive commands, three times; staged and
    unstaged stretches of at least 300 commands with every self-overlapping shape inside them"""
    wbits, comp, raw, log, meta = made["H-chains-cf"]
    assert sorted((d, u, l) for _, d, u, l in meta["chains"]) == sorted((d, u, l) for d in C.H_DEPTHS for u in C.H_UNITS for l in (0, 1))
    for at, depth, unit, lits in meta["chains"]:
        for k in range(at, at + depth):
            r, p = log[k], log[k - 1]
            assert r["copy_len"] == p["copy_len"] == unit and r["insert"] == lits and not r["word"]
            assert (r["pos"] - r["distance"], r["pos"] - r["distance"] + unit) == (p["pos"], p["pos"] + unit), (at, k)
        assert log[at + depth]["pos"] - log[at + depth]["distance"] != log[at + depth - 1]["pos"]   # (the chain ends here)
    assert len(meta["edges"]) == 16
    for at, depth, unit, kind in meta["edges"]:
        for k in range(at, at + depth):
            r, p = log[k], log[k - 1]
            src = (r["pos"] - r["distance"], r["pos"] - r["distance"] + unit - 1)
            assert (src[1] == p["pos"]) if kind == "last" else (src[0] == p["pos"] + unit - 1), (at, k, kind)
    assert len(meta["straddle"]) == 3
    for at in meta["straddle"]:
        run = log[at:at + 400]
        assert {r["copy_len"] for r in run} == set(range(2, 41)) and {r["pos"] - 300 - (r["pos"] - r["distance"] + r["copy_len"]) for r in run} == {0, 1, 2, 3}
    assert len({log[at]["pos"] % 4096 for at in meta["straddle"]}) == 3
    for at in meta["near"]:
        run = [r for r in log[at:at + 340] if r["copy_len"] <= 12]
        assert len(run) >= 300 and all(r["distance"] <= 60 for r in run) and sum(r["insert"] + r["total"] for r in run) < 32768
    for at in meta["far"]:
        run = [r for r in log[at:at + 340] if 1000 <= r["copy_len"] <= 3000 and r["distance"] >= 20000]
        assert len(run) >= 300
    assert collections.Counter((log[i]["distance"], log[i]["copy_len"]) for i in meta["self"]) == collections.Counter(C.H_SELF * 2)
    near = [i for i in meta["self"] if any(a <= i < a + 340 for a in meta["near"])]
    assert {(log[i]["distance"], log[i]["copy_len"]) for i in near} == set(C.H_SELF) and len(near) == 40
    assert made["H-chains-ctx"][2] == raw


def test_coverage_of_the_windows_edge(made):
    """W: at windows 10, 11 and 16 a copy at exactly the maximum distance at P = distance, one command before the window fills, on
    the command that fills it and 50 commands after, the implicit distance behind each; lengths 2, 16, 64 and 1008"""
    for wbits in (10, 11, 16):
        _, comp, raw, log, meta = made["W-edge-w%d-cf" % wbits]
        md = (1 << wbits) - 16
        at = meta["at"]
        far = [i for i, r in enumerate(log) if r["coding"] == "explicit" and r["distance"] == r["max_distance"] and (i in at.values() or i > at["after"])]
        assert len(far) >= 7 and all(log[i + 1]["coding"] == "implicit" and log[i + 1]["distance"] == log[i]["distance"] for i in far)
        first, before, on = log[at["first"]], log[at["before"]], log[at["on"]]
        assert first["pos"] == first["distance"] == 24 and at["first"] == 0
        assert before["pos"] == before["distance"] < md and before["pos"] + before["total"] < md and at["on"] == at["before"] + 2
        assert on["pos"] == on["distance"] < md <= on["pos"] + on["total"]
        assert at["after"] == at["on"] + 2 + 50
        late = [log[i] for i in far if i >= at["after"]]
        assert [r["copy_len"] for r in late] == [1008, 64, 16, 2] and all(r["distance"] == md == r["max_distance"] for r in late)
        assert {first["copy_len"], before["copy_len"], on["copy_len"]} == {2, 16, 64} and not any(r["word"] for r in log)
        if wbits == 10:
            assert late[0]["copy_len"] == md   # (the whole window)


def test_the_limit_streams_end_in_their_copy(made):
    """L: 3000 commands of T's make-up and one final copy of each execution shape"""
    got = []
    for label, (wbits, comp, raw, log, meta) in made.items():
        if label.startswith("L-") and label.endswith("-cf"):
            assert len(log) == 3001 and (log[-1]["copy_len"], log[-1]["distance"]) == tuple(meta["final"]) and log[-1]["coding"] == "explicit"
            assert log[-1]["pos"] + log[-1]["copy_len"] == len(raw) and made[label[:-2] + "ctx"][2] == raw
            got.append(tuple(meta["final"]))
    assert got == list(C.L_SHAPES)


def test_the_emitters_distance_symbols_agree_with_the_oracles():
    """for the nine (NPOSTFIX, NDIRECT) pairs every distance symbol at three extra-bit values (first, middle, last), each in a stream
    of one command (and closing literals) at P = 2, window 24: a distance beyond 2 names word (distance - 3) of the static dictionary, so the bytes that
    come out say which distance the oracle read -- as far as the words reach (121 transforms of 2048 words of 6 bytes: distances up
    to 247 810); the wider symbols are D's.  Localises a disagreement about the symbol arithmetic."""
    bits = E.tables()["size_bits"]
    clen = max(range(4, 25), key=lambda n: bits[n])
    limit = 2 + (E.NUM_TRANSFORMS << bits[clen])
    n = 0
    for npostfix, ndirect in C.PAIRS:
        p = E.Plan(npostfix=npostfix, ndirect=ndirect)
        dists, whole = set(range(1, ndirect + 1)), 0
        for sym in range(16 + ndirect, 16 + ndirect + (48 << npostfix)):
            first, last, nb = C._dist_range(sym, npostfix, ndirect)
            mid = first + ((last - first) // 2 >> npostfix << npostfix)
            assert [E.distance_symbol(d, npostfix, ndirect)[0] for d in (first, mid, last)] == [sym] * 3
            dists |= {d for d in (first, mid, last) if d <= limit}
            whole += last <= limit
        assert whole >= (2 * (15 - npostfix)) << npostfix and len(dists) >= ndirect + 2 * whole, (whole, len(dists))
        for d in sorted(dists):
            w = E.BitWriter(); E.write_stream_header(w, 24)
            log = []
            raw = E.emit_compressed(w, [(b"ab", clen, d), (b"c", 0, 0)], p, True, wbits=24, log=log)   # (literals behind it: a word may be empty)
            comp = w.finish()
            assert log[0]["word"] == (d > 2) and log[0]["distance"] == d
            info, out = oracle.decode(comp, len(raw) + 8, 0)
            assert (info.result, out) == (1, raw), (npostfix, ndirect, d, E.distance_symbol(d, npostfix, ndirect))
            n += 1
    print(n, "one-command streams")
