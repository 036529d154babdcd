"""tests/golden/emitter_literals/ on the CPU: the generator (tools/make_literal_vectors.py) writes the committed bytes again; the
emitter's idea of every stream equals the oracle's and libbrotlidec's; and the emitter's logs -- one record per literal (`llog`:
bit position, length, the two bytes in front, block type, mode, context, tree) and per command -- show that the vectors hold
every shape, run length, boundary phase, block end, LUT cell, source cell and word cell they are for, and that every probe tells
the right context from each wrong one.  The logs are the emitter's; no decoder is asked what a stream contains; the context of a
probe is worked out once more here, from RFC 7932 section 7.1 and not from the decoders' table.  Nothing here skips."""
import collections
import hashlib
import os
import re
import sys

import pytest

import libbrotli_ref as ref
import literal_vectors
import oracle_lib as oracle
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import make_literal_vectors as L  # noqa: E402


@pytest.fixture(scope="module")
def made():
    """{label: vector} as the generator makes them now"""
    return {v["label"]: v for v in L.vectors()}


@pytest.fixture(scope="module")
def committed():
    return literal_vectors.load()


def test_generator_writes_the_committed_bytes_again(made, committed):
    assert [e["label"] for e, _ in committed] == list(made)
    for e, comp in committed:
        v = made[e["label"]]
        assert comp == v["stream"], e["label"]
        assert (e["family"], e["window"], e["size"], e["runs"], e.get("probes", []), e.get("cells", [])) == \
               (v["family"], v["window"], len(v["output"]), v["runs"], v["probes"], v["cells"]), e["label"]
        assert e["sha"] == hashlib.sha256(v["output"]).hexdigest()[:16], e["label"]
        for k in L.NOTES:
            assert e.get(k) == v.get(k), (e["label"], k)
        parts = e.get("files", [0])
        assert len(parts) <= literal_vectors.MAX_PARTS and len(comp) <= literal_vectors.MAX_FILE * len(parts), e["label"]
        assert ("at" in e) == (len(comp) < 256)
    for name in os.listdir(literal_vectors.DIR):
        assert os.path.getsize(os.path.join(literal_vectors.DIR, name)) <= literal_vectors.MAX_FILE or name == "manifest.json", name
    assert os.path.getsize(os.path.join(literal_vectors.DIR, "manifest.json")) < 1 << 20
    assert len(committed) >= 200


def test_three_opinions_on_every_vector(made, committed):
    """the emitter's output, the oracle's and libbrotlidec's are the same bytes, the whole stream consumed; with the large-window flag alike"""
    for e, comp in committed:
        raw = made[e["label"]]["output"]
        info, out = oracle.decode(comp, e["size"], 0)
        assert (info.result, info.error_code, info.decoded_size, info.consumed) == (1, 1, len(raw), len(comp)) and out == raw, e["label"]
        assert [info.num_metablocks, info.num_commands] == e["counts"], e["label"]
        assert oracle.decode(comp, e["size"], literal_vectors.FLAG_LARGE_WINDOW)[1] == raw, e["label"]
        if ref.available():
            res, code, rout, used = ref.decode(comp, e["size"], False)
            assert res == 1 and rout == raw and used == len(comp), e["label"]


def test_the_llog_changes_nothing_and_tells_the_truth(made):
    """a stream emitted with `llog` is the one emitted without; every record's byte lies at its position in the output, its code word
    at its bit of the stream (read back bit by bit), its context is that of its p1 and p2, and its tree the map's"""
    for label in ("S-deep11-end", "E-stair-block-130-07", "X-maps", "X-boundary"):
        v = made[label]
        out, stream = v["output"], v["stream"]
        bit = lambda i: (stream[i >> 3] >> (i & 7)) & 1
        assert [r["k"] for r in v["llog"] if r["mb"] == 0] == list(range(sum(1 for r in v["llog"] if r["mb"] == 0)))
        for r in v["llog"]:
            assert out[r["pos"]] == r["byte"], (label, r)
            assert r["p1"] == (out[r["pos"] - 1] if r["pos"] >= 1 else 0) and r["p2"] == (out[r["pos"] - 2] if r["pos"] >= 2 else 0), (label, r)
            sc = v["mbs"][r["mb"]]["scheme"]
            if sc is not None:
                assert r["mode"] == sc.modes[r["type"]] and r["context"] == E.literal_context(r["mode"], r["p1"], r["p2"])
                assert r["tree"] == sc.lit_map[r["type"] * 64 + r["context"]], (label, r)
                word, n = E.canonical_codes(sc.trees[r["tree"]])[r["byte"]]
                assert n == r["nbits"] and all(bit(r["bit"] + i) == (word >> i) & 1 for i in range(n)), (label, r)
    w1, w2, ll = E.BitWriter(), E.BitWriter(), []
    cmds = [(b"abcabc", 4, 3), (b"xyz", 0, 0)]
    assert E.emit_compressed(w1, cmds, E.Plan(), True, wbits=22) == E.emit_compressed(w2, cmds, E.Plan(), True, wbits=22, llog=ll)
    assert w1.finish() == w2.finish() and [r["byte"] for r in ll] == list(b"abcabcxyz") and [r["cmd"] for r in ll] == [0] * 6 + [1] * 3


def test_the_kernels_constants_are_the_generators():
    """the lengths of the sweep and the long runs are the thresholds of the literal loops: if one has moved, regenerate"""
    csrc = os.path.join(ROOT, "rust-brotli-decompressor_amd", "csrc")
    k = open(os.path.join(csrc, "brotli_kernels.hip")).read()
    p = open(os.path.join(csrc, "brotli_path_engine.h")).read()

    def one(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0])
    got = {"SPEC_ROUND_MIN": one(k, r"constexpr uint32_t SPEC_ROUND_MIN = (\d+);"), "SP_MIN_MLEN": one(k, r"constexpr uint32_t SP_MIN_MLEN = (\d+)u;"),
           "ROOT_BITS": one(k, r"constexpr int ROOT_BITS = (\d+);"), "PE_RUN_MIN": one(p, r"#define BROTLI_AMD_PE_RUN_MIN (\d+)"),
           "PE_RUN_SB": one(p, r"#define BROTLI_AMD_PE_RUN_SB (\d+)"), "REC_INS_RUN": one(k, r"if \(ins > (\d+)u \|\| ins >= quota"),
           "REC_INS_LONG": one(k, r"if \(ins > (\d+)u\) long_cmd = true;"), "SPEC_WINDOWS": one(k, r"constexpr uint32_t SPEC_WINDOWS = (\d+);")}
    flushes = re.findall(r"if \(lit_n == (\d+)\) (?:FLUSH_LITERALS|\{ if \(lane < 64\) out\[lit_pos)", k)
    assert len(flushes) == 3 and len(set(flushes)) == 1, ("regenerate: the three context loops' flushes", flushes)
    got["LIT_FLUSH"] = int(flushes[0])
    want = {n: getattr(L, n) for n in got}
    assert got == want, "regenerate tests/golden/emitter_literals/ (tools/make_literal_vectors.py): a threshold of the literal loops has moved: %s" % \
        {n: (got[n], want[n]) for n in got if got[n] != want[n]}
    for n in (L.REC_INS_RUN, L.REC_INS_RUN + 1, L.REC_INS_LONG, L.REC_INS_LONG + 1, L.LIT_FLUSH - 1, L.LIT_FLUSH, L.LIT_FLUSH + 1, 2 * L.LIT_FLUSH + 1):
        assert n in L.SWEEP
    assert {L.SPEC_ROUND_MIN - 1, L.SPEC_ROUND_MIN, L.SPEC_ROUND_MIN + 1, L.PE_RUN_MIN - 1, L.PE_RUN_MIN, L.PE_RUN_MIN + 1, 2 * L.PE_RUN_MIN + 1} == set(L.LONG_RUNS)


# ------------------------------------------------------------------ S
def _commands(v, mb=0):
    return [r for r in v["clog"] if r["mb"] == mb]


def test_s_every_shape_has_its_lengths(made):
    """the code of every S vector is the shape it is named for: the lengths of the code words the log shows are the shape's, the
    shallowest and the deepest among them"""
    want = {"simple1": {0}, "simple2": {1}, "simple3": {1, 2}, "simple4a": {2}, "simple4b": {1, 2, 3}, "flat8": {8}, "stair": set(range(1, 16)),
            "deep9": set(range(1, 10)), "deep10": set(range(1, 9)) | {10}, "deep11": set(range(1, 9)) | {11}, "deep12": set(range(1, 9)) | {12}, "grid": {6, 9, 12, 15}}
    assert list(want) == L.SHAPES
    for shape, lens in want.items():
        for place in ("front", "end"):
            v = made["S-%s-%s" % (shape, place)]
            assert (v["shape"], v["place"]) == (shape, place)
            assert {r["nbits"] for r in v["llog"]} == lens, (shape, place)
            assert {r["tree"] for r in v["llog"]} == {0} and {r["type"] for r in v["llog"]} == {0}
    assert {s for s in L.SHAPES if L.depth_of(s) > L.ROOT_BITS} == {"stair", "deep9", "deep10", "deep11", "deep12", "grid"}
    assert [L.depth_of(s) - L.ROOT_BITS for s in ("deep9", "deep10", "deep11", "deep12")] == [1, 2, 3, 4]


def test_s_every_run_length_in_both_places(made):
    """every shape, front and end: one command per insert length 0 .. 140 in a row, a copy of 2 .. 4 bytes from 1 .. 5 back behind each;
    front: the long runs behind the sweep (40 000 for the three deepest shapes), more than 512 bytes of stream behind the sweep's
    last literal and that literal in front of the last 72 dwords; end: the first command a run of PE_RUN_MIN literals, and the
    sweep's last command the stream's last.  MLEN is SP_MIN_MLEN at least."""
    for shape in L.SHAPES:
        for place in ("front", "end"):
            v = made["S-%s-%s" % (shape, place)]
            cl = _commands(v)
            ins = [r["insert"] for r in cl]
            at = next(i for i in range(len(ins)) if ins[i:i + 141] == list(range(141)))
            pad = L.FRONT_PAD if (shape, place) == ("simple1", "front") else 0   # (commands without literals behind the long runs, whose
            assert all(r["insert"] == 0 and not r["word"] for r in cl[len(cl) - pad:])   # literals take no bits: their fields make the 512 bytes)
            cl = cl[:len(cl) - pad]
            ins = ins[:len(cl)]
            for r in cl:
                assert not r["word"] and 2 <= r["copy_len"] <= 4 and 1 <= r["distance"] <= 5 and r["coding"] == "explicit", (shape, place, r)
            assert len(v["output"]) >= L.SP_MIN_MLEN and len(v["mbs"]) == 1
            last_bit = max(r["bit"] + r["nbits"] for r in v["llog"] if r["cmd"] <= at + 140)
            if place == "front":
                assert ins[at + 141:] == L.LONG_RUNS + ([L.HUGE_RUN] if shape in L.DEEPEST3 else []), (shape, ins[at + 141:])
                assert last_bit + 8 * 512 <= 8 * len(v["stream"]) - 72 * 32, shape
            else:
                assert at + 141 == len(cl) and ins[0] == L.PE_RUN_MIN and L.SPEC_ROUND_MIN in ins[:at], shape
                assert 8 * len(v["stream"]) - last_bit < 64, shape   # (the last copy's command fields and the padding behind it)


def test_s_the_three_regimes(made):
    """every shape shows 64 literals in a row that are of its shallowest words only (where those are of one bit: 64 symbols in 64
    stream bits), 64 in a row of its deepest only (the staircase: four words of 15 bits in 64 bits -- the `i * 15` bound met
    exactly) and a stretch that mixes every length"""
    for shape in L.SHAPES:
        for place in ("front", "end"):
            v = made["S-%s-%s" % (shape, place)]
            lens = [r["nbits"] for r in v["llog"]]
            lo, hi = min(lens), max(lens)
            runs = {lo: 0, hi: 0}
            best = {lo: 0, hi: 0}
            for n in lens:
                for x in (lo, hi):
                    runs[x] = runs[x] + 1 if n == x else 0
                    best[x] = max(best[x], runs[x])
            assert best[lo] >= 64 and best[hi] >= 64, (shape, place, best)
            if len(set(lens)) > 2:
                assert any(len(set(lens[i:i + 40])) >= min(len(set(lens)), 4) for i in range(0, len(lens) - 40, 20)), (shape, place)
    n = 0
    for shape in L.SHAPES:
        for place in ("front", "end"):
            ll = made["S-%s-%s" % (shape, place)]["llog"]
            if min(r["nbits"] for r in ll) == 1:   # 64 words of one bit that fill one aligned 64-bit window of the stream
                assert any(ll[i]["bit"] % 64 == 0 and all(r["nbits"] == 1 for r in ll[i:i + 64]) for i in range(len(ll) - 64)), (shape, place)
                n += 1
            if L.depth_of(shape) == 15:            # four words of 15 bits inside one window: the most it holds
                assert any(all(r["nbits"] == 15 for r in ll[i:i + 4]) and ll[i]["bit"] // 64 == (ll[i + 3]["bit"] + 14) // 64 for i in range(len(ll) - 4)), (shape, place)
                n += 1
    assert n == 2 * 8 + 2 * 2, n   # (simple2, simple3, simple4b, the staircase and deep9 .. deep12; the staircase and the grid)


def test_s_boundary_phases(made):
    """for every shape of depth 9 or more, front and end: some code word ends exactly on a 64-bit boundary of the stream, some
    straddles one, and some second-level word (longer than ROOT_BITS) starts at every bit phase 0 .. 31; the shapes of depth 15
    have a 15-bit word that ends on bit 63"""
    n = 0
    for shape in L.SHAPES:
        depth = L.depth_of(shape)
        if depth <= L.ROOT_BITS:
            continue
        for place in ("front", "end"):
            ll = made["S-%s-%s" % (shape, place)]["llog"]
            assert any((r["bit"] + r["nbits"]) % 64 == 0 for r in ll), (shape, place)
            assert any(r["bit"] // 64 != (r["bit"] + r["nbits"] - 1) // 64 for r in ll), (shape, place)
            assert {r["bit"] % 32 for r in ll if r["nbits"] > L.ROOT_BITS} == set(range(32)), (shape, place)
            assert any(r["nbits"] > L.ROOT_BITS and (r["bit"] + r["nbits"]) % 64 == 0 for r in ll), (shape, place)
            if depth == 15:
                assert any(r["nbits"] == 15 and (r["bit"] + 15) % 64 == 0 for r in ll), (shape, place)
            n += 1
    assert n == 12
    # the path engine's parts of PE_RUN_SB stream bits: in the runs of PE_RUN_MIN literals or more, words that straddle two parts
    for shape in ("stair", "deep12", "grid", "flat8"):
        v = made["S-%s-front" % shape]
        long_cmds = {i for i, r in enumerate(_commands(v)) if r["insert"] >= L.PE_RUN_MIN}
        assert any(r["cmd"] in long_cmds and r["bit"] // L.PE_RUN_SB != (r["bit"] + r["nbits"] - 1) // L.PE_RUN_SB for r in v["llog"]), shape


# ------------------------------------------------------------------ E
def _run_literals(v, at, n):
    ll = [r for r in v["llog"] if at <= r["pos"] < at + n]
    assert [r["pos"] for r in ll] == list(range(at, at + n)), v["label"]
    return ll


def test_e_block_ends(made):
    """under the staircase and the flat code: a literal block ends after each of the first 66 literals of a run of 130, after literals
    766 .. 770 of a run of 800, and round literal 768 and 6000 of a run of 6100; the switch goes to a type whose code is another"""
    for code in L.E_CODES:
        seen = collections.Counter()
        for v in made.values():
            if not v["label"].startswith("E-%s-block-" % code):
                continue
            at, n = v["run"]
            ll = _run_literals(v, at, n)
            assert len({r["cmd"] for r in ll}) == 1
            firsts = [i for i, r in enumerate(ll) if r["first_of_block"] and i]
            assert firsts == v["ends"], v["label"]
            for i in firsts:
                assert ll[i]["type"] != ll[i - 1]["type"] and ll[i]["tree"] != ll[i - 1]["tree"], v["label"]
            assert len(v["output"]) >= L.SP_MIN_MLEN or n == 130
            seen[n] += 1
            for i in firsts:
                seen[(n, i)] += 1
        assert all(seen[(130, j)] == 1 for j in range(1, 67)) and seen[130] == 66, code
        assert all(seen[(800, j)] == 1 for j in range(L.SPEC_ROUND_MIN - 2, L.SPEC_ROUND_MIN + 3)), code
        assert all(seen[(6100, j)] == 1 for j in list(range(L.SPEC_ROUND_MIN - 2, L.SPEC_ROUND_MIN + 3)) + list(range(L.PE_RUN_MIN - 2, L.PE_RUN_MIN + 3))), code
    # no two vectors of E put out the same bytes, and every block end of the staircase's lies among code words of several lengths
    es = [v for v in made.values() if v["family"] == "E"]
    assert len({hashlib.sha256(v["output"]).hexdigest() for v in es}) == len(es)
    for v in es:
        if v["label"].startswith("E-stair-block-"):
            ll = _run_literals(v, *v["run"])
            for i in v["ends"]:
                assert len({r["nbits"] for r in ll[max(0, i - 40):i + 40]}) >= 4, (v["label"], i)
    # the two codes of a vector differ: the same byte has another word in them
    for code in L.E_CODES:
        a, b = (f(None, 256) for f in (L.e_plan(code).codes[("lit", 0)], L.e_plan(code).codes[("lit", 1)]))
        assert any(a.codes.get(s) != b.codes[s] for s in b.codes)


def test_e_last_commands_windows_metablocks_and_limits(made):
    for code in L.E_CODES:
        for n in L.LAST_RUNS:
            v = made["E-%s-last-%d" % (code, n)]
            last = v["clog"][-1]
            assert last["coding"] == "tail" and last["insert"] == n and v["run"] == [len(v["output"]) - n, n]
        assert L.LAST_RUNS == [1, 2, 3, 8, 63, 64, 65, 130]
        phases = set()
        for k in range(4):
            v = made["E-%s-window10-%d" % (code, k)]
            assert v["window"] == 10
            for at, n in (v["run"], v["run2"]):
                ll = _run_literals(v, at, n)
                assert len({r["cmd"] for r in ll}) == 1
                cross = [p for p in range(1024, len(v["output"]), 1024) if at < p < at + n]
                assert cross, (v["label"], at, n)   # a flush point of the ring of 1024 bytes inside the run
                phases.add((n, cross[0] - at))
        assert len({p for n, p in phases if n == 100}) >= 3 and len({p for n, p in phases if n == 2000}) >= 3, phases
        for n, m in ((1, 1), (2, 63), (65, 130), (130, 2), (800, 800)):
            v = made["E-%s-two-%d-%d" % (code, n, m)]
            at, total = v["run"]
            ll = _run_literals(v, at, total)
            assert total == n + m and [r["mb"] for r in ll] == [0] * n + [1] * m
            assert v["clog"][ll[0]["cmd"]]["coding"] == "tail" and ll[n]["k"] == 0
        for n in (130, L.SPEC_ROUND_MIN, L.PE_RUN_MIN):
            v = made["E-%s-cap-%d" % (code, n)]
            ll = _run_literals(v, *v["run"])
            assert len({r["cmd"] for r in ll}) == 1 and v["run"][1] == n and _commands(v)[ll[0]["cmd"]]["insert"] == n
            caps = L.cap_sweep(v)
            at = v["run"][0]
            if n == 130:
                assert caps == list(range(at - 2, at + 132))
            else:
                assert all(at + m + k in caps for m in (0, 64, 128, 192, 256) for k in (-2, -1, 0, 1, 2)) and all(at + n - k in caps for k in (1, 2, 3))
                assert n == 130 or len(v["output"]) >= L.SP_MIN_MLEN


# ------------------------------------------------------------------ X
def _lut_rows():
    """RFC 7932 section 7.1: Lut0, Lut1 and Lut2, written out from their description"""
    lut0 = [0] * 9 + [4, 4, 0, 0, 4] + [0] * 18 + [8, 12, 16, 12, 12, 20, 12, 16, 24, 28, 12, 12, 32, 12, 36, 12] + [44] * 10 + [32, 32, 24, 40, 28, 12]
    upper = [48, 52, 52, 52, 48, 52, 52, 52, 48, 52, 52, 52, 52, 52, 48, 52, 52, 52, 52, 52, 48, 52, 52, 52, 52, 52]
    lut0 += [12] + upper + [24, 12, 28, 12, 12] + [12] + [x + 8 for x in upper] + [24, 12, 28, 12, 0] + [0, 1] * 32 + [2, 3] * 32
    lut1 = [0] * 32 + [0] + [1] * 15 + [2] * 10 + [1] * 7 + [2] * 26 + [1] * 6 + [3] * 26 + [1] * 4 + [0] + [0] * 96 + [2] * 32
    lut2 = [0] + [1] * 15 + [2] * 48 + [3] * 64 + [4] * 64 + [5] * 48 + [6] * 15 + [7]
    assert len(lut0) == len(lut1) == len(lut2) == 256
    return lut0, lut1, lut2


def rfc_context(mode, p1, p2):
    lut0, lut1, lut2 = _lut_rows()
    return (p1 & 0x3F, p1 >> 2, lut0[p1] | lut1[p2], (lut2[p1] << 3) | lut2[p2])[mode]


def test_the_rfcs_contexts_are_the_tables():
    for mode in range(4):
        for p1 in range(256):
            for p2 in (0, 1, 31, 32, 47, 48, 64, 65, 96, 97, 127, 128, 191, 192, 223, 224, 255, p1):
                assert rfc_context(mode, p1, p2) == E.literal_context(mode, p1, p2) and rfc_context(mode, p2, p1) == E.literal_context(mode, p2, p1), (mode, p1, p2)


def _behind(v, pos):
    """the copy or word whose output lies last in front of `pos`, as tools/make_literal_vectors.alternatives wants it"""
    last = None
    for r in v["clog"]:
        if r["coding"] != "tail" and r["pos"] <= pos:
            last = r
    if last is None:
        return None
    return (last["pos"], last["total"], None if last["word"] else last["distance"])


def _wrong_contexts(v, pos, mode):
    """the wrong contexts of the literal at `pos`, stated here once more from the output and the command log, ids by RFC 7932:
    (a) swapped, (b) zeros, (d) one byte further back, (f) the other modes; and where the last command part in front of the literal
    put out a byte or more and ends at the literal or one literal in front of it: (c) what was in front of that part -- for the
    second literal, its own p1 and the byte in front of the part --, (e) for a copy longer than its distance the last bytes of its
    source as memory held them before the copy began, bytes the copy had yet to write being zero"""
    o = v["output"]
    at = lambda x: o[x] if x >= 0 else 0
    p1, p2 = at(pos - 1), at(pos - 2)
    out = {"a": rfc_context(mode, p2, p1), "b": rfc_context(mode, 0, 0), "d": rfc_context(mode, p2, at(pos - 3))}
    out.update({"f%d" % m: rfc_context(m, p1, p2) for m in range(4) if m != mode})
    parts = [r for r in v["clog"] if r["coding"] != "tail" and r["pos"] <= pos]
    if parts and parts[-1]["total"] > 0:
        part = parts[-1]
        start, end = part["pos"], part["pos"] + part["total"]
        before = lambda x: at(x) if x < start else 0
        overlaps = not part["word"] and part["distance"] < part["total"]
        tail = end - part["distance"] if overlaps else None   # (one behind the source's last byte)
        if pos == end:
            out["c"] = rfc_context(mode, at(start - 1), at(start - 2))
            if overlaps:
                out["e"] = rfc_context(mode, before(tail - 1), before(tail - 2))
        elif pos == end + 1:
            out["c"] = rfc_context(mode, p1, at(start - 1))
            if overlaps:
                out["e"] = rfc_context(mode, p1, before(tail - 1))
    return out


def _probes(v):
    """-> [(cell, literal record, {alternative: tree}, right tree, scheme)] of a vector's probes"""
    by_pos = {r["pos"]: r for r in v["llog"]}
    out = []
    for i in range(0, len(v["probes"]), 2):
        pos, cell = v["probes"][i], v["cells"][v["probes"][i + 1]]
        r = by_pos[pos]
        sc = v["mbs"][r["mb"]]["scheme"]
        o = v["output"]
        p1, p2 = (o[pos - 1] if pos >= 1 else 0), (o[pos - 2] if pos >= 2 else 0)
        mode = sc.modes[r["type"]]
        right = sc.lit_map[r["type"] * 64 + rfc_context(mode, p1, p2)]
        alts = _wrong_contexts(v, pos, mode)
        assert alts == L.alternatives(o, pos, mode, p1, p2, _behind(v, pos)), (v["label"], cell, pos)   # (the generator chose the byte against these)
        out.append((cell, r, {a: sc.lit_map[r["type"] * 64 + c] for a, c in alts.items()}, right, sc))
    return out


@pytest.fixture(scope="module")
def probes(made):
    return {label: _probes(v) for label, v in made.items() if v["family"] == "X"}


def test_x_every_probe_discriminates(made, probes):
    """every probe of every X vector: the emitter wrote it with the tree of the context that RFC 7932 gives its two bytes, and its code
    word, read with the tree of any wrong context -- swapped, zero, stale, shifted, the copy's source, the other modes -- that is
    another tree, gives another symbol or another length.  A failure names the vector, the cell and the position."""
    n = 0
    for label, ps in probes.items():
        for cell, r, alts, right, sc in ps:
            where = "%s: probe %s at %d (p1 %d, p2 %d, mode %d)" % (label, cell, r["pos"], r["p1"], r["p2"], r["mode"])
            assert r["tree"] == right, "the emitter's context is not the RFC's -- " + where
            word = E.canonical_codes(sc.trees[right])[r["byte"]]
            assert word[1] == r["nbits"], where
            for a, t in alts.items():
                assert t == right or E.canonical_codes(sc.trees[t]).get(r["byte"]) != word, "alternative %s reads the same -- %s" % (a, where)
            n += 1
    assert n >= 5000, n
    # the trees: one profile of depths 6 .. 15, tree i rotated by 5 i symbols, 64 a block type under the identity map
    assert sorted(set(L.PROFILE)) == list(range(6, 16)) and len(L.PROFILE) == 256
    sc = made["X-every-tree"]["mbs"][0]["scheme"]
    assert sc.lit_map == list(range(256)) and all(sc.trees[i] == [L.PROFILE[(s + 5 * i) % 256] for s in range(256)] for i in range(256))
    assert len({tuple(t) for t in sc.trees}) == 256
    assert {r["tree"] for r in made["X-every-tree"]["llog"]} == set(range(256))


def test_x_lut_cells(made, probes):
    """every mode 0 .. 3: every value of p1 with p2 held at two values and every value of p2 with p1 held at two -- each of the four
    bytes of each of the 64 lanes of both LUT rows"""
    for mode in range(4):
        v = made["X-lut-mode%d" % mode]
        h = v["held"]
        ps = [r for cell, r, _, _, _ in probes[v["label"]] if cell == "lut"]
        assert {r["mode"] for r in ps} == {mode}
        for held in set(h[:2]):
            assert {r["p1"] for r in ps if r["p2"] == held} == set(range(256)), (mode, held)
        for held in set(h[2:]):
            assert {r["p2"] for r in ps if r["p1"] == held} == set(range(256)), (mode, held)
        assert len(set(h[:2])) == 2 and len(set(h[2:])) == 2
        assert mode >= 2 or len({r["context"] for r in ps}) == 64


def test_x_source_cells(made, probes):
    """what lies in front of the probe, from the logs: the stream's start, one literal, literals 63, 64, 65, 127 and 128 of a run, copies
    of every listed length that do not overlap themselves, copies that do at distance 1, 2, 3 and 65, a word of two bytes or more, a
    block switch -- each under both block types (UTF8 and SIGNED) -- and a metablock boundary behind every kind of metablock"""
    v = made["X-source"]
    cl = _commands(v)
    seen = collections.defaultdict(set)
    for cell, r, _, _, _ in probes["X-source"]:
        prev = cl[r["cmd"] - 1] if r["cmd"] else None
        idx = r["pos"] - (prev["pos"] + prev["total"]) if prev else r["pos"]   # the literal's number in its command
        base = cell[:-2] if cell.endswith("+1") else cell
        assert idx == (1 if cell.endswith("+1") and not cell.startswith("start") else idx)
        if base.startswith("copy-"):
            n = int(base[5:])
            assert not prev["word"] and prev["copy_len"] == prev["total"] == n and prev["distance"] >= n and idx == (1 if cell.endswith("+1") else 0), cell
        elif base.startswith("overlap-"):
            d = int(base[8:])
            assert not prev["word"] and prev["distance"] == d < prev["copy_len"] and idx == (1 if cell.endswith("+1") else 0), cell
            seen[cell].add(("len", prev["copy_len"]))
        elif base == "word":
            assert prev["word"] and prev["total"] >= 2 and idx == (1 if cell.endswith("+1") else 0), cell
        elif base == "switch":
            assert r["first_of_block"] and r["k"] > 0, cell
        elif base == "literal":
            assert idx == 1 and prev["total"] >= 2
        elif base.startswith("wrap-"):
            assert idx == int(base[5:]), (cell, idx)
        else:
            assert cell in ("start+0", "start+1") and r["pos"] == int(cell[-1]) and r["p2"] == 0 and (r["pos"] or r["p1"] == 0), cell
        seen[cell].add(r["type"])
    for n in L.COPY_CELLS:
        assert {0, 1} <= seen["copy-%d" % n] and {0, 1} <= seen["copy-%d+1" % n], n
    for d in L.OVERLAP_CELLS:
        assert {0, 1} <= seen["overlap-%d" % d] and len({x for x in seen["overlap-%d" % d] if isinstance(x, tuple)}) == 3, d
    for k in L.WRAP_CELLS:   # (counted from nought and from one)
        assert {0, 1} <= seen["wrap-%d" % k] and {0, 1} <= seen["wrap-%d" % (k - 1)], k
    for cell in ("word", "word+1", "switch", "literal"):
        assert {0, 1} <= seen[cell], cell
    assert L.COPY_CELLS == [2, 3, 63, 64, 65, 79, 80, 81, 1023, 1024, 1025, 1041] and L.OVERLAP_CELLS == [1, 2, 3, 65] and L.WRAP_CELLS == [63, 64, 65, 127, 128]
    # metablock boundaries
    v = made["X-boundary"]
    kinds = [m["kind"] for m in v["mbs"]]
    got = set()
    for cell, r, _, _, _ in probes["X-boundary"]:
        if cell.startswith("after-") and cell.endswith("+0"):
            assert r["k"] == 0 and r["mb"] > 0 and r["pos"] == v["mbs"][r["mb"]]["at"]
            front = kinds[r["mb"] - 1]
            last = [c for c in v["clog"] if c["mb"] < r["mb"]][-1]
            name = cell[6:-2]
            if name in ("compressed", "stored", "metadata", "empty"):
                assert front == name, (cell, front)
            elif name == "copy-end":
                assert front == "compressed" and not last["word"] and last["pos"] + last["total"] == r["pos"] and last["total"] == 5
            else:
                assert name == "word-end" and front == "compressed" and last["word"] and last["pos"] + last["total"] == r["pos"]
            got.add(name)
    assert got == {"compressed", "stored", "metadata", "empty", "copy-end", "word-end"}
    assert all(r["pos"] in (0, 1) for cell, r, _, _, _ in probes["X-boundary"] if cell.startswith("start"))


def test_x_word_cells(made, probes):
    """predecessor x follower x (the word's command carries literals / none), each cell from the command log: the follower's words
    put out no byte or one, the probe is the first literal of the command behind them, the predecessor is what the cell says"""
    seen = collections.Counter()
    for label in ("X-words", "X-words-start"):
        v = made[label]
        for cell, r, _, _, _ in probes[label]:
            if "/" not in cell or cell.endswith("+1"):
                continue
            pred, fol, arm = cell.split("/")
            cl = _commands(v, r["mb"])
            c = r["cmd"]
            assert r["pos"] == cl[c - 1]["pos"] + cl[c - 1]["total"], cell   # the first literal of its command
            tiny = lambda x, n: x["word"] and x["total"] == n
            if fol == "w0":
                assert tiny(cl[c - 1], 0); wi = c - 1
            elif fol == "w1":
                assert tiny(cl[c - 1], 1); wi = c - 1
            elif fol == "w1w1":
                assert tiny(cl[c - 1], 1) and tiny(cl[c - 2], 1) and cl[c - 1]["insert"] == 0; wi = c - 2
            else:
                assert fol == "w1-copy2" and not cl[c - 1]["word"] and cl[c - 1]["copy_len"] == 2 and cl[c - 1]["insert"] == 0 and tiny(cl[c - 2], 1); wi = c - 2
            assert (cl[wi]["insert"] > 0) == (arm == "lits"), cell
            if pred == "start":
                assert wi == 0 and r["mb"] > 0, cell
            else:
                p = cl[wi - 1]
                ok = {"literal": tiny(p, 0) and p["insert"] > 0, "copy5": not p["word"] and p["copy_len"] == 5, "copy300": not p["word"] and p["copy_len"] == 300,
                      "word": p["word"] and p["total"] >= 2}[pred]
                assert ok, (cell, p)
            seen[cell] += 1
    cells = ["%s/%s/%s" % (p, f, a) for p in L.PREDECESSORS for f in L.FOLLOWERS for a in ("lits", "none")]
    assert len(cells) == 40 and all(seen[c] >= 2 for c in cells), [c for c in cells if seen[c] < 2]
    one = {L.E.transform_word(L.E.dictionary_word(l, i), t) for l, i, t in L.tiny_words()[1]}
    assert all(len(w) == 1 for w in one) and len(one) >= 8


def test_x_maps(made, probes):
    """block types of 64, 63, 2 and 1 distinct trees, the last one trivial while NTREES is 130; a run of 70 literals goes from the trivial
    type to a non-trivial one, and back, after each of its first 66 literals"""
    v = made["X-maps"]
    sc = v["mbs"][0]["scheme"]
    assert [len(set(sc.lit_map[t * 64:t * 64 + 64])) for t in range(4)] == [64, 63, 2, 1] and len(sc.trees) == 130
    ll = v["llog"]
    cl = _commands(v)
    start = {}   # command -> position of its first literal
    for r in ll:
        start.setdefault(r["cmd"], r["pos"])
    to_full, to_trivial = set(), set()
    for i, r in enumerate(ll):
        if r["first_of_block"] and i and cl[r["cmd"]]["insert"] == 70 and ll[i - 1]["cmd"] == r["cmd"]:
            j = r["pos"] - start[r["cmd"]]
            if ll[i - 1]["type"] == 3:
                assert r["type"] != 3; to_full.add(j)
            elif r["type"] == 3:
                to_trivial.add(j)
    assert to_full == set(range(1, 67)) and to_trivial == set(range(1, 67))
    cells = collections.Counter(cell for cell, _, _, _, _ in probes["X-maps"])
    assert cells["to-full"] == 66 and cells["to-trivial"] == 66 and all(cells["type%d" % t] >= 24 for t in range(4))
    for cell, r, _, _, _ in probes["X-maps"]:
        if cell in ("to-full", "to-trivial"):
            assert r["first_of_block"] and (r["type"] == 3) == (cell == "to-trivial")
    # the vector of 4 x 64 trees: every tree is in use under each type, so that the cache of one type's trees is full
    v = made["X-every-tree"]
    assert all(len({r["tree"] for r in v["llog"] if r["type"] == t}) == 64 for t in range(4))
    assert sum(1 for r in v["llog"] if r["first_of_block"]) >= 300


def test_x_every_alternative_is_a_real_one_in_every_cell(made, probes):
    """each of (a) .. (f) names another tree than the right one wherever the cell's place in the stream allows it (tools/make_literal_vectors.py,
    `required`, says what each place rules out and why): at every single probe of the cells whose front the generator draws; over all
    probes of a cell where the front is the cell itself (the LUT cells, every tree, the stream's start) or the block type has two
    trees (X-maps).  (f) means each of the other three modes."""
    assert L.required("copy-64", 2) == {"a", "b", "c", "d", "f0", "f1", "f3"} and L.required("copy-64+1", 1) == {"a", "b", "d", "f0", "f2", "f3"}
    assert L.required("overlap-3", 3) == {"a", "b", "c", "d", "e", "f0", "f1", "f2"} and L.required("overlap-1", 2) == {"b", "c", "e", "f0", "f1", "f3"}
    assert L.required("overlap-1+1", 2) == {"a", "b", "d", "e", "f0", "f1", "f3"} and L.required("copy5/w0/lits", 2) == {"a", "b", "d", "f0", "f1", "f3"}
    assert L.required("word/w1/none", 0) == {"a", "b", "c", "d", "f1", "f2", "f3"} and L.required("switch", 3) == {"a", "b", "d", "f0", "f1", "f2"}
    assert L.required("after-stored+0", 3) == {"a", "b", "d", "f0", "f1", "f2"} and L.required("after-copy-end+1", 3) == {"a", "b", "c", "d", "f0", "f1", "f2"}
    assert all(L.required(c, 2) == set() for c in L.AGGREGATE + L.TRIVIAL + ("start+0", "start+1", "to-trivial+1"))
    real, modes, single = collections.defaultdict(set), collections.defaultdict(set), 0
    for label, ps in probes.items():
        for cell, r, alts, right, sc in ps:
            got = {a for a, t in alts.items() if t != right}
            need = L.required(cell, r["mode"])
            assert need <= got, "%s: probe %s at %d: alternatives %s are no real ones" % (label, cell, r["pos"], sorted(need - got))
            single += bool(need)
            key = (label if cell == "lut" else "", cell)
            real[key] |= {(a, r["mode"]) if a.startswith("f") else a for a in got}
            modes[key].add(r["mode"])
    assert single >= 700, single
    n = 0
    for (label, cell), got in real.items():
        base = cell[:-2] if cell[-2:] in ("+0", "+1") else cell
        if base not in L.AGGREGATE:
            continue
        need = {"a", "b", "d"} | {("f%d" % m, mode) for mode in modes[(label, cell)] for m in range(4) if m != mode}
        if cell == "start+0":     # (every wrong context of the stream's first literal is (0, 0) like the right one, under every mode)
            need = set()
        elif cell == "start+1":   # (p2 is zero: (d) is (0, 0), which (b) is as well)
            need -= {"d"}
        assert need <= got, (label, cell, sorted(map(str, need - got)))
        n += 1
    assert n >= 4 + 1 + 2 + 5, n   # (the LUT cells of four modes, every tree, the start, those of X-maps)
    # a trivial type has one tree: nothing to tell apart, and the cells say so
    for cell, r, alts, right, sc in probes["X-maps"]:
        assert (cell[:-2] if cell.endswith("+1") else cell) not in L.TRIVIAL or set(alts.values()) == {right}
