#!/usr/bin/env python3
"""tests/golden/emitter_headers/: streams written by tools/brotli_emit.py that put every form of a metablock's header -- what
lies in front of the first command, and the block switches between the commands -- through the decoder: forms an encoder
library never writes.  The vectors of tests/golden/emitter_words/ and emitter_copies/ do that for the commands.

  P  the code-length reader: a prefix code with a chosen wire form (brotli_emit.WireCode) in the place of the literal code
     (alphabet 256), the command code (704) and a distance code (64; 520 under NPOSTFIX 3 / NDIRECT 120; 140 with max_symbol 74
     in a large-window stream): every bit phase, words on every side of a 64-bit step, chains of repeat words, every way for a
     code to end, every verdict, the one-symbol code-length codes, the deepest codes
  C  the context maps: NTREES x RLEMAX, every run-length code at both extremes, runs that end at or beyond the map's end,
     move-to-front indices up to 255, the map's own code simple and complex, what the maps select
  B  the block switches: every block-length code at both extremes, every type code, 2 .. 256 types, blocks of one symbol,
     last blocks that end at, in front of and behind the category's last symbol, a long form for the record loops
  M  the framing: MNIBBLES and MSKIPBYTES at their extremes and exuberant, the reserved bit, padding that is not zero,
     runs of metadata blocks, every window code

Every valid vector's literals and commands use the shallowest and the deepest symbol of the code under test (asserted here
and, from the log, in tests/test_emitter_headers_cpu.py), so that a wrong length changes bytes.  A vector whose header no
decoder accepts has a valid compressed metablock in front of it.  `vectors()` is deterministic; `main()` asks the oracle (and
libbrotlidec where there is one) about every stream before it writes.  The files are those of tools/make_copy_vectors.py, but
that the 700 streams of less than 256 bytes lie end to end in small.N.bin ("at": the offset) and not as hex in the manifest,
which has an entry a line and only what cannot be derived (tests/header_vectors.py fills in the rest); "first_command" is the
byte in which the first command of the last metablock begins."""
import hashlib
import itertools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import vector_store  # noqa: E402
from make_copy_vectors import _dist_range, t_commands  # noqa: E402
from vector_store import MAX_FILE, MAX_PARTS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "emitter_headers")
FRONT = [(b"a valid metablock in front; ", 9, 7), (b"then the header.", 0, 0)]
# slot -> (the plan's slot, alphabet, max_symbol, NPOSTFIX, NDIRECT, large window)
SLOTS = {"lit": ("lit", 256, 256, 0, 0, False), "cmd": ("cmd", 704, 704, 0, 0, False), "d64": ("dist", 64, 64, 0, 0, False),
         "d520": ("dist", 520, 520, 3, 120, False), "dlw": ("dist", 140, 74, 0, 0, True)}
assert E.max_distance_symbol(0, 0) == 74


class Stream:
    """a stream under construction: the writer, the output the emitter expects so far, both logs"""

    def __init__(self, wbits=22, large=False):
        self.w, self.out, self.hlog, self.clog, self.ring = E.BitWriter(), bytearray(), [], [], list(E.RING_INIT)
        self.wbits, self.large, self.valid, self.first_command = wbits, large, True, 0
        E.write_stream_header(self.w, wbits, large)

    def block(self, cmds, plan=None, last=False, unchecked=False, mlen=None, nibbles=None, literals=None):
        """one compressed metablock; an unchecked one's output is not the emitter's to say: the stream is marked"""
        plan = plan or E.Plan()
        plan.large_window = self.large
        raw = E.emit_compressed(self.w, cmds, plan, last, prev=bytes(self.out), wbits=self.wbits, log=self.clog, unchecked=unchecked, mlen=mlen,
                                ring_io=self.ring, hlog=self.hlog, nibbles=nibbles, literals=literals)
        self.first_command = [r for r in self.hlog if r["kind"] == "commands"][-1]["start"] // 8
        if unchecked:
            self.valid = False
        else:
            self.out += raw
        return self

    def stored(self, raw, pad=0):
        E.emit_stored(self.w, raw, pad)
        self.out += raw
        return self


# ------------------------------------------------------------------ P: data that shows a code
def _cmd_parts(sym):
    cell = sym >> 6
    ic = 8 * (0, 0, 0, 0, 1, 1, 0, 2, 1, 2, 2)[cell] + ((sym >> 3) & 7)
    cc = 8 * (0, 1, 0, 1, 0, 1, 2, 0, 2, 1, 2)[cell] + (sym & 7)
    return ic, cc


def _cheap(slot, sym, npostfix, ndirect):
    if slot == "lit":
        return True
    if slot == "cmd":
        ic, cc = _cmd_parts(sym)
        return ic <= 21 and cc <= 22
    return sym < 16 or 16 <= sym < 16 + ndirect and sym - 15 <= 250 or sym >= 16 + ndirect and _dist_range(sym, npostfix, ndirect)[0] <= 250


def pick(code, slot, npostfix=0, ndirect=0):
    """the symbols the data uses: the shallowest and the deepest of the code that a small stream can use, and up to six more"""
    usable = sorted(code.codes)
    pool = [s for s in usable if _cheap(slot, s, npostfix, ndirect)] or (usable if slot != "dist" else [])
    if not pool:   # (a distance code none of whose symbols a small stream can use: implicit distances only, the verdict is what shows)
        return []
    lo, hi = min(pool, key=lambda s: (code.full[s], s)), max(pool, key=lambda s: (code.full[s], -s))
    picked = []
    for s in [lo, hi] + pool[::max(1, len(pool) // 6)][:6]:
        if s not in picked:
            picked.append(s)
    return picked


def extremes_met(code, used):
    """do the symbols the data uses include one of the code's shallowest and one of its deepest?"""
    depths = [code.full[s] for s in code.codes]
    return bool(used) and (min(code.full[s] for s in used), max(code.full[s] for s in used)) == (min(depths), max(depths))


def commands_for(slot, picked, npostfix=0, ndirect=0, ring=E.RING_INIT):
    """-> (commands, the symbols of `picked` they use)"""
    text = b"header vectors, "
    if slot == "lit":
        body = bytes(picked) * (6 // max(1, len(picked)) + 1) if picked else b"lalala"
        return [(body, 4, 3), (body[::-1], 0, 0)], picked
    if slot == "cmd":
        cmds = []
        for s in sorted(picked, key=lambda s: -_cmd_parts(s)[0])[:1] + picked:   # (the longest insert first, so that copies have something behind them)
            ic, cc = _cmd_parts(s)
            ins = (text * (E._INS_BASE[ic] // len(text) + 1))[:E._INS_BASE[ic]] if ic < 16 else bytes(random.Random(s).choices(b"e ", cum_weights=(31, 32), k=E._INS_BASE[ic]))
            cmds.append((ins, E._COPY_BASE[cc], ("implicit",) if s < 128 else (lambda pos, ring, md: max(1, min(pos, 5)))))
        return cmds or [(b"lalala", 4, 3)], picked
    # distances: the ring of the last four is followed here, and a short code that would name no distance is left out
    cmds, used, ring = [], [], list(ring)
    explicit = lambda s: s - 15 if s < 16 + ndirect else _dist_range(s, npostfix, ndirect)[0]
    safe = [s for s in picked if s >= 16 and explicit(s) >= 4]
    todo = list(picked)
    for s in todo:
        if s >= 16:
            d = explicit(s)
        elif s < 4:
            d = ring[s]
        else:
            if min(ring[:2]) < 4 and safe and todo.count(s) == 1:
                todo += [safe[0], safe[0], s]   # (two explicit distances of four or more in front of it, then it fits)
                continue
            d = ring[(s - 4) // 6] + (1, 2, 3)[((s - 4) % 6) // 2] * (1 if s & 1 else -1)
            if d < 1:
                continue
        k = len(cmds)
        cmds.append((bytes(random.Random(5).choices(b"e ", cum_weights=(31, 32), k=300)) if k == 0 else text[:1 + k % 3], 2 + k % 5, ("ring", s) if s < 16 else d))
        used.append(s)
        if s != 0:
            ring = [d] + ring[:3]
    return (cmds or [(b"lalala", 4, ("implicit",))]) + [(b".", 0, 0)], used


def code_stream(slot, code, front=False, lead=0, wbits=22, stored=0):
    """a stream whose last metablock carries `code` in `slot`; `lead`: a metablock of that many one-bit literals in front (it moves
    every later bit of the stream by one place a literal); `stored`: a stored metablock of that many bytes in front of everything"""
    pslot, alphabet, max_symbol, npostfix, ndirect, large = SLOTS[slot]
    assert (code.alphabet, code.max_symbol) == (alphabet, max_symbol), (slot, code.alphabet, code.max_symbol)
    s = Stream(wbits, large)
    if stored:
        s.stored(bytes((k * k >> 3) & 255 for k in range(stored)))
    if front or pslot == "cmd":   # (the command code's own commands start with whatever symbol it has: give their copies something to copy)
        s.block(FRONT)
    if lead:
        s.block([((b"ab" * 16)[:lead], 0, 0)])
    picked = pick(code, pslot, npostfix, ndirect)
    valid = bool(code.codes)
    plan = E.Plan(npostfix=npostfix, ndirect=ndirect, codes={(pslot, 0): lambda hist, alphabet: code})
    cmds, used = commands_for(pslot, picked, npostfix, ndirect, s.ring)
    s.block(cmds, plan, last=True, unchecked=not valid)
    if valid and not code.simple and code.consumed < len(code.words):
        s.valid = False   # (words behind the code's end: a decoder reads them as whatever comes next)
    s.extremes, s.used = valid and extremes_met(code, used), used
    return s


# ------------------------------------------------------------------ P: the forms
def complete(words, max_symbol, lens=range(1, 16)):
    """`words` and literal lengths behind them that use the space up exactly, the largest that fits first (None: no room)"""
    words = list(words)
    while True:
        r = E.resolve_words(words, max_symbol)
        if r.space == 0 and r.used == len(words):
            return words
        if r.space is None or r.space < 0 or r.used < len(words):
            return None
        fit = [l for l in lens if (32768 >> l) <= r.space]
        if not fit:
            return None
        words.append(min(fit))


def run_len(n):
    """a length at which n symbols take at most half the code space"""
    return max(1, n.bit_length()) + 1


def chain_total(nbits, extras):
    """the symbols a chain of repeat words with these extra values names"""
    r = 0
    for e in extras:
        r = ((r - 2) << nbits if r else 0) + e + 3
    return r


def p_forms(alphabet, max_symbol):
    """-> [(label, WireCode keywords)] for one alphabet; a form that the alphabet has no room for is written all the same: its
    verdict is the oracle's"""
    A = max_symbol
    out = []

    def add(label, words=None, fill=True, lens=range(1, 16), **kw):
        if words is not None and fill:
            words = complete(words, A, lens) or words
        out.append((label, dict(kw, words=words)))
    for e in range(4):
        add("16first-e%d" % e, [(16, e)])
    add("16-behind-zeros", [5, 0, 0, (16, 1)])
    for k in range(1, 7):
        for e in range(4):
            n = chain_total(2, [0] * (k - 1) + [e])
            add("16chain-k%d-e%d" % (k, e), [1, min(15, run_len(n + 1))] + [(16, 0)] * (k - 1) + [(16, e)])
    for k in range(1, 5):
        for e in (0, 7):
            add("17chain-k%d-e%d" % (k, e), [(17, 0)] * (k - 1) + [(17, e)], lens=range(3, 16))
    add("16-17-16-17", [4, (16, 0), (17, 1), (16, 2), (17, 0)])
    add("16-broken-by-the-same-length", [6, (16, 0), 6, (16, 1)])
    # a repeat word as the first of a reader's 64-bit step: twelve words of five bits, a repeat word of four bits that ends on bit 64, and
    # the next one goes on with its run (the second link of a chain) or is the other repeat word (the run starts again)
    ls = (3, 4, 5) if A < 100 else (4, 5, 6)
    cl = _cl({0: 5, ls[2]: 5, 16: 2, 17: 1, ls[0]: 3, ls[1]: 4})
    for name, pair in (("on-16", [(16, 1), (16, 2)]), ("on-17", [(17, 1), (17, 0)]), ("turn-16-17", [(16, 1), (17, 2)]), ("turn-17-16", [(17, 1), (16, 1)])):
        add("step-" + name, [ls[2]] + [0] * 11 + pair, lens=ls, cl_lengths=cl)
    add("end-in-a-repeat", [1, 2, 4, (16, 0)], fill=False)
    add("end-at-max-symbol", [1, 2, 3, 4] + [0] * (A - 5) + [4], fill=False)
    add("end-at-max-symbol-repeat", [1, 2, 4] + [0] * (A - 6) + [(16, 0)], fill=False)
    add("zeros-behind-the-end", [1, 2, 4, (16, 0), 0, 0, 0], fill=False, unchecked=True)
    add("depth-plain", list(range(1, 16)) + [15], fill=False)
    add("depth-sixteens", list(range(1, 13)) + [15, (16, 0), (16, 0)], fill=False)
    for hskip in (0, 2):
        add("hskip%d-of-3" % hskip, [5, 5] + [6] * 12 + [5] * 24, fill=False, hskip=hskip, cl_lengths=_cl({5: 1, 6: 1}))
    add("hskip3-of-3", [5, 5] + [6] * 12 + [5] * 24, fill=False, cl_lengths=_cl({5: 1, 6: 1}))
    add("hskip0-of-2", [4, 4] + [5] * 12 + [4] * 8, fill=False, hskip=0, cl_lengths=_cl({4: 1, 5: 1}))
    # verdicts
    add("V-repeat-one-beyond", [2, 2, 2] + [0] * (A - 5) + [(17, 0)], fill=False, unchecked=True)
    for k in (3, 4, 16, 21):
        add("V-seventeens-%d" % k, [(17, 7)] * k, fill=False, unchecked=True, cl_lengths=_cl({17: 1, 0: 2, 2: 3, 3: 3}))
    add("V-space-over-by-a-length", [1, 2, 1] + [0] * (A - 3), fill=False, unchecked=True)
    add("V-space-over-by-a-repeat", [1, 2, (16, 0)] + [0] * (A - 5), fill=False, unchecked=True)
    add("V-space-left-at-max-symbol", [1, 2] + [0] * (A - 2), fill=False, unchecked=True)
    add("V-cl-space-left", [3, 3], fill=False, unchecked=True, cl_lengths=_cl({0: 2, 3: 2}))
    add("V-cl-space-over", [3, 3], fill=False, unchecked=True, cl_lengths=_cl({3: 2, 4: 1, 0: 1}))
    # the serial loop: a code-length code of one symbol, whose words take no bits
    add("one-16", [(16, 2), (16, 2), (16, 2), (16, 1)], fill=False, unchecked=True, cl_lengths=_cl({16: 3}))
    add("one-8", [8] * 256, fill=False, unchecked=True, cl_lengths=_cl({8: 2}))
    add("one-17", [(17, 5)] * 5, fill=False, unchecked=True, cl_lengths=_cl({17: 1}))
    add("one-1", [1, 1], fill=False, cl_lengths=_cl({1: 4}))
    # simple codes
    top = {256: [255, 254, 1, 0], 704: [383, 130, 1, 0]}.get(alphabet, [19, 16, 1, 0])   # (in wire order: not sorted)
    for n in (1, 2, 3):
        out.append(("simple-%d" % n, dict(simple=top[:n])))
    out.append(("simple-4-flat", dict(simple=top, tree_select=0)))
    out.append(("simple-4-deep", dict(simple=[2, 0, 3, 1], tree_select=1)))
    for i, j in ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)):
        syms = [3, 2, 1, 0]
        syms[j] = syms[i]
        out.append(("V-simple-same-%d%d" % (i + 1, j + 1), dict(simple=syms[:j + 1] if j < 3 else syms, tree_select=0 if j == 3 else None, unchecked=True)))
    abits = max(1, (alphabet - 1).bit_length())
    if A < (1 << abits):
        out.append(("V-simple-symbol-at-max-symbol", dict(simple=[1, A], unchecked=True)))
        if A < alphabet < (1 << abits):
            out.append(("V-simple-symbol-at-alphabet", dict(simple=[alphabet, 2, 1], unchecked=True)))
    return out


def _cl(lengths):
    return [lengths.get(s, 0) for s in range(18)]


_PERMS = ((1, 2, 3, 4, 5, 5), (5, 1, 2, 3, 4, 5), (5, 5, 1, 2, 3, 4), (4, 5, 5, 1, 2, 3), (3, 4, 5, 5, 1, 2), (2, 3, 4, 5, 5, 1))


def swept_code(rnd, alphabet, max_symbol, perm, ls):
    """a complete code of 20 .. 90 words over the six code-length symbols 0, 16, 17 and three lengths `ls`, whose own code has the
    lengths `perm`: zeros, lengths and short chains of both repeat words in seeded order -- the sweep that puts every kind of word
    on every side of a 64-bit step"""
    cl = _cl(dict(zip((0, 16, 17) + tuple(ls), perm)))
    while True:
        words, target = [], rnd.randrange(20, 90)
        while len(words) < target:
            r = rnd.random()
            if r < 0.3:
                more = [0] * rnd.randrange(1, 4)
            elif r < 0.6:
                more = [rnd.choice(ls)]
            elif r < 0.8:
                more = [(16, rnd.randrange(4))] * 1 + [(16, rnd.randrange(4))] * (rnd.random() < 0.3)
            else:
                more = [(17, rnd.randrange(8))] + [(17, rnd.randrange(8))] * (rnd.random() < 0.2)
            r = E.resolve_words(words + more, max_symbol)
            if r.space is None or r.space <= (32768 >> ls[0]) or r.used < len(words + more) or r.symbol + 24 > max_symbol:
                break
            words += more
        done = complete(words, max_symbol, ls)
        if done and len(done) >= 12:
            return E.WireCode(alphabet, words=done, cl_lengths=cl, max_symbol=max_symbol)


def p_vectors(add):
    for slot, (pslot, alphabet, max_symbol, npostfix, ndirect, large) in SLOTS.items():
        for label, kw in p_forms(alphabet, max_symbol):
            kw.pop("unchecked", None)
            code = E.WireCode(alphabet, max_symbol=max_symbol, unchecked=True, **kw)   # (the log says what was written, the arithmetic whether a decoder can accept it)
            s = code_stream(slot, code, front=not code.codes or (not code.simple and code.consumed < len(code.words)))
            add("P-%s-%s" % (slot, label), "P", s, form=label, slot=slot)
    # every bit phase: one-bit literals in front move the code (about) a bit at a time; the leads that bring a new phase are kept
    rnd = random.Random(64)
    for slot in ("lit", "cmd", "d64"):
        pslot, alphabet, max_symbol = SLOTS[slot][:3]
        seen = set()
        for lead in range(200):
            code = swept_code(rnd, alphabet, max_symbol, _PERMS[lead % 6], (3, 4, 5) if slot == "d64" else (4, 5, 6))
            s = code_stream(slot, code, lead=lead % 33, wbits=(10, 16, 17, 22)[lead % 4])
            phase = [r for r in s.hlog if r["kind"] == pslot + "0"][-1]["start"] % 32
            if s.extremes and phase not in seen:
                seen.add(phase)
                add("P-%s-phase%02d" % (slot, phase), "P", s, form="phase", slot=slot)
        assert len(seen) == 32, (slot, sorted(seen))
    # the sweep across the 64-bit steps: seeded codes, kept while they bring a word of a kind and width to a new place on a step's end
    want = {(kind, n, o) for kind, more in (("len", 0), (16, 2), (17, 3)) for n in range(1, 6) for o in range(1, n + more + 1)}
    runs_on = {("on", 16), ("on", 17), ("turn", 16, 17), ("turn", 17, 16)}
    for slot in SLOTS:
        pslot, alphabet, max_symbol = SLOTS[slot][:3]
        need = want | runs_on
        seen, k = set(), 0
        for tries in range(4000):
            code = swept_code(rnd, alphabet, max_symbol, _PERMS[tries % 6], (3, 4, 5) if max_symbol < 100 else (4, 5, 6) if tries % 2 else (5, 7, 8))
            ends = step_ends(code)
            new = (ends | {e[0] for e in ends if len(e) == 3 and e[0] not in ("on", "turn")}) - seen
            if not (new & need or new and k < 12):
                continue
            s = code_stream(slot, code)
            if s.extremes:
                seen |= new
                add("P-%s-sweep%02d" % (slot, k), "P", s, form="sweep", slot=slot); k += 1
        for place in sorted(need - seen, key=str):   # (what the seeded codes did not reach -- with 64 and 74 symbols they are a step or two long -- is built)
            if place not in seen:
                code = placed_code(alphabet, max_symbol, place, (3, 4, 5) if max_symbol < 100 else (4, 5, 6))
                s = code_stream(slot, code)
                assert s.extremes, (slot, place)
                seen |= step_ends(code)
                add("P-%s-sweep%02d" % (slot, k), "P", s, form="sweep", slot=slot); k += 1
        assert seen >= need, (slot, sorted(need - seen, key=str))


def placed_code(alphabet, max_symbol, place, ls):
    """a complete code in which a word of `place`'s kind, with a code of its width, has that many bits in front of bit 64 of the first
    step: zeros and the deepest length in front of it, under the first code-length code that lets them add up"""
    kind, n, o = place
    target = {"len": ls[2], 16: (16, 0), 17: (17, 0)}[kind]
    for perm in sorted(set(itertools.permutations((1, 2, 3, 4, 5, 5)))):
        bits = dict(zip((0, 16, 17) + tuple(ls), perm))
        if bits[ls[2] if kind == "len" else kind] != n:
            continue
        for b in range(1, 7):
            rest = 64 - o - b * bits[ls[2]]
            if rest >= 0 and rest % bits[0] == 0 and rest // bits[0] + b <= 24:
                done = complete([ls[2]] * b + [0] * (rest // bits[0]) + [target], max_symbol, ls)
                if done:
                    code = E.WireCode(alphabet, words=done, cl_lengths=_cl(bits), max_symbol=max_symbol)
                    if place in step_ends(code):
                        return code
    raise ValueError(place)


def step_ends(code):
    """{(kind of word, bits of its code, bits of the word in front of bit 64 of its step)} for the words that end on or straddle the
    end of a 64-bit step (brotli_emit.WireCode.write_code has the rule), and what the first word of a step does to a run"""
    out, base, at, before = set(), 0, 0, 0
    for k, wd in enumerate(code.words[:code.consumed]):
        sym = wd if isinstance(wd, int) else wd[0]
        n = code.cl_codes[sym][1]
        bits = n + (sym - 14 if sym >= 16 else 0)
        if at - base >= 64:
            base = at
            if sym >= 16 and code.depth[k] >= 2:
                out.add(("on", sym))       # the first word of a step goes on with the run of the step before
            elif sym >= 16 and before >= 16:
                out.add(("turn", before, sym))   # ... or is the other repeat word than the one before: the run starts again
        before = sym
        if at - base < 64 <= at - base + bits:
            out.add(("len" if sym < 16 else sym, n, 64 - (at - base)))
        at += bits
    return out


# ------------------------------------------------------------------ C: the context maps
def _lit_data(rnd, nbt, per=3):
    """literal blocks of `per` literals for each of `nbt` types in turn, the literals from six values whose low bits differ: under
    LSB6 every literal's context is the byte before it"""
    blocks = [(t, per) for t in range(nbt - 1)] + [(nbt - 1, per + 8)]
    lits = bytes(rnd.choice(b"\x00\x01\x3f\x40\x7fz") for _ in range(per * nbt))
    return blocks, lits


def map_stream(lit=None, dist=None, front=False, unchecked=False, lit_code=None, stored=0):
    """lit / dist: (the map, its form) or None.  The literal data visits every block type of the map, the copies every distance
    block type with lengths 2, 3, 4 and 5"""
    rnd = random.Random(7)
    s = Stream(22)
    if stored:
        s.stored(bytes((k * k >> 3) & 255 for k in range(stored)))
    if front:
        s.block(FRONT)
    plan = E.Plan()
    if lit:
        cmap, form = lit
        nbt = len(cmap) // 64
        plan.lit_map, plan.map_forms["lit"] = list(cmap), form
        plan.lit_blocks, lits = _lit_data(rnd, nbt) if nbt > 1 else (None, bytes(rnd.choice(b"\x00\x01\x3f\x40\x7fz") for _ in range(40)))
        if lit_code:
            plan.codes[("lmap", 0)] = lit_code
    else:
        lits = b"context maps. " * 3
    cmds = []
    if dist:
        dmap, dform = dist
        nbd = len(dmap) // 4
        plan.dist_map, plan.map_forms["dist"] = list(dmap), dform
        ncopies = max(8, 2 * nbd)
        if nbd > 1:
            plan.dist_blocks = [(t % nbd, 2) for t in range(ncopies // 2)]
        step = max(1, len(lits) // ncopies)
        cmds.append((lits[:8], 2, 3))
        at = 8
        for k in range(1, ncopies):
            cmds.append((lits[at:at + step], 2 + k % 4 + (k % 8 == 7), 1 + (k * 5) % 8)); at += step   # (copy lengths 2, 3, 4, 5 and 6)
        cmds.append((lits[at:] or b".", 0, 0))
    else:
        cmds = [(lits[:len(lits) // 2], 5, 3), (lits[len(lits) // 2:], 0, 0)]
    s.block(cmds, plan, last=True, unchecked=unchecked)
    return s


def spread(size, ntrees, every=None):
    """a map of `size` entries that names every tree: tree v at v * every, zeros between"""
    every = every or max(1, size // ntrees)
    m = [0] * size
    for v in range(1, ntrees):
        m[min(size - 1, v * every - (every > 1))] = v
    assert set(m) == set(range(ntrees)), (size, ntrees)
    return m


def indices_to_values(indices):
    """the map whose move-to-front form is `indices`"""
    mtf, out = list(range(256)), []
    for i in indices:
        v = mtf.pop(i); out.append(v); mtf.insert(0, v)
    return out


MTF_SEQ = [255, 0, 0, 1, 0, 63, 64, 65, 127, 128, 129, 255, 0, 0, 0, 64, 0, 128, 1]   # (single zeros, and runs of them)


def c_vectors(add):
    for ntrees in (2, 3, 64, 65, 255, 256):
        for rlemax in (0, 1, 5, 16):
            size = 64 * max(2, (ntrees + 31) // 32)
            imtf = (ntrees + rlemax) % 2
            add("C-lit-n%d-r%d" % (ntrees, rlemax), "C", map_stream(lit=(spread(size, ntrees), {"rlemax": rlemax, "imtf": imtf})), ntrees=ntrees, rlemax=rlemax)
    for ntrees in (2, 4, 65, 256):
        for rlemax in (0, 3, 16):
            add("C-dist-n%d-r%d" % (ntrees, rlemax), "C", map_stream(dist=(spread(4 * max(2, (ntrees + 1) // 2), ntrees), {"rlemax": rlemax, "imtf": rlemax == 3})), ntrees=ntrees, rlemax=rlemax)
    # every run-length code at both extremes of its extra bits; codes 1 .. 8 in one map of 16384 entries, the wider ones one a map
    big = 16384

    def table(pairs):
        by = {(1 << c) + e: [(c, e)] for c, e in pairs}
        return lambda n, rlemax: by.get(n) or E.zero_run_pieces(n, rlemax)
    pairs = [(c, e) for c in range(1, 9) for e in (0, (1 << c) - 1)]
    m = []
    for k, (c, e) in enumerate(pairs):
        m += [0] * ((1 << c) + e) + [1 + k % 3]
    m += [0] * (big - len(m) - 1) + [3]
    add("C-runs-1-8", "C", map_stream(lit=(m, {"rlemax": 16, "runs": table(pairs)})), run_codes=pairs)
    for c in range(9, 17):
        for e in (0, (1 << c) - 1):
            n = (1 << c) + e
            if n < big:   # the run, one entry that is not zero, the rest; with code 13's widest run the map ends on the run
                m = [2] + [0] * n + ([1] + [0] * (big - n - 3) + [3] if n < big - 3 else [1] * (big - n - 1))
                if c % 2:   # (with the transform: these are the indices)
                    m = indices_to_values(m)
                add("C-run-c%d-%s" % (c, "ones" if e else "zeros"), "C", map_stream(lit=(m, {"rlemax": 16, "runs": table([(c, e)]), "imtf": c % 2})), run_codes=[(c, e)])
            elif n == big:
                add("C-run-c%d-zeros-whole-map" % c, "C", map_stream(lit=([0] * big, {"rlemax": 16, "ntrees": 2 + c % 3, "items": [("run", c, e)]})), run_codes=[(c, e)])
            else:   # (beyond any map: a decoder's verdict)
                add("C-V-run-c%d-%s" % (c, "ones" if e else "zeros"), "C", map_stream(lit=([0] * big, {"rlemax": 16, "ntrees": 2 + c % 3, "items": [("run", c, e)]}), front=True, unchecked=True), run_codes=[(c, e)])
    # run ends
    add("C-run-ends-the-map", "C", map_stream(lit=([1, 2] + [0] * 126, {"rlemax": 6, "items": [("v", 1), ("v", 2), ("run", 6, 62)]})))
    add("C-V-run-one-beyond", "C", map_stream(lit=([1, 2] + [0] * 126, {"rlemax": 6, "items": [("v", 1), ("v", 2), ("run", 6, 63)]}), front=True, unchecked=True))
    add("C-dist-V-run-one-beyond", "C", map_stream(dist=([1] + [0] * 7, {"rlemax": 2, "items": [("v", 1), ("v", 0), ("run", 2, 3)]}), front=True, unchecked=True))
    add("C-one-run-n2", "C", map_stream(lit=([0] * 128, {"rlemax": 7, "ntrees": 2, "items": [("run", 7, 0)]})))
    add("C-dist-one-run-n3", "C", map_stream(dist=([0] * 8, {"rlemax": 3, "ntrees": 3, "items": [("run", 3, 0)]})))
    # move to front
    seq = MTF_SEQ
    front_all = [255] * 256   # (the last of the list each time: every tree comes to the front once)
    for name, indices, size in (("edges", seq, 128), ("every-tree", seq + front_all, 512), ("big", (seq + front_all + [0] * 700) * 8, big)):
        indices = indices + [0] * (size - len(indices))
        assert len(indices) == size
        for rlemax in (0, 9):
            add("C-imtf-%s-r%d" % (name, rlemax), "C", map_stream(lit=(indices_to_values(indices), {"rlemax": rlemax, "imtf": 1})), mtf="imtf")
            if name != "big":
                add("C-plain-%s-r%d" % (name, rlemax), "C", map_stream(lit=(indices, {"rlemax": rlemax, "imtf": 0})), mtf="plain")
    # the map's own code
    add("C-code-simple", "C", map_stream(lit=([0, 1] * 64, {"rlemax": 0}), dist=([0, 1, 1, 0] * 2, {"rlemax": 2})))
    repeats = lambda hist, alphabet: E.WireCode(alphabet, lengths=E.limited_lengths(hist, 15), repeats=True)
    some = [0] * 512   # (trees 10 .. 40, 100 .. 140 and 254 of 255: runs of zeros and of equal lengths in the map's own code)
    for k, v in enumerate(list(range(10, 41)) + list(range(100, 141)) + [254]):
        some[5 * k + 3] = v
    add("C-code-repeats", "C", map_stream(lit=(some, {"rlemax": 4, "imtf": 0}), lit_code=repeats))
    # what the maps select
    mixed = []
    for t in range(6):
        mixed += [t] * 64 if t % 2 else [(t + k % 3) % 6 for k in range(64)]
    add("C-some-types-trivial", "C", map_stream(lit=(mixed, {"rlemax": 3})))
    add("C-all-trivial-and-different", "C", map_stream(lit=([t for t in (3, 0, 2, 1, 4) for _ in range(64)], {"rlemax": 6, "imtf": 1})))
    add("C-dist-each-context-its-tree", "C", map_stream(dist=([0, 1, 2, 3, 3, 2, 1, 0, 1, 0, 3, 2], {"rlemax": 0, "imtf": 1})))


# ------------------------------------------------------------------ B: the block switches
def _bl(code, ones):
    return E._BL_BASE[code] + (((1 << E._BL_EXTRA[code]) - 1) if ones else 0)


def b_data(rnd, n_cmds):
    """commands of a literal or two (seven in the first), a short copy and an explicit distance each -> commands"""
    cmds = [(bytes(rnd.choice(b"block switches") for _ in range(7)), 3, 2)]
    for k in range(1, n_cmds):
        cmds.append((bytes(rnd.choice(b"block switches") for _ in range(1 + k % 2)), 2 + k % 3, 1 + (k * 3) % 7))
    return cmds


def _counts(cmds):
    return (sum(len(c[0]) for c in cmds), len(cmds), sum(1 for c in cmds if not (isinstance(c[2], tuple) and c[2][0] == "implicit") and c[1]))


def b_plan(cat, blocks, **kw):
    return E.Plan(**dict({("lit_blocks", "cmd_blocks", "dist_blocks")[cat]: blocks}, **kw))


def b_vectors(add):
    rnd = random.Random(11)
    names = ("lit", "cmd", "dist")
    # every block-length code: those up to 17 run out and switch (all in one metablock), the wider ones are a metablock's last block
    for cat in range(3):
        blocks = [(k % 2, _bl(c, ones)) for k, (c, ones) in enumerate((c, ones) for c in range(18) for ones in (0, 1))]
        need = sum(c for _, c in blocks)
        cmds = b_data(rnd, need)
        if cat == 0:
            blocks.append((0, _counts(cmds)[0] - need))
        s = Stream(22).block(cmds, b_plan(cat, blocks, type_codes="ring"))
        wide = [(c, _bl(c, ones)) for c in range(18, 26) for ones in (0, 1)] + [(25, 16625 + 1), (25, 16625 + 65536 + 9)]
        for k, (c, n) in enumerate(wide):
            s.block(b_data(rnd, 5), b_plan(cat, [(0, 2), (1, n)]), last=k == len(wide) - 1)
        add("B-%s-every-length-code" % names[cat], "B", s, cat=cat)
    # type codes and numbers of types
    for nbt in (2, 3, 255, 256):
        for cat in range(3):
            order = list(range(nbt)) + [0, 1, 0, nbt - 1, 0, nbt // 2, nbt - 1, nbt // 2, 0]   # (+1 all the way and round the end, second last, explicit)
            blocks = [(t, 1 + (k % 3 == 0)) for k, t in enumerate(order)]
            need = sum(c for _, c in blocks)
            cmds = b_data(rnd, need)
            if cat == 0:
                blocks.append(((order[-1] + 1) % nbt, 1 << 12))
            for how in ("ring", "direct"):
                add("B-%s-n%d-%s" % (names[cat], nbt, how), "B", Stream(22).block(cmds, b_plan(cat, blocks, type_codes=how), last=True), cat=cat, nbt=nbt)
    # the block-type code simple (two types: three symbols used at most) and complex (above); blocks of one symbol
    cmds = b_data(rnd, 40)
    nl, nc, nd = _counts(cmds)
    ones = lambda n, nbt: [(k % nbt, 1) for k in range(n)]
    add("B-ones-lit", "B", Stream(22).block(cmds, E.Plan(lit_blocks=ones(nl, 2), type_codes="ring"), last=True))
    add("B-ones-cmd", "B", Stream(22).block(cmds, E.Plan(cmd_blocks=ones(nc, 3), type_codes="ring"), last=True))
    add("B-ones-dist", "B", Stream(22).block(cmds, E.Plan(dist_blocks=ones(nd, 2)), last=True))
    add("B-ones-all", "B", Stream(22).block(cmds, E.Plan(lit_blocks=ones(nl, 3), cmd_blocks=ones(nc, 2), dist_blocks=ones(nd, 4), type_codes="ring"), last=True))
    # the last block: its count ends at, one in front of, one behind the category's last symbol; in a last metablock and in one that is not
    for cat in range(3):
        for name, off in (("exact", 0), ("one-short", -1), ("one-over", 1)):
            for last in (True, False):
                n = _counts(cmds)[cat]
                blocks = [(0, 5), (1, n - 5 + off)] + ([(0, 1)] if off < 0 else [])
                s = Stream(22).block(cmds, b_plan(cat, blocks), last=last)
                if not last:
                    s.block(FRONT, last=True)
                add("B-%s-last-block-%s-%s" % (names[cat], name, "last" if last else "inner"), "B", s, cat=cat, end=name)
    # switch positions
    cmds = [(b"abcdefg", 4, 3), (b"hijkl", 3, ("implicit",)), (b"mn", 5, 2), (b"opq", 2, ("ring", 0)), (b"rs", 4, 6), (b"tuvw", 3, ("ring", 0)), (b"xyz", 0, 0)]
    add("B-lit-switch-first-middle-last", "B", Stream(22).block(cmds, E.Plan(lit_blocks=[(0, 7), (1, 2), (0, 2), (1, 3), (0, 2), (1, 50)]), last=True))
    add("B-cmd-switch-behind-implicit", "B", Stream(22).block(cmds, E.Plan(cmd_blocks=[(0, 2), (1, 50)]), last=True))
    add("B-dist-switch-before-ring0", "B", Stream(22).block(cmds, E.Plan(dist_blocks=[(0, 2), (1, 2), (0, 50)]), last=True))
    # the long form: a switch every 1 .. 40 symbols in each category, three types each, no context modelling
    cmds = t_commands(random.Random(12), 4000) + [(4, 0, 0)]
    lits = bytearray()

    def literal(p1, p2, k):
        return b"etaoin shrdlu"[(p1 * 7 + p2 * 3 + k) % 13]
    real = []
    E.emit_compressed(E.BitWriter(), cmds, E.Plan(), True, wbits=22, literals=literal, realised=real)
    nl, nc, nd = sum(len(c[0]) for c in real), len(real), len(real)
    split = lambda n: [(k % 3 if k % 5 else (k + 1) % 3, rnd.randrange(1, 41)) for k in range(n // 10)] + [(0, 1 << 20)]
    first = lambda blocks: [(0, blocks[0][1])] + blocks[1:]
    plan = E.Plan(lit_blocks=first(split(nl)), cmd_blocks=first(split(nc)), dist_blocks=first(split(nd)), type_codes="ring")
    add("B-long", "B", Stream(22).block(real, plan, last=True))


# ------------------------------------------------------------------ M: the framing
def m_vectors(add):
    def one(n):   # a compressed metablock of n bytes: a few literals and one long copy
        return [(b"framing!", n - 8, 3)] if n > 8 else [(b"framing!"[:n], 0, 0)]
    for n, nib in ((1, 4), (65536, 4), (65537, 5), (1 << 20, 5), ((1 << 20) + 1, 6), (1 << 24, 6), (7, 5), (7, 6), (65537, 6)):
        least = max(4, ((n - 1).bit_length() + 3) // 4)
        s = Stream(24)
        if nib > least:
            s.block(FRONT)
        s.block(one(n), last=True, nibbles=nib, unchecked=nib > least)
        add("M-%smlen-%d-nibbles-%d" % ("V-" if nib > least else "", n, nib), "M", s, big=n > 1 << 22, mlen=n, nibbles=nib)
    tail = [(b"behind the metadata.", 6, 9), (b"!", 0, 0)]
    for n in (0, 1, 128, 129, 256, 65536, 65537):
        s = Stream(22).block(FRONT)
        E.emit_metadata(s.w, bytes((k * 7) & 255 for k in range(n)))
        add("M-metadata-%d" % n, "M", s.block(tail, last=True), metadata=n, nbytes=0 if n == 0 else max(1, ((n - 1).bit_length() + 7) // 8))
    for name, kw in (("V-metadata-exuberant-2", dict(nbytes=2, payload=b"x" * 200)), ("V-metadata-exuberant-3", dict(nbytes=3, payload=b"x" * 300)),
                     ("V-metadata-exuberant-3-of-1", dict(nbytes=3, payload=b"x")), ("V-metadata-reserved", dict(reserved=1, payload=b"xy")),
                     ("V-metadata-padding", dict(pad=0x55, payload=b"xy"))):
        s = Stream(22).block(FRONT)
        E.emit_metadata(s.w, **kw)
        s.block(tail, last=True)
        s.valid = False
        add("M-" + name, "M", s, **{k: (len(v) if k == "payload" else v) for k, v in kw.items()})
    s = Stream(22).block(FRONT)
    s.stored(b"stored behind padding that is not zero", pad=0x2A).block(tail, last=True)
    s.valid = False
    add("M-V-stored-padding", "M", s)
    for extra in (b"", b"!", b"!!", b"!?"):   # (a stream that does not end on a byte boundary: there is padding to set)
        s = Stream(22).block(FRONT).block([(tail[0][0] + extra,) + tail[0][1:], tail[1]], last=True)
        if 0 < s.w.n < 7:
            break
    assert 0 < s.w.n < 7
    s.w.put(0, 1); s.w.put(1, 1)
    s.valid = False
    add("M-V-final-padding", "M", s)
    for count in (1, 2, 200):
        for size in (0, 1):
            s = Stream(22)
            for k in range(count):
                E.emit_metadata(s.w, b"m" * size)
            s.block(FRONT).block(tail, last=True)
            add("M-metadata-run-%dx%d" % (count, size), "M", s, run=(count, size))
    s = Stream(22).block(FRONT).block(tail)
    E.emit_last_empty(s.w)
    add("M-last-empty-behind-compressed", "M", s)
    for wbits in range(10, 25):
        add("M-window-%d" % wbits, "M", Stream(wbits).block(FRONT).block(tail, last=True), wbits=wbits)
    for wbits in (10, 22, 30):
        add("M-large-window-%d" % wbits, "M", Stream(wbits, large=True).block(FRONT).block(tail, last=True), wbits=wbits)
    for name, bits in (("reserved-bit", ((1, 1), (0, 3), (1, 3), (1, 1), (22, 6))), ("9", ((1, 1), (0, 3), (1, 3), (0, 1), (9, 6))), ("31", ((1, 1), (0, 3), (1, 3), (0, 1), (31, 6)))):
        s = Stream(22)
        s.w = E.BitWriter()
        for v, n in bits:
            s.w.put(v, n)
        s.large = True
        s.block(FRONT, last=True)
        s.valid, s.out = False, bytearray()
        add("M-V-large-window-%s" % name, "M", s)


def behind_stored(size=8192):
    """headers no decoder accepts, and two it does, behind a stored metablock of `size` bytes and a valid compressed one: streams of
    more than `size` bytes whose fault lies in a header (test_gpu_headers.py: the launch that asks the device about its streams
    first takes batches with a mean of 8 KiB a stream) -> [(label, stream, the output in front of the last metablock)]"""
    out = []
    for slot in ("lit", "cmd", "d64"):
        pslot, alphabet, max_symbol = SLOTS[slot][:3]
        forms = dict(p_forms(alphabet, max_symbol))
        for form in ("V-seventeens-21", "V-repeat-one-beyond", "V-space-over-by-a-repeat", "V-cl-space-over", "V-simple-same-24", "one-17", "depth-sixteens", "16chain-k3-e2"):
            kw = dict(forms[form]); kw.pop("unchecked", None)
            s = code_stream(slot, E.WireCode(alphabet, max_symbol=max_symbol, unchecked=True, **kw), front=True, stored=size)
            out.append(("P-%s-%s" % (slot, form), s.w.finish(), bytes(s.out)))
    for label, kw in (("C-V-run-one-beyond", dict(lit=([1, 2] + [0] * 126, {"rlemax": 6, "items": [("v", 1), ("v", 2), ("run", 6, 63)]}), unchecked=True)),
                      ("C-dist-V-run-one-beyond", dict(dist=([1] + [0] * 7, {"rlemax": 2, "items": [("v", 1), ("v", 0), ("run", 2, 3)]}), unchecked=True)),
                      ("C-V-run-c16-ones", dict(lit=([0] * 16384, {"rlemax": 16, "ntrees": 3, "items": [("run", 16, 65535)]}), unchecked=True)),
                      ("C-imtf-every-tree", dict(lit=(indices_to_values((MTF_SEQ + [255] * 256 + [0] * 512)[:512]), {"rlemax": 9, "imtf": 1})))):
        s = map_stream(front=True, stored=size, **kw)
        out.append((label, s.w.finish(), bytes(s.out)))
    return out


# ------------------------------------------------------------------ the vectors
def vectors(families="PCBM"):
    """-> [{"label", "family", "window", "large", "stream", "output" (what the emitter expects; of a stream no decoder accepts: what it
    put out in front of the offending metablock), "valid", "hlog", "clog", "first_command", "extremes", the family's own notes}]"""
    out = []

    def add(label, family, s, **meta):
        comp = s.w.finish()
        assert len(comp) <= MAX_FILE * MAX_PARTS, (label, len(comp))
        assert not any(v["label"] == label for v in out), label
        out.append(dict(meta, label=label, family=family, window=s.wbits, large=s.large, stream=comp, output=bytes(s.out), valid=s.valid, hlog=s.hlog, clog=s.clog,
                        first_command=s.first_command, extremes=getattr(s, "extremes", None)))
    for family, make in (("P", p_vectors), ("C", c_vectors), ("B", b_vectors), ("M", m_vectors)):
        if family in families:
            make(add)
    return out


def entries():
    """(manifest entry, stream) of every vector, checked with the oracle and libbrotlidec"""
    import libbrotli_ref as ref
    import oracle_lib as oracle
    for v in vectors():
        comp, raw, label = v["stream"], v["output"], v["label"]
        flags = 1 if v["large"] else 0
        info, got = oracle.decode(comp, len(raw) + 64, flags)
        if v["valid"]:
            assert info.result == 1 and got == raw and info.consumed == len(comp), (label, info.result, info.error_code, info.decoded_size, len(raw))
        if ref.available():
            r = ref.decode(comp, len(raw) + 64, bool(flags))
            assert (r[0] == 1) == (info.result == 1) and (r[2] == got or info.result != 1 and (got.startswith(r[2]) or r[2].startswith(got))), (label, r[0], r[1], info.result, info.error_code)
        e = {"label": label, "size": len(raw), "first_command": v["first_command"]}
        if v["window"] != 22:
            e["window"] = v["window"]
        if v["large"]:
            e["large"] = True
        if v["valid"]:   # (the oracle's answer is (1, 1, size); its counts are pinned with the output's digest)
            e["sha"] = hashlib.sha256(raw).hexdigest()[:16]
            e["counts"] = [info.num_metablocks, info.num_commands]
        else:
            e["oracle"] = [info.result, info.error_code, info.decoded_size]
        e["csize"] = len(comp)
        yield e, comp
        print(e)   # (placed by now)


def main():
    vector_store.write(OUT, entries(), small="pack", style="lines")


if __name__ == "__main__":
    main()
