#!/usr/bin/env python3
"""tests/golden/emitter_dict/: streams written by tools/brotli_emit.py FOR a custom (LZ77 prefix) dictionary, which put every shape
of a copy out of the dictionary, the three window regimes, the dictionary's far edge and the words behind it, ring codes that name
distances into the dictionary and the literal context behind a dictionary copy through the decoder.  The plans, the literal source
and the text-like make-up are those of tools/make_word_vectors.py and tools/make_copy_vectors.py; the probes of E those of
tools/make_literal_vectors.py.

Notation: D = the dictionary's bytes in reach, P = the output position at the copy, MB = (1 << wbits) - 16, before = distance - P
(the bytes in front of position 0 at which the copy starts), n = the copy length, reach = min(P + D, MB).

  A  copy shapes out of the dictionary: the matrix before x n at sixteen destination alignments for eighteen dictionary sizes (all
     residues mod 16), copies as a stream's first command at P = 0, 1, 2, 15, 16, 17 that repeat themselves through the dictionary's
     end, the copy as the metablock's and the stream's last command, and copies that overrun MLEN (invalid on purpose)
  B  the three window regimes at window 10 -- P + D < MB, P < MB <= P + D, P >= MB -- copies at the largest distance and the word
     one beyond it at the six positions round the regimes' borders, for five dictionary sizes; one form at window 16
  C  the far edge: distance = reach (a copy) and reach + 1 (word 0, transform 0) for every word length, the largest word number
     and the one beyond it, lengths 2, 3 and 25 beyond reach, the invalid ring forms of make_word_vectors, three kinds of transform
     for every length in every regime, a run of 80 dictionary copies
  D  the ring: short codes 0 .. 15 and the implicit distance on an entry that reached into the dictionary
  E  a probe literal (make_literal_vectors.Build.probe) directly behind a dictionary copy, under each of the four context modes
  F  carriers for the command paths: the text-like streams T (make_copy_vectors) and C (make_word_vectors) with one command in
     twenty a cell of A, C or D, and C with one in three hundred (F-S: the stream the path engine keeps inside its passes)
  G  four final copies out of the dictionary for the output limits

A dictionary is not stored: `dictionary(seed, size)` makes it again (dict_gen.text); the manifest holds seed, size and SHA-256 of each once ("dictionaries"),
a stream's entry its (seed, size).
`vectors()` is deterministic.  `main()` asks the oracle (brotli_oracle_decode_dict) about every stream before it writes.  Streams
of less than 256 bytes live in the manifest ("hex"), the others in files of at most 64 466 bytes ("file" / "files")."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import dict_gen as DG  # noqa: E402
import make_copy_vectors as CV  # noqa: E402
import make_literal_vectors as LV  # noqa: E402
import make_word_vectors as WV  # noqa: E402
import vector_store  # noqa: E402
from make_word_vectors import ring_or  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "emitter_dict")
from vector_store import MAX_FILE, MAX_PARTS  # noqa: E402
ALPHABET = "etaoinshrdlucmfwypvbgkqjxz ,.0123456789"

A_BEFORE = [1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025]   # (and D - 1, D)
A_LEN = [2, 3, 4, 15, 16, 17, 24, 25, 62, 63, 64, 65, 1023, 1024, 1025, 1040, 3000]
A_POS = [0, 1, 2, 15, 16, 17]
A_SIZES = [1, 15, 16, 17, 300, 70000, 1026, 1027, 1028, 69, 70, 71, 40, 41, 1034, 1035, 1037, 1038]
assert {s % 16 for s in A_SIZES} == set(range(16))
A_FIRST_DIST = [15, 16, 17, 33]   # (and P + 1, P + 2): a stream's first copy, which repeats itself below, at and above a distance of 16
B_SIZES = [600, 1007, 1008, 1009, 2500]
B_WBITS = 10
C_EDGE = [(22, 1), (22, 300), (10, 600), (10, 2500)]
D_SCENARIOS = ("into", "inside", "zero", "zero+1", "reach", "reach+1")
G_SHAPES = [(2, 1), (40, 17), (300, 64), (3000, 1025)]   # (n, before): `before` inside n
F_EVERY = 20


def dictionary(seed, size):
    """the dictionary of a vector: word salad over ALPHABET, made again from its seed (dict_gen.text)"""
    d = DG.text(random.Random(seed), size + 8, ALPHABET, 400)[:size]   # (text may come a byte short: its last word has no blank behind it)
    assert len(d) == size
    return d


def mb_of(wbits):
    return (1 << wbits) - 16


# ------------------------------------------------------------------ emit
def emit(blocks, kind, wbits, dictionary=b"", unchecked=False, mlen=None, literals=None):
    """a list of metablocks (command lists) under plan `kind` -> (stream, output the emitter expects, log, realised blocks); the ring
    runs on from one metablock to the next; `unchecked` / `mlen` belong to the last one"""
    w = E.BitWriter(); E.write_stream_header(w, wbits)
    p = WV.plan(kind)
    out, log, real, ring = bytearray(), [], [], list(E.RING_INIT)
    for i, cmds in enumerate(blocks):
        last = i == len(blocks) - 1
        r = []
        out += E.emit_compressed(w, cmds, p, last, prev=bytes(out), dictionary=dictionary, wbits=wbits, log=log, literals=literals, realised=r, ring_io=ring,
                                 unchecked=unchecked and last, mlen=mlen if last else None)
        real.append(r)
    return w.finish(), bytes(out), log, real


def dc(before):
    """a copy that starts `before` bytes in front of position 0"""
    return lambda pos, ring, md: pos + before


def dc_or(before):
    """the same where the distance is in reach, else the largest distance"""
    return lambda pos, ring, md: min(pos + before, md)


def far(pos, ring, md):
    return md


def beyond(k=1):
    """the distance k beyond reach, as it stands (a word, or no valid one)"""
    return lambda pos, ring, md: ("raw", md + k)


class Cmds:
    """a command list whose position is known while it is written: every copy part is a copy of its length (words are added with
    their totals)"""

    def __init__(self):
        self.cmds, self.pos = [], 0

    def add(self, ins, n, what, total=None):
        self.cmds.append((ins, n, what)); self.pos += ins + (n if total is None else total)
        return self

    def goto(self, target, ins=0):
        """a plain command that brings P to `target` - `ins`: nine literals and one long copy from close by -> the literals the caller's
        command needs to stand at `target` (all of a short way)"""
        gap = target - self.pos
        assert gap >= 0, (target, self.pos)
        if gap < ins + 12:
            return gap
        self.add(9, gap - ins - 9, CV.at_most(5))
        return ins


def word_total(n, idx, t):
    return len(E.transform_word(E.dictionary_word(n, idx), t))


# ------------------------------------------------------------------ A
def a_cells(size):
    """-> [(before, n)] for a dictionary of `size` bytes: per `before` the lengths on either side of position 0, and every length of
    A_LEN with some `before`"""
    befores = sorted(({b for b in A_BEFORE if b <= size} | {size - 1, size}) - {0})
    cells = []
    for b in befores:
        below, above = [n for n in A_LEN if n < b], [n for n in A_LEN if n > b + 1]
        ns = {b + 1} | ({b} if b >= 2 else set()) | ({below[0], below[-1]} if below else set()) | ({above[0]} if above else set())
        cells += [(b, n) for n in sorted(ns)]
    cells += [(befores[(5 * k) % len(befores)], n) for k, n in enumerate(A_LEN)]
    return cells


def a_matrix(size):
    """the cells of a_cells; the literals in front of cell k put its destination at address (7 k) mod 16"""
    c = Cmds().add(1, 2, dc(1))
    for k, (b, n) in enumerate(a_cells(size)):
        c.add((7 * k - c.pos) % 16, n, dc(b))
    return c.add(3, 0, 0).cmds


def a_first():
    """-> [(label, blocks)]: one copy as the stream's first command at P of A_POS, distances P + 1, P + 2 and A_FIRST_DIST, lengths
    2, distance, distance + 1, 65 and 1040 (beyond the distance: the copy repeats itself through the dictionary's end and the
    output).  In turn the copy is followed by literals, is its metablock's last command with MLEN used up (another metablock
    follows), and is the stream's last."""
    out, k = [], 0
    for p in A_POS:
        for dist in [p + 1, p + 2] + [d for d in A_FIRST_DIST if d > p + 2]:
            for n in sorted({2, dist, dist + 1, 65, 1040} - {1}):
                first = [(p, n, dc(dist - p))]
                blocks = ([first + [(3, 0, 0)]], [first, [(4, 3, CV.at_most(2)), (2, 0, 0)]], [first])[k % 3]
                out.append(("A-first-p%d-d%d-n%d-%s" % (p, dist, n, ("lits", "mbend", "last")[k % 3]), blocks)); k += 1
    return out


def a_invalid():
    """a dictionary copy that overruns MLEN -> [(label, window, commands, MLEN short by)]: far from a ring boundary, across the one at
    1024 of window 10, and with its source wholly inside the dictionary"""
    return [("A-overrun-w22", 22, [(3, 40, dc(5))], 1), ("A-overrun-w10-cross", 10, [(10, 990, CV.at_most(3)), (0, 40, dc(5))], 1),
            ("A-overrun-inside", 22, [(3, 40, dc(200))], 39)]


# ------------------------------------------------------------------ B
def b_targets(size, wbits=B_WBITS):
    mb = mb_of(wbits)
    r = min(size, mb)
    return [p for p in (mb - r - 1, mb - r, mb - r + 1, mb - 1, mb, mb + 1) if p >= 0]


def regime(pos, size, wbits):
    mb = mb_of(wbits)
    return 1 if pos + size < mb else 2 if pos < mb else 3


def b_stream(size, target, what, k, wbits=B_WBITS):
    """-> metablocks: plain commands up to `target`, the command under test there (what: "copy" at the largest distance, "word" one
    beyond it), then 50 text-like commands, a copy that takes the output past three windows, and copies at the largest distance"""
    c = Cmds()
    ins = c.goto(target, 4)
    n = (2, 16, 63, 64, 200, 1040)[k % 6] if what == "copy" else 4 + k % 21
    c.add(ins, n, far if what == "copy" else ("word", 0, 0), total=None if what == "copy" else word_total(n, 0, 0))
    head = c.cmds
    mid = [(2, 5, ("implicit",)), (1, 6, ("ring", 1))] + CV.t_commands(random.Random(size + target), 50, max_dist=mb_of(wbits), first=False)
    tail = [(3, 3 << wbits, CV.at_most(1000)), (2, 17, far), (1, 6, ("implicit",)), (3, 0, 0)]
    return [head, mid, tail]


def b_w16():
    """the regimes in one stream of window 16, dictionary of 60000 bytes: copies at the largest distance at MB - D - 1 (two bytes, so
    that the next stands at MB - D + 1), at MB - 1 and at MB + 1, the word one beyond behind each"""
    mb, size = mb_of(16), 60000
    c = Cmds()
    for target, n in ((mb - size - 1, 2), (mb - 1, 2)):
        ins = c.goto(target, 4)
        c.add(ins, n, far).add(0, 5, far).add(1, 9, ("word", 0, 0), total=9).add(2, 7, dc_or(33))
    c.add(3, 3 << 16, CV.at_most(4000)).add(2, 17, far).add(3, 0, 0)
    return [c.cmds]


# ------------------------------------------------------------------ C
def classes():
    """-> {n: (transform that keeps the length, one that lengthens, one that shortens)} for word 0 of every length"""
    got = {}
    for n in range(4, 25):
        same = next(t for t in range(E.NUM_TRANSFORMS) if word_total(n, 0, t) == n)
        more = next(t for t in range(E.NUM_TRANSFORMS) if word_total(n, 0, t) > n)
        less = next(t for t in range(E.NUM_TRANSFORMS) if 0 < word_total(n, 0, t) < n)
        got[n] = (same, more, less)
    return got


C_REG_WBITS, C_REG_SIZE = 11, 1000


def c_regimes():
    """for every copy length 4 .. 24 a word under a transform that keeps the length, one that lengthens and one that shortens, in each
    of the three regimes (window 11, a dictionary of 1000 bytes: P < 1032, P < 2032, beyond); a dictionary copy between them while
    one is in reach"""
    mb = mb_of(C_REG_WBITS)
    c = Cmds()
    cl = classes()
    for start in (0, mb - C_REG_SIZE, mb):
        ins = c.goto(start, 1) if start else 1
        for n in range(4, 25):
            for t in cl[n]:
                idx = (n * 7 + t) % WV.nwords(n)
                c.add(ins, n, ("word", idx, t), total=word_total(n, idx, t)); ins = 0
            c.add(0, 2 + n % 3, dc_or(1 + n))
    return [c.add(3, 0, 0).cmds]


def c_edge(wbits, size):
    """the distance at reach (the dictionary's first byte in reach: a copy) and one beyond (word 0, transform 0) for every word length"""
    cmds = []
    for n in range(4, 25):
        cmds += [(1, n, far), (1, n, ("word", 0, 0))]
    return [cmds + [(3, 0, 0)]]


def c_last_words():
    """the largest valid word number of every length: the last word under transform 120"""
    return [[(1, n, ("word", WV.nwords(n) - 1, E.NUM_TRANSFORMS - 1)) for n in range(4, 25)] + [(3, 0, 0)]]


def c_invalid():
    """-> [(label, window, dictionary size, commands)]: the word number one beyond the largest (ERROR_FORMAT_TRANSFORM) and lengths 2,
    3 and 25 at reach + 1 (ERROR_FORMAT_DICTIONARY), in regime 1 (window 22) and, the latter, in regimes 2 and 3 (window 10)"""
    out = []
    bits = E.tables()["size_bits"]
    for n in (4, 11, 24):
        out.append(("C-transform-n%d" % n, 22, 300, [(2, 5, dc(2)), (1, n, ("word", WV.nwords(n) - 1, 120)), (1, n, (lambda n: lambda pos, ring, md: ("raw", md + 1 + (121 << bits[n])))(n))]))
    for n in (2, 3, 25):
        out.append(("C-dictionary-n%d" % n, 22, 300, [(2, 5, dc(2)), (1, n, beyond())]))
        for reg, target in ((2, 700), (3, 1100)):
            c = Cmds(); ins = c.goto(target, 2)
            out.append(("C-dictionary-n%d-regime%d" % (n, reg), 10, 600, c.cmds + [(ins, n, beyond())]))
    return out


def c_ring_forms():
    """the ring forms of make_word_vectors (E: ring codes that name a word at P = 0 .. 12) for a dictionary of one byte: those whose
    ring distance lies beyond P + 1, the others one literal earlier where that puts it there (code 8 at the stream's start names
    distance 1, which any dictionary has in reach) -> [(label, commands, valid)]"""
    out = []
    for label, cmds, valid in WV.ring_word_streams():
        pos, _, what = cmds[0]
        code = what[1]
        d = E.RING_INIT[code] if code < 4 else E.RING_INIT[(code - 4) // 6] + (1, 2, 3)[((code - 4) % 6) // 2] * (1 if code & 1 else -1)
        if d <= pos + 1 and pos >= 1:
            pos -= 1
            cmds = [(pos,) + tuple(cmds[0][1:])] + cmds[1:]
        if d > pos + 1:
            out.append(("C-" + label, cmds, valid))
    return out


def c_run():
    """80 consecutive dictionary copies, a literal in front of every third"""
    return [[(2, 5, dc(9))] + [(1 if k % 3 == 0 else 0, 2 + (k * 5) % 23, dc(1 + (k * 37) % 290)) for k in range(80)] + [(3, 0, 0)]]


# ------------------------------------------------------------------ D
def code_parts(code):
    """short code (None: the implicit distance) -> (ring entry, what is added to it)"""
    if code is None or code < 4:
        return code or 0, 0
    return (code - 4) // 6, (1, 2, 3)[((code - 4) % 6) // 2] * (1 if code & 1 else -1)


def d_stream(code, scen, wbits, size):
    """four copies whose distances reach into the dictionary fill the ring, then `code` names one of them at P2, where the distance it
    gives is: "into" five bytes into the dictionary, "inside" three bytes inside the output, "zero" position 0 itself, "zero+1" the
    dictionary's last byte, "reach" the dictionary's first byte in reach, "reach+1" one beyond (a word, which pushes nothing).
    The implicit distance and a ring code 1 follow.  -> commands, or None where the ring cannot hold such an entry (a distance is
    at most the reach of its own position, so only codes that add reach reach + 1, and only those that do not subtract reach)"""
    e, delta = code_parts(code)
    mb = mb_of(wbits)
    for ln in (2, 3, 4, 6, 8):
        for ins in (0, 1, 2, 3):
            at = [(1 + ln) * i + 1 for i in range(4)]
            p2 = (1 + ln) * 4 + ins
            reach = min(p2 + size, mb)
            target = {"into": p2 + 5, "inside": p2 - 3, "zero": p2, "zero+1": p2 + 1, "reach": reach, "reach+1": reach + 1}[scen]
            base = target - delta
            pe = at[3 - e]
            if not (pe < base <= min(pe + size, mb) and 1 <= target):
                continue
            cmds = []
            for i in range(4):
                d = base if i == 3 - e else at[i] + 1 + (i * 5 + (code or 0)) % min(size, 9)
                if i != 3 - e and d == base:
                    d += 1
                assert at[i] < d <= min(at[i] + size, mb)
                cmds.append((1, ln, d))
            n = 4 + (code or 0) % 21 if scen == "reach+1" else (2, 5, 17, 3)[(code or 0) % 4]
            cmds.append((ins, n, ("implicit",) if code is None else ("ring", code)))
            return cmds + [(2, 3, ("implicit",)), (1, 4, ("ring", 1)), (2, 0, 0)]
    return None


def d_streams():
    """-> [(label, window, dictionary size, commands, code, scenario)]"""
    out = []
    for wbits, size in ((22, 40), (10, 2500)):
        for scen in D_SCENARIOS:
            for code in list(range(16)) + [None]:
                cmds = d_stream(code, scen, wbits, size)
                if cmds is not None:
                    out.append(("D-w%d-%s-%s" % (wbits, "implicit" if code is None else "code%d" % code, scen), wbits, size, cmds, code, scen))
    return out


# ------------------------------------------------------------------ E
E_SIZE = 300


def e_vector(mode, seed):
    """under context mode `mode` (64 trees, the identity map): a probe and the literal behind it directly behind a dictionary copy at
    P = 0, behind copies of 2 bytes that lie wholly in the dictionary, and behind copies whose last two bytes straddle position 0
    (the last byte is the stream's first) -> the Build"""
    d = dictionary(500 + mode, E_SIZE)
    b = LV.Build(dictionary=d); b.rnd = rnd = random.Random(seed)
    b.begin(LV.x_scheme([mode], cheap=True))

    def both(cell):
        b.probe(cell); b.probe(cell + "+1")

    def at_zero():
        n = rnd.choice((2, 2, 3, 5, 17))
        b.copy(n, rnd.randrange(n, E_SIZE)); both("copy-p0")

    def two():
        b.rlit(rnd.randrange(1, 4)); b.copy(2, len(b.out) + rnd.randrange(2, E_SIZE)); both("copy-dict2")

    def straddle(n):
        b.rlit(rnd.randrange(0, 3))
        b.copy(n, len(b.out) + n - 1); both("copy-straddle")

    def first():   # (the two bytes in front of a straddling copy's probe are the dictionary's last and the stream's first: drawn with the first copy)
        at_zero()
        for n in (2, 3, 9, 40):
            straddle(n)
    b.cell(first)
    for _ in range(6):
        b.cell(two)
    b.rlit(3)
    b.end(last=True)
    return b


# ------------------------------------------------------------------ F
F_SIZE = 70000
_F_BEFORE = A_BEFORE + [F_SIZE - 1, F_SIZE]
_F_LEN = [2, 3, 4, 15, 16, 17, 24, 25, 62, 63]
_F_LONG = [64, 65, 1023, 1024, 1025, 1040, 3000]


def f_embed(cmds, every=F_EVERY, clip=False):
    """one command in `every` becomes a cell: a dictionary copy (A's `before` x n, one in eight a long one), the copy at reach and the
    word beyond it (C), and behind every second cell a ring code on the distance just pushed (D)"""
    cmds = list(cmds)
    k = 0
    for i in range(7, len(cmds) - 2, every):
        ins = cmds[i][0]
        sel = k % 8
        if sel == 6:
            cmds[i] = (ins, 4 + (k // 8) % 21, far)
        elif sel == 7:
            cmds[i] = (ins, 4 + (k // 8) % 21, ("word", 0, 0))
        else:
            n = _F_LONG[(k // 8) % len(_F_LONG)] if sel == 5 else _F_LEN[k % len(_F_LEN)]
            cmds[i] = (ins, n, (dc_or if clip else dc)(_F_BEFORE[k % len(_F_BEFORE)]))   # (clip: for a dictionary or a window that does not reach so far)
        if k % 2 == 0:
            cmds[i + 1] = (min(cmds[i + 1][0], 9), min(cmds[i + 1][1], 63), ring_or((k // 2) % 16, 300 + k))
        k += 1
    return cmds


def own(cmds):
    """the same commands with every distance that is theirs to choose kept inside the stream's own output: they are told that the
    largest distance is P (words keep their numbers: the emitter counts the dictionary for those)"""
    return [(ins, n, (lambda f: lambda pos, ring, md: f(pos, ring, min(pos, md)))(what)) if callable(what) else (ins, n, what) for ins, n, what in cmds]


F_SPARSE = 300
F_W = (16, 600)   # (window, dictionary size) of F-W


def f_carriers():
    """-> [(label, commands, kinds, seed, least compressed size)].  F-S is C's make-up with a cell every 300 commands only and no other
    distance beyond P: a dictionary copy ends a pass of the path engine, and one command in twenty being one leaves the engines next
    to nothing of F-T and F-C (every invocation "gets nowhere"); in F-S they run regions of words, whose numbers the dictionary
    moves, and plain copies, with a dictionary copy now and then.  F-W is the same make-up at window 16 with a dictionary of 600
    bytes (F_W): with a dictionary attached a stream leaves the lean form for the path engine's general one -- pe_dict_word, classify --
    only where P has passed the window (csrc/brotli_kernels.hip, `form_raw >> 10`), and two thirds of F-W lie there"""
    return [("F-W", f_embed(WV.text_commands(random.Random(74), 6000, max_dist=30000), every=F_SPARSE, clip=True) + [(4, 0, 0)], ("cf", "ctx"), 705, 0),
            ("F-S", f_embed(own(WV.text_commands(random.Random(73), 6000)), every=F_SPARSE) + [(4, 0, 0)], ("cf", "ctx"), 704, 0),
            ("F-T", f_embed(CV.t_commands(random.Random(70), 6000)) + [(4, 0, 0)], ("cf", "ctx", "cf4"), 701, 0),
            ("F-C", f_embed(WV.text_commands(random.Random(71), 6000)) + [(4, 0, 0)], ("cf", "ctx"), 702, 0),
            ("F-T2-long", f_embed(CV.t_commands(random.Random(72), 16000)) + [(4, 0, 0)], ("cf",), 703, 65536)]


# ------------------------------------------------------------------ G
def g_stream(n, before):
    base = f_embed(CV.t_commands(random.Random(80), 300), every=10)
    return [base + [(2, n, dc(before))]]


# ------------------------------------------------------------------ the vectors
def vectors():
    """-> [{"label", "window", "dseed", "dsize", "kind", "valid", "comp", "raw" (for an invalid stream: what the emitter put out), "log",
    "meta"}]"""
    out = []

    def add(label, blocks, wbits, dspec, seed, kinds=("cf", "ctx"), valid=True, short=None, meta=None, min_size=0):
        d = dictionary(*dspec)
        lits = CV.LongLiterals(seed)
        _, rraw, _, real = emit(blocks, "cf", wbits, d, unchecked=True, mlen=1 << 24, literals=lits)   # (the stream written here is thrown away)
        mlen = None
        if not valid:   # (a word that is no valid one gets room behind it: a metablock that is complete behind its literals ignores the copy)
            assert len(real) == 1
            mlen = len(rraw) + 100 if short is None else len(rraw) - short
        first = None
        for kind in kinds:
            comp, raw, log, _ = emit(real, kind, wbits, d, unchecked=not valid, mlen=mlen)
            assert first is None or raw == first, label
            first = raw
            assert min_size <= len(comp) <= MAX_FILE * MAX_PARTS, (label, kind, len(comp))
            out.append({"label": label + "-" + kind, "window": wbits, "dseed": dspec[0], "dsize": dspec[1], "kind": kind, "valid": valid, "comp": comp, "raw": raw,
                        "log": log, "meta": dict(meta or {})})

    # A
    for size in A_SIZES:
        add("A-matrix-D%d" % size, [a_matrix(size)], 22, (1000 + size, size), 100 + size % 97, meta={"family": "A"})
    for label, blocks in a_first():
        add(label, blocks, 22, (1300, 300), 101, kinds=("cf", "ctx") if "-lits" in label else ("cf",), meta={"family": "A-first"})   # (a plan with context where literals follow)
    for label, wbits, cmds, short in a_invalid():
        add(label, [cmds], wbits, (1300, 300), 102, valid=False, short=short, meta={"family": "A-invalid"})
    # B
    k = 0
    for size in B_SIZES:
        for target in b_targets(size):
            for what in ("copy", "word"):
                blocks = b_stream(size, target, what, k)
                several = size in (600, 2500) and what == "copy"
                add("B-D%d-p%d-%s" % (size, target, what), blocks if several else [sum(blocks, [])], B_WBITS, (2000 + size, size), 200 + k,
                    kinds=("cf", "ctx") if several else ("cf",), meta={"family": "B", "target": target, "what": what})
                k += 1
    add("B-w16-D60000", b_w16(), 16, (2016, 60000), 299, meta={"family": "B16"})
    # C
    for wbits, size in C_EDGE:
        add("C-edge-w%d-D%d" % (wbits, size), c_edge(wbits, size), wbits, (3000 + size, size), 300, meta={"family": "C-edge"})
    add("C-last-words", c_last_words(), 22, (3300, 300), 301, meta={"family": "C-last"})
    for label, wbits, size, cmds in c_invalid():
        add(label, [cmds], wbits, (3000 + size, size), 302, kinds=("cf",), valid=False, meta={"family": "C-invalid"})
    for label, cmds, valid in c_ring_forms():
        add(label, [cmds], 22, (3001, 1), 303, kinds=("cf",), valid=valid, meta={"family": "C-ring"})
    add("C-regimes", c_regimes(), C_REG_WBITS, (3011, C_REG_SIZE), 304, meta={"family": "C-regimes"})
    add("C-run", c_run(), 22, (3300, 300), 305, meta={"family": "C-run"})
    # D
    for label, wbits, size, cmds, code, scen in d_streams():
        add(label, [cmds], wbits, (4000 + size, size), 400, kinds=("cf",), meta={"family": "D", "code": code, "scenario": scen})
    # E
    for mode in range(4):
        b = e_vector(mode, 600 + mode)
        out.append({"label": "E-mode%d-ctx" % mode, "window": 22, "dseed": 500 + mode, "dsize": E_SIZE, "kind": "ctx", "valid": True, "comp": b.w.finish(), "raw": bytes(b.out),
                    "log": b.clog, "meta": {"family": "E", "mode": mode, "probes": list(b.probes), "cells": list(b.cells), "llog": b.llog}})
    # F
    for label, cmds, kinds, seed, least in f_carriers():
        wbits, dspec = (F_W[0], (5001, F_W[1])) if label == "F-W" else (22, (5000, F_SIZE))
        add(label, [cmds], wbits, dspec, seed, kinds=kinds, meta={"family": "F"}, min_size=least)
    # G
    for n, before in G_SHAPES:
        add("G-n%d-b%d" % (n, before), g_stream(n, before), 22, (5000, F_SIZE), 800, meta={"family": "G", "final": (n, before)})
    return out


def entry(v, oracle_decode_dict):
    """the manifest's entry of a vector, with the oracle's answer"""
    d = dictionary(v["dseed"], v["dsize"])
    info, got = oracle_decode_dict(v["comp"], len(v["raw"]) + 64, 0, d)
    e = {"label": v["label"], "window": v["window"], "dict": [v["dseed"], v["dsize"]], "kind": v["kind"],
         "valid": v["valid"], "size": len(v["raw"]), "csize": len(v["comp"]), "sha256": hashlib.sha256(v["raw"] if v["valid"] else got).hexdigest(),
         "oracle": [info.result, info.error_code, info.decoded_size]}
    if v["valid"]:
        assert info.result == 1 and got == v["raw"] and info.consumed == len(v["comp"]), (v["label"], info.result, info.error_code, info.decoded_size, len(v["raw"]))
        assert info.num_commands == len(v["log"]), (v["label"], info.num_commands, len(v["log"]))
        e["success"] = [info.consumed, info.num_commands, info.num_metablocks]
    else:
        assert info.result == 0 and info.error_code < 0 and got[:len(v["raw"])] == v["raw"][:len(got)], (v["label"], info.result, info.error_code)
    return e


def main():
    import dict_streams
    made = vectors()
    dicts = dict.fromkeys((v["dseed"], v["dsize"]) for v in made)   # (in the order of their first use)
    rows = [{"seed": seed, "size": size, "sha256": hashlib.sha256(dictionary(seed, size)).hexdigest()} for seed, size in dicts]
    for e in vector_store.write(OUT, ((entry(v, dict_streams.oracle_decode_dict), v["comp"]) for v in made), dictionaries=rows):
        print({k: x for k, x in e.items() if k != "hex"})


if __name__ == "__main__":
    main()
