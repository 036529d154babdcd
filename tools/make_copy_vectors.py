#!/usr/bin/env python3
"""tests/golden/emitter_copies/: streams written by tools/brotli_emit.py that put every command symbol, every distance symbol
under nine (NPOSTFIX, NDIRECT) pairs and every shape of LZ77 copy through the decoder, in places an encoder library never
writes them.  The plans, the literal source and the text-like make-up are those of tools/make_word_vectors.py; nothing here
names a word of the static dictionary (every generator asserts that from the emitter's log).

  S  command symbols: S1a / S1b hold all 704 symbols with both extremes of their extra fields, S2 stacks the widest fields
  D  distance symbols: every reachable symbol at its first and last distance, windows 18 and 24
  M  the copy matrix: 92 distances x 41 lengths, sixteen destination alignments per length
  T  copies in the engines' kind of stream (text_commands' make-up without words)
  H  chains of dependent copies, sources that straddle a region's start, staged and unstaged stretches
  W  copies at exactly the maximum distance while and after the window fills
  L  3000 commands and one final copy of each execution shape (output limits)

A vector is a list of metablocks (command lists); the ring of the last four distances runs on from one to the next.
`vectors()` is deterministic.  `main()` checks every stream with the oracle and libbrotlidec before it writes.  Streams of
less than 256 bytes live in the manifest ("hex"), the others in files of at most 64 466 bytes ("file" / "files"); a stream that
would need more than four files is refused (none does)."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import vector_store  # noqa: E402
import make_word_vectors as WV  # noqa: E402
from make_word_vectors import Literals, plan, ring_or  # noqa: E402,F401

OUT = os.path.join(ROOT, "tests", "golden", "emitter_copies")
from vector_store import MAX_FILE, MAX_PARTS  # noqa: E402
PAIRS = ((0, 0), (0, 15), (1, 0), (1, 2), (1, 30), (2, 4), (2, 60), (3, 8), (3, 120))  # D's (NPOSTFIX, NDIRECT)
M_DIST = list(range(1, 70)) + [95, 96, 97, 127, 128, 129, 255, 256, 257, 511, 512, 1022, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097, 65535, 65536, 65537]
M_LEN = list(range(2, 10)) + [15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63, 64, 65, 66, 79, 80, 81, 127, 128, 129, 255, 256, 257,
                              1007, 1008, 1009, 1023, 1024, 1025, 1039, 1040, 1041, 2049]
assert len(M_DIST) == 92 and len(M_LEN) == 41
L_SHAPES = ((2, 5), (16, 100), (63, 63), (64, 64), (65, 200), (1024, 1024), (1025, 5000), (700, 100), (700, 64), (700, 7), (3000, 1), (3000, 2000))
H_DEPTHS, H_UNITS = (1, 2, 5, 6, 7, 8, 20, 130), (9, 16, 17, 64)
H_SELF = [(d, n) for d in (1, 2, 3, 7, 63, 64, 65, 1023) for n in (64, 65, 1024, 1025, 5000)]
W_LENS = (2, 16, 64, 1008)


class LongLiterals(Literals):
    """Literals for metablocks of more than 86 800 literals: the block type of every literal the CTX plan has room for"""

    def __init__(self, seed):
        Literals.__init__(self, seed)
        self.type_of = [t for t, c in WV._LIT_BLOCKS for _ in range(c)]


MAX_LITS = 800000  # (a metablock's literals: the CTX plan's literal blocks hold 868 000)


def emit(blocks, kind, wbits, npostfix=0, ndirect=0, literals=None, dictionary=b""):
    """make_word_vectors.emit for a list of metablocks and any (NPOSTFIX, NDIRECT) -> (stream, output, log, realised blocks)"""
    w = E.BitWriter(); E.write_stream_header(w, wbits)
    p = plan(kind)
    p.npostfix, p.ndirect = npostfix, ndirect
    out, log, real, ring = bytearray(), [], [], list(E.RING_INIT)
    for i, cmds in enumerate(blocks):
        r = []
        out += E.emit_compressed(w, cmds, p, i == len(blocks) - 1, prev=bytes(out), dictionary=dictionary, wbits=wbits, log=log, literals=literals, realised=r, ring_io=ring)
        assert len(out) <= (i + 1) << 24
        real.append(r)
    assert not any(r["word"] for r in log), "a command became a dictionary word"
    return w.finish(), bytes(out), log, real


def realise(blocks, wbits, seed, npostfix=0, ndirect=0, dictionary=b""):
    """counts of literals and functions for distances -> bytes and plain forms (make_word_vectors.realise)"""
    return emit(blocks, "cf", wbits, npostfix, ndirect, literals=LongLiterals(seed), dictionary=dictionary)[3]


def split(cmds):
    """one command list -> metablocks of at most MAX_LITS literals and 2^24 bytes of output"""
    blocks, lits, size = [[]], 0, 0
    for c in cmds:
        n = c[0] if isinstance(c[0], int) else len(c[0])
        if blocks[-1] and (lits + n > MAX_LITS or size + n + c[1] > 1 << 24):
            blocks.append([]); lits = size = 0
        blocks[-1].append(c); lits += n; size += n + c[1]
    return blocks


def size_of(cmds):
    return sum((c[0] if isinstance(c[0], int) else len(c[0])) + c[1] for c in cmds)


def at_most(d):
    return lambda pos, ring, md: min(d, md)


def far(pos, ring, md):
    return md


# ------------------------------------------------------------------ T: the engines' kind of stream
_T_LEN = [n for n in M_LEN if n <= 63]


def t_commands(rnd, n, max_dist=66000, first=True):
    """make_word_vectors.text_commands without words: 0 .. 12 literals, copies of 2 .. 63 bytes (rarely 64 .. 70: its comment on
    rec_off), 30 % explicit distances, 50 % ring codes in rotation, 20 % the implicit distance.  Lengths and distances come from
    M's lists; a tenth of the copies is 15 .. 17 bytes long, a tenth 62 or 63 (64 is one of the rare ones).  Distances below the
    copy length and the copies of more than 63 bytes come in bursts of 20 commands, one burst in 300 commands or so, with four
    distances of 64 and more behind each, which clear the ring: the record loop of the kernel takes copies that do not overlap themselves, and gives a
    metablock up when its calls stay short (rec_poor in csrc/brotli_kernels.hip) -- so the overlapping copies meet the checked
    stages in a row, and the others the record loop."""
    cmds = [(24, 8, 5), (6, 12, 17)] if first else []
    dists = [d for d in M_DIST if d <= max_dist]
    rot, start, burst = 0, len(cmds), 0

    def clear_of(clen):  # (mostly 64 and more: the ring codes and the implicit distance use it again, with other copy lengths)
        return rnd.choice([d for d in dists if d >= (64 if rnd.random() < 0.97 else clen)])
    while len(cmds) - start < n - (2 if first else 0):
        ins = rnd.randrange(0, 13)
        r = rnd.random()
        clen = rnd.choice((15, 16, 17)) if r < 0.104 else rnd.choice((62, 63)) if r < 0.204 else rnd.choice(_T_LEN)
        r = rnd.random()
        if burst == 0 and rnd.random() < 0.0035:
            burst = 24
        if burst:
            burst -= 1
            if burst >= 4 and rnd.random() < 0.07:
                clen = rnd.randrange(64, 71)
            d = rnd.randrange(1, clen) if burst >= 4 else clear_of(64)
            cmds.append((ins, clen, at_most(d)))
        elif r < 0.3:
            cmds.append((ins, clen, at_most(clear_of(clen))))
        elif r < 0.5:
            cmds.append((min(ins, 9), min(clen, 69), ("implicit",)))
        else:
            cmds.append((ins, clen, ring_or(rot & 15, clear_of(clen)))); rot += 1
    return cmds


# ------------------------------------------------------------------ S: command symbols
def _skewed(rnd, n):
    """a long insert: two symbols, one of them 31 times in 32 -- about a bit a literal"""
    return bytes(rnd.choices(b"e ", cum_weights=(31, 32), k=n))


def _extremes(base, extra, code):
    """the values of a length code whose extra field is all zeros and all ones (a 24-bit field: 0 and 1)"""
    return (base[code], base[code] + ((1 << extra[code]) - 1 if extra[code] <= 14 else 1))


def s1_commands(ins_codes, seed):
    """every (insert code, copy code) pair of `ins_codes` x 0 .. 23 with an explicit distance, and those of the 8 x 16 pairs again
    with the implicit one; each twice, the extra fields all zeros and all ones; the 24-bit fields at 0, 1 and 65536 + 5"""
    rnd = random.Random(seed)
    cmds, k = [(3000, 4, 7)], 0

    def ins_of(n):
        return n if n < 64 else _skewed(rnd, n)
    for ic in ins_codes:
        for cc in range(24):
            for which in (0, 1):
                ins, clen = _extremes(E._INS_BASE, E._INS_EXTRA, ic)[which], _extremes(E._COPY_BASE, E._COPY_EXTRA, cc)[which]
                k += 1
                cmds.append((ins_of(ins), clen, at_most(1 + (k * 131) % 2900)))
                if ic < 8 and cc < 16:
                    cmds.append((ins_of(ins), clen, ("implicit",)))
    if 23 in ins_codes:
        cmds.append((ins_of(E._INS_BASE[23] + 65536 + 5), 9, 300))
        cmds.append((2, E._COPY_BASE[23] + 65536 + 5, 1500))
    cmds.append((3, 0, 0))
    return cmds


def _preface(target):
    """commands that bring P to at least `target` cheaply: 1009 literals and a few long copies whose distances share no period"""
    cmds, size = [(1009, 3000, 1009)], 4009
    for ins, d in ((5, 2003), (7, 3989), (3, 190001), (6, 1000003), (4, 4000037)):
        if size >= target:
            break
        d = min(d, size - 1)
        n = min(max(target - size - ins, 2), 8 * size, (1 << 24) - size - ins)
        cmds.append((ins, n, d)); size += ins + n
    assert target <= size <= 1 << 24, (size, target)
    return cmds


def _dist_range(sym, npostfix, ndirect):
    """distance symbol >= 16 + NDIRECT -> (first distance, last distance, extra bits) (RFC 7932 section 4)"""
    s = sym - 16 - ndirect
    lcode, hx = s & ((1 << npostfix) - 1), s >> npostfix
    nb = 1 + (hx >> 1)
    offset = ((2 + (hx & 1)) << nb) - 4
    return ((offset << npostfix) + lcode + ndirect + 1, ((offset + (1 << nb) - 1) << npostfix) + lcode + ndirect + 1, nb)


def s2_commands():
    """64 commands with insert code 22 / 23, copy code 22 / 23 and a distance symbol of 20 / 22 extra bits, each field all zeros or
    all ones in every combination (the 24-bit fields: 0 and, for the insert, 8191 and once 65536 + 255, for the copy 2^18 - 1), and 136 short ones between them: two literals
    or none.  -> metablocks, the preface first"""
    rnd = random.Random(22)
    pre = _preface((1 << 24) - 64)
    cmds, k = [], 0
    for nb in (20, 22):
        first, last, got = _dist_range(16 + 2 * (nb - 1), 0, 0)
        assert got == nb
        for ic in (22, 23):
            for cc in (22, 23):
                for bits in range(8):
                    iv = 0 if not bits & 1 else (1 << 14) - 1 if ic == 22 else 65536 + 255 if k == 7 else 8191
                    cv = 0 if not bits & 2 else (1 << 10) - 1 if cc == 22 else (1 << 18) - 1
                    cmds.append((_skewed(rnd, E._INS_BASE[ic] + iv), E._COPY_BASE[cc] + cv, last if bits & 4 else first))
                    k += 1
                    for j in range(2 + (k % 8 == 0)):
                        cmds.append((2 * ((k + j) & 1), 2 + (k + j) % 7, ("ring", 1 + (k + j) % 3)))
    cmds.append((3, 0, 0))
    assert len(cmds) >= 200, len(cmds)
    return [pre] + split(cmds)


# ------------------------------------------------------------------ D: distance symbols
def d_commands(npostfix, ndirect, max_distance):
    """every direct code and every distance symbol whose first distance is at most `max_distance`, at its first distance and at its
    last one or the maximum distance and one between; explicit distances equal to each ring entry, ring codes 1, 2, 3 behind each"""
    cmds, k = [], 0
    lens = (2, 3, 4, 9, 17, 70)

    def add(d):
        nonlocal k
        cmds.append((k % 4, lens[k % 6], d)); k += 1
    for d in range(1, ndirect + 1):
        add(d)
    for sym in range(16 + ndirect, 16 + ndirect + (48 << npostfix)):
        first, last, nb = _dist_range(sym, npostfix, ndirect)
        if first > max_distance:
            continue
        assert E.distance_symbol(first, npostfix, ndirect) == (sym, 0, nb) and E.distance_symbol(last, npostfix, ndirect) == (sym, (1 << nb) - 1, nb)
        top = first + ((min(last, max_distance) - first) >> npostfix << npostfix)  # (the symbol's last distance within the maximum distance)
        add(first); add(top)
        if top - first > 2 << npostfix:
            add(first + ((top - first) // 2 >> npostfix << npostfix))
    add(max_distance)
    for entry in range(4):
        for rep in range(3):
            for _ in range(4):  # (four new distances, so that the ring's entries differ)
                add(200 + 17 * k)
            cmds.append((k % 4, lens[k % 6], (lambda e: lambda pos, ring, md: ring[e])(entry))); k += 1
            for code in (1, 2, 3):
                cmds.append((k % 3, lens[(k + code) % 6], ("ring", code))); k += 1
    cmds.append((3, 0, 0))
    return cmds


# ------------------------------------------------------------------ M: the copy matrix
def m_commands(order, wbits, dists=M_DIST, lens=M_LEN, preface=None):
    """a cell per (distance, length); the literals in front of a cell put its destination at address (7 * i + 3 * j) mod 16, so that
    every length meets all sixteen.  Distances beyond the maximum distance are written as the maximum distance."""
    md = (1 << wbits) - 16
    cmds = list(preface if preface is not None else [(4200, 30000, 4200), (3, 33000, 20011)])
    pos = size_of(cmds)
    assert pos >= min(max(dists), md) + 16
    for i, j in order:
        ins = ((7 * i + 3 * j) - pos) % 16
        cmds.append((ins, lens[j], min(dists[i], md)))
        pos += ins + lens[j]
    cmds.append((3, 0, 0))
    return cmds


def m_orders():
    rows = [(i, j) for i in range(len(M_DIST)) for j in range(len(M_LEN))]
    mixed = list(rows)
    random.Random(92 * 41).shuffle(mixed)
    return (("rows", rows), ("mixed", mixed))


def m_small_commands():
    """the cut-down matrix: distances 1 .. 20 x lengths up to 17, at most 2000 bytes of output"""
    dists, lens = list(range(1, 21)), [n for n in M_LEN if n <= 20]
    order = [(i, j) for j in range(len(lens)) for i in range(len(dists))]
    cmds = [(20, lens[0], dists[0])]
    for k, (i, j) in enumerate(order[1:]):
        cmds.append((k & 1, lens[j], dists[i]))
    assert size_of(cmds) <= 2000, size_of(cmds)
    return cmds


def m_dict_commands(dict_size):
    """the cut-down matrix against a custom dictionary: every copy starts 1 .. 20 bytes inside the dictionary's end and runs over
    into the output (the longest first, while P is small and the copy overlaps itself as well)"""
    lens = sorted((n for n in M_LEN if n <= 20), reverse=True)
    cmds = []
    for n in lens:
        for j in range(1, min(20, dict_size) + 1):
            cmds.append((0 if not cmds else 1 + (len(cmds) & 1), n, (lambda j: lambda pos, ring, md: pos + j)(j)))
    cmds.append((2, 0, 0))
    return cmds


# ------------------------------------------------------------------ H: chains and region edges
def h_chain(depth, unit, lits):
    """`depth` copies of `unit` bytes, each reading exactly what the one before wrote, `lits` literals between them"""
    return [(unit + 5, unit, unit)] + [(lits, unit, unit + lits)] * depth


def h_commands(rnd):
    """-> (commands, {"chains": [(index of the first link, depth, unit, literals between)], "edges": [(index, depth, unit, kind)], ...})"""
    cmds = [(3000, 14000, 3000), (4, 15000, 7001)]
    meta = {"chains": [], "edges": [], "straddle": [], "near": [], "far": [], "self": []}
    for lits in (0, 1):
        for unit in H_UNITS:
            for depth in H_DEPTHS:
                meta["chains"].append((len(cmds) + 1, depth, unit, lits))
                cmds += h_chain(depth, unit, lits)
    # only the last byte of the source is the first byte the copy before wrote -- and only the first is the last it wrote
    for lits in (0, 1):
        for unit in H_UNITS:
            for kind, dist in (("last", 2 * unit - 1 + lits), ("first", 1 + lits)):
                cmds.append((unit + 3, unit, 400 + unit))
                meta["edges"].append((len(cmds), 8, unit, kind))
                cmds += [(lits, unit, dist)] * 8
    # sources of 2 .. 40 bytes that end 0 .. 3 bytes behind P - 300, at every one of 400 consecutive commands, three times
    for gap in (0, 1, 2):
        cmds += t_commands(rnd, 150 + 137 * gap, max_dist=20000, first=False)
        meta["straddle"].append(len(cmds))
        for k in range(400):
            n = 2 + k % 39
            cmds.append((k % 3, n, 300 + n + k % 4))
    # stretches of short copies from close by and of long ones from far back; the self-overlapping shapes inside both
    shapes = list(H_SELF)
    for rep in range(2):
        meta["near"].append(len(cmds))
        for k in range(320):
            cmds.append((k % 4, 2 + k % 11, 1 + (k * 7) % 60))
            if k % 16 == 15:
                d, n = shapes[(k // 16 + 20 * rep) % 40]
                meta["self"].append(len(cmds)); cmds.append((k % 3, n, d))
        meta["far"].append(len(cmds))
        for k in range(320):
            cmds.append((k % 4, 1000 + (k * 37) % 2001, 20000 + (k * 911) % 9000))
            if k % 16 == 15:
                d, n = shapes[(k // 16 + 20 * rep) % 40]
                meta["self"].append(len(cmds)); cmds.append((k % 3, n, d))
    cmds.append((3, 0, 0))
    return cmds, meta


def h_small_commands():
    """one chain of depth 8 (and a last-byte one) in at most 2000 bytes of output"""
    cmds = [(40, 5, 9)] + h_chain(8, 17, 0) + h_chain(8, 16, 1) + [(19, 16, 16)] + [(0, 16, 31)] * 8 + [(2, 0, 0)]
    assert size_of(cmds) <= 2000
    return cmds


# ------------------------------------------------------------------ W: the window's edge
def w_commands(wbits, rnd, lens=W_LENS, gap=50, between=3):
    """copies at exactly the maximum distance: at P = distance (they read the stream's first byte), one command before the window
    fills, on the command that fills it and 50 commands after; the implicit distance behind each -> (commands, {position: index})"""
    md = (1 << wbits) - 16
    lens = [min(n, md) for n in lens]
    cmds, at = [(24, lens[0], far), (1, 5, ("implicit",))], {"first": 0}
    while True:
        more = t_commands(rnd, 1, max_dist=md, first=False)
        if size_of(cmds) + size_of(more) > md - 120:
            break
        cmds += more
    at["before"] = len(cmds)
    cmds += [(md - 20 - lens[1] - size_of(cmds), lens[1], far), (0, 3, ("implicit",))]
    assert size_of(cmds) == md - 17
    at["on"] = len(cmds)
    cmds += [(3, lens[2], far), (2, 4, ("implicit",))]
    cmds += t_commands(rnd, gap, max_dist=md, first=False)
    at["after"] = len(cmds)
    for n in lens[::-1]:
        cmds += [(2, n, far), (1, 6, ("implicit",))] + t_commands(rnd, between, max_dist=md, first=False)
    cmds.append((3, 0, 0))
    return cmds, at


def w_small_commands(wrap):
    """W at window 10 in at most 2000 bytes of output; without `wrap` in less than 1024, so that the stream fits the ring buffer a
    decoder of window 10 keeps: the copy on which the window fills and one copy behind it, each with the implicit distance"""
    cmds, at = w_commands(10, random.Random(10), lens=(2, 16, 64, 200), gap=5, between=1)
    if not wrap:
        cmds = cmds[:at["on"]] + [(3, 16, far), (2, 4, ("implicit",)), (1, 2, far), (0, 2, ("implicit",)), (1, 0, 0)]
    assert size_of(cmds) <= (2000 if wrap else 1023), size_of(cmds)
    return cmds


# ------------------------------------------------------------------ the vectors
def vectors():
    """-> [(label, window, stream, output the emitter expects, log, {"npostfix", "ndirect", family's own notes})]"""
    out = []

    def add(label, blocks, wbits, seed, kinds=("cf", "ctx"), npostfix=0, ndirect=0, meta=None, min_size=0):
        real = realise(blocks, wbits, seed, npostfix, ndirect)
        first = None
        for kind in kinds:
            comp, raw, log, _ = emit(real, kind, wbits, npostfix, ndirect)
            assert first is None or raw == first, label
            first = raw
            assert min_size <= len(comp) <= MAX_FILE * MAX_PARTS, (label, kind, len(comp))
            out.append((label + "-" + kind, wbits, comp, raw, log, dict(meta or {}, npostfix=npostfix, ndirect=ndirect)))

    # S
    add("S1a-symbols", split(s1_commands(range(23), 1)), 22, 101)
    add("S1b-symbols", split(s1_commands((23,), 2)), 22, 102)
    add("S2-wide-fields", s2_commands(), 24, 103)
    # D
    for npostfix, ndirect in PAIRS:
        wbits = 24 if (npostfix, ndirect) in ((0, 0), (3, 120)) else 18
        md = (1 << wbits) - 16
        blocks = [_preface(md), d_commands(npostfix, ndirect, md)] if wbits == 24 else [_preface(md + 64) + d_commands(npostfix, ndirect, md)]
        add("D-p%d-d%d" % (npostfix, ndirect), blocks, wbits, 110 + npostfix * 16 + ndirect, npostfix=npostfix, ndirect=ndirect)
    # M
    for name, order in m_orders():
        add("M-%s-w22" % name, [m_commands(order, 22)], 22, 120)
        add("M-%s-w16" % name, [m_commands(order, 16)], 16, 121, npostfix=3, ndirect=120)
    # T
    add("T-text", [t_commands(random.Random(30), 6000) + [(4, 0, 0)]], 22, 130, kinds=("cf", "ctx", "cf4"))
    add("T2-text-long", [t_commands(random.Random(31), 16000) + [(4, 0, 0)]], 22, 131, kinds=("cf",), min_size=65536)
    # H
    cmds, meta = h_commands(random.Random(40))
    add("H-chains", [cmds], 22, 140, meta=meta)
    # W
    for wbits in (10, 11, 16):
        cmds, at = w_commands(wbits, random.Random(50 + wbits))
        add("W-edge-w%d" % wbits, [cmds], wbits, 150 + wbits, meta={"at": at})
    # L
    base = t_commands(random.Random(60), 3000)
    for n, dist in L_SHAPES:
        add("L-n%d-d%d" % (n, dist), [base + [(2, n, dist)]], 22, 160, meta={"final": (n, dist)})
    return out


def entries():
    """(manifest entry, stream) of every vector, checked with the oracle and libbrotlidec"""
    import libbrotli_ref as ref
    import oracle_lib as oracle
    for label, wbits, comp, raw, log, meta in vectors():
        info, got = oracle.decode(comp, len(raw) + 64, 0)
        assert info.result == 1 and got == raw and info.consumed == len(comp), (label, info.result, info.error_code, info.decoded_size, len(raw))
        assert info.num_commands == len(log), (label, info.num_commands, len(log))
        if ref.available():
            r = ref.decode(comp, len(raw) + 64, False)
            assert r[0] == 1 and r[2] == raw, (label, r[0], r[1])
        e = {"label": label, "window": wbits, "valid": True, "csize": len(comp), "size": len(raw), "sha256": hashlib.sha256(raw).hexdigest(),
             "npostfix": meta["npostfix"], "ndirect": meta["ndirect"], "metablocks": info.num_metablocks, "commands": info.num_commands}
        yield e, comp
        print({k: v for k, v in e.items() if k != "hex"})   # (placed by now)


def main():
    vector_store.write(OUT, entries())


if __name__ == "__main__":
    main()
