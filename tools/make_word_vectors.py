#!/usr/bin/env python3
"""tests/golden/emitter_words/: streams written by tools/brotli_emit.py that put every (copy length, transform) pair of the
static dictionary, every short ("ring") distance code and the implicit distance through the decoder, in places where an
encoder library never writes them -- words of zero and one byte, ring codes that land beyond the maximum distance, chains
of words without literals between them, words at the point where the window fills, and references that are invalid on
purpose.  Every vector is emitted from one command list under several plans: CF (literals without context, one distance
tree), CTX (two literal block types, modes UTF8 and SIGNED, 18 literal trees whose alphabets differ) and, for the text-like
vector, CF4 (a distance tree per distance context).

`vectors()` is deterministic.  `main()` checks every valid stream with the oracle and libbrotlidec before it writes, and
records the oracle's (result, error_code, decoded_size) for the invalid ones.  Streams of less than 256 bytes live in the
manifest itself ("hex"); the others are files, one stream of more than 64 KiB -- the size from which a batch's launch gives a
stream a gang of blocks -- a file per part ("files")."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import vector_store  # noqa: E402
from vector_store import MAX_FILE  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "emitter_words")

# ------------------------------------------------------------------ plans
_ALPHABET = b" etaoinshrdlucmfw,.0123456789ETAOINSH\n\"'()-;:\xc3\xa9\xe4\xb8\xad"
_LIT_BLOCKS = [(k & 1, 97 + 60 * (k % 5)) for k in range(4000)]  # two literal block types in turn, blocks of 97 .. 337 literals
_LIT_MODES = [2, 3]  # UTF8, SIGNED
_LIT_MAP = [(c * 5 + (c >> 3) + 9 * t) % 18 for t in range(2) for c in range(64)]
assert len(set(_LIT_MAP)) >= 16


def plan(kind):
    if kind == "cf":
        return E.Plan()
    if kind == "cf4":
        return E.Plan(dist_map=[0, 1, 2, 3])
    assert kind == "ctx"
    return E.Plan(lit_blocks=list(_LIT_BLOCKS), modes=list(_LIT_MODES), lit_map=list(_LIT_MAP))


class Literals:
    """the literal source of a command list: the byte behind (p1, p2) comes from an alphabet of ten symbols that belongs to the
    literal tree the CTX plan reads it with, so that the trees' prefix codes differ and a decoder that takes a wrong p1 / p2
    behind a word reads the literal with a wrong code"""

    def __init__(self, seed):
        self.rnd = random.Random(seed)
        self.type_of = [t for t, c in _LIT_BLOCKS[:400] for _ in range(c)]

    def __call__(self, p1, p2, k):
        t = self.type_of[k]
        tree = _LIT_MAP[t * 64 + E.literal_context(_LIT_MODES[t], p1, p2)]
        j = min(int(self.rnd.expovariate(0.45)), 9)
        return _ALPHABET[(tree * 7 + j * 3) % len(_ALPHABET)]


def emit(cmds, kind, wbits, dictionary=b"", unchecked=False, mlen=None, literals=None):
    """-> (stream, output, log, realised commands)"""
    w = E.BitWriter(); E.write_stream_header(w, wbits)
    log, real = [], []
    out = E.emit_compressed(w, cmds, plan(kind), True, dictionary=dictionary, wbits=wbits, log=log, unchecked=unchecked, mlen=mlen, literals=literals, realised=real)
    return w.finish(), out, log, real


def realise(cmds, wbits, seed):
    """a command list with counts for literals and functions for distances -> the same with bytes and plain forms"""
    return emit(cmds, "cf", wbits, literals=Literals(seed), unchecked=True, mlen=1 << 20)[3]  # (the bytes written here are thrown away)


# ------------------------------------------------------------------ command lists
def nwords(length):
    return 1 << E.tables()["size_bits"][length]


def multibyte_words():
    """[(length, idx)]: 24 words with a two-byte UTF-8 lead byte and 24 with a three-byte one, spread over the lengths"""
    t = E.tables()
    two, three = [], []
    for length in range(4, 25):
        a = b = 0
        for idx in range(nwords(length)):
            wd = E.dictionary_word(length, idx)
            if a < 2 and any(0xC0 <= c < 0xE0 for c in wd) and not any(c >= 0xE0 for c in wd):
                two.append((length, idx)); a += 1
            elif b < 2 and any(c >= 0xE0 for c in wd):
                three.append((length, idx)); b += 1
    assert len(two) >= 20 and len(three) >= 20, (len(two), len(three))
    return two[:24] + three[:24]


def uppercase_transforms():
    return [t for t, (_, kind, _) in enumerate(E.tables()["transforms"]) if kind in (10, 11)]


def matrix_commands(rnd):
    """A, first part: the 21 x 121 pairs, word index 0 / last / seeded in turn, two or three literals behind every word"""
    cmds, k = [], 0
    for transform in range(E.NUM_TRANSFORMS):
        for length in range(4, 25):
            idx = (0, nwords(length) - 1, rnd.randrange(nwords(length)))[k % 3]; k += 1
            cmds.append((2 + (k % 7 == 0), length, ("word", idx, transform)))
    return cmds


def multibyte_commands():
    """A, second part: each of the multi-byte words through every transform built on the two uppercase ones"""
    return [(2, length, ("word", idx, t)) for length, idx in multibyte_words() for t in uppercase_transforms()]


def ring_or(code, fallback):
    """short code `code` where it gives a copy (a distance of 1 .. the maximum distance), else the explicit distance"""
    def what(pos, ring, max_distance):
        d = ring[code] if code < 4 else ring[(code - 4) // 6] + (1, 2, 3)[((code - 4) % 6) // 2] * (1 if code & 1 else -1)
        return ("ring", code) if 1 <= d <= max_distance else min(fallback, max_distance)
    return what


def text_commands(rnd, n, max_dist=60000):
    """C's make-up: a word every 8 commands on average; of the others 30 % explicit distances, 50 % ring codes 0 .. 15 in
    rotation, 20 % the implicit distance; 0 .. 12 literals.  Behind a word come, in turn, the implicit distance and the next ring
    code of a rotation of its own, behind a code-0 command the next ring code of a third rotation: the two predecessors that do
    not push."""
    cmds = [(24, 8, 5), (6, 12, 17)]
    rot = after_word = after_zero = 0
    prev = "plain"
    while len(cmds) < n:
        ins = rnd.randrange(0, 13)
        # (copies of 2 .. 70 bytes; those of more than 63 are rare: each ends a call of the record loop, and six such calls in a row that took
        # less than 64 commands make the kernel give a metablock without context back to the one-wave loop -- rec_off in csrc/brotli_kernels.hip)
        r = rnd.random()
        clen = rnd.randrange(64, 71) if r < 0.004 else rnd.choice((2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21, 25, 33, 47, 62, 63)) if r < 0.5 else rnd.randrange(2, 64)
        fallback = rnd.randrange(4, max_dist)
        kind = None
        if prev == "word":
            kind = "implicit" if after_word & 1 else ("ring", (after_word >> 1) & 15)
            after_word += 1
        elif prev == "zero":
            kind = ("ring", after_zero & 15); after_zero += 1
        elif rnd.random() < 0.125:
            kind = "word"
        else:
            r = rnd.random()
            kind = "explicit" if r < 0.3 else "implicit" if r < 0.5 else ("ring", rot & 15)
            if r >= 0.5:
                rot += 1
        if kind == "word":
            length = rnd.randrange(4, 25)
            cmds.append((ins, length, ("word", rnd.randrange(nwords(length)), rnd.randrange(E.NUM_TRANSFORMS)))); prev = "word"
        elif kind == "implicit":
            cmds.append((min(ins, 9), min(clen, 69), ("implicit",))); prev = "plain"
        elif kind == "explicit":
            cmds.append((ins, clen, (lambda f: lambda pos, ring, md: min(f, md))(fallback))); prev = "plain"
        else:
            cmds.append((ins, clen, ring_or(kind[1], fallback))); prev = "zero" if kind[1] == 0 else "plain"
    return cmds


def chain_commands(rnd):
    """D: chains of k one-word commands without literals, 300 bytes of plain commands between them.  Every word has index 0
    or the last one of its length and a transform whose neighbour gives another total: a lane that takes P short or long by
    the words in front of it lands in the neighbouring transform and gets another length."""
    def total(length, t):
        return len(E.transform_word(E.dictionary_word(length, 0), t))
    cmds = [(250, 20, 7)]  # (the plain commands between the chains reach back up to 200 bytes)
    for variant in range(3):
        for k in (2, 8, 9, 20, 64):
            for j in range(k):
                length = rnd.randrange(4, 25)
                last = (variant == 1) or (variant == 2 and j & 1)
                while True:
                    t = rnd.randrange(E.NUM_TRANSFORMS)
                    nb = t + 1 if last else t - 1  # (word numbers beyond the last index run on into the next transform)
                    if 0 <= nb < E.NUM_TRANSFORMS and total(length, nb) != total(length, t) and total(length, t) > 0:
                        break
                cmds.append((0, length, ("word", nwords(length) - 1 if last else 0, t)))
            for _ in range(10):
                cmds.append((10, 20, rnd.randrange(1, 200)))
    cmds.append((5, 0, 0))
    return cmds


def small_commands(rnd):
    """H: at most 600 bytes of output with 30 words in them"""
    cmds = [(6, 4, 3)]
    for k in range(30):
        length = rnd.randrange(4, 13)
        cmds.append((rnd.randrange(0, 4), length, ("word", rnd.randrange(nwords(length)), rnd.choice((0, 0, 3, 9, 12, 44, 49, rnd.randrange(E.NUM_TRANSFORMS))))))
        if k % 3 == 0:
            cmds.append((rnd.randrange(0, 3), rnd.randrange(2, 6), ("implicit",) if k % 2 else ring_or(k % 16, 5)))
    cmds.append((3, 0, 0))
    return cmds


def _pos_after(real, wbits):
    return len(emit(real, "cf", wbits, unchecked=True, mlen=1 << 20)[1])


def ring_word_streams():
    """E: ring codes that name a word.  -> [(label, commands, valid)] for window 22"""
    out = []
    tail = [(6, 5, ("implicit",)), (9, 7, ("ring", 1)), (2, 0, 0)]  # (behind the word the ring is as it was: 4 and 11 are copies by now)
    for pos in (0, 1, 2, 3, 5, 12):
        for code in range(4):
            if E.RING_INIT[code] > pos:
                out.append(("E-p%d-code%d" % (pos, code), [(pos, 4 + (pos + 5 * code) % 21, ("ring", code))] + tail, True))
    # codes 4 .. 15: the ring's value -+ 1 .. 3 lands on P + 1 .. P + 3
    for code in range(4, 16):
        value = E.RING_INIT[(code - 4) // 6] + (1, 2, 3)[((code - 4) % 6) // 2] * (1 if code & 1 else -1)
        beyond = 1 + code % 3
        pos = value - beyond
        if pos < 0:
            pos, beyond = 0, value
        out.append(("E-code%d-beyond%d" % (code, beyond), [(pos, 4 + (3 * code) % 21, ("ring", code))] + tail, True))
    for label, pos, code in (("p0-code0", 0, 0), ("p5-code2", 5, 2), ("p4-code9", 4, 9)):
        for clen in (2, 3, 25):
            out.append(("E-%s-len%d" % (label, clen), [(pos, clen, ("ring", code))], False))
    return out


def vectors():
    """-> [(label, window, stream, output the emitter expects (for an invalid stream: up to the offending command), log, valid)]"""
    out = []

    def add(label, cmds, wbits, kinds=("cf", "ctx"), valid=True, mlen=None, parts=1):
        first = None
        if not valid and mlen is None:  # (room for the offending command: a metablock that is complete behind its literals ignores the copy)
            mlen = _pos_after(cmds, wbits) + 100
        for kind in kinds:
            comp, raw, log, _ = emit(cmds, kind, wbits, unchecked=not valid, mlen=mlen)
            assert first is None or raw == first, label
            first = raw
            assert len(comp) <= MAX_FILE * parts and (parts == 1 or len(comp) >= 65536), (label, kind, len(comp))
            out.append((label + "-" + kind, wbits, comp, raw, log, valid))

    # A: the matrix, window 22
    rnd = random.Random(20261018)
    matrix = realise(matrix_commands(rnd) + [(3, 0, 0)], 22, 1)
    multi = realise(multibyte_commands() + [(3, 0, 0)], 22, 2)
    add("A1-matrix", matrix, 22)
    add("A2-multibyte", multi, 22)
    # B: the matrix again, a stretch of plain copies up to 700 bytes short of 65520, 140 one-word commands, at windows 10 and 16
    body = matrix[:-1]
    fill = 65520 - 700 - _pos_after(body, 22)
    assert fill > 0, fill
    body = body + realise([(8, 62, 1 + (k * 37) % 400) for k in range(fill // 70)], 22, 3)
    body = body + [(65520 - 700 - _pos_after(body, 22), 4, 9)]
    run = [(0, 4 + (k * 5) % 21, ("word", rnd.randrange(nwords(4 + (k * 5) % 21)), (0, 3, 9, 12, 44, 49, 68)[k % 7])) for k in range(140)]
    bcmds = body[:-1] + realise([body[-1]] + run + [(2, 0, 0)], 22, 4)
    for wbits in (10, 16):
        add("B-matrix-w%d" % wbits, bcmds, wbits)
    # C: text-like
    text = realise(text_commands(random.Random(3), 6000) + [(4, 0, 0)], 22, 5)
    add("C-text", text, 22, kinds=("cf", "ctx", "cf4"))
    # C2: twice as long, so that the stream is of the size that gets a gang of blocks; CF, the gangs' kind
    add("C2-text-long", realise(text_commands(random.Random(9), 12000) + [(4, 0, 0)], 22, 12), 22, kinds=("cf",), parts=2)
    # D: dependent words
    add("D-chains", realise(chain_commands(random.Random(4)), 22, 6), 22)
    # E: ring codes that name a word
    for label, cmds, valid in ring_word_streams():
        add(label, realise(cmds, 22, 7), 22, valid=valid)
    # E2: the same deep inside a stream, where the engines are at work: a copy at the maximum distance, then a ring code that adds
    # 1 .. 3 to it -- a word, named by the ring -- and the implicit distance behind it (the copy's: the word pushed nothing); at
    # window 16, before the window is full (the copy is two bytes long and code 9 lands on P + 1) and after (codes 5 .. 15)
    rnd = random.Random(10)
    deep = text_commands(random.Random(11), 400, max_dist=30000)
    for k in range(60):
        full = k >= 12
        if k == 12:
            deep += text_commands(random.Random(12), 2300, max_dist=30000)[2:]   # (P passes 65520 in here)
        length = 4 + (k * 5) % 21
        far = lambda pos, ring, md: md
        if full:
            code = (5, 7, 9, 11, 13, 15)[k % 6]
            first = [(3, 2 + k % 9, far)] if code < 10 else [(3, 2 + k % 9, far), (1, 3, 40 + k)]   # (codes 10 .. 15: the second last distance)
            deep += first + [(k % 4, length, ("ring", code)), (2, 5, ("implicit",))]
        else:
            deep += [(3, 2, far), (0, length, ("ring", 9)), (2, 5, ("implicit",))]
        deep += text_commands(random.Random(100 + k), 12, max_dist=3000)[2:]
    deep = realise(deep + [(3, 0, 0)], 16, 13)
    add("E2-ring-words-deep", deep, 16)
    # F: one fault each, behind 3000 valid commands of C's make-up
    base = realise(text_commands(random.Random(5), 3000), 22, 8)
    faults = [("t121", [(2, 4, lambda pos, ring, md: ("raw", md + 1 + (121 << 10)))]),
              ("tmax", [(2, 24, ("raw", (1 << 26) - 4))]),
              ("len3", [(2, 3, lambda pos, ring, md: ("raw", md + 1))]),
              ("len25", [(2, 25, lambda pos, ring, md: ("raw", md + 1))]),
              ("ring-zero", [(2, 5, 1), (1, 6, ("ring", 4))]),
              ("ring-minus2", [(2, 5, 1), (1, 6, ("ring", 8))])]
    for label, extra in faults:
        add("F-" + label, base + realise_after(base, extra, 22), 22, valid=False)
    add("F-boundary", base + realise_after(base, [(2, 4, lambda pos, ring, md: md + 1), (2, 4, lambda pos, ring, md: md), (3, 0, 0)], 22), 22)
    over = base + realise_after(base, [(2, 9, ("word", 5, 0))], 22)
    add("F-mlen-plus1", over, 22, valid=False, mlen=_pos_after(over, 22) - 1)
    base16 = realise(text_commands(random.Random(6), 3000, max_dist=30000), 16, 9)
    p = _pos_after(base16, 16)
    end = (p + 4096 + 65535) // 65536 * 65536
    base16 = base16 + realise_after(base16, [(8, 62, 1 + (k * 37) % 400) for k in range((end - p - 200) // 70)], 16)
    over = base16 + realise_after(base16, [(end + 1 - 9 - _pos_after(base16, 16), 9, ("word", 5, 0))], 16)
    assert _pos_after(over, 16) == end + 1
    add("F-mlen-plus1-ring-end", over, 16, valid=False, mlen=end)
    # G: streams that end in a word of total 1, of total 2, and in a three-byte-UTF-8 uppercase-all word with prefix and suffix
    gbase = realise(text_commands(random.Random(7), 3000), 22, 10)
    three = [(l, i) for l, i in multibyte_words() if any(c >= 0xE0 for c in E.dictionary_word(l, i))][0]
    both = [t for t in uppercase_transforms() if E.tables()["transforms"][t][1] == 11 and E.tables()["transforms"][t][0] and E.tables()["transforms"][t][2]][0]
    for label, last in (("total1", (2, 4, ("word", 7, 23))), ("total2", (2, 4, ("word", 7, 27))), ("utf8-upper", (2, three[0], ("word", three[1], both)))):
        cmds = gbase + realise_after(gbase, [last], 22)
        add("G-" + label, cmds, 22)
    # H: small ones
    add("H-small", realise(small_commands(random.Random(8)), 22, 11), 22)
    return out


def realise_after(base, extra, wbits):
    """`extra` realised as the continuation of the realised list `base`"""
    return emit(base + extra, "cf", wbits, literals=Literals(len(base)), unchecked=True, mlen=1 << 20)[3][len(base):]


def h_commands():
    """H's command list, for re-emission with a custom dictionary (the word numbers move by the dictionary's size)"""
    return realise(small_commands(random.Random(8)), 22, 11)


def entries():
    """(manifest entry, stream) of every vector, checked with the oracle and libbrotlidec"""
    import libbrotli_ref as ref
    import oracle_lib as oracle
    for label, wbits, comp, raw, log, valid in vectors():
        info, got = oracle.decode(comp, len(raw) + 64, 0)
        e = {"label": label, "window": wbits, "valid": valid, "csize": len(comp), "size": len(raw), "sha256": hashlib.sha256(raw).hexdigest()}
        if valid:
            assert info.result == 1 and got == raw and info.consumed == len(comp), (label, info.result, info.error_code, info.decoded_size, len(raw))
            assert info.num_commands == len(log), (label, info.num_commands, len(log))
            if ref.available():
                r = ref.decode(comp, len(raw) + 64, False)
                assert r[0] == 1 and r[2] == raw, (label, r[0], r[1])
            e.update({"metablocks": info.num_metablocks, "commands": info.num_commands})
        else:
            assert info.result == 0 and got[:len(raw)] == raw[:len(got)], (label, info.result, info.error_code)
            e.update({"oracle": [info.result, info.error_code, info.decoded_size]})
        yield e, comp
        print({k: v for k, v in e.items() if k != "hex"})   # (placed by now)


def main():
    vector_store.write(OUT, entries())


if __name__ == "__main__":
    main()
