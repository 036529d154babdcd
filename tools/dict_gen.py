"""Seeded generators of streams made for a custom (LZ77 prefix) dictionary, over the repository's own emitter (brotli_emit.py):
word-salad text, data that a dictionary helps with, a context-modelled plan, and the emit of command lists or of data matched
greedily against a dictionary.  Used by tools/dict_batch.py and, through tests/dict_streams.py, by the tests."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brotli_emit as E  # noqa: E402


def text(rnd, n, alphabet="etaoinshrdlucmfw", nwords=200):
    """word salad: n bytes of words drawn from a seeded vocabulary"""
    words = ["".join(rnd.choice(alphabet) for _ in range(rnd.randrange(2, 9))) for _ in range(nwords)]
    s, have = [], 0
    while have < n:
        s.append(rnd.choice(words)); have += len(s[-1]) + 1
    return (" ".join(s)).encode("latin1")[:n]


def related(rnd, dictionary, n, fresh=0.3):
    """n bytes that a dictionary helps with: pieces of it, in any order, between runs of fresh text"""
    out = bytearray()
    while len(out) < n:
        if dictionary and rnd.random() >= fresh:
            ln = rnd.randrange(4, 80)
            at = rnd.randrange(0, max(1, len(dictionary) - ln))
            out += dictionary[at:at + ln]
        else:
            out += text(rnd, rnd.randrange(3, 40), "abcdefghijklmnopqrstuvwxyz ,.", 30)
    return bytes(out[:n])


def context_plan(rnd, cmds, ntypes=4):
    """a context-modelled plan: literal block types in modes 0 .. 3 with a chosen map over five trees, two distance types"""
    nl = sum(len(i) for i, _, _ in cmds)
    blocks, total = [], 0
    while total < nl or len(blocks) < ntypes:
        blocks.append((len(blocks) % ntypes, rnd.randrange(20, 200))); total += blocks[-1][1]
    return E.Plan(lit_blocks=blocks, modes=[(t + 2) % 4 for t in range(ntypes)],   # (the first block: UTF8, both context bytes count)
                  lit_map=[(t * 3 + (c >> 2) + (c & 1)) % 5 for t in range(ntypes) for c in range(64)])


def emit(cmds, wbits, dictionary, plan=None, tail=None):
    """one stream of one compressed metablock (and, with `tail`, further ones: [(cmds, plan)]) -> (compressed, data)"""
    w = E.BitWriter(); E.write_stream_header(w, wbits)
    parts = [(cmds, plan)] + list(tail or [])
    data = b""
    for k, (c, p) in enumerate(parts):
        data += E.emit_compressed(w, c, p or E.Plan(), k + 1 == len(parts), prev=data, dictionary=dictionary)
    return w.finish(), data


def stream_for(data, wbits, dictionary, plan=None, rnd=None, chunk=None):
    """`data` compressed against `dictionary` by the emitter's greedy matcher (distances within the window, copies into
    the dictionary where it has the bytes); chunk: bytes per metablock (None: one).  plan: None (context-free), "context"
    (context_plan per metablock) or a Plan -> compressed bytes"""
    maxb = (1 << wbits) - 16
    hist = bytes(dictionary)[-maxb:] if dictionary else b""
    pieces = [data] if not chunk else [data[i:i + chunk] for i in range(0, len(data), chunk)]
    parts, done = [], b""
    for piece in pieces:
        cmds = E.greedy_commands(piece, max_dist=maxb, history=(hist + done)[-maxb:])
        parts.append((cmds, context_plan(rnd, cmds) if plan == "context" else plan))
        done += piece
    comp, out = emit(parts[0][0], wbits, dictionary, parts[0][1], parts[1:])
    assert out == data
    return comp
