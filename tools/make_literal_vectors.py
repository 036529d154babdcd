#!/usr/bin/env python3
"""tests/golden/emitter_literals/: streams written by tools/brotli_emit.py that put every shape of a literal prefix code, every
run length at which a literal loop changes its way, and every source of the two bytes in front of a literal through the decoder.
The vectors of tests/golden/emitter_words/, emitter_copies/ and emitter_headers/ do that for the words, the copies and the headers.

  S  code shapes x run lengths, no context modelling: the simple codes of 1 .. 4 symbols (both tree selects), a flat 8-bit code,
     the staircase 1, 2, .., 14, 15, 15, codes whose deepest words have 9, 10, 11 and 12 bits, a code on the grid 6 / 9 / 12 / 15;
     data in three regimes (shallowest symbols only, deepest only, a mix); one command per insert length 0 .. 140 with a copy of
     2 .. 4 bytes from 1 .. 5 back between them, and the long runs; every shape with the sweep in front of the long runs
     ("front") and at the very end of the stream ("end")
  E  where a run ends, under the staircase and the flat code: a literal block that ends after each of the first 66 literals of a
     run of 130 (and round literal 768 and 6000 of longer ones), a last command of literals only, a window of 10 bits whose ring
     flushes inside a run, a run over a metablock boundary, and the vectors whose output limits test_gpu_literals.py sweeps
  X  contexts: 64 trees a block type under the identity map, tree i one fixed profile of depths 6 .. 15 rotated by 5 i symbols;
     probes -- literals whose code word, read with the tree of any wrong context, gives another symbol or length -- in LUT cells
     (every p1 and p2 under every mode), source cells (what lies in front of the probe), word cells (words of zero and one byte)
     and maps of 1, 2, 63 and 64 distinct trees with switches between trivial and non-trivial types

The constants of the kernels that the lengths come from (tests/test_emitter_literals_cpu.py reads them out of the sources and
fails with "regenerate" if one has moved):
  SPEC_ROUND_MIN = 768   csrc/brotli_kernels.hip `constexpr uint32_t SPEC_ROUND_MIN`: literals a run must have for a helper round
  SP_MIN_MLEN = 4096     csrc/brotli_kernels.hip `constexpr uint32_t SP_MIN_MLEN`: smaller metablocks do not wake the helper waves
  ROOT_BITS = 8          csrc/brotli_kernels.hip `constexpr int ROOT_BITS`: longer code words go through a second-level table
  PE_RUN_MIN = 6000      csrc/brotli_path_engine.h `BROTLI_AMD_PE_RUN_MIN`: literal runs from here on get regions of their own
  PE_RUN_SB = 256        csrc/brotli_path_engine.h `BROTLI_AMD_PE_RUN_SB`: stream bits of such a region a lane decodes
  REC_INS_RUN = 16, REC_INS_LONG = 63   csrc/brotli_kernels.hip lean_rec_commands: `ins > 16u` leaves the run, `ins > 63u` sets long_cmd
  LIT_FLUSH = 64         csrc/brotli_kernels.hip `if (lit_n == 64)`: the context loops flush their literals
  SPEC_WINDOWS = 64      csrc/brotli_kernels.hip `constexpr uint32_t SPEC_WINDOWS`: windows of 64 bits in a helper wave's chunk

`vectors()` is deterministic; `main()` asks the oracle (and libbrotlidec where there is one) about every stream before it writes.
The files and the manifest are those of tools/make_header_vectors.py; an entry's "runs" is [position, length, ...] of its literal
runs of 16 literals or more, "probes" [position, cell number, ...] with "cells" the cells' names."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import brotli_emit as E  # noqa: E402
import vector_store  # noqa: E402
from vector_store import MAX_FILE, MAX_PARTS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "emitter_literals")
SPEC_ROUND_MIN, SP_MIN_MLEN, ROOT_BITS, PE_RUN_MIN, PE_RUN_SB, REC_INS_RUN, REC_INS_LONG, LIT_FLUSH, SPEC_WINDOWS = 768, 4096, 8, 6000, 256, 16, 63, 64, 64
SWEEP = list(range(0, 141))
LONG_RUNS = [SPEC_ROUND_MIN - 1, SPEC_ROUND_MIN, SPEC_ROUND_MIN + 1, PE_RUN_MIN - 1, PE_RUN_MIN, PE_RUN_MIN + 1, 2 * PE_RUN_MIN + 1]
HUGE_RUN = 40000
FRONT_BYTES, SAFE_DWORDS, FRONT_PAD = 512, 72, 400   # (csrc/brotli_kernels.hip `safe_dw = br.end_dw > 72u ? br.end_dw - 72u : 0u`)
BLOCK_ENDS = list(range(1, 67))
LAST_RUNS = [1, 2, 3, 8, 63, 64, 65, 130]
COPY_CELLS = [2, 3, 63, 64, 65, 79, 80, 81, 1023, 1024, 1025, 1041]
OVERLAP_CELLS = [1, 2, 3, 65]
WRAP_CELLS = [63, 64, 65, 127, 128]


# ------------------------------------------------------------------ code shapes
def _spread(i):
    """the i-th symbol of a code under test: byte values all over the alphabet"""
    return (i * 37 + 11) % 256


def shape_lengths(name):
    """-> the 256 code lengths of a complex shape"""
    if name == "flat8":
        return [8] * 256
    if name == "stair":
        per = list(range(1, 16)) + [15]
    elif name.startswith("deep"):
        d = int(name[4:])   # 1 .. 7, one word of 8, and 2^(d - 8) words of d bits: d - ROOT_BITS bits behind the root table
        per = list(range(1, 8)) + [8] + [d] * (1 << (d - 8))
    else:
        assert name == "grid"   # 56 / 64 + 56 / 512 + 56 / 4096 + 64 / 32768 = 1: every code word a multiple of three behind six, so that
        per = [6] * 56 + [9] * 56 + [12] * 56 + [15] * 64   # two chains of code words that start apart never meet
    lengths = [0] * 256
    for i, l in enumerate(per):
        lengths[_spread(i)] = l
    assert sum(32768 >> l for l in lengths if l) == 32768
    return lengths


SIMPLE = {"simple1": ([0x61], None), "simple2": ([0x20, 0xE3], None), "simple3": ([0x65, 0x0A, 0xC3], None), "simple4a": ([0x00, 0x41, 0x7F, 0xFF], 0),
          "simple4b": ([0x74, 0x80, 0x09, 0xBF], 1)}
COMPLEX = ["flat8", "stair", "deep9", "deep10", "deep11", "deep12", "grid"]
SHAPES = list(SIMPLE) + COMPLEX
DEEPEST3 = ["stair", "deep12", "grid"]


def shape_code(name, rotate=0):
    """-> a function of (histogram, alphabet) for Plan.codes; `rotate`: the same lengths over the same symbols, moved on by `rotate` symbols"""
    if name in SIMPLE:
        syms, ts = SIMPLE[name]
        syms = syms[rotate % len(syms):] + syms[:rotate % len(syms)]
        return lambda h, a: E.WireCode(256, simple=syms, tree_select=ts)
    lengths = shape_lengths(name)
    if rotate:
        used = [s for s in range(256) if lengths[s]]
        moved = [0] * 256
        for i, s in enumerate(used):
            moved[used[(i + rotate) % len(used)]] = lengths[s]
        lengths = moved
    return lambda h, a: E.WireCode(256, lengths=lengths)


def depth_of(name):
    return max(shape_code(name)(None, 256).full)


class Data:
    """the seeded generator of a shape's literals: stretches of 1 .. 300 literals in one regime after the other -- the shallowest
    symbols only, the deepest only, a mix (a length at random, then a symbol of that length)"""

    def __init__(self, code, seed, stretches=(1, 2, 5, 17, 64, 65, 130, 300), first=0):
        """`first`: the regime of the first stretch (0 shallowest, 1 deepest, 2 mix)"""
        self.rnd = random.Random(seed)
        self.stretches = stretches
        full = code.full
        self.by_len = {}
        for s, l in enumerate(full):
            if l or code.simple and s in code.syms:
                self.by_len.setdefault(l, []).append(s)
        self.lens = sorted(self.by_len)
        self.regime, self.left = (first + 2) % 3, 0

    def __call__(self):
        if self.left == 0:
            self.regime = (self.regime + 1) % 3
            self.left = self.rnd.choice(self.stretches)
        self.left -= 1
        l = (self.lens[0], self.lens[-1], self.rnd.choice(self.lens))[self.regime]
        return self.rnd.choice(self.by_len[l])

    def take(self, n):
        return bytes(self() for _ in range(n))


# ------------------------------------------------------------------ a stream under construction
def alternatives(out, pos, mode, p1, p2, behind):
    """the wrong contexts of the literal at `pos` -> {name: context id}.  `out` = the stream's output in front of it, (p1, p2) the two
    bytes the decoder has in front of it, `behind` = None or (position, bytes put out, distance or None) of the copy or word whose
    last byte lies at most one literal in front.
      a   p1 and p2 swapped
      b   both zero
      c   the two bytes in front of that copy or word (stale registers; behind one literal: p1 and the stale p1)
      d   the bytes at P - 2 and P - 3
      e   behind a copy that overlaps itself (distance < length): the last two bytes of its source as they were before the copy
          wrote anything -- what a copy that read its whole source first would leave; a byte it had not written yet reads as zero
      f0 .. f3   the same bytes under each of the other three modes"""
    g = lambda x: out[x] if x >= 0 else 0
    ctx = E.literal_context
    alts = {"a": ctx(mode, p2, p1), "b": ctx(mode, 0, 0), "d": ctx(mode, g(pos - 2), g(pos - 3))}
    for m in range(4):
        if m != mode:
            alts["f%d" % m] = ctx(m, p1, p2)
    if behind is not None:
        cp, n, dist = behind
        k = pos - (cp + n)
        s1, s2 = g(cp - 1), g(cp - 2)
        if k in (0, 1) and n > 0:
            alts["c"] = ctx(mode, s1, s2) if k == 0 else ctx(mode, p1, s1)
            if dist is not None and dist < n:
                src = lambda x: g(x) if x < cp else 0
                e1, e2 = src(cp - dist + n - 1), src(cp - dist + n - 2)
                alts["e"] = ctx(mode, e1, e2) if k == 0 else ctx(mode, p1, e1)
    return alts


_codes_of = {}


def tree_codes(lengths):
    key = tuple(lengths)
    if key not in _codes_of:
        _codes_of[key] = E.canonical_codes(lengths)
    return _codes_of[key]


def discriminates(trees, right, wrong, byte):
    """the code word of `byte` in tree `right`, read with each tree of `wrong`, gives another symbol or another length: a prefix
    code reads (word, n) as `byte` exactly when `byte` has that very word in it"""
    word = tree_codes(trees[right])[byte]
    return all(tree_codes(trees[t]).get(byte) != word for t in wrong if t != right)


# cells whose two bytes in front are the cell itself, and the cells of X-maps, where a block type of two trees makes every second
# alternative no real one: their alternatives are counted over all of the cell's probes
AGGREGATE = ("lut", "tree", "start", "type0", "type1", "type2", "full-last", "to-full")
TRIVIAL = ("trivial-last", "to-trivial", "type3")   # cells in a block type of one tree: no context is a wrong one


def required(cell, mode):
    """the alternatives that must be real ones -- name another tree than the right one -- at every single probe of a cell (the generator
    builds a cell again until they are): (a), (b), (d) and (f) under each other mode everywhere; (c) behind a copy or a word; (e) behind a
    copy that overlaps itself.  What a cell's place in the stream rules out:
      - behind a word of no byte nothing is stale: no (c);
      - the second literal behind a copy or word differs from its (c) and (e) in p2 alone, which LSB6 and MSB6 do not look at;
      - behind a copy at distance 1 the two bytes in front are the same byte, and so are those at P - 2 and P - 3: no (a), no (d); at the
        literal behind that, the stale p1 is that byte again: no (c);
      - AGGREGATE and TRIVIAL cells: see there."""
    second = cell.endswith("+1")
    base = cell[:-2] if cell[-2:] in ("+0", "+1") else cell
    if base in AGGREGATE or base in TRIVIAL:
        return set()
    need = {"a", "b", "d"} | {"f%d" % m for m in range(4) if m != mode}
    behind = base.startswith(("copy-", "overlap-")) or base == "word" or "/" in base or base in ("after-copy-end", "after-word-end")
    blind = second and mode < 2
    if behind and not blind and "/w0/" not in base:
        need.add("c")
    if base.startswith("overlap-") and not blind:
        need.add("e")
    if base == "overlap-1":
        need -= {"c"} if second else {"a", "d"}
    return need


class Scheme:
    """the literal side of a metablock: modes per block type, the context map, the trees' lengths"""

    def __init__(self, modes, lit_map, trees, repeats=False):
        self.modes, self.lit_map, self.trees, self.repeats = modes, lit_map, trees, repeats

    def plan(self, lit_blocks):
        codes = {("lit", i): (lambda h, a, l=l: E.WireCode(256, lengths=l, repeats=self.repeats)) for i, l in enumerate(self.trees)}
        return E.Plan(lit_blocks=lit_blocks, modes=list(self.modes), lit_map=list(self.lit_map), codes=codes)


class Build:
    """a stream command by command: the output is kept here as well (the emitter's must agree), so that a probe can be chosen from
    everything in front of it"""

    def __init__(self, wbits=22, dictionary=b""):
        self.w, self.out, self.llog, self.clog, self.ring = E.BitWriter(), bytearray(), [], [], list(E.RING_INIT)
        self.wbits, self.dictionary, self.probes, self.cells, self.runs, self.mbs = wbits, dictionary, [], [], [], []
        self.rnd, self.unmet = None, []
        E.write_stream_header(self.w, wbits)

    # -- a metablock
    def begin(self, scheme=None, plan=None):
        self.scheme, self.plan = scheme, plan
        self.cmds, self.ins, self.blocks, self.behind, self.mb_at = [], bytearray(), [[0, 0]], None, len(self.out)

    def switch(self, t):
        """the literals from here on belong to block type t (the first block of a metablock is of type 0)"""
        if self.blocks[-1][1] == 0:
            assert len(self.blocks) > 1 or t == 0
            self.blocks[-1][0] = t
        elif self.blocks[-1][0] != t:
            self.blocks.append([t, 0])
        else:   # (a switch to the same type is one the format cannot say with two types; with more it could: not used)
            raise AssertionError("switch to the type in use")

    def _close(self, clen, what):
        n = len(self.ins)
        if n >= REC_INS_RUN:
            self.runs += [len(self.out) - n, n]
        self.cmds.append((bytes(self.ins), clen, what))
        self.ins = bytearray()

    def lit(self, data):
        for b in bytes(data):
            self.out.append(b); self.ins.append(b); self.blocks[-1][1] += 1

    def copy(self, n, dist):
        assert 1 <= dist <= len(self.out) + len(self.dictionary) and n >= 2, (n, dist, len(self.out))
        self._close(n, dist)
        cp = len(self.out)
        for _ in range(n):   # (a distance beyond the stream's first byte reaches into the custom dictionary, counted from its end)
            self.out.append(self.out[-dist] if dist <= len(self.out) else self.dictionary[len(self.out) - dist])
        self.behind = (cp, n, dist)

    def word(self, length, idx, transform):
        self._close(length, ("word", idx, transform))
        cp = len(self.out)
        made = E.transform_word(E.dictionary_word(length, idx), transform)
        self.out += made
        self.behind = (cp, len(made), None)

    def end(self, last=False):
        """closes the metablock; literals that no copy follows become its last command"""
        if self.ins or not self.cmds:
            self._close(0, 0)
        blocks = [tuple(b) for b in self.blocks if b[1]]
        if self.scheme is not None:
            plan = self.scheme.plan(blocks)
        else:
            plan = self.plan
            plan.lit_blocks = blocks if len(blocks) > 1 else None
        llog, clog = [], []
        raw = E.emit_compressed(self.w, self.cmds, plan, last, prev=bytes(self.out[:self.mb_at]), dictionary=self.dictionary, wbits=self.wbits, log=clog,
                                ring_io=self.ring, llog=llog)
        assert raw == bytes(self.out[self.mb_at:]), "the builder's output is not the emitter's"
        for r in llog:
            r["mb"] = len(self.mbs)
        for r in clog:
            r["mb"] = len(self.mbs)
        self.llog += llog; self.clog += clog
        self.mbs.append({"at": self.mb_at, "kind": "compressed", "scheme": self.scheme})
        return self

    def stored(self, raw):
        E.emit_stored(self.w, raw); self.mbs.append({"at": len(self.out), "kind": "stored"}); self.out += raw

    def metadata(self, payload):
        E.emit_metadata(self.w, payload); self.mbs.append({"at": len(self.out), "kind": "metadata" if payload else "empty"})

    # -- probes
    def context_now(self):
        """-> (type, mode, p1, p2) of the next literal"""
        t = self.blocks[-1][0]
        at = len(self.out)
        p1 = self.out[at - 1] if at >= 1 else 0   # (zeros in front of the stream's first byte, with a custom dictionary as well)
        p2 = self.out[at - 2] if at >= 2 else 0
        return t, self.scheme.modes[t], p1, p2

    def probe(self, cell):
        """a literal chosen so that every wrong context named by `alternatives` whose tree is another than the right one reads another
        symbol or length; the alternatives that `required` names for the cell and are no real ones here are noted for `cell()`"""
        sc = self.scheme
        t, mode, p1, p2 = self.context_now()
        pos = len(self.out)
        alts = alternatives(self.out, pos, mode, p1, p2, self.behind)
        right = sc.lit_map[t * 64 + E.literal_context(mode, p1, p2)]
        wrong = {sc.lit_map[t * 64 + c] for c in alts.values()} - {right}
        self.unmet += [(cell, a) for a in required(cell, mode) if a not in alts or sc.lit_map[t * 64 + alts[a]] == right]
        for _ in range(4096):
            b = self.rnd.randrange(256)
            if sc.trees[right][b] and discriminates(sc.trees, right, wrong, b):
                break
        else:
            raise AssertionError(("no byte discriminates", cell, pos))
        if cell not in self.cells:
            self.cells.append(cell)
        self.probes += [pos, self.cells.index(cell)]
        self.lit([b])
        return b

    def cell(self, build, tries=20000):
        """builds a cell -- `build()`: commands inside one metablock -- again and again, with the next seeded bytes, until every probe in it
        has every alternative `required` names as a real one"""
        for _ in range(tries):
            mark = (len(self.out), bytes(self.ins), len(self.cmds), [list(x) for x in self.blocks], len(self.probes), len(self.cells), len(self.runs), self.behind)
            self.unmet = []
            build()
            if not self.unmet:
                return
            del self.out[mark[0]:]; self.ins = bytearray(mark[1]); del self.cmds[mark[2]:]; self.blocks = [list(x) for x in mark[3]]
            del self.probes[mark[4]:]; del self.cells[mark[5]:]; del self.runs[mark[6]:]; self.behind = mark[7]
        raise AssertionError(("a cell whose alternatives cannot all be real", self.unmet))

    def rlit(self, n):
        """n seeded literals that the trees their contexts select can write"""
        for _ in range(n):
            t, mode, p1, p2 = self.context_now()
            tree = self.scheme.trees[self.scheme.lit_map[t * 64 + E.literal_context(mode, p1, p2)]]
            while True:
                b = self.rnd.randrange(256)
                if tree[b]:
                    break
            self.lit([b])


# ------------------------------------------------------------------ S
def s_vector(name, place, seed):
    """one shape, the sweep in `place`: "front" (lead, sweep, long runs) or "end" (a first command of PE_RUN_MIN literals, a run of
    SPEC_ROUND_MIN, the sweep as the stream's last commands); "first": no sweep, a first command of PE_RUN_MIN literals and every
    long run behind it -- a stream of more than 64 KiB whose first command a gang declines"""
    for attempt in range(20):
        b = Build()
        rnd = random.Random(seed * 100 + attempt)
        code = shape_code(name)
        data = Data(code(None, 256), seed * 100 + attempt)
        b.begin(plan=E.Plan(codes={("lit", 0): code}))

        def run(n):
            b.lit(data.take(n))
            b.copy(rnd.randrange(2, 5), rnd.randrange(1, 6) if len(b.out) >= 5 else 1)
        if place == "front":
            run(7)
            for n in SWEEP:
                run(n)
            for n in LONG_RUNS + ([HUGE_RUN] if name in DEEPEST3 else []):
                run(n)
            if name == "simple1":   # (its literals take no bits: commands without literals, their lengths and distances spread so
                for _ in range(FRONT_PAD):   # that they take some, until the sweep lies as far in front of the end as any other shape's)
                    b.copy(rnd.randrange(2, 200), rnd.randrange(1, 3000))
        elif place == "end":
            run(PE_RUN_MIN); run(SPEC_ROUND_MIN)
            for n in SWEEP:
                run(n)
        else:
            assert place == "first"   # (not committed: tests/literal_vectors.leg_set builds it)
            for n in [PE_RUN_MIN] + LONG_RUNS + [HUGE_RUN]:
                run(n)
        b.end(last=True)
        if place == "front":   # the sweep's last literal, 512 bytes of stream, and the last 72 dwords, where only the checked loop runs
            sweep_end = max(r["bit"] + r["nbits"] for r in b.llog if r["cmd"] <= 1 + len(SWEEP))
            assert sweep_end + 8 * FRONT_BYTES <= 8 * len(b.w.out) + b.w.n - 32 * SAFE_DWORDS, (name, sweep_end, len(b.w.out))
        if s_phases(b.llog, depth_of(name)) is None:
            return b
    raise AssertionError(("no seed gives every phase", name, place))


def s_phases(llog, depth):
    """what a shape of depth 9 or more must show (None: it does): a code word that ends on a 64-bit boundary of the stream, one that
    straddles one, a second-level word at every bit phase 0 .. 31; the shapes of depth 15 a 15-bit word that ends on bit 63 and four
    15-bit words in one 64-bit window; where the shallowest word has one bit, 64 of them that fill one window"""
    if depth <= ROOT_BITS:
        return None if window_of(llog, 1, 64) else ("no window of one-bit words",)
    ends = any((r["bit"] + r["nbits"]) % 64 == 0 for r in llog)
    straddles = any(r["bit"] // 64 != (r["bit"] + r["nbits"] - 1) // 64 for r in llog if r["nbits"])
    phases = {r["bit"] % 32 for r in llog if r["nbits"] > ROOT_BITS}
    deep_end = depth < 15 or any(r["nbits"] == 15 and (r["bit"] + 15) % 64 == 0 for r in llog)
    full = window_of(llog, 1, 64) and (depth < 15 or window_of(llog, 15, 4))
    if ends and straddles and len(phases) == 32 and deep_end and full:
        return None
    return (ends, straddles, sorted(set(range(32)) - phases), deep_end, full)


def window_of(llog, nbits, count):
    """`count` code words of `nbits` bits in a row that lie in one 64-bit window of the stream: 64 words of one bit fill it, four of 15
    bits are the most it holds (the `i * 15` bound); True as well where the code has no word of one bit"""
    if nbits == 1 and not any(r["nbits"] == 1 for r in llog):
        return True
    run = 0
    for i, r in enumerate(llog):
        run = run + 1 if r["nbits"] == nbits else 0
        if run >= count:
            first = llog[i - count + 1]
            if first["bit"] // 64 == (r["bit"] + nbits - 1) // 64 and r["bit"] + nbits - first["bit"] == count * nbits:
                return True
    return False


def s_vectors(add):
    for i, name in enumerate(SHAPES):
        for j, place in enumerate(("front", "end")):
            add("S-%s-%s" % (name, place), "S", s_vector(name, place, 1000 + 2 * i + j), shape=name, place=place)


# ------------------------------------------------------------------ E
E_CODES = ("stair", "flat8")


def e_plan(name):
    """type 0 has the code under test, type 1 another: the staircase moved on by five symbols; under the flat code (which every
    order of its symbols leaves the same) the staircase"""
    other = shape_code("stair", 5) if name == "stair" else shape_code("stair")
    return E.Plan(codes={("lit", 0): shape_code(name), ("lit", 1): other})


class EData:
    """E's literals: stretches of at most 33 literals, the first one a mix, so that every end of a run -- the runs are short here -- lies
    among code words of several lengths"""

    def __init__(self, name, seed):
        short = (1, 2, 5, 9, 17, 33)
        self.own, self.other = Data(shape_code(name)(None, 256), seed, short, 2), Data(shape_code("stair")(None, 256), seed + 1, short, 2)   # (the staircase's symbols whatever their order)

    def take(self, b, n):
        for _ in range(n):
            b.lit([self.own() if b.blocks[-1][0] == 0 else self.other()])


def e_run(b, d, n, ends):
    """a run of n literals with block ends after the literals `ends` (type 0 -> 1 -> 0 ..)"""
    at = 0
    for k, e in enumerate(list(ends) + [n]):
        d.take(b, e - at); at = e
        if e < n:
            b.switch(1 - b.blocks[-1][0])


def e_vectors(add):
    seed = 2000
    for name in E_CODES:
        def start(wbits=22):
            nonlocal seed
            seed += 1
            b = Build(wbits); b.begin(plan=e_plan(name))
            return b, EData(name, seed), random.Random(seed)

        def filler(b, d, rnd, total):
            """commands of 20 .. 100 literals until the metablock holds `total` bytes"""
            while len(b.out) - b.mb_at < total:
                if b.blocks[-1][0]:
                    b.switch(0)
                d.take(b, rnd.randrange(20, 101)); b.copy(rnd.randrange(2, 5), rnd.randrange(1, 6))
        for j in BLOCK_ENDS:
            b, d, rnd = start()
            d.take(b, 3); b.copy(2, 1)
            e_run(b, d, 130, [j]); b.copy(3, 2)
            b.switch(0); d.take(b, 4)
            add("E-%s-block-130-%02d" % (name, j), "E", b.end(last=True), run=[5, 130], ends=[j])
        for n, pairs in ((800, [(j,) for j in range(SPEC_ROUND_MIN - 2, SPEC_ROUND_MIN + 3)]),
                         (6100, [(SPEC_ROUND_MIN + j, PE_RUN_MIN + j) for j in range(-2, 3)])):
            for ends in pairs:
                b, d, rnd = start()
                d.take(b, 3); b.copy(2, 1)
                e_run(b, d, n, ends); b.copy(3, 2)
                filler(b, d, rnd, SP_MIN_MLEN + 200)
                add("E-%s-block-%d-%s" % (name, n, "-".join(map(str, ends))), "E", b.end(last=True), run=[5, n], ends=list(ends))
        for n in LAST_RUNS:
            b, d, rnd = start()
            d.take(b, 5); b.copy(3, 2)
            d.take(b, n)
            add("E-%s-last-%d" % (name, n), "E", b.end(last=True), run=[8, n])
        for k in range(4):   # a window of 10 bits: a ring of 1024 bytes, which a run of 100 and one of 2000 cross at seeded phases
            b, d, rnd = start(10)
            off = rnd.randrange(1, 100)
            d.take(b, 1024 - 3 - off - 40 * k); b.copy(3, rnd.randrange(1, 6))
            if k:
                d.take(b, 40 * k - 2); b.copy(2, 1)
            at = len(b.out)
            d.take(b, 100); b.copy(rnd.randrange(2, 5), rnd.randrange(1, 1009))
            d.take(b, rnd.randrange(1, 200)); b.copy(4, 1000)
            at2 = len(b.out)
            d.take(b, 2000); b.copy(4, 3)
            d.take(b, 9)
            assert at < 1024 < at + 100 and at == 1024 - off
            add("E-%s-window10-%d" % (name, k), "E", b.end(last=True), run=[at, 100], run2=[at2, 2000])
        for n, m in ((1, 1), (2, 63), (65, 130), (130, 2), (800, 800)):
            b, d, rnd = start()
            d.take(b, 5); b.copy(3, 2)
            if n + m > 1000:
                filler(b, d, rnd, SP_MIN_MLEN)
            at = len(b.out)
            d.take(b, n); b.end()
            b.begin(plan=e_plan(name))
            d.take(b, m); b.copy(3, 2)
            if n + m > 1000:
                filler(b, d, rnd, SP_MIN_MLEN)
            d.take(b, 3)
            add("E-%s-two-%d-%d" % (name, n, m), "E", b.end(last=True), run=[at, n + m])
        for n in (130, SPEC_ROUND_MIN, PE_RUN_MIN):
            b, d, rnd = start()
            d.take(b, 5); b.copy(3, 2)
            d.take(b, n); b.copy(3, 2)
            if n == SPEC_ROUND_MIN:
                filler(b, d, rnd, SP_MIN_MLEN + 100)
            d.take(b, 6)
            add("E-%s-cap-%d" % (name, n), "E", b.end(last=True), run=[8, n])


def cap_sweep(e):
    """the output limits of an E-*-cap-* vector: the run of 130 every limit from P_run - 2 to P_run + 131; the others +-2 round every
    multiple of 64 in the run's first 256 literals and at its last three"""
    at, n = e["run"]
    if n == 130:
        return list(range(at - 2, at + 132))
    caps = [at + m + k for m in range(0, 257, 64) for k in range(-2, 3)] + [at + n - 3, at + n - 2, at + n - 1, at + n]
    return sorted(set(caps))


# ------------------------------------------------------------------ X
def _profile():
    """one complete code of 256 symbols with every depth 6 .. 15: 20 x 6, 20 x 7, 62 x 8, 147 x 9, one each of 10 .. 14, 2 x 15"""
    per = [6] * 20 + [7] * 20 + [8] * 62 + [9] * 147 + [10, 11, 12, 13, 14, 15, 15]
    assert len(per) == 256 and sum(32768 >> l for l in per) == 32768
    return per


PROFILE_SORTED = _profile()
PROFILE = list(PROFILE_SORTED)
random.Random(64).shuffle(PROFILE)


def x_tree(i, profile=PROFILE):
    """tree i: the profile rotated by 5 i symbols (5 and 256 have no common factor: 256 different trees)"""
    return [profile[(s + 5 * i) % 256] for s in range(256)]


def x_scheme(modes, cheap=False):
    """64 trees a block type under the identity map; `cheap`: the sorted profile, whose lengths lie in runs that repeat words
    write in a few bytes -- for vectors of many metablocks"""
    n = len(modes)
    return Scheme(modes, list(range(64 * n)), [x_tree(i, PROFILE_SORTED if cheap else PROFILE) for i in range(64 * n)], repeats=cheap)


def tiny_words():
    """-> {0: [...], 1: [...]}: (length, idx, transform) of words that put out no byte and one byte"""
    got = {0: [], 1: []}
    for t, (prefix, kind, suffix) in enumerate(E.tables()["transforms"]):
        if prefix or suffix:
            continue
        for length in range(4, 11):
            for idx in (0, 1, 2, 3, 5, 8, 13, 21):
                n = len(E.transform_word(E.dictionary_word(length, idx), t))
                if n in got and (n == 0 and len(got[0]) < 12 or n == 1):
                    got[n].append((length, idx, t))
    assert len(got[0]) >= 4 and len({E.transform_word(E.dictionary_word(l, i), t) for l, i, t in got[1]}) >= 8
    return got


def x_start(b, cell="start"):
    """the first two literals of a metablock as probes"""
    b.probe(cell + "+0"); b.probe(cell + "+1")


def x_lut(mode, seed):
    """every p1 with p2 held at two values, every p2 with p1 held at two: triples (p2, p1, probe) in commands of 1 .. 30 triples"""
    b = Build(); b.rnd = rnd = random.Random(seed)
    b.begin(x_scheme([mode]))
    x_start(b)
    held = [rnd.randrange(256) for _ in range(4)]
    triples = [(held[0], v) for v in range(256)] + [(held[1], v) for v in range(256)] + [(v, held[2]) for v in range(256)] + [(v, held[3]) for v in range(256)]
    rnd.shuffle(triples)
    left = 0
    for p2, p1 in triples:
        if left == 0:
            b.copy(rnd.randrange(2, 5), rnd.randrange(1, min(6, len(b.out) + 1)))
            left = rnd.randrange(1, 31)
        b.lit([p2, p1]); b.probe("lut")
        left -= 1
    b.end(last=True)
    b.held = held
    return b


def x_every_tree(seed):
    """4 types x 64 trees, a mode each: every tree of every type behind a block switch and in runs; switches every 1 .. 5 literals at the end"""
    b = Build(); b.rnd = rnd = random.Random(seed)
    sc = x_scheme([0, 1, 2, 3])
    b.begin(sc)
    x_start(b)
    pairs = {}
    for m in range(4):
        for p1 in range(256):
            for p2 in range(0, 256, 5):
                pairs.setdefault((m, E.literal_context(m, p1, p2)), []).append((p1, p2))
    assert len(pairs) == 256
    order = [(t, c) for t in range(4) for c in range(64)]
    rnd.shuffle(order)
    for k, (t, c) in enumerate(order):
        if b.blocks[-1][0] != t:
            b.switch(t)
        p1, p2 = rnd.choice(pairs[(t, c)])
        b.lit([p2, p1]); b.probe("tree")
        if k % 7 == 3:
            b.copy(rnd.randrange(2, 5), rnd.randrange(1, 6))
    for k in range(300):
        def one():
            b.rlit(2)
            b.switch(rnd.choice([x for x in range(4) if x != b.blocks[-1][0]]))
            b.probe("switch"); b.rlit(rnd.randrange(0, 4))
        b.cell(one)
        if k % 11 == 0:
            b.copy(rnd.randrange(2, 5), rnd.randrange(1, 6))
    b.end(last=True)
    return b


def x_source(seed, dictionary=b""):
    """what lies in front of the probe: one literal, a run that wraps lit_n == 64, copies that do not overlap themselves, copies that do,
    a word of two bytes or more, a block switch -- under UTF8 (type 0) and SIGNED (type 1), each cell under both"""
    b = Build(dictionary=dictionary); b.rnd = rnd = random.Random(seed)
    b.begin(x_scheme([2, 3]))
    x_start(b)
    b.rlit(1100); b.copy(2, 1)

    def both(cell):
        """the probe and the literal behind it"""
        b.probe(cell); b.probe(cell + "+1")

    def switch(t):
        b.rlit(3); b.switch(t); b.probe("switch")

    def literal():
        b.rlit(2); b.copy(3, rnd.randrange(1, 6)); b.rlit(1); b.probe("literal")

    def wrap():   # (the probes are literals 63, 64, 65, 127 and 128 of a run, counted from one and from nought)
        for k in range(129):
            if k + 1 in WRAP_CELLS or k in WRAP_CELLS:
                b.probe("wrap-%d" % k)
            else:
                b.rlit(1)

    def copy(n):
        b.rlit(2)
        if n <= len(dictionary) and n < 63:   # (with a custom dictionary the short copies lie in it: the kernels' from_cdict)
            b.copy(n, len(b.out) + rnd.randrange(n, len(dictionary) + 1))
        else:
            b.copy(n, rnd.randrange(n, min(len(b.out), n + 40) + 1))
        both("copy-%d" % n)

    def overlap(d, n):
        b.copy(2, rnd.randrange(6, 90))
        b.rlit(d + 3); b.copy(n, d); both("overlap-%d" % d)   # (the copy's whole source is drawn with the cell)

    def word(length, transform):
        b.rlit(rnd.randrange(0, 3))
        b.word(length, rnd.randrange(1 << E.tables()["size_bits"][length]), transform)
        assert b.behind[1] >= 2
        both("word")
    for t in (1, 0, 1, 0):
        b.cell(lambda: switch(t))
        b.cell(literal)
        b.copy(2, 2)
        b.cell(wrap)
        for n in COPY_CELLS:
            b.cell(lambda: copy(n))
        for d in OVERLAP_CELLS:
            for n in (d + 1, d + 7, 199):   # (no multiple of the distance: behind one the stale bytes are the right ones again)
                b.cell(lambda: overlap(d, n))
        for length in (4, 7, 13, 24):
            for transform in (0, 3, 49, 9):
                b.cell(lambda: word(length, transform))
    b.end(last=True)
    return b


def _front_ok(out, mode, cell, behind=None):
    """would a probe of `cell` behind `out`, under `mode` and the identity map, have every required alternative as a real one?"""
    pos = len(out)
    p1, p2 = (out[pos - 1] if pos >= 1 else 0), (out[pos - 2] if pos >= 2 else 0)
    alts = alternatives(out, pos, mode, p1, p2, behind)
    right = E.literal_context(mode, p1, p2)
    return all(a in alts and alts[a] != right for a in required(cell, mode))


def x_boundary(seed):
    """a probe as the first literal of a metablock behind a compressed, a stored, a metadata and an empty metablock, and behind
    metablocks that end in a copy and in a word; the bytes in front of the boundary are chosen like those of any cell"""
    b = Build(); b.rnd = rnd = random.Random(seed)
    modes = {"compressed": 2, "stored": 3, "metadata": 0, "empty": 1, "copy-end": 3, "word-end": 2}

    def two(cell):
        b.probe(cell + "+0"); b.probe(cell + "+1")

    def closing(kind):
        """the end of a compressed metablock in front of the boundary of `kind`"""
        def tail():
            b.rlit(9)
            if not _front_ok(b.out, modes[kind], "after-%s+0" % kind):
                b.unmet.append(kind)
        b.cell(tail)
        b.end()
    b.begin(x_scheme([2], cheap=True)); x_start(b); b.rlit(40); b.copy(3, 7)
    for kind in ("compressed", "stored", "metadata", "empty"):
        closing(kind)
        if kind == "stored":
            while True:
                raw = bytes(rnd.randrange(256) for _ in range(37))
                if _front_ok(b.out + raw, modes[kind], "after-stored+0"):
                    break
            b.stored(raw)
        elif kind == "metadata":
            b.metadata(b"between two metablocks")
        elif kind == "empty":
            b.metadata(b"")
        b.begin(x_scheme([modes[kind]], cheap=True))
        b.cell(lambda: two("after-" + kind))
        b.rlit(30); b.copy(4, 9)
    # a metablock that ends in a copy, and one that ends in a word: what lay in front of them is stale in the next one as well
    def copy_end():
        b.rlit(20); b.copy(5, rnd.randrange(5, 60))
        if not _front_ok(b.out, modes["copy-end"], "after-copy-end+0", b.behind):
            b.unmet.append("copy-end")
    b.cell(copy_end); keep = b.behind; b.end()
    b.begin(x_scheme([modes["copy-end"]], cheap=True)); b.behind = keep
    b.cell(lambda: two("after-copy-end"))

    def word_end():
        b.rlit(5); b.word(6, rnd.randrange(1 << E.tables()["size_bits"][6]), 0)
        if not _front_ok(b.out, modes["word-end"], "after-word-end+0", b.behind):
            b.unmet.append("word-end")
    b.cell(word_end); keep = b.behind; b.end()
    b.begin(x_scheme([modes["word-end"]], cheap=True)); b.behind = keep
    b.cell(lambda: two("after-word-end"))
    b.rlit(3); b.copy(4, 9); b.rlit(5)
    b.end(last=True)
    return b


PREDECESSORS = ("literal", "copy5", "copy300", "word", "start")
FOLLOWERS = ("w0", "w1", "w1w1", "w1-copy2")


def x_words(seed, dictionary=b"", preds=PREDECESSORS[:4], cheap=False):
    """predecessor x follower x (the word's command carries literals / carries none).  The predecessor is what lies in front of the
    word's command: literals (the command in front is then one whose word put out nothing, so that the last bytes are literals), a
    copy of 5, a copy of 300, a word of two bytes or more, the metablock's start.  The followers: a word of no byte, of one byte,
    two of one byte, and a word of one byte, a copy of 2 without literals and then the probe."""
    b = Build(dictionary=dictionary); b.rnd = rnd = random.Random(seed)
    tiny = tiny_words()
    mode = 2
    b.begin(x_scheme([mode], cheap)); x_start(b); b.rlit(400); b.copy(2, 1)
    nine = 1 << E.tables()["size_bits"][9]

    def build(pred, fol, lits, cell):
        if pred == "literal":
            b.rlit(3); b.word(*tiny[0][rnd.randrange(len(tiny[0]))])
        elif pred == "copy5":   # (with a custom dictionary of five bytes or more: out of it)
            b.rlit(1); b.copy(5, rnd.randrange(5, 200) if len(dictionary) < 5 else len(b.out) + rnd.randrange(5, min(len(dictionary), 200) + 1))
        elif pred == "copy300":
            b.rlit(1); b.copy(300, rnd.randrange(300, 400))
        elif pred == "word":
            b.rlit(1); b.word(9, rnd.randrange(nine), 0)
        if lits:
            b.rlit(rnd.choice([1, 2, 3, 17]))
        one = lambda: tiny[1][rnd.randrange(len(tiny[1]))]
        if fol == "w0":
            b.word(*tiny[0][rnd.randrange(len(tiny[0]))])
        elif fol == "w1":
            b.word(*one())
        elif fol == "w1w1":
            b.word(*one()); b.word(*one())
        else:
            b.word(*one()); b.copy(2, rnd.randrange(1, 60))
        b.probe(cell); b.probe(cell + "+1")
    for rep in range(2):
        for pred in preds:
            for fol in FOLLOWERS:
                for lits in (True, False):
                    cell = "%s/%s/%s" % (pred, fol, "lits" if lits else "none")
                    if pred == "start":   # (the bytes in front of the metablock are those of the one before: they are drawn with it)
                        def closing():
                            b.rlit(2); b.copy(3, 3); b.rlit(4)
                        b.cell(closing); b.end()
                        mode = (mode + 1) % 4
                        b.begin(x_scheme([mode], cheap))
                    b.cell(lambda: build(pred, fol, lits, cell))
    b.rlit(3)
    b.end(last=True)
    return b


def maps_scheme():
    """four block types of 64, 63, 2 and 1 distinct trees (the last is trivial while NTREES = 130), modes LSB6, MSB6, UTF8, SIGNED"""
    lit_map = list(range(64)) + [64 + min(c, 62) for c in range(64)] + [127 + (c & 1) for c in range(64)] + [129] * 64
    return Scheme([0, 1, 2, 3], lit_map, [x_tree(i) for i in range(130)])


def x_maps(seed):
    b = Build(); b.rnd = rnd = random.Random(seed)
    b.begin(maps_scheme()); x_start(b)
    b.rlit(20); b.copy(3, 4)
    for t in (1, 2, 3, 0, 2, 1, 3, 0):
        b.switch(t)
        for _ in range(12):
            def one():
                b.rlit(rnd.randrange(2, 4)); b.probe("type%d" % t)
            b.cell(one)
        b.copy(rnd.randrange(2, 5), rnd.randrange(1, 6))
    # a run of 70 literals that leaves the trivial type for a non-trivial one, and the other way, after each of its first 66 literals
    for j in BLOCK_ENDS:
        for first, then in ((3, j % 3), (j % 3, 3)):
            def run():
                if b.blocks[-1][0] != first:
                    b.switch(first)
                b.rlit(j - 1)
                b.probe("%s-last" % ("trivial" if first == 3 else "full"))
                b.switch(then)
                b.probe("to-%s" % ("full" if first == 3 else "trivial")); b.probe("to-%s+1" % ("full" if first == 3 else "trivial"))
                b.rlit(70 - j - 2)
                b.copy(rnd.randrange(2, 5), rnd.randrange(1, 6))
            b.cell(run)
    b.end(last=True)
    return b


def x_vectors(add):
    for mode in range(4):
        b = x_lut(mode, 3000 + mode)
        add("X-lut-mode%d" % mode, "X", b, held=b.held)
    add("X-every-tree", "X", x_every_tree(3010))
    add("X-source", "X", x_source(3020))
    add("X-boundary", "X", x_boundary(3030))
    add("X-words", "X", x_words(3040))
    add("X-words-start", "X", x_words(3050, preds=("start",), cheap=True))
    add("X-maps", "X", x_maps(3060))


# ------------------------------------------------------------------ the vectors
def vectors(families="SEX"):
    """-> [{"label", "family", "window", "stream", "output" (what the emitter expects), "llog", "clog", "mbs", "runs", "probes",
    "cells", the family's own notes}]"""
    out = []

    def add(label, family, b, **meta):
        comp = b.w.finish()
        assert len(comp) <= MAX_FILE * MAX_PARTS, (label, len(comp))
        assert not any(v["label"] == label for v in out), label
        out.append(dict(meta, label=label, family=family, window=b.wbits, stream=comp, output=bytes(b.out), llog=b.llog, clog=b.clog, mbs=b.mbs,
                        runs=b.runs, probes=b.probes, cells=b.cells))
    for family, make in (("S", s_vectors), ("E", e_vectors), ("X", x_vectors)):
        if family in families:
            make(add)
    return out


NOTES = ("shape", "place", "run", "run2", "ends", "held")


def entries():
    """(manifest entry, stream) of every vector, checked with the oracle and libbrotlidec"""
    import libbrotli_ref as ref
    import oracle_lib as oracle
    for v in vectors():
        comp, raw, label = v["stream"], v["output"], v["label"]
        info, got = oracle.decode(comp, len(raw) + 64, 0)
        assert info.result == 1 and got == raw and info.consumed == len(comp), (label, info.result, info.error_code, info.decoded_size, len(raw))
        if ref.available():
            r = ref.decode(comp, len(raw) + 64, False)
            assert r[0] == 1 and r[2] == raw, (label, r[0], r[1])
        e = {"label": label, "size": len(raw)}
        if v["window"] != 22:
            e["window"] = v["window"]
        e["sha"] = hashlib.sha256(raw).hexdigest()[:16]
        e["counts"] = [info.num_metablocks, info.num_commands]
        for k in NOTES:
            if k in v:
                e[k] = v[k]
        e["runs"] = v["runs"]
        if v["probes"]:
            e["cells"], e["probes"] = v["cells"], v["probes"]
        e["csize"] = len(comp)
        print(label, len(comp), len(raw))
        yield e, comp


def main():
    vector_store.write(OUT, entries(), small="pack", style="lines")


if __name__ == "__main__":
    main()
