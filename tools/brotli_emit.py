#!/usr/bin/env python3
"""A deterministic Brotli (RFC 7932) stream emitter -- test tooling.

It writes what an encoder library cannot be steered to: any number of block types per category with chosen switch
points, chosen literal context modes (MSB6 included) and context maps, chosen NPOSTFIX / NDIRECT, and any sequence of
compressed, stored, metadata and empty metablocks.  It is not a compressor: the caller supplies the commands (or lets
`greedy_commands` find some) and the plan; the emitter builds the prefix codes from the resulting histograms and
serialises everything.  Its output is validated against Google's libbrotlidec where that library exists
(tools/make_emitter_vectors.py, tools/make_word_vectors.py, tools/make_copy_vectors.py) and pinned by the committed vectors in
tests/golden/emitter/, tests/golden/emitter_words/ and tests/golden/emitter_copies/.

    w = BitWriter(); write_stream_header(w, 22)
    emit_compressed(w, commands, plan, is_last=False); emit_stored(w, raw); emit_metadata(w, b"..."); emit_last_empty(w)
    stream = w.finish()

A command is (insert bytes, copy_len, what), `what` being
    an int                         an explicit distance (one beyond the maximum distance names a dictionary word, as in any decoder),
    ("word", word_idx, transform)  a word of the static dictionary: the emitter computes the distance at the command's position,
    ("ring", k)                    short distance code k (0 .. 15) against the ring of the last four distances, (4, 11, 15, 16) at first,
    ("implicit",)                  a command symbol below 128: the last distance, no distance symbol,
    ("raw", distance)              an explicit distance written as given (`unchecked=True`: streams that are invalid on purpose).
Words need `wbits` (the maximum distance is min(P + len(dictionary), (1 << wbits) - 16)).  The words and their 121
transforms are restated here in plain Python from RFC 7932 Appendix A / B (`dictionary_word`, `transform_word`), over
the tables of csrc/brotli_tables_gen.h and data/dictionary.bin; no decoder is called, so that the bytes the emitter
expects are an opinion of their own beside the oracle's and libbrotlidec's.  `log=[]` receives one record per command.

The header can be chosen as well (tools/make_header_vectors.py, tests/golden/emitter_headers/): `Plan(codes=...)` puts a WireCode
-- a prefix code from explicit lengths or words, with its HSKIP, its code-length code, its sixteens and seventeens, its
trailing zeros, or the simple form in any order -- in the place of any code of the metablock; `Plan(map_forms=...)` gives a
context map its RLEMAX, its split into zero runs and its IMTF (the forward move-to-front is done here); write_mlen,
emit_metadata and emit_stored take MNIBBLES, MSKIPBYTES, the reserved bit and padding as given.  `unchecked` writes what no
decoder accepts.  `hlog=[]` receives one record per such code, per context map and per category's block switches, with the
bit positions of every word, the runs the repeat words resolved to and the 64-bit steps a wide reader takes over them.

`llog=[]` receives one record per literal: where its code word lies in the stream, the two bytes in front of it, its block type,
mode, context and tree (tools/make_literal_vectors.py, tests/golden/emitter_literals/).
"""
import heapq

# ------------------------------------------------------------------ bits
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0, (value, nbits)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def bits(self):
        """the number of bits written so far"""
        return 8 * len(self.out) + self.n

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def finish(self):
        self.align()
        return bytes(self.out)


# ------------------------------------------------------------------ prefix codes (RFC 7932 section 3)
def limited_lengths(hist, limit=15):
    """code lengths (0 = unused) of a complete prefix code for the symbols with hist > 0, none longer than `limit`"""
    syms = [s for s, c in enumerate(hist) if c > 0]
    lengths = [0] * len(hist)
    if len(syms) <= 1:
        return lengths  # zero or one symbol: a zero-length code, written as a simple code by the caller
    scale = 0
    while True:
        heap = [(max(1, hist[s] >> scale), s, None, None) for s in syms]
        heapq.heapify(heap)
        nxt = len(hist)
        while len(heap) > 1:
            a = heapq.heappop(heap); b = heapq.heappop(heap)
            heapq.heappush(heap, (a[0] + b[0], nxt, a, b)); nxt += 1
        depth = {}
        stack = [(heap[0], 0)]
        while stack:
            node, d = stack.pop()
            if node[2] is None:
                depth[node[1]] = d
            else:
                stack.append((node[2], d + 1)); stack.append((node[3], d + 1))
        if max(depth.values()) <= limit:
            for s, d in depth.items():
                lengths[s] = d
            return lengths
        scale += 1


def canonical_codes(lengths):
    """symbol -> (code bits as they go on the wire, i.e. already bit-reversed, length)"""
    codes, code = {}, 0
    for L in range(1, 16):
        for s, l in enumerate(lengths):
            if l == L:
                rev = int(format(code, "0%db" % L)[::-1], 2)
                codes[s] = (rev, L)
                code += 1
        code <<= 1
    return codes


_CL_ORDER = [1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15]
_CL_VLC = {0: (0, 2), 1: (7, 4), 2: (3, 3), 3: (2, 2), 4: (1, 2), 5: (15, 4)}  # value -> (bits LSB first, length), section 3.5


class PrefixCode:
    """a prefix code over `alphabet` symbols built from a histogram; knows how to write itself and its symbols"""

    def __init__(self, hist, alphabet):
        self.alphabet = alphabet
        hist = list(hist) + [0] * (alphabet - len(hist))
        self.used = [s for s, c in enumerate(hist) if c > 0]
        if not self.used:
            self.used = [0]
        if len(self.used) <= 4:
            self.simple = True
            order = sorted(self.used, key=lambda s: (-hist[s], s))
            n = len(order)
            if n == 1:
                self.lengths = {order[0]: 0}; self.syms = order; self.tree_select = None
            elif n == 2:
                self.syms = sorted(order); self.lengths = {s: 1 for s in self.syms}; self.tree_select = None
            elif n == 3:
                self.syms = [order[0]] + sorted(order[1:]); self.lengths = {self.syms[0]: 1, self.syms[1]: 2, self.syms[2]: 2}; self.tree_select = None
            else:
                # tree-select 0: lengths 2,2,2,2 over the sorted symbols; 1: lengths 1,2,3,3 (the last two sorted)
                if hist[order[0]] > hist[order[1]] + hist[order[2]] + hist[order[3]]:
                    self.syms = [order[0], order[1]] + sorted(order[2:]); self.tree_select = 1
                    self.lengths = {self.syms[0]: 1, self.syms[1]: 2, self.syms[2]: 3, self.syms[3]: 3}
                else:
                    self.syms = sorted(order); self.tree_select = 0
                    self.lengths = {s: 2 for s in self.syms}
            full = [0] * alphabet
            for s, l in self.lengths.items():
                full[s] = l
            self.codes = canonical_codes(full) if n > 1 else {order[0]: (0, 0)}
        else:
            self.simple = False
            self.full = limited_lengths(hist, 15)
            self.codes = canonical_codes(self.full)

    def write_code(self, w):
        if self.simple:
            abits = max(1, (self.alphabet - 1).bit_length())
            w.put(1, 2)
            w.put(len(self.syms) - 1, 2)
            for s in self.syms:
                w.put(s, abits)
            if len(self.syms) == 4:
                w.put(self.tree_select, 1)
            return
        lens = self.full[:max(self.used) + 1]
        cl_hist = [0] * 18
        for l in lens:
            cl_hist[l] += 1
        cl_len = limited_lengths(cl_hist, 5)
        if sum(1 for c in cl_hist if c) == 1:  # every symbol has the same length: a code-length code of one symbol is not
            other = 0 if cl_hist[0] == 0 else 1  # allowed to be empty on the wire, give a second symbol a length too
            cl_hist[other] += 1
            cl_len = limited_lengths(cl_hist, 5)
        # HSKIP: leading entries of the order that are zero may be skipped (0, 2 or 3 of them)
        seq = [cl_len[s] for s in _CL_ORDER]
        hskip = 3 if seq[0] == seq[1] == seq[2] == 0 else 2 if seq[0] == seq[1] == 0 else 0
        w.put(hskip, 2)
        space, last = 32, 0
        for i in range(17, -1, -1):
            if seq[i]:
                last = i
                break
        # the decoder stops reading code-length-code lengths once the space is used up: write exactly until then
        for i in range(hskip, 18):
            v = seq[i]
            bits, n = _CL_VLC[v]
            w.put(bits, n)
            if v:
                space -= 32 >> v
                if space <= 0:
                    break
        assert space == 0 or sum(1 for v in seq if v) == 1, (space, seq, last)
        cl_codes = canonical_codes(cl_len)
        if sum(1 for v in cl_len if v) == 1:
            cl_codes = {s: (0, 0) for s, v in enumerate(cl_len) if v}
        total = 0
        for l in lens:
            c, n = cl_codes[l]
            w.put(c, n)
            if l:
                total += 32768 >> l
                if total == 32768:
                    break  # the decoder stops once the code is complete; trailing zeros are not written
        assert total == 32768, total

    def put(self, w, sym):
        c, n = self.codes[sym]
        w.put(c, n)


class Resolved:
    """what resolve_words found: `lengths`; per word read `runs` (None, or the number of symbols its repeat added), `depth` (its place in
    its chain of repeat words, 1 = the first) and `values` (the length it gave its symbols); `used` = the number of words read
    before the code was complete or the alphabet full; `symbol` = the symbols passed; `space` = the code space left (None: a
    repeat passed the alphabet's end, which ends the reading with the decoders' verdict)"""


def resolve_words(words, max_symbol):
    """the code-length words of section 3.5 as a decoder reads them: a word is a length 0 .. 15, (16, extra 0 .. 3) or
    (17, extra 0 .. 7) -> Resolved"""
    symbol, space, prev, repeat, repeat_len = 0, 32768, 8, 0, 0
    r = Resolved()
    r.lengths, r.runs, r.depth, r.values, r.used, d = [0] * max_symbol, [], [], [], 0, 0
    for word in words:
        if symbol >= max_symbol or space == 0:   # (an over-used space is not zero: the decoders read on to the alphabet's end)
            break
        r.used += 1
        if isinstance(word, int):
            assert 0 <= word <= 15
            repeat, d = 0, 0
            if word:
                r.lengths[symbol] = word; prev = word; space -= 32768 >> word
            symbol += 1
            r.runs.append(None); r.depth.append(0); r.values.append(word)
            continue
        code, extra = word
        nbits = code - 14
        assert code in (16, 17) and 0 <= extra < (1 << nbits), word
        new_len = prev if code == 16 else 0
        if repeat_len != new_len:
            repeat, repeat_len, d = 0, new_len, 0
        old = repeat
        if repeat > 0:
            repeat = (repeat - 2) << nbits
        repeat += extra + 3
        d = d + 1 if old else 1
        delta = repeat - old
        r.runs.append(delta); r.depth.append(d); r.values.append(repeat_len)
        if symbol + delta > max_symbol:
            symbol, space = max_symbol, None
            break
        if repeat_len:
            for _ in range(delta):
                r.lengths[symbol] = repeat_len; symbol += 1
            space -= delta << (15 - repeat_len)
        else:
            symbol += delta
    r.symbol, r.space = symbol, space
    return r


def words_of(lengths, repeats=False, trailing_zeros=False):
    """plain words for `lengths` (up to the last non-zero one, or all of them); with `repeats` every run that a chain of
    sixteens or seventeens can express exactly is written as one (greedily, the decoder's arithmetic run backwards)"""
    last = max((i for i, l in enumerate(lengths) if l), default=-1)
    lens = list(lengths) if trailing_zeros else list(lengths[:last + 1])
    if not repeats:
        return lens
    out, i, prev = [], 0, 8
    while i < len(lens):
        l = lens[i]
        j = i
        while j < len(lens) and lens[j] == l:
            j += 1
        n = j - i
        if l and l != prev:
            out.append(l); prev = l; i += 1
            continue
        code, nbits = (16, 2) if l else (17, 3)
        chain = _chain_for(n, nbits)
        if chain is None:
            out.append(l); i += 1   # (a literal word: it also ends any chain in front of it)
            continue
        # a chain continues a repeat word of the same kind directly in front of it: break it with nothing, the total is what counts
        if out and not isinstance(out[-1], int) and out[-1][0] == code:
            out.append(l); i += 1
            continue
        out += [(code, e) for e in chain]; i += n
    return out


def _chain_for(n, nbits):
    """extra values of a chain of repeat words whose total is exactly n, or None (n < 3)"""
    if n < 3:
        return None
    chain = []
    while True:
        if n - 3 < (1 << nbits):
            chain.append(n - 3)
            return chain[::-1]
        e = (n - 3) & ((1 << nbits) - 1)
        chain.append(e)
        n = ((n - 3 - e) >> nbits) + 2
        if n < 3:
            return None


class WireCode:
    """a prefix code with its wire form chosen by the caller (PrefixCode chooses its own): write_code / put / codes as there.

    complex form: `words` (see resolve_words) or `lengths` (then one word per length up to the last non-zero one, `trailing_zeros`
    for all of them; `repeats` for words_of's repeat words); `cl_lengths` = the code-length code's own 18 lengths (default: from the words'
    histogram; one non-zero entry = the one-symbol code whose words take no bits); `hskip` 0, 2 or 3 (default: the largest the
    zeros allow).  simple form: `simple` = the symbols in wire order, `tree_select` for four of them.
    `max_symbol` below the alphabet for the large-window distance codes.  `unchecked`: written as given even where no decoder
    accepts it; symbols of an incomplete code are then written as nothing."""

    def __init__(self, alphabet, lengths=None, words=None, cl_lengths=None, hskip=None, trailing_zeros=False, repeats=False, simple=None, tree_select=None,
                 max_symbol=None, unchecked=False):
        self.alphabet, self.unchecked = alphabet, unchecked
        self.max_symbol = alphabet if max_symbol is None else max_symbol
        self.simple = simple is not None
        self.codes = {}
        if self.simple:
            self.syms, self.tree_select = list(simple), tree_select
            n = len(self.syms)
            assert 1 <= n <= 4 and (n == 4) == (tree_select is not None)
            ok = len(set(self.syms)) == n and all(s < self.max_symbol for s in self.syms)
            assert ok or unchecked
            shape = {1: [0], 2: [1, 1], 3: [1, 2, 2], 4: [1, 2, 3, 3] if tree_select else [2, 2, 2, 2]}[n]
            self.full = [0] * alphabet
            if ok:
                for s, l in zip(self.syms, shape):
                    self.full[s] = l
                self.codes = canonical_codes(self.full) if n > 1 else {self.syms[0]: (0, 0)}
            return
        if words is None:
            words = words_of(lengths, repeats, trailing_zeros)
        self.words = list(words)
        r = self.resolved = resolve_words(self.words, self.max_symbol)
        self.full, self.runs, self.depth, self.consumed, self.space = r.lengths, r.runs, r.depth, r.used, r.space
        assert lengths is None or list(lengths[:self.max_symbol]) + [0] * (self.max_symbol - len(lengths)) == self.full or unchecked, "the words do not give the lengths"
        if cl_lengths is None:
            h = [0] * 18
            for wd in self.words:
                h[wd if isinstance(wd, int) else wd[0]] += 1
            if sum(1 for c in h if c) == 1:
                h[0 if h[0] == 0 else 1] += 1
            cl_lengths = limited_lengths(h, 5)
        self.cl_lengths = list(cl_lengths)
        assert len(self.cl_lengths) == 18 and all(0 <= v <= 5 for v in self.cl_lengths)
        seq = [self.cl_lengths[s] for s in _CL_ORDER]
        most = 3 if seq[0] == seq[1] == seq[2] == 0 else 2 if seq[0] == seq[1] == 0 else 0
        self.hskip = most if hskip is None else hskip
        assert self.hskip in (0, 2, 3) and (self.hskip <= most or unchecked)
        nz = [v for v in self.cl_lengths if v]
        self.cl_single = len(nz) == 1
        self.cl_space = 32 - sum(32 >> v for v in nz)
        if self.cl_single:
            self.cl_codes = {s: (0, 0) for s, v in enumerate(self.cl_lengths) if v}
        elif self.cl_space == 0:
            self.cl_codes = canonical_codes(self.cl_lengths)
        else:
            assert unchecked, "the code-length code is not complete"
            self.cl_codes = None
        if self.space == 0 and self.cl_codes is not None:
            self.codes = canonical_codes(self.full)
        else:
            assert unchecked, ("the code is not complete", self.space)

    def write_code(self, w, log=None, kind=None):
        rec = {"kind": kind, "form": "simple" if self.simple else "complex", "alphabet": self.alphabet, "max_symbol": self.max_symbol, "start": w.bits(),
               "unchecked": self.unchecked}
        if log is not None:
            log.append(rec)
        if self.simple:
            abits = max(1, (self.alphabet - 1).bit_length())
            w.put(1, 2); w.put(len(self.syms) - 1, 2)
            for s in self.syms:
                w.put(s, abits)
            if len(self.syms) == 4:
                w.put(self.tree_select, 1)
            rec.update(nsym=len(self.syms), symbols=list(self.syms), tree_select=self.tree_select, end=w.bits())
            return
        w.put(self.hskip, 2)
        seq = [self.cl_lengths[s] for s in _CL_ORDER]
        space = 32
        for i in range(self.hskip, 18):  # (a decoder reads until the space is used up, or over-used)
            bits, n = _CL_VLC[seq[i]]
            w.put(bits, n)
            if seq[i]:
                space -= 32 >> seq[i]
                if space <= 0:
                    break
        rec.update(hskip=self.hskip, cl_lengths=list(self.cl_lengths), cl_symbols=sum(1 for v in self.cl_lengths if v), cl_space=self.cl_space,
                   words_start=w.bits(), words=[], consumed=self.consumed, space=self.space, symbols=sum(1 for l in self.full if l), reached=self.resolved.symbol,
                   depth=max(self.full) if any(self.full) else 0)
        if self.cl_codes is None:
            rec["end"] = w.bits()
            return
        for k, wd in enumerate(self.words):
            code, extra = (wd, None) if isinstance(wd, int) else wd
            at = w.bits()
            c, n = self.cl_codes[code]
            w.put(c, n)
            if extra is not None:
                w.put(extra, code - 14)
            read = k < self.consumed
            rec["words"].append({"word": code, "extra": extra, "start": at, "mid": at + n, "end": w.bits(), "read": read,
                                 "run": self.runs[k] if read else None, "chain": self.depth[k] if read else None, "value": self.resolved.values[k] if read else None})
        # a reader that takes 64 stream bits a step takes every word that starts inside them: the next step starts where the last of them ends
        base, step = rec["words_start"], 0
        for wd in rec["words"]:
            if wd["start"] - base >= 64:
                base, step = wd["start"], step + 1
            wd["step"], wd["at"] = step, wd["start"] - base
        rec["end"] = w.bits()

    def put(self, w, sym):
        if sym not in self.codes:
            assert self.unchecked, sym
            return
        c, n = self.codes[sym]
        w.put(c, n)


# ------------------------------------------------------------------ small encodings
def write_stream_header(w, wbits, large=False):
    """section 9.1, standard windows (10 .. 24); `large`: the large-window form (any six-bit value, as given)"""
    if large:
        w.put(1, 1); w.put(0, 3); w.put(1, 3); w.put(0, 1); w.put(wbits, 6)
    elif wbits == 16:
        w.put(0, 1)
    elif wbits == 17:
        w.put(1, 1); w.put(0, 3); w.put(0, 3)
    elif 18 <= wbits <= 24:
        w.put(1, 1); w.put(wbits - 17, 3)
    else:
        assert 10 <= wbits <= 15
        w.put(1, 1); w.put(0, 3); w.put(wbits - 8, 3)


def write_varlen8(w, v):  # 0..255 in 1 + 3 + n bits (section 9.2: NBLTYPES - 1, NTREES - 1)
    if v == 0:
        w.put(0, 1)
        return
    n = v.bit_length() - 1
    w.put(1, 1); w.put(n, 3); w.put(v - (1 << n), n)


def write_mlen(w, is_last, mlen, is_uncompressed=False, nibbles=None):
    """`nibbles`: MNIBBLES as given (4, 5 or 6), more than MLEN - 1 needs included -- which no decoder accepts"""
    w.put(1 if is_last else 0, 1)
    if is_last:
        w.put(0, 1)  # ISLASTEMPTY = 0
    nib = max(4, ((mlen - 1).bit_length() + 3) // 4)
    assert nib <= 6
    if nibbles is not None:
        assert nib <= nibbles <= 6
        nib = nibbles
    w.put(nib - 4, 2)
    w.put(mlen - 1, nib * 4)
    if not is_last:
        w.put(1 if is_uncompressed else 0, 1)


def pad_to_byte(w, pad=0):
    """the bits up to the next byte boundary: zeros, or the low bits of `pad` (no decoder accepts others than zeros)"""
    if w.n:
        k = 8 - w.n
        w.put(pad & ((1 << k) - 1), k)


def emit_stored(w, raw, pad=0):
    assert 0 < len(raw) <= 1 << 24
    write_mlen(w, False, len(raw), True)
    pad_to_byte(w, pad)
    w.out += raw


def emit_metadata(w, payload, nbytes=None, reserved=0, pad=0):
    """`nbytes`: MSKIPBYTES as given (more than the length needs: no decoder accepts that); `reserved`: the reserved bit; `pad`: pad_to_byte"""
    w.put(0, 1); w.put(3, 2); w.put(reserved, 1)  # ISLAST = 0, MNIBBLES = 0 (code 3), reserved
    n = len(payload)
    least = 0 if n == 0 else max(1, ((n - 1).bit_length() + 7) // 8)
    if nbytes is None:
        nbytes = least
    assert least <= nbytes <= 3
    w.put(nbytes, 2)
    if nbytes:
        w.put(max(0, n - 1), 8 * nbytes)
    pad_to_byte(w, pad)
    w.out += payload


def emit_last_empty(w):
    w.put(1, 1); w.put(1, 1)


_INS_BASE = [0, 1, 2, 3, 4, 5, 6, 8, 10, 14, 18, 26, 34, 50, 66, 98, 130, 194, 322, 578, 1090, 2114, 6210, 22594]
_INS_EXTRA = [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 14, 24]
_COPY_BASE = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 18, 22, 30, 38, 54, 70, 102, 134, 198, 326, 582, 1094, 2118]
_COPY_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 24]
_BL_BASE = [1, 5, 9, 13, 17, 25, 33, 41, 49, 65, 81, 97, 113, 145, 177, 209, 241, 305, 369, 497, 753, 1265, 2289, 4337, 8433, 16625]
_BL_EXTRA = [2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 7, 8, 9, 10, 11, 12, 13, 24]


def _code_of(value, base, extra):
    for c in range(len(base) - 1, -1, -1):
        if value >= base[c]:
            assert value - base[c] < (1 << extra[c]), value
            return c, value - base[c], extra[c]
    raise ValueError(value)


def command_symbol(ins_code, copy_code, implicit):
    """section 5: the 704 insert-and-copy symbols as an 11-cell grid"""
    ir, cr = ins_code >> 3, copy_code >> 3
    if implicit:
        assert ir == 0 and cr <= 1
        cell = cr
    else:
        cell = {(0, 0): 2, (0, 1): 3, (1, 0): 4, (1, 1): 5, (0, 2): 6, (2, 0): 7, (1, 2): 8, (2, 1): 9, (2, 2): 10}[(ir, cr)]
    return (cell << 6) | ((ins_code & 7) << 3) | (copy_code & 7)


def distance_symbol(distance, npostfix, ndirect):
    """section 4: explicit distance -> (symbol, extra value, extra bits); short codes are not produced here"""
    if distance <= ndirect:
        return 15 + distance, 0, 0
    d = distance - ndirect - 1 + (1 << (npostfix + 2))
    bucket = d.bit_length() - 2 - npostfix  # = ndistbits
    # d = ((2 + hcode) << (ndistbits + npostfix)) + (dextra << npostfix) + lcode, hcode the bit below the top one
    nb = bucket
    hcode = (d >> (nb + npostfix)) & 1
    lcode = d & ((1 << npostfix) - 1)
    dextra = (d >> npostfix) & ((1 << nb) - 1)
    sym = 16 + ndirect + ((2 * (nb - 1) + hcode) << npostfix) + lcode
    return sym, dextra, nb


_CTX_LUT = None


def literal_context(mode, p1, p2):
    """section 7.1; modes 0 LSB6, 1 MSB6, 2 UTF8, 3 SIGNED -- through the table the decoders use
    (csrc/brotli_tables_gen.h, pinned against the reference's src/context.rs by tests/test_tables_vs_reference.py)"""
    global _CTX_LUT
    if _CTX_LUT is None:
        import os
        import re
        h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust-brotli-decompressor_amd", "csrc", "brotli_tables_gen.h")).read()
        m = re.search(r"kContextLookup\[2048\]\s*=\s*\{(.*?)\};", h, re.S)
        _CTX_LUT = [int(x) for x in re.findall(r"\d+", m.group(1))]
        assert len(_CTX_LUT) == 2048
    return _CTX_LUT[mode * 512 + p1] | _CTX_LUT[mode * 512 + 256 + p2]


# ------------------------------------------------------------------ the static dictionary (RFC 7932 section 8, appendices A and B)
_TABLES = None
RING_INIT = (4, 11, 15, 16)  # last, second last, third last, fourth last distance at the start of a stream (section 4)
NUM_TRANSFORMS = 121


def tables():
    """{"size_bits": [25], "offsets": [25], "transforms": [(prefix, type, suffix)] * 121, "words": the 122784 bytes} out of
    csrc/brotli_tables_gen.h (pinned against the reference by tests/test_tables_vs_reference.py) and data/dictionary.bin"""
    global _TABLES
    if _TABLES is None:
        import os
        import re
        pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust-brotli-decompressor_amd")
        h = open(os.path.join(pkg, "csrc", "brotli_tables_gen.h")).read()

        def array(name):
            m = re.search(name + r"\[[^\]]*\]\s*=\s*\{(.*?)\};", h, re.S)
            return [int(x) for x in re.findall(r"\d+", m.group(1))]
        pool, tr = bytes(array("kAffixPool")), array("kTransforms")
        assert len(tr) == 3 * NUM_TRANSFORMS
        affix = lambda off: pool[off:pool.index(0, off)]  # (NUL-terminated strings)
        _TABLES = {"size_bits": array("kDictSizeBitsByLength"), "offsets": array("kDictOffsetsByLength"),
                   "transforms": [(affix(tr[3 * t]), tr[3 * t + 1], affix(tr[3 * t + 2])) for t in range(NUM_TRANSFORMS)],
                   "words": open(os.path.join(pkg, "data", "dictionary.bin"), "rb").read()}
        assert len(_TABLES["size_bits"]) == 25 and len(_TABLES["offsets"]) == 25 and len(_TABLES["words"]) == 122784
    return _TABLES


def dictionary_word(length, idx):
    t = tables()
    assert 4 <= length <= 24 and 0 <= idx < (1 << t["size_bits"][length]), (length, idx)
    at = t["offsets"][length] + idx * length
    return t["words"][at:at + length]


def _uppercase_one(b, i):
    """appendix B: the "UTF-8 uppercase" of the character at b[i]; -> its length in bytes (a character that sticks out of
    the word is changed as far as the word reaches)"""
    c = b[i]
    if c < 0xC0:
        if 97 <= c <= 122:
            b[i] = c ^ 32
        return 1
    if c < 0xE0:
        if i + 1 < len(b):
            b[i + 1] ^= 32
        return 2
    if i + 2 < len(b):
        b[i + 2] ^= 5
    return 3


def transform_word(word, transform):
    """appendix B: prefix + elementary transform of the word + suffix.  Types as csrc/brotli_tables_gen.h numbers them:
    0 identity, 1 .. 9 omit last N, 10 uppercase first, 11 uppercase all, 12 .. 20 omit first N - 11."""
    prefix, kind, suffix = tables()["transforms"][transform]
    b = bytearray(word)
    if 1 <= kind <= 9:
        b = b[:max(0, len(b) - kind)]
    elif kind >= 12:
        b = b[kind - 11:]
    elif kind == 10:
        if b:
            _uppercase_one(b, 0)
    elif kind == 11:
        i = 0
        while i < len(b):
            i += _uppercase_one(b, i)
    return bytes(prefix) + bytes(b) + bytes(suffix)


# ------------------------------------------------------------------ the compressed metablock
class Plan:
    """what the caller chooses: block splits per category as [(type, count), ...] covering every symbol of the category
    (literals, commands, explicit distances), literal context modes per literal block type, the context maps."""

    def __init__(self, lit_blocks=None, cmd_blocks=None, dist_blocks=None, modes=None, lit_map=None, dist_map=None, npostfix=0, ndirect=0, type_codes="direct",
                 codes=None, map_forms=None, large_window=False):
        """`codes`: {(slot, index): function of (histogram, alphabet) -> a WireCode} for the prefix codes whose wire form the caller
        chooses -- slots "lit", "cmd", "dist" (index = the tree), "btype", "blen" (index = the category), "lmap", "dmap" (index 0: the
        context map's own code); every other code is a PrefixCode of its histogram.  `map_forms`: {"lit" / "dist": a form for
        write_context_map}.  `large_window`: the distance alphabet of a large-window stream."""
        self.lit_blocks, self.cmd_blocks, self.dist_blocks = lit_blocks, cmd_blocks, dist_blocks
        self.modes, self.lit_map, self.dist_map = modes, lit_map, dist_map
        self.npostfix, self.ndirect, self.type_codes = npostfix, ndirect, type_codes
        self.codes, self.map_forms, self.large_window = codes or {}, map_forms or {}, large_window


def max_distance_symbol(ndirect, npostfix):
    """the number of distance symbols a large-window stream may use (distances up to 2^31 - 4), as the decoders compute it"""
    bound, diff, postfix = (0, 4, 12, 28)[npostfix], (73, 126, 228, 424)[npostfix], 1 << npostfix
    if ndirect < bound:
        return ndirect + diff + postfix
    if ndirect > bound + postfix:
        return ndirect + diff
    return bound + diff + postfix


def forward_mtf(values):
    """section 7.3 backwards: values -> move-to-front indices"""
    mtf, out = list(range(256)), []
    for v in values:
        i = mtf.index(v)
        out.append(i)
        mtf.insert(0, mtf.pop(i))
    return out


def zero_run_pieces(n, rlemax):
    """a run of n zeros as the longest pieces RLEMAX allows: [(code, extra)], code 0 = a single zero"""
    out = []
    while n:
        c = min(rlemax, n.bit_length() - 1)
        if c == 0:
            out.append((0, 0)); n -= 1
        else:
            take = min(n, (2 << c) - 1)
            out.append((c, take - (1 << c))); n -= take
    return out


def write_context_map(w, cmap, ntrees, form=None, code_for=None, log=None, kind=None, unchecked=False):
    """section 7.3.  `form`: {"rlemax": 0 .. 16, "imtf": 0 / 1, "runs": function of (length of a run of zeros, RLEMAX) ->
    [(code, extra)] (code 0 = one zero; default zero_run_pieces), "items": the symbols as they go on the wire, [("v", index)] and
    [("run", code, extra)] -- unchecked: they need not add up to the map; "ntrees": NTREES where the map does not name them all}.  With IMTF = 1 the forward move-to-front is done here.
    `code_for(histogram, alphabet)` -> the map's own prefix code (default PrefixCode)."""
    form = form or {}
    rlemax, imtf = form.get("rlemax", 0), form.get("imtf", 0)
    write_varlen8(w, ntrees - 1)
    rec = {"kind": kind, "form": "map", "ntrees": ntrees, "size": len(cmap), "start": w.bits()}
    if log is not None:
        log.append(rec)
    if ntrees < 2:
        return
    if rlemax:
        w.put(1, 1); w.put(rlemax - 1, 4)
    else:
        w.put(0, 1)
    values = forward_mtf(cmap) if imtf else list(cmap)
    items = form.get("items")
    if items is None:
        items, pieces, i = [], form.get("runs", zero_run_pieces), 0
        while i < len(values):
            if values[i]:
                items.append(("v", values[i])); i += 1
                continue
            j = i
            while j < len(values) and values[j] == 0:
                j += 1
            got = pieces(j - i, rlemax)
            assert sum((1 << c) + e if c else 1 for c, e in got) == j - i and all(c <= rlemax and 0 <= e < (1 << c) for c, e in got), (j - i, got)
            items += [("run", c, e) if c else ("v", 0) for c, e in got]
            i = j
    alphabet = ntrees + rlemax
    h = [0] * alphabet
    for it in items:
        h[it[1] if it[0] == "run" else it[1] + rlemax if it[1] else 0] += 1
    code = (code_for or PrefixCode)(h, alphabet)
    if isinstance(code, WireCode):
        code.write_code(w, log, kind + "_code")
    else:
        code.write_code(w)
    rec.update(rlemax=rlemax, imtf=imtf, runs=[], indices=sorted({it[1] for it in items if it[0] == "v"}), mtf_max=max([it[1] for it in items if it[0] == "v"], default=0),
               items_start=w.bits(), filled=0, items=list(items), map=list(cmap))
    for it in items:
        if it[0] == "run":
            code.put(w, it[1]); w.put(it[2], it[1])
            rec["runs"].append((it[1], it[2], rec["filled"]))
            rec["filled"] += (1 << it[1]) + it[2]
        else:
            code.put(w, it[1] + rlemax if it[1] else 0)
            rec["filled"] += 1
    w.put(imtf, 1)
    rec["end"] = w.bits()


def greedy_commands(data, min_match=4, max_dist=1 << 16, start=0, history=b""):
    """a small hash-chain-free LZ77: [(insert bytes, copy_len, distance)]; distance 0 = no copy (tail)"""
    buf = history + data
    base = len(history)
    table, cmds, i, lit_start = {}, [], base, base
    n = len(buf)
    for j in range(max(0, base - max_dist), base - min_match + 1):
        table[buf[j:j + min_match]] = j
    while i + min_match <= n:
        key = buf[i:i + min_match]
        j = table.get(key)
        table[key] = i
        if j is not None and i - j <= max_dist and i - j >= 1:
            L = min_match
            while i + L < n and buf[j + L] == buf[i + L] and L < 2000:
                L += 1
            cmds.append((buf[lit_start:i], L, i - j))
            for k in range(i + 1, min(i + L, n - min_match + 1)):
                table[buf[k:k + min_match]] = k
            i += L
            lit_start = i
        else:
            i += 1
    if lit_start < n:
        cmds.append((buf[lit_start:n], 0, 0))
    return cmds


def emit_compressed(w, commands, plan, is_last, prev=b"", dictionary=b"", wbits=None, log=None, unchecked=False, mlen=None, literals=None, realised=None, ring_io=None, hlog=None, nibbles=None, llog=None):
    """commands: [(insert bytes, copy_len, distance)]; distance 0 with copy_len 0 only as the final literals-only command
    (it is written with copy length 2 and an implicit distance that the decoder never executes: the metablock is complete
    after its literals).  `prev` = the stream's output so far (copies may reach into it; its last two bytes are the literal
    context of the first literal).  `dictionary` = a custom (LZ77 prefix) dictionary the stream is decoded with: its bytes lie in front
    of the stream's first output byte for copies alone -- a copy may start in it and run on into the output -- while the first two
    literals of the stream have context (0, 0) whatever its last bytes are.  Returns the metablock's own output bytes.

    In place of the distance a command may carry ("word", word_idx, transform), ("ring", k), ("implicit",) or ("raw", distance)
    (the module's docstring).  `wbits` = the stream's window: with it a distance beyond min(P + len(dictionary), (1 << wbits) - 16)
    is a word of the static dictionary, whichever way the distance was written, and the ring of the last four distances is kept
    as section 4 says (code 0, the implicit distance and words do not push).  Without it every distance is a copy, as before.
    `log`: a list that receives one dict per command -- "coding" (explicit / ring / implicit / tail), "code" (the short code or
    None), "insert" (the number of literals), "word" (bool), "copy_len", "word_idx", "transform", "total" (bytes the copy part put out), "pos" (stream position of
    the copy part), "distance", "max_distance".  `unchecked`: the last command may be invalid (a distance below 1, a word with a
    copy length outside 4 .. 24 or a transform beyond 120): it is written as it stands, its log record says "invalid", and the
    bytes returned end in front of its copy part -- what a decoder makes of the stream is not the emitter's to say.  `mlen`
    declares another MLEN than the commands add up to (unchecked streams again).

    For generators that cannot know the stream's state ahead of time: the insert part may be a count, and `literals(p1, p2, k)`
    then supplies each byte from the two bytes in front of it and the literal's number in the metablock; `what` may be a function of (pos, ring, max_distance) that returns
    one of the forms above.  `realised` receives the command list with both resolved: emitting it again, under any plan,
    gives the same output.

    `ring_io`: the ring of the last four distances as a list that is read at the start and written back at the end -- a stream of
    several metablocks (`prev=`) keeps its ring from one to the next, as a decoder does; without it every metablock starts from RING_INIT.

    `hlog`: a list that receives one record per prefix code whose wire form the plan chooses (WireCode.write_code) and per context
    map (write_context_map), each with its bit positions in the stream, {"kind": "metablock", "start"} in front of them and
    {"kind": "commands", "start"} where the first command begins.

    `llog`: a list that receives one record per literal -- "k" (its number in the metablock), "cmd" (the command it belongs to), "pos"
    (its output position in the stream), "bit" (the stream bit its code word starts at, behind a block switch if one stands in front of
    it), "nbits", "byte", "p1", "p2" (the two bytes in front of it as the decoder has them: zeros in front of the stream's start and,
    with a custom dictionary, in place of the dictionary's last bytes), "type" (the literal block type), "mode", "context", "tree" and "first_of_block" (a
    block switch was written in front of it)."""
    npf, ndir = plan.npostfix, plan.ndirect
    max_backward = (1 << wbits) - 16 if wbits else None
    ring = list(RING_INIT) if ring_io is None else list(ring_io)
    # --- the data and symbol sequences
    out = bytearray()
    lits, cmd_syms, dist_syms = [], [], []
    lit_at = []    # per literal: its offset in the metablock's output
    has_dist = []  # per command: does a distance symbol follow its literals?
    inserts = []   # per command: its literals
    pad = 2 - min(2, len(prev))  # (zero bytes that stand for the context in front of the stream's first byte: not output)
    history = bytearray(pad) + bytearray(prev)
    start = len(history)
    invalid_at = None
    for ci, (ins, clen, what) in enumerate(commands):
        assert invalid_at is None, "an invalid command must be the last one"
        if isinstance(ins, int):
            made = bytearray()
            for _ in range(ins):
                b = literals(history[-1], history[-2], len(lits))
                lits.append((b, history[-1], history[-2])); lit_at.append(len(history) - start)
                history.append(b); made.append(b)
            ins = bytes(made)
        else:
            for b in ins:
                lits.append((b, history[-1], history[-2])); lit_at.append(len(history) - start)
                history.append(b)
        inserts.append(ins)
        if clen == 0:
            # (copy length 2 that is never executed: the metablock is complete after the literals, and the decoder looks
            # at neither the distance nor the copy then -- decode.rs:2552-2556)
            ic, iv, ib = _code_of(len(ins), _INS_BASE, _INS_EXTRA)
            cmd_syms.append((command_symbol(ic, 0, ic < 8), iv, ib, 0, 0))
            has_dist.append(False)
            if realised is not None:
                realised.append((ins, 0, 0))
            if log is not None:
                log.append({"coding": "tail", "code": None, "insert": len(ins), "word": False, "copy_len": 0, "word_idx": None, "transform": None, "total": 0,
                            "pos": len(history) - pad, "distance": 0, "max_distance": None})
            continue
        pos = len(history) - pad
        max_distance = min(pos + len(dictionary), max_backward) if max_backward is not None else None
        coding, code = "explicit", None
        if callable(what):
            what = what(pos, tuple(ring), max_distance)
        if realised is not None:
            realised.append((ins, clen, what))
        if isinstance(what, tuple):
            assert max_backward is not None, "words, ring codes and implicit distances need wbits"
            if what[0] == "word":
                _, word_idx, transform = what
                assert 4 <= clen <= 24 and 0 <= word_idx < (1 << tables()["size_bits"][clen]) and 0 <= transform < NUM_TRANSFORMS, what
                dist = max_distance + 1 + (transform << tables()["size_bits"][clen]) + word_idx
            elif what[0] == "ring":
                coding, code = "ring", what[1]
                assert 0 <= code <= 15
                if code < 4:
                    dist = ring[code]
                else:
                    dist = ring[(code - 4) // 6] + (1, 2, 3)[((code - 4) % 6) // 2] * (1 if code & 1 else -1)
            elif what[0] == "implicit":
                coding, dist = "implicit", ring[0]
            else:
                assert what[0] == "raw" and unchecked, what
                dist = what[1]
        else:
            dist = what
        ic, iv, ib = _code_of(len(ins), _INS_BASE, _INS_EXTRA)
        cc, cv, cb = _code_of(clen, _COPY_BASE, _COPY_EXTRA)
        cmd_syms.append((command_symbol(ic, cc, coding == "implicit"), iv, ib, cv, cb))
        has_dist.append(coding != "implicit")
        if coding == "explicit":
            dist_syms.append((distance_symbol(dist, npf, ndir), min(3, cc) if cc <= 2 else 3))
        elif coding == "ring":
            dist_syms.append(((code, 0, 0), min(3, cc) if cc <= 2 else 3))
        rec = {"coding": coding, "code": code, "insert": len(ins), "word": False, "copy_len": clen, "word_idx": None, "transform": None, "total": 0, "pos": pos,
               "distance": dist, "max_distance": max_distance}
        if log is not None:
            log.append(rec)
        if max_distance is not None and (dist > max_distance or dist <= 0):
            # a word of the static dictionary (decode.rs:2593-2640); it leaves the ring alone
            rec["word"] = True
            word_id = dist - max_distance - 1
            bits = tables()["size_bits"][clen] if 4 <= clen <= 24 else 0
            word_idx, transform = word_id & ((1 << bits) - 1), word_id >> bits
            if dist <= 0 or not 4 <= clen <= 24 or transform >= NUM_TRANSFORMS:
                assert unchecked, (ci, clen, dist, max_distance)
                rec["invalid"] = True
                invalid_at = ci
                continue
            bytes_ = transform_word(dictionary_word(clen, word_idx), transform)
            rec["word_idx"], rec["transform"], rec["total"] = word_idx, transform, len(bytes_)
            history += bytes_
            continue
        rec["total"] = clen
        if not (coding == "implicit" or code == 0):
            ring = [dist] + ring[:3]
        left = clen
        while left and dictionary and len(history) - dist < pad:
            history.append(dictionary[len(history) - dist - pad]); left -= 1  # (at - pad < 0: counted from the dictionary's end)
        while left:  # (a self-overlapping copy repeats its first `dist` bytes)
            at = len(history) - dist
            n = min(left, dist)
            history += history[at:at + n]; left -= n
    if ring_io is not None:
        ring_io[:] = ring
    if mlen is None:
        mlen = len(history) - start
    else:
        assert unchecked
    # --- block splits
    def expand(blocks, n):
        if not blocks:
            return [(0, n)] if n else [(0, 1 << 24)]
        assert sum(c for _, c in blocks) >= n, (sum(c for _, c in blocks), n)
        return blocks
    lit_blocks = expand(plan.lit_blocks, len(lits))
    cmd_blocks = expand(plan.cmd_blocks, len(cmd_syms))
    dist_blocks = expand(plan.dist_blocks, len(dist_syms))
    nbt = [max(t for t, _ in b) + 1 for b in (lit_blocks, cmd_blocks, dist_blocks)]
    modes = plan.modes or [0] * nbt[0]
    lit_map = plan.lit_map or [t for t in range(nbt[0]) for _ in range(64)]
    dist_map = plan.dist_map or [t for t in range(nbt[2]) for _ in range(4)]
    ntrees_l = max(max(lit_map) + 1, plan.map_forms.get("lit", {}).get("ntrees", 1))   # (a form may declare trees that the map does not name)
    ntrees_d = max(max(dist_map) + 1, plan.map_forms.get("dist", {}).get("ntrees", 1))

    def assign(blocks, n):
        types = []
        for t, c in blocks:
            types += [t] * min(c, n - len(types))
            if len(types) >= n:
                break
        return types
    lit_types, cmd_types, dist_types = assign(lit_blocks, len(lits)), assign(cmd_blocks, len(cmd_syms)), assign(dist_blocks, len(dist_syms))
    # --- histograms
    dist_alpha = 16 + ndir + ((124 if plan.large_window else 48) << npf)
    dist_max = max_distance_symbol(ndir, npf) if plan.large_window else dist_alpha

    def make_code(slot, index, hist, alphabet):
        chosen = plan.codes.get((slot, index))
        return chosen(hist, alphabet) if chosen else PrefixCode(hist, alphabet)

    def write_code(code, slot, index):
        if isinstance(code, WireCode):
            code.write_code(w, hlog, "%s%d" % (slot, index))
        else:
            code.write_code(w)
    h_lit = [[0] * 256 for _ in range(ntrees_l)]
    lit_tree_of = []
    for (b, p1, p2), t in zip(lits, lit_types):
        tree = lit_map[t * 64 + literal_context(modes[t], p1, p2)]
        lit_tree_of.append(tree)
        h_lit[tree][b] += 1
    h_cmd = [[0] * 704 for _ in range(nbt[1])]
    for (sym, *_), t in zip(cmd_syms, cmd_types):
        h_cmd[t][sym] += 1
    h_dist = [[0] * dist_alpha for _ in range(ntrees_d)]
    dist_tree_of = []
    for ((sym, _, _), ctx), t in zip(dist_syms, dist_types):
        tree = dist_map[t * 4 + ctx]
        dist_tree_of.append(tree)
        h_dist[tree][sym] += 1
    # --- header
    if hlog is not None:
        hlog.append({"kind": "metablock", "start": w.bits()})
    write_mlen(w, is_last, mlen, nibbles=nibbles)
    switch_codes = []
    for cat, blocks in enumerate((lit_blocks, cmd_blocks, dist_blocks)):
        write_varlen8(w, nbt[cat] - 1)
        if nbt[cat] < 2:
            switch_codes.append(None)
            continue
        # block type symbols of the switches (first block is type 0 by definition; its length is sent here)
        assert blocks[0][0] == 0
        ring = [1, 0]  # (second last, last) as the decoder keeps them: starts as 1, 0
        tsyms = []
        for t, _ in blocks[1:]:
            if plan.type_codes == "ring" and t == ring[0]:
                s = 0
            elif plan.type_codes == "ring" and t == (ring[1] + 1) % nbt[cat]:
                s = 1
            else:
                s = t + 2
            tsyms.append(s)
            ring = [ring[1], t]
        h_t = [0] * (nbt[cat] + 2)
        for s in tsyms:
            h_t[s] += 1
        h_l = [0] * 26
        lsyms = [_code_of(c, _BL_BASE, _BL_EXTRA) for _, c in blocks]
        for c, _, _ in lsyms:
            h_l[c] += 1
        tcode, lcode = make_code("btype", cat, h_t, nbt[cat] + 2), make_code("blen", cat, h_l, 26)
        write_code(tcode, "btype", cat); write_code(lcode, "blen", cat)
        c, v, nb = lsyms[0]
        lcode.put(w, c); w.put(v, nb)
        switch_codes.append((tcode, lcode, tsyms, lsyms))
        if hlog is not None:
            hlog.append({"kind": "switches", "cat": cat, "nbt": nbt[cat], "type_codes": tsyms, "lengths": lsyms, "counts": [c for _, c in blocks],
                         "symbols": (len(lits), len(cmd_syms), len(dist_syms))[cat], "simple": (tcode.simple, lcode.simple)})
    w.put(npf, 2); w.put(ndir >> npf, 4)
    for t in range(nbt[0]):
        w.put(modes[t], 2)

    write_context_map(w, lit_map[:nbt[0] * 64], ntrees_l, plan.map_forms.get("lit"), plan.codes.get(("lmap", 0)), hlog, "lit_map", unchecked)
    write_context_map(w, dist_map[:nbt[2] * 4], ntrees_d, plan.map_forms.get("dist"), plan.codes.get(("dmap", 0)), hlog, "dist_map", unchecked)
    lit_codes = [make_code("lit", i, h, 256) for i, h in enumerate(h_lit)]
    cmd_codes = [make_code("cmd", i, h, 704) for i, h in enumerate(h_cmd)]
    dist_codes = [make_code("dist", i, h, dist_alpha) for i, h in enumerate(h_dist)]
    for slot, group in (("lit", lit_codes), ("cmd", cmd_codes), ("dist", dist_codes)):
        for i, c in enumerate(group):
            write_code(c, slot, i)
    if hlog is not None:
        hlog.append({"kind": "commands", "start": w.bits()})
    # --- the commands, with block switches where a block's count runs out
    state = []
    for cat, blocks in enumerate((lit_blocks, cmd_blocks, dist_blocks)):
        state.append({"left": blocks[0][1], "next": 0})

    def consume(cat):
        st = state[cat]
        switched = st["left"] == 0
        if switched:
            tcode, lcode, tsyms, lsyms = switch_codes[cat]
            k = st["next"]
            tcode.put(w, tsyms[k])
            c, v, nb = lsyms[k + 1]
            lcode.put(w, c); w.put(v, nb)
            st["left"] = (lit_blocks, cmd_blocks, dist_blocks)[cat][k + 1][1]
            st["next"] = k + 1
        st["left"] -= 1
        return switched
    li = di = 0
    for ci, ins in enumerate(inserts):
        consume(1)
        sym, iv, ib, cv, cb = cmd_syms[ci]
        cmd_codes[cmd_types[ci]].put(w, sym)
        w.put(iv, ib); w.put(cv, cb)
        for b in ins:
            switched = consume(0)
            at = w.bits()
            lit_codes[lit_tree_of[li]].put(w, b)
            if llog is not None:
                _, p1, p2 = lits[li]
                t = lit_types[li]
                llog.append({"k": li, "cmd": ci, "pos": len(prev) + lit_at[li], "bit": at, "nbits": w.bits() - at, "byte": b, "p1": p1, "p2": p2, "type": t,
                             "mode": modes[t], "context": literal_context(modes[t], p1, p2), "tree": lit_tree_of[li], "first_of_block": switched})
            li += 1
        if has_dist[ci]:
            consume(2)
            (dsym, dv, dn), _ = dist_syms[di]
            dist_codes[dist_tree_of[di]].put(w, dsym)
            w.put(dv, dn)
            di += 1
    return bytes(history[start:])
