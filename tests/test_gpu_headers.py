"""Every form of a metablock's header on every path of the device (needs a real MI355X).

What lies in front of the first command is where the kernel departs furthest from the reference's loop: read_symbol_lengths_wide
reads code lengths 64 stream bits a step (a chain of words by pointer doubling, repeat runs as numbers in base four or eight,
32-bit prefix sums, ballots), decode_context_map has its own zero-run decoder and an inverse move-to-front of 64 entries a step,
block_switch / read_block_length are reached from four loops, and the launch that asks the device about its streams parses the
header in code of its own.  An encoder library writes a sliver of these forms.  The streams of tests/golden/emitter_headers/
(tools/make_header_vectors.py, pinned on the CPU by test_emitter_headers_cpu.py) hold every one by construction; here they go
through each path, against the oracle: result, error code, decoded size, every byte, and for successes consumed, num_commands,
num_metablocks."""
import hashlib
import json
import os
import random
import subprocess
import sys
import time

import pytest

import header_vectors
import stream_model as sm
from conftest import ROOT
from test_gpu_copies import _child_env
from test_gpu_stream_set import Run
from test_gpu_words import _LEGS, _product_seq, _variants

pytestmark = pytest.mark.gpu
LW = header_vectors.FLAG_LARGE_WINDOW


def _gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_header_vectors
    return make_header_vectors


def _check(pkg, datas, caps, what, flags=0, batch=None):
    """test_gpu_words._check against header_vectors.expected"""
    own = batch is None
    batch = batch or pkg.Batch(len(datas))
    results, outs = batch.decode_host(datas, caps, flags)
    if own:
        batch.close()
    bad = []
    for i, (d, cap) in enumerate(zip(datas, caps)):
        info, exp = header_vectors.expected(d, cap, flags & LW)
        r = results[i]
        ok = (r.result, r.error_code, r.decoded_size, outs[i]) == (info.result, info.error_code, info.decoded_size, exp)
        if ok and info.result == 1:
            ok = r.consumed == info.consumed and r.num_commands == info.num_commands and r.num_metablocks == info.num_metablocks
        if not ok:
            first = next((k for k in range(min(len(outs[i]), len(exp))) if outs[i][k] != exp[k]), None)
            bad.append((i, what, (r.result, r.error_code, r.decoded_size), (info.result, info.error_code, info.decoded_size), r.consumed, info.consumed, len(d), cap, first))
    assert not bad, (len(bad), bad[:10])
    return results


def _in_batches(pkg, datas, caps, what, flags=0, size=240):
    for at in range(0, len(datas), size):
        _check(pkg, datas[at:at + size], caps[at:at + size], "%s %d.." % (what, at), flags)


def _family(family):
    return [(e, c) for e, c in header_vectors.load() if e["family"] == family]


@pytest.mark.parametrize("family", ["P", "C", "B", "M"])
def test_every_vector_whole_short_truncated_and_damaged(pkg, family):
    """every stream of tests/golden/emitter_headers/ with exact, one-short, half and roomy output buffers (a random one too:
    test_gpu_words._variants) and two truncated and two bit-flipped copies each; the one of 16 MiB of output exact and one short;
    without FLAG_LARGE_WINDOW and with it (the large-window streams: with it); batches of at most 240 streams"""
    t0 = time.time()
    rnd = random.Random(2019)
    by_flags = {0: ([], []), LW: ([], [])}
    for e, comp in _family(family):
        datas, caps = by_flags[header_vectors.flags_of(e)]
        if header_vectors.big(e):
            datas += [comp, comp]; caps += [e["size"], e["size"] - 1]
            continue
        d, c = _variants(rnd, comp, e["size"])
        d, c = d[:5], c[:5]
        for k in range(2):
            d.append(comp[:rnd.randrange(1, len(comp))]); c.append(e["size"] + 4096)
        for k in range(2):
            f = bytearray(comp); f[rnd.randrange(len(f))] ^= 1 << rnd.randrange(8)
            d.append(bytes(f)); c.append(e["size"] + 4096)
        datas += d; caps += c
        if not e["large"]:
            by_flags[LW][0].extend(d); by_flags[LW][1].extend(c)
    n = 0
    for flags, (datas, caps) in by_flags.items():
        _in_batches(pkg, datas, caps, family, flags)
        n += len(datas)
    print("wall time %.1f s, %d vectors, %d streams" % (time.time() - t0, len(_family(family)), n))


_CUTS = [("P", "lit"), ("P", "cmd"), ("P", "d64"), ("P", "d520"), ("P", "dlw"), ("C", ""), ("B", ""), ("M", "")]


@pytest.mark.parametrize("family,slot", _CUTS)
def test_every_header_cut_at_every_byte(pkg, family, slot):
    """every vector with at most 700 bytes in front of the first command of its last metablock, cut after each of those bytes (and
    after the first byte of the commands): verdict -- NEEDS_MORE_INPUT, or the fault where it lies in front of the cut -- and
    delivered bytes are the oracle's; without FLAG_LARGE_WINDOW and with it"""
    t0 = time.time()
    by_flags = {0: ([], []), LW: ([], [])}
    n = 0
    for e, comp in _family(family):
        if e["first_command"] > 700 or not e["label"].startswith("P-%s-" % slot if slot else family):
            continue
        for flags in ((LW,) if e["large"] else (0, LW)):
            datas, caps = by_flags[flags]
            for cut in range(0, min(len(comp), e["first_command"] + 2)):   # (room for what lies in front of the header: never more than 64 KiB)
                datas.append(comp[:cut]); caps.append(min(e["size"], 1 << 16) + 64)
        n += 1
    for flags, (datas, caps) in by_flags.items():
        _in_batches(pkg, datas, caps, "%s%s cuts" % (family, slot), flags)
    assert n >= 40
    print("wall time %.1f s, %d vectors, %d streams" % (time.time() - t0, n, sum(len(d) for d, _ in by_flags.values())))


def test_the_other_setting_of_the_large_window_flag(pkg):
    """every vector whole under FLAG_LARGE_WINDOW (a stream of a standard window decodes alike), and the large-window streams --
    the distance codes whose max_symbol lies below their alphabet among them -- without it (E_WINDOW_BITS)"""
    t0 = time.time()
    vectors = [(e, c) for e, c in header_vectors.load() if not header_vectors.big(e)]
    _in_batches(pkg, [c for e, c in vectors], [header_vectors.cap_of(e) for e, c in vectors], "with the flag", LW)
    large = [(e, c) for e, c in vectors if e["large"]]
    assert len(large) >= 80
    results = _check(pkg, [c for e, c in large], [header_vectors.cap_of(e) for e, c in large], "without the flag", 0)
    assert all((r.result, r.error_code) == (0, -13) for r in results)
    print("wall time %.1f s, %d + %d streams" % (time.time() - t0, len(vectors), len(large)))


_LEG_SCRIPT = r"""
import importlib.util, json, os, sys, hashlib
ROOT = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, "tests"))
import header_vectors
spec = importlib.util.spec_from_file_location("rust_brotli_decompressor_amd", os.path.join(ROOT, "rust-brotli-decompressor_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec); sys.modules["rust_brotli_decompressor_amd"] = pkg; spec.loader.exec_module(pkg)
streams = header_vectors.leg_set()
rows, gangs = [], []
for part in (streams[:header_vectors.SPLIT], streams[header_vectors.SPLIT:]):
    for flags in sorted({f for _, _, _, f in part}):
        sel = [s for s in part if s[3] == flags]
        b = pkg.Batch(len(sel))
        res, outs = b.decode_host([c for _, c, _, _ in sel], [cap for _, _, cap, _ in sel], flags)
        if flags == 0:
            gangs.append(b.last_gang())
        b.close()
        rows += [[l, r.result, r.error_code, r.decoded_size, r.consumed, r.num_commands, r.num_metablocks, r.engine_commands, hashlib.sha256(o).hexdigest()]
                 for (l, _, _, _), r, o in zip(sel, res, outs)]
print(json.dumps({"rows": rows, "gangs": gangs}))
"""


def test_every_command_path_agrees_with_the_oracle_and_the_others(pkg):
    """header_vectors.leg_set (two batches, each led by a stream of more than 64 KiB, the size from which a launch forms gangs) in
    a fresh process per leg of test_gpu_words._LEGS.  All legs return the oracle's status words and SHA-256s, and one another's.
    `engine_commands` says which path ran and is printed per leg; what the code guarantees is asserted: none without records, some
    for B's long form (a switch every 1 .. 40 symbols in each category, no context modelling) under the record loop, and gangs in
    the gang leg."""
    t0 = time.time()
    streams = header_vectors.leg_set()
    by = {l: (c, cap, f) for l, c, cap, f in streams}
    got = {}
    running = [(name, subprocess.Popen([sys.executable, "-c", _LEG_SCRIPT, ROOT], env=_child_env(env), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)) for name, env in _LEGS]
    try:
        for name, p in running:
            out, err = p.communicate(timeout=600)
            assert p.returncode == 0, (name, err[-2000:])
            got[name] = json.loads(out.strip().splitlines()[-1])
    finally:
        for _, p in running:
            if p.poll() is None:
                p.kill(); p.wait()
    for name, g in got.items():
        print("engine_commands of num_commands,", name, {r[0]: (r[7], r[5]) for r in g["rows"] if "/" not in r[0] and r[5] >= 40}, "gangs:", g["gangs"])
    for name, g in got.items():
        bad = []
        assert len(g["rows"]) == len(streams)
        for r in g["rows"]:
            comp, cap, flags = by[r[0]]
            info, exp = header_vectors.expected(comp, cap, flags)
            ok = r[1:4] == [info.result, info.error_code, info.decoded_size] and r[8] == hashlib.sha256(exp).hexdigest()
            if ok and info.result == 1:
                ok = r[4:7] == [info.consumed, info.num_commands, info.num_metablocks]
            if not ok:
                bad.append((r[:7], (info.result, info.error_code, info.decoded_size, info.consumed, info.num_commands)))
        assert not bad, (name, len(bad), bad[:8])
    strip = lambda rs: [r[:7] + r[8:] for r in rs]   # (everything but engine_commands)
    for name, g in got.items():
        assert strip(g["rows"]) == strip(got["general"]["rows"]), name
    eng = lambda name, label: next(r[7] for r in got[name]["rows"] if r[0] == label)
    assert all(r[7] == 0 for r in got["norec"]["rows"])
    assert eng("records", "B-long") > 0, eng("records", "B-long")
    assert all(g >= 2 for g in got["gang8"]["gangs"]) and len(got["gang8"]["gangs"]) == 2, got["gang8"]["gangs"]
    print("wall time %.1f s, %d streams a leg" % (time.time() - t0, len(streams)))


def _arena_set():
    """vectors with many and with large tables, maps that are parked in the cold arena, several metablocks"""
    by = {e["label"]: (e, c) for e, c in header_vectors.load()}
    names = ["B-lit-n256-ring", "B-cmd-n256-direct", "B-dist-n256-ring", "B-lit-n255-direct", "C-lit-n256-r16", "C-lit-n255-r5", "C-dist-n256-r16", "C-imtf-big-r9",
             "C-runs-1-8", "C-some-types-trivial", "B-long", "B-lit-every-length-code", "B-cmd-every-length-code", "B-ones-all", "P-cmd-depth-sixteens",
             "P-lit-one-16", "P-cmd-17chain-k4-e0", "P-d520-16chain-k5-e1", "P-dlw-depth-plain", "P-lit-V-seventeens-21", "C-V-run-c16-ones", "M-metadata-run-200x1"]
    return [by[n] for n in names]


@pytest.mark.parametrize("arena", [256, 4096])
def test_small_lds_arenas(pkg, arena):
    """Batch(n, lds_arena_bytes=256) and 4096, spilling in place (the tables and the parked map lie in the block's global scratch:
    the cold allocations of read_huffman_code) and with the second pass from a metablock boundary"""
    t0 = time.time()
    rnd = random.Random(arena)
    for flags in (0, LW):
        sel = [(e, c) for e, c in _arena_set() if header_vectors.flags_of(e) == flags]
        datas, caps = [], []
        for e, c in sel:
            datas += [c, c, c[:rnd.randrange(len(c) // 2, len(c))]]; caps += [header_vectors.cap_of(e), e["size"] // 2, e["size"] + 64]
        for spill in (pkg.FLAG_SPILL_IN_PLACE, 0):
            batch = pkg.Batch(len(datas), lds_arena_bytes=arena)
            results = _check(pkg, datas, caps, "arena %d spill %d" % (arena, spill), flags | spill, batch)
            batch.close()
            if spill and flags == 0 and arena == 256:
                assert sum(r.spilled_metablocks for r in results) > 0
    print("wall time %.1f s" % (time.time() - t0))


def test_one_wave_blocks(pkg):
    """4 * CUs + 1 streams cycling over eight vectors: more than four blocks a CU, which are blocks of one wave and the small
    automatic arena whatever the streams are"""
    import torch
    t0 = time.time()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    by = {e["label"]: (e, c) for e, c in header_vectors.load()}
    eight = [by[n] for n in ("B-long", "B-lit-n256-ring", "C-imtf-every-tree-r9", "C-some-types-trivial", "P-cmd-depth-sixteens", "P-lit-one-16", "P-cmd-16chain-k5-e3",
                             "P-lit-V-seventeens-21")]
    n = 4 * cus + 1
    _check(pkg, [eight[i % 8][1] for i in range(n)], [header_vectors.cap_of(eight[i % 8][0]) for i in range(n)], "one-wave blocks")
    print("wall time %.1f s, %d streams" % (time.time() - t0, n))


_PROBE_SCRIPT = r"""
import sys, os, json, hashlib
sys.path.insert(0, sys.argv[1])
import conftest, test_gpu_headers as t
print(json.dumps(t._probe_batch(conftest.load_pkg())))
"""


def _probe_streams(cus):
    """CUs + 1 streams with a mean of 8 KiB or more compressed: the vectors of 256 block types, B's long form and its
    every-length-code streams, and headers with faults behind a stored metablock of 8 KiB (make_header_vectors.behind_stored)"""
    by = {e["label"]: (e, c) for e, c in header_vectors.load()}
    pool = [(c, header_vectors.cap_of(e)) for e, c in (by[n] for n in ("B-long", "B-lit-n256-ring", "B-lit-every-length-code", "B-lit-n255-direct",
                                                                          "B-cmd-every-length-code", "B-long", "B-dist-every-length-code", "B-lit-n256-direct"))]
    pool += [(c, len(raw) + 64) for _, c, raw in _gen().behind_stored()]
    n = cus + 1
    streams = [pool[i % len(pool)] for i in range(n)]
    assert sum(len(c) for c, _ in streams) >= 8192 * n, sum(len(c) for c, _ in streams) / n
    return streams


def _probe_batch(pkg):
    import torch
    streams = _probe_streams(torch.cuda.get_device_properties(0).multi_processor_count)
    results = _check(pkg, [c for c, _ in streams], [cap for _, cap in streams], "probe")
    return [len(streams), sum(1 for r in results if r.result == 1)]


def test_the_launch_that_asks_first(pkg):
    """a batch of CUs + 1 streams with a mean of 8 KiB or more compressed is one the launch asks the device about first: that
    launch decodes the distance context map and both tree groups in code of its own.  In a child with BROTLI_AMD_DEBUG_PROBE=1:
    stderr shows that it ran, and every result is the oracle's."""
    t0 = time.time()
    out = subprocess.run([sys.executable, "-c", _PROBE_SCRIPT, os.path.join(ROOT, "tests")], env=_child_env({"BROTLI_AMD_DEBUG_PROBE": "1"}),
                         capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    n, good = json.loads(out.stdout.strip().splitlines()[-1])
    assert "probe: %d streams" % n in out.stderr, out.stderr[-2000:]
    assert 0 < good < n
    print(out.stderr.strip().splitlines()[-1])
    print("wall time %.1f s, %d streams" % (time.time() - t0, n))


# (C in twelve parts, B in two, the longest streams dealt round -- the longest of all, a map of 16384 entries behind 1.5 KB of header, takes
# some seven seconds byte by byte on its own, and a vector cannot be split: a call costs a pass over the header, and theirs are maps of 16384 entries and codes for 256 types)
_STREAMED = [(f, s, 0, 1) for f, s in _CUTS if f in "PM"] + [("C", "", k, 12) for k in range(12)] + [("B", "", k, 2) for k in range(2)]


def _small_streams(family, slot):
    """the valid vectors of a family (of P: of one place a code stands in) with less than 1 KiB of output at window 10 and at
    most 4 KiB otherwise -- under every ring -- and less than 2 KiB of stream.  That leaves out the 23 vectors that are large on
    purpose: B's long form, its every-length-code streams and the literal and distance forms of 255 and 256 types, one
    move-to-front map of 16384 entries, M's MLEN and metadata sizes from 64 KiB on, and three command codes whose symbols insert
    hundreds of literals -> [(entry, stream)]"""
    return [(e, c) for e, c in header_vectors.load() if e["valid"] and e["size"] < (1024 if e["window"] == 10 else 4097) and e["csize"] < 2048
            and e["label"].startswith("P-%s-" % slot if slot else family)]


@pytest.mark.parametrize("chunks", [(1, 1), (3, 3), (65536, 1)])
@pytest.mark.parametrize("family,slot,part,parts", _STREAMED)
def test_small_streams_byte_by_byte(pkg, family, slot, part, parts, chunks):
    """every small vector of P, C, B and M through BrotliDecoderDecompressStream: call for call what the model of the reference's
    driver returns (tests/stream_model.py), and the oracle's bytes; product and model both with the large-window setting on, under
    which the streams of a standard window decode alike"""
    t0 = time.time()
    ic, oc = chunks
    streams = _small_streams(family, slot)
    assert len(streams) >= {"P": 60, "C": 40, "B": 30, "M": 30}[family], len(streams)
    streams = sorted(streams, key=lambda x: -x[0]["csize"] - x[0]["size"])[part::parts]
    for e, comp in streams:
        got, out = _product_seq(pkg, comp, ic, oc)
        m = sm.ReferenceStream(comp)
        want = sm.run_schedule(lambda pending, cap: m.call(len(pending), cap), comp, ic, oc, drain=True)
        assert got == want, (e["label"], chunks, next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w))
        assert out == header_vectors.expected(comp, e["size"], header_vectors.flags_of(e))[1] and hashlib.sha256(out).hexdigest()[:16] == e["sha"], e["label"]
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(streams)))


def test_four_vectors_in_a_stream_set(pkg):
    """one vector of each family with chunks (64, 37): four states stepped by a StreamSet and the same four stepped alone give the
    same calls and bytes, and the bytes are the oracle's"""
    by = {e["label"]: (e, c) for e, c in header_vectors.load()}
    t0 = time.time()
    names = ["P-cmd-depth-sixteens", "C-imtf-every-tree-r9", "B-ones-all", "M-metadata-run-200x1"]
    jobs = [dict(data=by[n][1], ic=64, oc=37, lw=False) for n in names]
    run, twin = Run(pkg, jobs).run(), Run(pkg, jobs).run(how=lambda k: "solo")
    try:
        for i, n in enumerate(names):
            assert run.seq[i] == twin.seq[i] and run.seq[i][-1][0] == 1, n
            exp = header_vectors.expected(by[n][1], by[n][0]["size"], 0)[1]
            assert run.bytes_of(i) == twin.bytes_of(i) == exp and hashlib.sha256(exp).hexdigest()[:16] == by[n][0]["sha"], n
    finally:
        run.close(); twin.close()
    print("wall time %.1f s" % (time.time() - t0))
