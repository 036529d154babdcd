"""Every literal code shape, run length and context on every path of the device (needs a real MI355X).

The loops that decode literals are the kernel's most hand-written code: the batch decode of lean_commands (two symbols a step
through ds_bpermute), the wave-parallel decode of process_commands, three copies of the one-at-a-time context loop with their
LUT rows kept four entries a lane, the command records, the helper waves' rounds and the path engine's regions of a long run --
and every hand-over between them passes the two bytes in front of the next literal on.  An encoder derives its codes from the
data and its runs from the matches it finds.  The streams of tests/golden/emitter_literals/ (tools/make_literal_vectors.py,
pinned on the CPU by test_emitter_literals_cpu.py) hold every shape, length and context source by construction; here they go
through each path, against the oracle: result, error code, decoded size, every byte, and for successes consumed, num_commands,
num_metablocks.  A failure names the first differing byte and the probe or run it belongs to."""
import hashlib
import json
import os
import random
import subprocess
import sys
import time

import pytest

import dict_streams
import literal_vectors
import stream_model as sm
from conftest import ROOT
from test_gpu_copies import _child_env
from test_gpu_stream_set import Run
from test_gpu_words import _LEGS, _product_seq, _variants

pytestmark = pytest.mark.gpu
LW = literal_vectors.FLAG_LARGE_WINDOW


def _gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_literal_vectors
    return make_literal_vectors


def _check(pkg, datas, caps, what, flags=0, batch=None, entries=None):
    """test_gpu_headers._check against literal_vectors.expected; `entries`: the manifest entry of each stream, to name what a
    differing byte belongs to"""
    own = batch is None
    batch = batch or pkg.Batch(len(datas))
    results, outs = batch.decode_host(datas, caps, flags)
    if own:
        batch.close()
    bad = []
    for i, (d, cap) in enumerate(zip(datas, caps)):
        info, exp = literal_vectors.expected(d, cap, flags & LW)
        r = results[i]
        ok = (r.result, r.error_code, r.decoded_size, outs[i]) == (info.result, info.error_code, info.decoded_size, exp)
        if ok and info.result == 1:
            ok = r.consumed == info.consumed and r.num_commands == info.num_commands and r.num_metablocks == info.num_metablocks
        if not ok:
            first = next((k for k in range(min(len(outs[i]), len(exp))) if outs[i][k] != exp[k]), None)
            e = entries[i] if entries else None
            bad.append((i, what, e and e["label"], (r.result, r.error_code, r.decoded_size), (info.result, info.error_code, info.decoded_size), r.consumed, info.consumed,
                        len(d), cap, first, e and literal_vectors.where(e, first)))
    assert not bad, (len(bad), bad[:10])
    return results


def _in_batches(pkg, datas, caps, what, flags=0, size=240, entries=None):
    for at in range(0, len(datas), size):
        _check(pkg, datas[at:at + size], caps[at:at + size], "%s %d.." % (what, at), flags, entries=entries and entries[at:at + size])


def _family(family):
    return [(e, c) for e, c in literal_vectors.load() if e["family"] == family]


@pytest.mark.parametrize("family", ["S", "E", "X"])
def test_every_vector_whole_short_truncated_and_damaged(pkg, family):
    """every stream of tests/golden/emitter_literals/ with exact, one-short, half and roomy output buffers (a random one too:
    test_gpu_words._variants) and two truncated and two bit-flipped copies each; without FLAG_LARGE_WINDOW and with it; batches of
    at most 240 streams"""
    t0 = time.time()
    rnd = random.Random(2020)
    datas, caps, entries = [], [], []
    for e, comp in _family(family):
        d, c = _variants(rnd, comp, e["size"])
        d, c = d[:5], c[:5]
        for k in range(2):
            d.append(comp[:rnd.randrange(1, len(comp))]); c.append(e["size"] + 4096)
        for k in range(2):
            f = bytearray(comp); f[rnd.randrange(len(f))] ^= 1 << rnd.randrange(8)
            d.append(bytes(f)); c.append(e["size"] + 4096)
        datas += d; caps += c; entries += [e] * len(d)
    for flags in (0, LW):
        _in_batches(pkg, datas, caps, family, flags, entries=entries)
    print("wall time %.1f s, %d vectors, %d streams" % (time.time() - t0, len(_family(family)), 2 * len(datas)))


_LEG_SCRIPT = r"""
import importlib.util, json, os, sys, hashlib
ROOT = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, "tests"))
import literal_vectors
spec = importlib.util.spec_from_file_location("rust_brotli_decompressor_amd", os.path.join(ROOT, "rust-brotli-decompressor_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec); sys.modules["rust_brotli_decompressor_amd"] = pkg; spec.loader.exec_module(pkg)
streams = literal_vectors.leg_set()
rows, gangs = [], []
for part in (streams[:literal_vectors.SPLIT], streams[literal_vectors.SPLIT:]):
    b = pkg.Batch(len(part))
    res, outs = b.decode_host([c for _, c, _, _ in part], [cap for _, _, cap, _ in part], 0)
    gangs.append(b.last_gang())
    b.close()
    first = []
    for (l, c, cap, _), o in zip(part, outs):
        exp = literal_vectors.expected(c, cap, 0)[1]
        first.append(next((k for k in range(min(len(o), len(exp))) if o[k] != exp[k]), None))
    rows += [[l, r.result, r.error_code, r.decoded_size, r.consumed, r.num_commands, r.num_metablocks, r.engine_commands, hashlib.sha256(o).hexdigest(), f]
             for (l, _, _, _), r, o, f in zip(part, res, outs, first)]
print(json.dumps({"rows": rows, "gangs": gangs}))
"""


def test_every_command_path_agrees_with_the_oracle_and_the_others(pkg):
    """literal_vectors.leg_set (two batches, each led by a stream of more than 64 KiB -- the staircase's runs of 40 000 and
    2 x PE_RUN_MIN + 1 literals -- the size from which a launch forms gangs; the second one's, and the "end" vectors', first
    command is a run of PE_RUN_MIN literals, which a gang declines) in a fresh process per leg of test_gpu_words._LEGS.  All legs return the oracle's
    status words and SHA-256s, and one another's.  `engine_commands` says which path ran and is printed per leg; what the code
    guarantees is asserted: none without records, and gangs in the gang leg."""
    t0 = time.time()
    streams = literal_vectors.leg_set()
    entries = literal_vectors.by_label()
    by = {l: (c, cap, f) for l, c, cap, f in streams}
    for _, comp, cap, flags in streams:   # (the oracle is built and its answers are known before the legs, which ask it for the first differing byte, start)
        literal_vectors.expected(comp, cap, flags)
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
        print("engine_commands of num_commands,", name, {r[0]: (r[7], r[5]) for r in g["rows"] if "/" not in r[0]}, "gangs:", g["gangs"])
    for name, g in got.items():
        bad = []
        assert len(g["rows"]) == len(streams)
        for r in g["rows"]:
            comp, cap, flags = by[r[0]]
            info, exp = literal_vectors.expected(comp, cap, flags)
            ok = r[1:4] == [info.result, info.error_code, info.decoded_size] and r[8] == hashlib.sha256(exp).hexdigest()
            if ok and info.result == 1:
                ok = r[4:7] == [info.consumed, info.num_commands, info.num_metablocks]
            if not ok:
                e = entries.get(r[0].split("/")[0], ({},))[0]
                bad.append((r[:7], (info.result, info.error_code, info.decoded_size, info.consumed, info.num_commands), r[9], literal_vectors.where(e, r[9])))
        assert not bad, (name, len(bad), bad[:8])
    strip = lambda rs: [r[:7] + r[8:] for r in rs]   # (everything but engine_commands)
    for name, g in got.items():
        assert strip(g["rows"]) == strip(got["general"]["rows"]), name
    assert all(r[7] == 0 for r in got["norec"]["rows"])
    assert all(g >= 2 for g in got["gang8"]["gangs"]) and len(got["gang8"]["gangs"]) == 2, got["gang8"]["gangs"]
    print("wall time %.1f s, %d streams a leg" % (time.time() - t0, len(streams)))


def _arena_set():
    """one vector per shape (the sweep in front for the simple codes, at the end for the others, the staircase both), the vector of
    256 trees and the one whose types are trivial and not"""
    by = literal_vectors.by_label()
    names = ["S-%s-front" % s for s in ("simple1", "simple2", "simple3", "simple4a", "simple4b", "stair")]
    names += ["S-%s-end" % s for s in ("flat8", "stair", "deep9", "deep10", "deep11", "deep12", "grid")] + ["X-every-tree", "X-maps"]
    return [by[n] for n in names]


@pytest.mark.parametrize("arena", [256, 4096])
def test_small_lds_arenas(pkg, arena):
    """Batch(n, lds_arena_bytes=256) and 4096, spilling in place and with the second pass from a metablock boundary: the generic
    loop with its tables in global scratch, where the default arena has the 64 trees of a block type in its cache"""
    t0 = time.time()
    rnd = random.Random(arena)
    datas, caps, entries = [], [], []
    for e, c in _arena_set():
        datas += [c, c, c[:rnd.randrange(len(c) // 2, len(c))]]; caps += [e["size"], e["size"] // 2, e["size"] + 64]; entries += [e] * 3
    for spill in (pkg.FLAG_SPILL_IN_PLACE, 0):
        batch = pkg.Batch(len(datas), lds_arena_bytes=arena)
        results = _check(pkg, datas, caps, "arena %d spill %d" % (arena, spill), spill, batch, entries)
        batch.close()
        if spill and arena == 256:
            assert sum(r.spilled_metablocks for r in results) > 0
    print("wall time %.1f s" % (time.time() - t0))


@pytest.mark.parametrize("per_cu", [4, 2])
def test_blocks_of_one_and_four_waves(pkg, per_cu):
    """4 * CUs + 1 streams (more than four blocks a CU: blocks of one wave and the small automatic arena) and 2 * CUs + 1 (blocks
    of four waves), cycling over eight vectors: the staircase in front and at the end, the grid code, a simple code of two symbols,
    the LUT cells of two modes, the word cells and the vector of 256 trees"""
    import torch
    t0 = time.time()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    by = literal_vectors.by_label()
    eight = [by[n] for n in ("S-stair-front", "S-stair-end", "S-grid-end", "S-simple2-front", "X-lut-mode1", "X-lut-mode3", "X-words", "X-every-tree")]
    n = per_cu * cus + 1
    _check(pkg, [eight[i % 8][1] for i in range(n)], [eight[i % 8][0]["size"] for i in range(n)], "%d blocks a CU" % per_cu, entries=[eight[i % 8][0] for i in range(n)])
    print("wall time %.1f s, %d streams" % (time.time() - t0, n))


def test_the_output_limits_of_e(pkg):
    """the run of 130 literals with every output limit from two in front of the run to one behind it, the runs of SPEC_ROUND_MIN and
    PE_RUN_MIN literals with limits +-2 round every multiple of 64 in their first 256 literals and at their last three: one batch"""
    t0 = time.time()
    L = _gen()
    datas, caps, entries = [], [], []
    for e, c in _family("E"):
        if "-cap-" in e["label"]:
            for cap in L.cap_sweep(e):
                datas.append(c); caps.append(cap); entries.append(e)
    assert len(datas) >= 2 * (134 + 2 * 25)
    results = _check(pkg, datas, caps, "output limits", entries=entries)
    assert all(r.decoded_size == cap for r, cap in zip(results, caps))   # (every limit lies inside the stream's output)
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(datas)))


def _small_streams():
    """test_gpu_headers._small_streams's rule: less than 1 KiB of output at window 10 and at most 4 KiB otherwise, and less than
    2 KiB of stream -> [(entry, stream)], the longest first"""
    small = [(e, c) for e, c in literal_vectors.load() if e["size"] < (1024 if e["window"] == 10 else 4097) and e["csize"] < 2048]
    return sorted(small, key=lambda x: -x[0]["csize"] - x[0]["size"])


_PARTS = 6


@pytest.mark.parametrize("chunks", [(1, 1), (3, 3), (65536, 1)])
@pytest.mark.parametrize("part", range(_PARTS))
def test_small_streams_byte_by_byte(pkg, part, chunks):
    """every small vector through BrotliDecoderDecompressStream: call for call what the model of the reference's driver returns
    (tests/stream_model.py), and the oracle's bytes"""
    t0 = time.time()
    ic, oc = chunks
    streams = _small_streams()
    assert len(streams) >= 150, len(streams)
    streams = streams[part::_PARTS]
    for e, comp in streams:
        got, out = _product_seq(pkg, comp, ic, oc)
        m = sm.ReferenceStream(comp)
        want = sm.run_schedule(lambda pending, cap: m.call(len(pending), cap), comp, ic, oc, drain=True)
        assert got == want, (e["label"], chunks, next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w))
        exp = literal_vectors.expected(comp, e["size"], 0)[1]
        first = next((k for k in range(min(len(out), len(exp))) if out[k] != exp[k]), None)
        assert out == exp and hashlib.sha256(out).hexdigest()[:16] == e["sha"], (e["label"], first, literal_vectors.where(e, first))
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(streams)))


def test_three_vectors_in_a_stream_set(pkg):
    """one vector of each sub-family with chunks (64, 37): three states stepped by a StreamSet and the same three stepped alone give
    the same calls and bytes, and the bytes are the oracle's"""
    by = literal_vectors.by_label()
    t0 = time.time()
    names = ["S-deep9-end", "E-stair-block-800-768", "X-words"]
    jobs = [dict(data=by[n][1], ic=64, oc=37, lw=False) for n in names]
    run, twin = Run(pkg, jobs).run(), Run(pkg, jobs).run(how=lambda k: "solo")
    try:
        for i, n in enumerate(names):
            assert run.seq[i] == twin.seq[i] and run.seq[i][-1][0] == 1, n
            exp = literal_vectors.expected(by[n][1], by[n][0]["size"], 0)[1]
            assert run.bytes_of(i) == twin.bytes_of(i) == exp and hashlib.sha256(exp).hexdigest()[:16] == by[n][0]["sha"], n
    finally:
        run.close(); twin.close()
    print("wall time %.1f s" % (time.time() - t0))


def test_the_cells_with_custom_dictionaries(pkg):
    """the word cells and the source cells emitted again for seeded dictionaries of 1, 17, 300 and 70000 bytes (dict_streams.text):
    the copies of 5 and the short copies of the source cells lie in the dictionary (from_cdict), and the stream's first two
    literals have the context (0, 0) whatever the dictionary ends in.  Against brotli_oracle_decode_dict through dict_streams.check:
    whole, short, half and cut."""
    t0 = time.time()
    L = _gen()
    rnd = random.Random(302)
    datas, caps, dicts = [], [], []
    for size in (1, 17, 300, 70000):
        dictionary = dict_streams.text(rnd, size)
        for b in (L.x_words(3040 + size, dictionary), L.x_source(3020 + size, dictionary)):
            comp, raw = b.w.finish(), bytes(b.out)
            assert size < 5 or any(r["distance"] > r["pos"] and not r["word"] for r in b.clog)
            info, out = dict_streams.expected(comp, len(raw), 0, dictionary)
            assert info.result == 1 and out == raw
            for cap in (len(raw), len(raw) - 1, len(raw) // 2, len(raw) + 1000):
                datas.append(comp); caps.append(cap); dicts.append(dictionary)
            datas.append(comp[:len(comp) * 2 // 3]); caps.append(len(raw)); dicts.append(dictionary)
    dict_streams.check(pkg, datas, caps, dicts, flags=0, what="cells with custom dictionaries")
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(datas)))
