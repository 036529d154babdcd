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
import random
import time

import pytest

import literal_vectors
import path_harness as H

import dict_gen  # noqa: I100  (tools/, which path_harness has put on the path)
import make_literal_vectors as L  # noqa: I100

pytestmark = pytest.mark.gpu
LW = literal_vectors.FLAG_LARGE_WINDOW


def _check(pkg, datas, caps, what, flags=0, batch=None, entries=None):
    """path_harness.check; `entries`: the manifest entry of each stream, to name what a differing byte belongs to"""
    return H.check(pkg, datas, caps, None, flags, what, batch, entries, literal_vectors.where)


def _family(family):
    return [(e, c) for e, c in literal_vectors.load() if e["family"] == family]


@pytest.mark.parametrize("family", ["S", "E", "X"])
def test_every_vector_whole_short_truncated_and_damaged(pkg, family):
    """every stream of tests/golden/emitter_literals/ with exact, one-short, half and roomy output buffers (a random one too:
    path_harness.variants) and two truncated and two bit-flipped copies each; without FLAG_LARGE_WINDOW and with it; batches of
    at most 240 streams"""
    t0 = time.time()
    rnd = random.Random(2020)
    datas, caps, entries = [], [], []
    for e, comp in _family(family):
        d, c = H.variants(rnd, comp, e["size"], "tails")
        datas += d; caps += c; entries += [e] * len(d)
    for flags in (0, LW):
        H.in_batches(pkg, datas, caps, None, flags, family, entries=entries, where=literal_vectors.where)
    print("wall time %.1f s, %d vectors, %d streams" % (time.time() - t0, len(_family(family)), 2 * len(datas)))


def test_every_command_path_agrees_with_the_oracle_and_the_others(pkg):
    """literal_vectors.leg_set (two batches, each led by a stream of more than 64 KiB -- the staircase's runs of 40 000 and
    2 x PE_RUN_MIN + 1 literals -- the size from which a launch forms gangs; the second one's, and the "end" vectors', first
    command is a run of PE_RUN_MIN literals, which a gang declines) in a fresh process per leg of path_harness.LEGS.  All legs return the oracle's
    status words and SHA-256s, and one another's.  `engine_commands` says which path ran and is printed per leg; what the code
    guarantees is asserted: none without records, and gangs in the gang leg."""
    t0 = time.time()
    entries = literal_vectors.by_label()
    got = H.run_legs(literal_vectors, where=lambda label, k: literal_vectors.where(entries.get(label.split("/")[0], ({},))[0], k))
    assert all(r[H.ENGINE] == 0 for r in got["norec"]["rows"].values())
    assert all(g >= 2 for g in got["gang8"]["gangs"]) and len(got["gang8"]["gangs"]) == 2, got["gang8"]["gangs"]
    print("wall time %.1f s, %d streams a leg" % (time.time() - t0, len(got["general"]["rows"])))


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
    t0 = time.time()
    by = literal_vectors.by_label()
    eight = [by[n] for n in ("S-stair-front", "S-stair-end", "S-grid-end", "S-simple2-front", "X-lut-mode1", "X-lut-mode3", "X-words", "X-every-tree")]
    _, n = H.blocks_a_cu(pkg, eight, per_cu, "%d blocks a CU" % per_cu, literal_vectors.where)
    print("wall time %.1f s, %d streams" % (time.time() - t0, n))


def test_the_output_limits_of_e(pkg):
    """the run of 130 literals with every output limit from two in front of the run to one behind it, the runs of SPEC_ROUND_MIN and
    PE_RUN_MIN literals with limits +-2 round every multiple of 64 in their first 256 literals and at their last three: one batch"""
    t0 = time.time()
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
        out = H.streamed_like_the_model(pkg, comp, ic, oc, e["label"])
        exp = literal_vectors.expected(comp, e["size"], 0)[1]
        first = H.first_difference(out, exp)
        assert out == exp and hashlib.sha256(out).hexdigest()[:16] == e["sha"], (e["label"], first, literal_vectors.where(e, first))
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(streams)))


def test_three_vectors_in_a_stream_set(pkg):
    """one vector of each sub-family with chunks (64, 37): three states stepped by a StreamSet and the same three stepped alone give
    the same calls and bytes, and the bytes are the oracle's"""
    by = literal_vectors.by_label()
    t0 = time.time()
    names = ["S-deep9-end", "E-stair-block-800-768", "X-words"]
    jobs = [dict(data=by[n][1], ic=64, oc=37, lw=False) for n in names]
    want = [literal_vectors.expected(by[n][1], by[n][0]["size"], 0)[1] for n in names]
    assert [hashlib.sha256(exp).hexdigest()[:16] for exp in want] == [by[n][0]["sha"] for n in names]
    H.stream_set_like_solo(pkg, jobs, names, want)
    print("wall time %.1f s" % (time.time() - t0))


def test_the_cells_with_custom_dictionaries(pkg):
    """the word cells and the source cells emitted again for seeded dictionaries of 1, 17, 300 and 70000 bytes (dict_gen.text):
    the copies of 5 and the short copies of the source cells lie in the dictionary (from_cdict), and the stream's first two
    literals have the context (0, 0) whatever the dictionary ends in.  Against brotli_oracle_decode_dict through path_harness.check:
    whole, short, half and cut."""
    t0 = time.time()
    rnd = random.Random(302)
    datas, caps, dicts = [], [], []
    for size in (1, 17, 300, 70000):
        dictionary = dict_gen.text(rnd, size)
        for b in (L.x_words(3040 + size, dictionary), L.x_source(3020 + size, dictionary)):
            comp, raw = b.w.finish(), bytes(b.out)
            assert size < 5 or any(r["distance"] > r["pos"] and not r["word"] for r in b.clog)
            info, out = H.expected(comp, len(raw), 0, dictionary)
            assert info.result == 1 and out == raw
            for cap in (len(raw), len(raw) - 1, len(raw) // 2, len(raw) + 1000):
                datas.append(comp); caps.append(cap); dicts.append(dictionary)
            datas.append(comp[:len(comp) * 2 // 3]); caps.append(len(raw)); dicts.append(dictionary)
    H.check(pkg, datas, caps, dicts, flags=0, what="cells with custom dictionaries")
    print("wall time %.1f s, %d streams" % (time.time() - t0, len(datas)))
